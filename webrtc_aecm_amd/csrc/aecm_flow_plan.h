// The session wrapper and the frame adapter of ONE session as position arithmetic, for the device.
//
// Between the public ABI and WebRtcAecm_ProcessBlock the reference only MOVES samples (aecm_session_flow.h restates
// that machinery generically; reference aecm/echo_control_mobile.cc:215-408, 534-594, aecm/aecm_core.cc:501-572,
// aecm/ring_buffer.c).  Every one of its buffers is written front to back, so a buffer never has to be simulated
// sample by sample: the jitter buffer is the pair (samples accepted so far, samples consumed so far) over an absolute
// "far stream", the frame rings are the pair (samples framed, samples blocked) over the stream of 80-sample frames,
// the output ring is the pair (block outputs produced, output samples delivered).  A tick of a session is then a
// handful of integer updates -- FlowTick below -- that yield a PLAN: which input samples the jitter buffer accepts
// and where they go, where each 80-sample far frame comes from (the far stream or the replay copy of an underrun),
// how many blocks each frame completes, and where each output frame is read.  On the device a tick is two launches:
// aecm_flow_plan_kernel runs FlowTick with ONE LANE PER SESSION (64 sessions per wavefront; the state is stored field-
// major so that the lanes' accesses coalesce) and leaves each session's plan as kFlowPlanWords words; aecm_tick_flow_kernel
// (one wavefront per session) reads its plan into scalar registers and moves the samples it names around the blocks.
// Nothing about a session lives on the host, so every session may have its own msInSndCardBuf and call pattern.
//
// All positions are uint32 counters that wrap; only differences and positions modulo a power-of-two ring are used.
#ifndef AECM_AMD_FLOW_PLAN_H_
#define AECM_AMD_FLOW_PLAN_H_

#include <stdint.h>

#include <initializer_list>

#if defined(__HIPCC__)
#define AECM_FLOW_HD __host__ __device__ __forceinline__
#else
#define AECM_FLOW_HD inline
#endif

// Every data-dependent decision of the Flow* functions below carries a marker, AECM_FLOW_MARK(id, outcome) -- in the style of
// AECM_LEAN_COUNT (aecm_wave.h).  It expands to nothing in every build but the coverage harness (tests/sim/sim_flowcov.cpp defines
// it before including this header), which records (decision, outcome) per tick and session: tools/flow_coverage.py computes from
// that record whether two sessions of one wavefront of a planning kernel ever disagreed on a decision within one launch, which
// branch counters cannot say.  AECM_FLOW_MARK_IF(guard, ...) marks a decision that is only evaluated under `guard` (the second
// operand of a || or &&).  The outcome expressions repeat the conditions next to them and have no side effects.
#ifndef AECM_FLOW_MARK
#define AECM_FLOW_MARK(id, outcome) ((void)0)
#define AECM_FLOW_MARK_IF(guard, id, outcome) ((void)0)
#endif
#define AECM_FLOW_DECISIONS(X) \
    X(MRP_BY_READABLE) X(MRP_BY_FREE) X(DC_FIRES) X(DC_NADD_FLOOR) X(DC_NADD_CEILING) X(FC_STARTUP) X(FC_TRUNCATED) X(FC_NOTHING_FITS) \
    X(BB_OFFERED_FITS) X(BB_IN_ROW) X(BB_AGED) X(EB_SHORT) X(EB_ACC_NOT_POSITIVE) X(EB_DIFF_HIGH) X(EB_HIGH_LAST_LOW) X(EB_DIFF_LOW) \
    X(EB_KNOWN_POSITIVE) X(EB_LOW_LAST_HIGH) X(EB_CHANGE) X(EB_KNOWN_FLOOR) X(SU_CHECKING) X(SU_COUNTER_ZERO) X(SU_D_NEGATIVE) X(SU_TOL_ABS) \
    X(SU_TOL_REL) X(SU_COUNTER_LIMIT) X(SU_CLAMP_MEAN) X(SU_CTR_LIMIT) X(SU_CLAMP_LAST) X(SU_CHECKED) X(SU_FILLED_EQ) X(SU_FILLED_GT) \
    X(RS_LAGGING) X(MN_SAME_PLACE) X(MN_BACKWARDS) X(LS_WAVE_BEFORE) X(T_FS16) X(T_SPLIT_FLAG) X(T_SPLIT_N) X(T_SPILL_IN_ROW) X(T_SPILL_AGED) \
    X(T_MS_NEGATIVE) X(T_MS_HIGH) X(T_NO_SECOND_CALL) X(T_NO_FAREND) X(T_STARTUP) X(T_NO_SECOND_FRAME) X(T_FRESH) X(T_REPLAY_IN_RING) X(T_EST) \
    X(T_FROM_STREAM) X(T_NEW_RUN) X(T_TWO_BLOCKS) X(T_STUFF) X(T_SPILL_SET) X(T_SPILL_NOT_REFRESHED) X(T_ACTIVE0) X(T_ACTIVE1) X(T_DIRECT) \
    X(T_FF_WAS_DIRECT) X(T_LEFT_PENDING) X(TM_HALF_FLAG) X(TM_HALF_N) X(PK_HALF_FLAG) X(PK_HALF_N) X(K_LIVE) X(K_RESYNC)
#define AECM_FLOW_DECISION_ENUM(name) FD_##name,
namespace aecm {
enum FlowDecision : int { AECM_FLOW_DECISIONS(AECM_FLOW_DECISION_ENUM) kFlowDecisions };   // K_*: decisions of the planning kernels' own text
}

namespace aecm {

// One session's wrapper state: kFlowFieldsUsed int32, stored field-major on the device (state[field * S + session],
// SessionBatch::flow_state_).
enum FlowField : int {
    F_BUF_SIZE_START = 0,       // AecMobile::bufSizeStart            echo_control_mobile.cc:42-79
    F_KNOWN_DELAY,              // knownDelay
    F_COUNTER,                  // counter
    F_SUM,                      // sum
    F_FIRST_VAL,                // firstVal
    F_CHECK_BUF_SIZE_CTR,       // checkBufSizeCtr
    F_MS,                       // msInSndCardBuf (after the +10 of :266)
    F_FILT_DELAY,               // filtDelay
    F_TIME_FOR_DELAY_CHANGE,    // timeForDelayChange
    F_EC_STARTUP,               // ECstartup
    F_CHECK_BUFF_SIZE,          // checkBuffSize
    F_DELAY_CHANGE,             // delayChange
    F_LAST_DELAY_DIFF,          // lastDelayDiff
    F_FAR_RP,                   // far stream: samples the jitter buffer has handed out (its read pointer; moves both ways)
    F_FAR_WP,                   // far stream: samples the jitter buffer has accepted
    F_FRM_POS,                  // frame stream: samples written into the frame rings (far and near alike)
    F_BLK_POS,                  // frame stream: samples consumed as blocks = 64 * blocks processed = output stream written
    F_OUT_RP,                   // output stream: read pointer of the output frame ring (moves back when stuffing)
    F_RUN_POS,                  // frame stream: from this position on the framed far end is ONE run of the far stream ...
    F_RUN_DELTA,                // ... namely frame-stream position x = far-stream position x + F_RUN_DELTA
    F_FF_VALID,                 // the framed-far ring holds the pending frame-stream samples [F_BLK_POS, F_FRM_POS)
    F_OLD_POS0, F_OLD_POS1,     // farendOld[i] (the frame replayed on an underrun) = far stream [F_OLD_POS_i, + 80) ...
    F_OLD_ROW0, F_OLD_ROW1,     // ... unless 1: it has been copied to replay row i (initially: the zeroed row)
    F_NEAR_LAG,                 // near-end samples the OBJECT has ticked since this session last did (idle ticks, below); 0: in step
    kFlowFieldsUsed,
    kFlowTickFields = F_NEAR_LAG,   // what FlowTick reads and writes: a tick of sessions that are all in step leaves the lag alone
    kFlowWords = 32
};

constexpr int kFlowFrame = 80;                      // FRAME_LEN
constexpr int kFlowBlock = 64;                      // PART_LEN
constexpr int kFlowJitterCapacity = 50 * 80;        // kBufSizeSamp = BUF_SIZE_FRAMES * FRAME_LEN (:29-36)
constexpr int kFlowFarFrameRing = 256;              // ring of the framed far stream on the device (>= 143 + 80, power of two)
constexpr int kFlowNoFarend = 1, kFlowSplitCalls = 2;   // = SessionBatch::kNoFarend / kSplitCalls
constexpr int kFlowIdle = 4;                        // = SessionBatch::kIdle: the session makes no call at all in this tick (FlowIdleTick)
constexpr int kFlowHalfCall = 8;                    // = SessionBatch::kHalfCall: one call pair of 80 samples in a 160-sample tick (FlowTickMixed)
constexpr int kFlowFarRing = 8192;                  // far ring of the device: positions older than this many accepted samples are gone
constexpr int kFlowOldAge = kFlowFarRing - 5 * kFlowFrame;   // a replay frame this far behind the write position moves to its row

// The near-end rings are indexed by the OBJECT's tick position.  A session that sits out ticks falls behind it by
// F_NEAR_LAG samples: a multiple of 80 (ticks are 80 or 160 samples), kept modulo kFlowLagPeriod = lcm(80, ring length) --
// only the lag modulo the ring length places anything, and 2^32 is no multiple of 80, so a free-running counter would
// stop being a multiple of 80 after 74 hours of 10 ms ticks.
constexpr int kFlowLagPeriod = 5 * kFlowFarRing;    // 40 960 = lcm(80, 8 192)
static_assert(kFlowLagPeriod % 80 == 0 && kFlowLagPeriod % kFlowFarRing == 0, "lag period");

struct FlowFarPiece {          // far_in[src, src + count) -> far stream positions [pos, pos + count)
    int32_t src, count;
    uint32_t pos;
};
struct FlowFrame {             // one 80-sample frame of the tick (input samples [80 f, 80 f + 80))
    int32_t active;            // 0: its call was served by the start-up copy (out = clean or noisy near-end, :285-291)
    int32_t far_from_stream;   // 1: far frame = far stream [far_pos, far_pos + 80) (a fresh frame, or the replay of one that is
                               // still in the far ring); 0: replay row old_idx
    uint32_t far_pos;
    int32_t old_idx;
    uint32_t frm_pos;          // where the frame lands in the frame stream
    int32_t n_blocks;          // blocks this frame completes
    uint32_t out_pos;          // output stream position of this frame's 80 output samples
};
struct FlowPlan {
    FlowFarPiece far[2];       // per call
    FlowFrame frame[2];
    int32_t n_calls, n_frames, n_blocks;
    uint32_t blk_pos0;         // frame-stream / output-stream position of the tick's first block
    uint32_t near_base;        // frame-stream position x of the near end sits at near-ring position near_base + x
    // direct: every far sample the tick's blocks consume belongs to one run of the far stream (no replay, re-read or skip
    // since the oldest of them was framed): block sample x is far-stream sample x + far_delta, the blocks fetch from the
    // far ring itself and nothing is framed.  Otherwise the tick's frames go through the framed-far ring, preceded --
    // when the previous ticks were direct -- by the left_count pending samples [blk_pos0, ..) = far stream + left_delta.
    int32_t direct;
    uint32_t far_delta;
    int32_t left_count;
    uint32_t left_delta;
    int32_t spill[2];          // replay frame i is about to leave the far ring: far stream [spill_pos[i], + 80) -> replay row i
    uint32_t spill_pos[2];
};

struct FlowRegs {              // FlowField values in registers
    int32_t v[kFlowFieldsUsed];
};

AECM_FLOW_HD int32_t FlowAsShort(int32_t x) { return (int32_t)(int16_t)x; }
AECM_FLOW_HD int32_t FlowMin(int32_t a, int32_t b) { return a < b ? a : b; }
AECM_FLOW_HD int32_t FlowMax(int32_t a, int32_t b) { return a > b ? a : b; }

// State after WebRtcAecm_Init (echo_control_mobile.cc:142-191): everything 0 except the three start-up flags (and the
// flags that say where the device keeps things).
AECM_FLOW_HD bool FlowFieldStartsAtOne(int f) {
    return f == F_DELAY_CHANGE || f == F_CHECK_BUFF_SIZE || f == F_EC_STARTUP || f == F_FF_VALID || f == F_OLD_ROW0 || f == F_OLD_ROW1;
}
AECM_FLOW_HD void FlowInit(int32_t words[kFlowWords]) {
    for (int i = 0; i < kFlowWords; ++i) words[i] = i < kFlowFieldsUsed && FlowFieldStartsAtOne(i) ? 1 : 0;
}

// Is this wrapper state one FlowTick and the tick kernel may run on (WebRtcAecmSessions_ImportSession)?  Everything they
// turn into a loop count, a lane count or a 4-bit field of the plan: the pending frame-stream samples (< one block: the block
// loop of a frame and the plan's left_count), the jitter buffer's fill, the output ring's fill, the flags; and everything
// that names far-ring samples a later tick will read (replay frames, pending samples of direct ticks) must name samples the
// ring still holds.  Positions themselves are free-running counters: any value is a position.  tests/sim/sim_flow.cpp checks
// that every state a session passes through is accepted.  Returns 0 or the 1-based index of the offending field.
AECM_FLOW_HD int FlowStateDefect(const int32_t v[kFlowWords]) {
    for (int f : {F_EC_STARTUP, F_CHECK_BUFF_SIZE, F_DELAY_CHANGE, F_FF_VALID, F_OLD_ROW0, F_OLD_ROW1})
        if (v[f] != 0 && v[f] != 1) return f + 1;
    if (v[F_BUF_SIZE_START] < 0 || v[F_BUF_SIZE_START] > 50) return F_BUF_SIZE_START + 1;          // BUF_SIZE_FRAMES (:29-36, :322,:332)
    if (v[F_MS] < 0 || v[F_MS] > 510) return F_MS + 1;                                                // clamped to [0, 500], + 10 (:258-266)
    for (int f : {F_KNOWN_DELAY, F_COUNTER, F_SUM, F_FIRST_VAL, F_CHECK_BUF_SIZE_CTR, F_FILT_DELAY, F_LAST_DELAY_DIFF})
        if (v[f] < -32768 || v[f] > 32767) return f + 1;                                              // the reference's short members
    const uint32_t readable = (uint32_t)v[F_FAR_WP] - (uint32_t)v[F_FAR_RP];
    if (readable > (uint32_t)kFlowJitterCapacity) return F_FAR_RP + 1;
    const uint32_t pending = (uint32_t)v[F_FRM_POS] - (uint32_t)v[F_BLK_POS];
    if (pending >= (uint32_t)kFlowBlock) return F_BLK_POS + 1;
    const uint32_t out_fill = (uint32_t)v[F_BLK_POS] - (uint32_t)v[F_OUT_RP];
    if (out_fill > (uint32_t)(kFlowFrame + kFlowBlock)) return F_OUT_RP + 1;                          // the output frame ring holds FRAME_LEN + PART_LEN (aecm_core.cc:204-205)
    // A replay frame that still lives in the far ring only has not been lapped there: FlowTick / FlowBurstBegin move it to
    // its row before the write position gets further than kFlowOldAge + one tick ahead of it.
    for (int i = 0; i < 2; ++i)
        if (!v[F_OLD_ROW0 + i] && (uint32_t)v[F_FAR_WP] - (uint32_t)v[F_OLD_POS0 + i] > (uint32_t)(kFlowOldAge + 2 * kFlowFrame)) return F_OLD_POS0 + i + 1;
    // Pending samples that were left in the far ring by direct ticks (F_FF_VALID == 0) are one run of the far stream that
    // ends before the jitter buffer's read pointer and is as young as anything the jitter buffer can still hand out
    // (the read pointer never falls back by more than the buffer's capacity; a frame and the pending samples lie before it).
    if (!v[F_FF_VALID]) {
        const uint32_t behind = (uint32_t)v[F_FAR_WP] - ((uint32_t)v[F_BLK_POS] + (uint32_t)v[F_RUN_DELTA]);    // write position - far position of the first pending sample
        if (behind < pending || behind > (uint32_t)(kFlowJitterCapacity + 2 * kFlowFrame + kFlowBlock)) return F_RUN_DELTA + 1;
        if ((uint32_t)v[F_BLK_POS] - (uint32_t)v[F_RUN_POS] > (uint32_t)(4 * kFlowBlock)) return F_RUN_POS + 1;  // FlowTick keeps it at the last tick's first block
    }
    if (v[F_NEAR_LAG] < 0 || v[F_NEAR_LAG] >= kFlowLagPeriod || v[F_NEAR_LAG] % kFlowFrame != 0) return F_NEAR_LAG + 1;   // whole ticks
    for (int f = kFlowFieldsUsed; f < kFlowWords; ++f)
        if (v[f] != 0) return f + 1;
    return 0;
}

// WebRtc_MoveReadPtr of the jitter buffer (ring_buffer.c:176-211): clamped to what is readable / free.
AECM_FLOW_HD void FlowMoveFarReadPtr(FlowRegs &s, int32_t n) {
    const int32_t readable = (int32_t)((uint32_t)s.v[F_FAR_WP] - (uint32_t)s.v[F_FAR_RP]);
    const int32_t free_elems = kFlowJitterCapacity - readable;
    AECM_FLOW_MARK(FD_MRP_BY_READABLE, n > readable);
    n = FlowMin(n, readable);
    AECM_FLOW_MARK(FD_MRP_BY_FREE, n < -free_elems);
    n = FlowMax(n, -free_elems);
    s.v[F_FAR_RP] = (int32_t)((uint32_t)s.v[F_FAR_RP] + (uint32_t)n);
}

// WebRtcAecm_DelayComp (:575-594).
AECM_FLOW_HD void FlowDelayComp(FlowRegs &s, int mult) {
    const int32_t n_samp_far = (int32_t)((uint32_t)s.v[F_FAR_WP] - (uint32_t)s.v[F_FAR_RP]);
    const int32_t n_samp_snd_card = s.v[F_MS] * 8 * mult;
    const int32_t delay_new = n_samp_snd_card - n_samp_far;
    AECM_FLOW_MARK(FD_DC_FIRES, delay_new > 256 - kFlowFrame * mult);
    if (delay_new > 256 - kFlowFrame * mult) {
        AECM_FLOW_MARK(FD_DC_NADD_FLOOR, (n_samp_snd_card >> 1) - n_samp_far < kFlowFrame);
        int32_t n_add = FlowMax((n_samp_snd_card >> 1) - n_samp_far, kFlowFrame);
        AECM_FLOW_MARK(FD_DC_NADD_CEILING, n_add > 10 * kFlowFrame);
        n_add = FlowMin(n_add, 10 * kFlowFrame);
        FlowMoveFarReadPtr(s, -n_add);
        s.v[F_DELAY_CHANGE] = 1;
    }
}

// One WebRtcAecm_BufferFarend call of len samples (:215-234): delay compensation once the start-up phase is over, then
// the jitter buffer takes what fits -- a full buffer drops the rest (ring_buffer.c:142-150).  Returns the number of
// samples accepted; they land at far-stream positions [F_FAR_WP before the call, + accepted).
AECM_FLOW_HD int32_t FlowFarendCall(FlowRegs &s, int mult, int len) {
    AECM_FLOW_MARK(FD_FC_STARTUP, s.v[F_EC_STARTUP] != 0);
    if (!s.v[F_EC_STARTUP]) FlowDelayComp(s, mult);
    const int32_t readable = (int32_t)((uint32_t)s.v[F_FAR_WP] - (uint32_t)s.v[F_FAR_RP]);
    AECM_FLOW_MARK(FD_FC_TRUNCATED, len > kFlowJitterCapacity - readable);
    AECM_FLOW_MARK(FD_FC_NOTHING_FITS, readable == kFlowJitterCapacity);
    const int32_t accepted = FlowMin(len, kFlowJitterCapacity - readable);
    s.v[F_FAR_WP] = (int32_t)((uint32_t)s.v[F_FAR_WP] + (uint32_t)accepted);
    return accepted;
}

// WebRtcAecm_BufferFarend calls that come WITHOUT a WebRtcAecm_Process (a far-end burst: the network delivered several
// frames between two ticks; WebRtcAecmSessions_BufferFarend).  Each is FlowFarendCall; the only other thing a burst has to
// mind is the far ring of the device, which is longer than the jitter buffer but finite: a replay frame that lives in the
// ring only (F_OLD_ROWi == 0) moves to its row before the burst's samples can lap it.  FlowBurstBegin decides that from
// an upper bound of what `calls` calls of `len` samples can add (what is free now: delay compensation only ever makes
// the buffer fuller), so the copy can be made before the first sample of the burst is written; a row taking over a
// little early reads the same samples.  The wrapper fields a burst reads / writes: FlowBurstReads / FlowBurstWrites.
struct FlowBurst {
    int32_t spill[2];
    uint32_t spill_pos[2];
};
AECM_FLOW_HD void FlowBurstBegin(FlowRegs &s, int len, int calls, FlowBurst &b) {
    const int32_t readable = (int32_t)((uint32_t)s.v[F_FAR_WP] - (uint32_t)s.v[F_FAR_RP]);
    const int64_t offered = (int64_t)len * calls;
    AECM_FLOW_MARK(FD_BB_OFFERED_FITS, offered < (int64_t)(kFlowJitterCapacity - readable));
    const int32_t most = (int32_t)(offered < (int64_t)(kFlowJitterCapacity - readable) ? offered : (int64_t)(kFlowJitterCapacity - readable));
    for (int i = 0; i < 2; ++i) {
        b.spill_pos[i] = (uint32_t)s.v[F_OLD_POS0 + i];
        AECM_FLOW_MARK(FD_BB_IN_ROW, s.v[F_OLD_ROW0 + i] != 0);
        AECM_FLOW_MARK_IF(!s.v[F_OLD_ROW0 + i], FD_BB_AGED, (int32_t)((uint32_t)s.v[F_FAR_WP] + (uint32_t)most - (uint32_t)s.v[F_OLD_POS0 + i]) > kFlowOldAge);
        b.spill[i] = !s.v[F_OLD_ROW0 + i] && (int32_t)((uint32_t)s.v[F_FAR_WP] + (uint32_t)most - (uint32_t)s.v[F_OLD_POS0 + i]) > kFlowOldAge;
        if (b.spill[i]) s.v[F_OLD_ROW0 + i] = 1;
    }
}
template <class Fn>
AECM_FLOW_HD void FlowBurstReads(Fn &&fn) {
    for (int f : {F_FAR_RP, F_FAR_WP, F_MS, F_EC_STARTUP, F_DELAY_CHANGE, F_OLD_POS0, F_OLD_POS1, F_OLD_ROW0, F_OLD_ROW1}) fn(f);
}
template <class Fn>
AECM_FLOW_HD void FlowBurstWrites(Fn &&fn) {
    for (int f : {F_FAR_RP, F_FAR_WP, F_DELAY_CHANGE, F_OLD_ROW0, F_OLD_ROW1}) fn(f);
}

// WebRtcAecm_EstBufDelay (:534-573).
AECM_FLOW_HD void FlowEstBufDelay(FlowRegs &s, int mult) {
    const int32_t n_samp_far = FlowAsShort((int32_t)((uint32_t)s.v[F_FAR_WP] - (uint32_t)s.v[F_FAR_RP]));
    const int32_t n_samp_snd_card = FlowAsShort(s.v[F_MS] * 8 * mult);
    int32_t delay_new = FlowAsShort(n_samp_snd_card - n_samp_far);
    AECM_FLOW_MARK(FD_EB_SHORT, delay_new < kFlowFrame);
    if (delay_new < kFlowFrame) {
        FlowMoveFarReadPtr(s, kFlowFrame);
        delay_new = FlowAsShort(delay_new + kFlowFrame);
    }
    const int32_t acc = 8 * s.v[F_FILT_DELAY] + 2 * delay_new;            // C division truncates towards zero; negative -> max(0, .) = 0
    AECM_FLOW_MARK(FD_EB_ACC_NOT_POSITIVE, acc <= 0);
    s.v[F_FILT_DELAY] = FlowAsShort(acc <= 0 ? 0 : (int32_t)((uint32_t)acc / 10u));
    const int32_t diff = FlowAsShort(s.v[F_FILT_DELAY] - s.v[F_KNOWN_DELAY]);
    AECM_FLOW_MARK(FD_EB_DIFF_HIGH, diff > 224);
    AECM_FLOW_MARK_IF(diff > 224, FD_EB_HIGH_LAST_LOW, s.v[F_LAST_DELAY_DIFF] < 96);
    AECM_FLOW_MARK_IF(!(diff > 224), FD_EB_DIFF_LOW, diff < 96);
    AECM_FLOW_MARK_IF(!(diff > 224) && diff < 96, FD_EB_KNOWN_POSITIVE, s.v[F_KNOWN_DELAY] > 0);
    AECM_FLOW_MARK_IF(!(diff > 224) && diff < 96 && s.v[F_KNOWN_DELAY] > 0, FD_EB_LOW_LAST_HIGH, s.v[F_LAST_DELAY_DIFF] > 224);
    if (diff > 224) {
        s.v[F_TIME_FOR_DELAY_CHANGE] = s.v[F_LAST_DELAY_DIFF] < 96 ? 0 : s.v[F_TIME_FOR_DELAY_CHANGE] + 1;
    } else if (diff < 96 && s.v[F_KNOWN_DELAY] > 0) {
        s.v[F_TIME_FOR_DELAY_CHANGE] = s.v[F_LAST_DELAY_DIFF] > 224 ? 0 : s.v[F_TIME_FOR_DELAY_CHANGE] + 1;
    } else {
        s.v[F_TIME_FOR_DELAY_CHANGE] = 0;
    }
    s.v[F_LAST_DELAY_DIFF] = diff;
    AECM_FLOW_MARK(FD_EB_CHANGE, s.v[F_TIME_FOR_DELAY_CHANGE] > 25);
    AECM_FLOW_MARK_IF(s.v[F_TIME_FOR_DELAY_CHANGE] > 25, FD_EB_KNOWN_FLOOR, s.v[F_FILT_DELAY] - 160 < 0);
    if (s.v[F_TIME_FOR_DELAY_CHANGE] > 25) s.v[F_KNOWN_DELAY] = FlowMax(s.v[F_FILT_DELAY] - 160, 0);
}

// The start-up phase of WebRtcAecm_Process (:285-356), n_frames 80-sample frames in this call.
AECM_FLOW_HD void FlowStartup(FlowRegs &s, int mult, int n_frames) {
    const int32_t n_blocks_10ms = n_frames / mult;
    const int32_t avail = (int32_t)((uint32_t)s.v[F_FAR_WP] - (uint32_t)s.v[F_FAR_RP]);
    const int32_t filled = FlowAsShort(FlowAsShort(avail) / kFlowFrame);
    const int32_t ms = s.v[F_MS];
    AECM_FLOW_MARK(FD_SU_CHECKING, s.v[F_CHECK_BUFF_SIZE] != 0);
    if (s.v[F_CHECK_BUFF_SIZE]) {
        s.v[F_CHECK_BUF_SIZE_CTR] = FlowAsShort(s.v[F_CHECK_BUF_SIZE_CTR] + 1);
        AECM_FLOW_MARK(FD_SU_COUNTER_ZERO, s.v[F_COUNTER] == 0);
        if (s.v[F_COUNTER] == 0) {
            s.v[F_FIRST_VAL] = ms;
            s.v[F_SUM] = 0;
        }
        // |firstVal - ms| < max(0.2 * ms, 8.0) in doubles (:310-312): 0.2 * ms rounds to ms / 5 exactly whenever that is an
        // integer (ms <= 510), so the comparison with an integer is d < 8 || 5 d < ms.
        int32_t d = s.v[F_FIRST_VAL] - ms;
        AECM_FLOW_MARK(FD_SU_D_NEGATIVE, d < 0);
        d = d < 0 ? -d : d;
        AECM_FLOW_MARK(FD_SU_TOL_ABS, d < 8);
        AECM_FLOW_MARK_IF(!(d < 8), FD_SU_TOL_REL, 5 * d < ms);
        if (d < 8 || 5 * d < ms) {
            s.v[F_SUM] = FlowAsShort(s.v[F_SUM] + ms);
            s.v[F_COUNTER] = FlowAsShort(s.v[F_COUNTER] + 1);
        } else {
            s.v[F_COUNTER] = 0;
        }
        // Both comparisons are made in size_t in the reference (short counter * size_t nBlocks10ms, :320,:330): a counter
        // that has wrapped negative -- more than 32 767 start-up calls of 80 samples at 16 kHz, where nBlocks10ms is 0 and
        // neither limit can fire -- is a huge unsigned product there.
        AECM_FLOW_MARK(FD_SU_COUNTER_LIMIT, (uint64_t)(int64_t)s.v[F_COUNTER] * (uint64_t)n_blocks_10ms >= 6u);
        if ((uint64_t)(int64_t)s.v[F_COUNTER] * (uint64_t)n_blocks_10ms >= 6u) {
            AECM_FLOW_MARK(FD_SU_CLAMP_MEAN, (3 * s.v[F_SUM] * mult) / (s.v[F_COUNTER] * 40) > 50);
            s.v[F_BUF_SIZE_START] = FlowAsShort(FlowMin((3 * s.v[F_SUM] * mult) / (s.v[F_COUNTER] * 40), 50));
            s.v[F_CHECK_BUFF_SIZE] = 0;
        }
        AECM_FLOW_MARK(FD_SU_CTR_LIMIT, (uint64_t)(int64_t)s.v[F_CHECK_BUF_SIZE_CTR] * (uint64_t)n_blocks_10ms > 50u);
        if ((uint64_t)(int64_t)s.v[F_CHECK_BUF_SIZE_CTR] * (uint64_t)n_blocks_10ms > 50u) {
            AECM_FLOW_MARK(FD_SU_CLAMP_LAST, (3 * ms * mult) / 40 > 50);
            s.v[F_BUF_SIZE_START] = FlowAsShort(FlowMin((3 * ms * mult) / 40, 50));
            s.v[F_CHECK_BUFF_SIZE] = 0;
        }
    }
    AECM_FLOW_MARK(FD_SU_CHECKED, !s.v[F_CHECK_BUFF_SIZE]);
    AECM_FLOW_MARK_IF(!s.v[F_CHECK_BUFF_SIZE], FD_SU_FILLED_EQ, filled == s.v[F_BUF_SIZE_START]);
    AECM_FLOW_MARK_IF(!s.v[F_CHECK_BUFF_SIZE] && filled != s.v[F_BUF_SIZE_START], FD_SU_FILLED_GT, filled > s.v[F_BUF_SIZE_START]);
    if (!s.v[F_CHECK_BUFF_SIZE]) {
        if (filled == s.v[F_BUF_SIZE_START]) {
            s.v[F_EC_STARTUP] = 0;
        } else if (filled > s.v[F_BUF_SIZE_START]) {
            FlowMoveFarReadPtr(s, avail - s.v[F_BUF_SIZE_START] * kFlowFrame);
            s.v[F_EC_STARTUP] = 0;
        }
    }
}

// A tick the session sits out (kFlowIdle): no WebRtcAecm_BufferFarend, no WebRtcAecm_Process -- the reference instance is
// simply not called, so nothing of its state moves and what is pending stays pending.  On the device the session's rings
// are not written either (they are per session: however long the stretch, nothing is lost); all that happens is that the
// object's near position runs ahead of the session by another n samples.
AECM_FLOW_HD int32_t FlowIdleTick(int32_t lag, int n) { return (int32_t)(((uint32_t)lag + (uint32_t)n) % (uint32_t)kFlowLagPeriod); }

// The first tick a session makes after idle ticks brings it back in step BEFORE FlowTick runs: the only near-end (and clean)
// samples a later block can still ask for are the pending ones, fewer than one block, [F_BLK_POS, F_FRM_POS) of the frame
// stream; they sit just behind the session's own position near_pos - lag and move to just behind near_pos, where the tick's
// samples continue them.  From then on the session is indistinguishable from one that never idled: FlowTick, the plan and
// the tick kernel know nothing of lags.  (A session in its start-up phase has framed nothing: nothing moves.)
struct FlowNearMove {          // near ring (and clean ring) positions [src, src + count) -> [dst, dst + count), count < 64
    int32_t count;
    uint32_t src, dst;
};
AECM_FLOW_HD void FlowResync(FlowRegs &s, uint32_t near_pos, FlowNearMove &m) {
    const uint32_t pending = (uint32_t)s.v[F_FRM_POS] - (uint32_t)s.v[F_BLK_POS];
    AECM_FLOW_MARK(FD_RS_LAGGING, s.v[F_NEAR_LAG] != 0);
    m.count = s.v[F_NEAR_LAG] != 0 ? (int32_t)pending : 0;
    m.dst = near_pos - pending;
    m.src = m.dst - (uint32_t)s.v[F_NEAR_LAG];
    s.v[F_NEAR_LAG] = 0;
}
// The move itself, sample by sample in the order that is right for ranges that overlap in the ring (a lag of 8 240 is a
// ring distance of 48): the destination lies d = (dst - src) mod ring ahead of the source; with d < count the copy runs
// backwards, otherwise forwards (then the destination is either clear of the source or behind it).
template <class T>
AECM_FLOW_HD void FlowMoveNear(T *ring, uint32_t mask, const FlowNearMove &m) {
    const uint32_t d = (m.dst - m.src) & mask;
    AECM_FLOW_MARK(FD_MN_SAME_PLACE, d == 0);
    if (d == 0) return;
    AECM_FLOW_MARK(FD_MN_BACKWARDS, d < (uint32_t)m.count);
    if (d < (uint32_t)m.count) {
        for (int32_t k = m.count - 1; k >= 0; --k) ring[(m.dst + (uint32_t)k) & mask] = ring[(m.src + (uint32_t)k) & mask];
    } else {
        for (int32_t k = 0; k < m.count; ++k) ring[(m.dst + (uint32_t)k) & mask] = ring[(m.src + (uint32_t)k) & mask];
    }
}

// Which launches a tick of an OBJECT takes (SessionBatch::Enqueue; tests/sim/sim_sparse.cpp drives this very function).
// The object keeps two things about lags: may_lag -- some session may be behind the object's near position (a session sat
// out a tick since the last tick everybody made) -- and deferred_lag, the samples of ticks NOBODY made: those launch nothing,
// so the sessions learn of them from the next planning launch, which adds deferred_lag to every session's lag first.
//   launch == false  nobody calls: nothing is launched, the object's position moves on
//   sparse_plan      the planning launch is the one that knows lags and idle lanes (aecm_flow_plan_sparse_kernel); it is
//                    handed deferred_lag.  false: every session calls and every session is in step -- the launches of an
//                    object that knows no idle sessions
//   sparse_tick      the tick launch runs by the live list (somebody sits out, or the diagnostics switch); else the dense
//                    tick kernel over everybody
struct FlowObjectLag {
    int32_t deferred_lag = 0;
    bool may_lag = false;
};
struct FlowTickRoute {
    bool launch, sparse_plan, sparse_tick;
    int32_t deferred_lag;       // what the planning launch adds to every lag (sparse_plan)
};
inline FlowTickRoute FlowRouteTick(FlowObjectLag &o, int32_t live, int32_t n_sessions, int n, bool force_sparse) {
    FlowTickRoute r{live > 0, false, false, 0};
    if (!r.launch) {
        o.deferred_lag = FlowIdleTick(o.deferred_lag, n);
        o.may_lag = true;
        return r;
    }
    r.sparse_tick = live < n_sessions || force_sparse;
    r.sparse_plan = r.sparse_tick || o.may_lag;
    if (r.sparse_plan) {
        r.deferred_lag = o.deferred_lag;
        o.deferred_lag = 0;
        o.may_lag = live < n_sessions;        // everybody called: everybody is in step again
    }
    return r;
}

// The same decision for an object that knows half calls (kFlowHalfCall) and sessions of another rate than its own.  Without
// either -- half_calls: some session that calls in this tick makes a half call; other_rates: the object holds a session of
// another rate -- it IS FlowRouteTick, and *mixed_plan is false: the launches of an object that knows neither.  Otherwise the
// planning launch is the one that knows per-session rates, call sizes and lags (aecm_flow_plan_mixed_kernel; it does all the
// sparse planning kernel does, so sparse_plan is true and it is handed deferred_lag), and a half call leaves its session 80
// samples behind the object's near position: the object is out of step whoever else called.
inline FlowTickRoute FlowRouteTickMixed(FlowObjectLag &o, int32_t live, int32_t n_sessions, int n, bool force_sparse, bool half_calls,
                                        bool other_rates, bool *mixed_plan) {
    FlowTickRoute r = FlowRouteTick(o, live, n_sessions, n, force_sparse);
    *mixed_plan = r.launch && (half_calls || other_rates);
    if (*mixed_plan) {
        if (!r.sparse_plan) {                     // (everybody calls, everybody in step: nothing was deferred)
            r.sparse_plan = true;
            r.deferred_lag = o.deferred_lag;
            o.deferred_lag = 0;
        }
        if (half_calls) o.may_lag = true;
    }
    return r;
}

// The live list of a tick in which sessions idle: the ids of the sessions that do call, ascending, so that wavefront w of
// the tick kernel serves session live[w].  Built without atomics, in two halves.  The host half, in the pass over the flags
// the host makes anyway: bases[b] = live sessions among the first kFlowPlanBlock * b, returns the live count.  The device
// half, in the planning kernel (kFlowPlanBlock lanes per workgroup, one per session): a live lane's slot is its workgroup's
// base + the live lanes of the wavefronts before it in the workgroup + the live lanes before it in its wavefront.
constexpr int kFlowPlanBlock = 256;
inline int32_t FlowLiveBlockBases(const uint8_t *flags, int32_t n_sessions, uint32_t *bases) {
    int32_t live = 0;
    for (int32_t first = 0, b = 0; first < n_sessions; first += kFlowPlanBlock, ++b) {
        bases[b] = (uint32_t)live;
        const int32_t end = first + kFlowPlanBlock < n_sessions ? first + kFlowPlanBlock : n_sessions;
        int32_t idle = 0;
        for (int32_t s = first; s < end; ++s) idle += (flags[s] >> 2) & 1;
        live += (end - first) - idle;
    }
    return live;
}
static_assert(kFlowIdle == 4, "FlowLiveBlockBases counts bit 2");
// wave_counts[w] = live lanes of wavefront w of the workgroup, ballot = the live lanes of this lane's wavefront.
AECM_FLOW_HD uint32_t FlowLiveSlot(uint32_t block_base, const uint32_t wave_counts[kFlowPlanBlock / 64], int wave, uint64_t ballot, int lane) {
    uint32_t slot = block_base;
    for (int w = 0; w < kFlowPlanBlock / 64; ++w) {
        AECM_FLOW_MARK(FD_LS_WAVE_BEFORE, w < wave);
        slot += w < wave ? wave_counts[w] : 0u;
    }
    const uint64_t below = ballot & ((uint64_t(1) << lane) - 1u);
    return slot + (uint32_t)__builtin_popcountll(below);
}

// One tick: [WebRtcAecm_BufferFarend] + WebRtcAecm_Process of n samples (80 or 160), or two such pairs of 80 samples
// (kFlowSplitCalls, n = 160).  ms = the caller's msInSndCardBuf, near_pos = near-ring position of the tick's first
// near-end sample.  Advances s and fills the plan.  The session is in step (F_NEAR_LAG == 0; FlowResync first otherwise).
AECM_FLOW_HD void FlowTick(FlowRegs &s, int fs, int n, int ms, int flags, uint32_t near_pos, FlowPlan &p) {
    AECM_FLOW_MARK(FD_T_FS16, fs == 16000);
    const int mult = fs == 16000 ? 2 : 1;
    AECM_FLOW_MARK(FD_T_SPLIT_FLAG, (flags & kFlowSplitCalls) != 0);
    AECM_FLOW_MARK_IF((flags & kFlowSplitCalls) != 0, FD_T_SPLIT_N, n == 2 * kFlowFrame);
    const bool split = (flags & kFlowSplitCalls) != 0 && n == 2 * kFlowFrame;
    const int n_calls = split ? 2 : 1;
    const int len = split ? kFlowFrame : n;
    const int frames_per_call = len / kFlowFrame;
    p.n_calls = n_calls;
    p.n_frames = n / kFlowFrame;
    p.n_blocks = 0;
    p.blk_pos0 = (uint32_t)s.v[F_BLK_POS];
    p.near_base = 0;
    p.direct = 0;
    p.far_delta = p.left_delta = 0;
    p.left_count = 0;
    const uint32_t frm_start = (uint32_t)s.v[F_FRM_POS], run_delta_start = (uint32_t)s.v[F_RUN_DELTA];
    // A replay frame that still lives in the far ring only is copied to its row before the ring's write position laps it.
    // The row takes over from the NEXT tick on: a replay in this tick still reads the ring, so nothing in the tick depends
    // on the copy.
    int32_t refreshed[2] = {0, 0};
    for (int i = 0; i < 2; ++i) {
        p.spill_pos[i] = (uint32_t)s.v[F_OLD_POS0 + i];
        AECM_FLOW_MARK(FD_T_SPILL_IN_ROW, s.v[F_OLD_ROW0 + i] != 0);
        AECM_FLOW_MARK_IF(!s.v[F_OLD_ROW0 + i], FD_T_SPILL_AGED, (int32_t)((uint32_t)s.v[F_FAR_WP] - (uint32_t)s.v[F_OLD_POS0 + i]) > kFlowOldAge);
        p.spill[i] = !s.v[F_OLD_ROW0 + i] && (int32_t)((uint32_t)s.v[F_FAR_WP] - (uint32_t)s.v[F_OLD_POS0 + i]) > kFlowOldAge;
    }
    for (int f = 0; f < 2; ++f) p.frame[f] = FlowFrame{0, 0, 0u, 0, 0u, 0, 0u};
    for (int c = 0; c < 2; ++c) p.far[c] = FlowFarPiece{c * len, 0, (uint32_t)s.v[F_FAR_WP]};
    AECM_FLOW_MARK(FD_T_MS_NEGATIVE, ms < 0);
    AECM_FLOW_MARK_IF(!(ms < 0), FD_T_MS_HIGH, ms > 500);
    ms = ms < 0 ? 0 : ms > 500 ? 500 : ms;                                                   // :258-265 (the warning is the host's business)
    // Frame slot of frame i of call c: c * frames_per_call + i = c + i for the three shapes there are (1 x 1, 1 x 2,
    // 2 x 1); both loops have constant bounds so that the plan stays in registers on the device.
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int c = 0; c < 2; ++c) {
        AECM_FLOW_MARK_IF(c == 1, FD_T_NO_SECOND_CALL, c >= n_calls);
        if (c >= n_calls) break;
        // ---- WebRtcAecm_BufferFarend (:215-234) ----
        AECM_FLOW_MARK(FD_T_NO_FAREND, (flags & kFlowNoFarend) != 0);
        if (!(flags & kFlowNoFarend)) {
            p.far[c].pos = (uint32_t)s.v[F_FAR_WP];
            p.far[c].count = FlowFarendCall(s, mult, len);
        }
        // ---- WebRtcAecm_Process (:236-408) ----
        s.v[F_MS] = ms + 10;
        AECM_FLOW_MARK(FD_T_STARTUP, s.v[F_EC_STARTUP] != 0);
        if (s.v[F_EC_STARTUP]) {
            FlowStartup(s, mult, frames_per_call);
            continue;
        }
#if defined(__HIPCC__)
#pragma unroll
#endif
        for (int i = 0; i < 2; ++i) {
            AECM_FLOW_MARK_IF(i == 1, FD_T_NO_SECOND_FRAME, i >= frames_per_call);
            if (i >= frames_per_call) break;
            FlowFrame &fr = p.frame[(c + i) & 1];
            fr.active = 1;
            fr.old_idx = i;
            const int32_t avail = (int32_t)((uint32_t)s.v[F_FAR_WP] - (uint32_t)s.v[F_FAR_RP]);
            AECM_FLOW_MARK(FD_T_FRESH, FlowAsShort(FlowAsShort(avail) / kFlowFrame) > 0);
            AECM_FLOW_MARK_IF(!(FlowAsShort(FlowAsShort(avail) / kFlowFrame) > 0), FD_T_REPLAY_IN_RING, !s.v[F_OLD_ROW0 + i]);
            if (FlowAsShort(FlowAsShort(avail) / kFlowFrame) > 0) {                              // :369-375
                fr.far_from_stream = 1;
                fr.far_pos = (uint32_t)s.v[F_FAR_RP];
                s.v[F_OLD_POS0 + i] = (int32_t)fr.far_pos;                                       // farendOld[i] = this frame (:373)
                s.v[F_OLD_ROW0 + i] = 0;
                refreshed[i] = 1;
                s.v[F_FAR_RP] = (int32_t)((uint32_t)s.v[F_FAR_RP] + (uint32_t)kFlowFrame);
            } else if (!s.v[F_OLD_ROW0 + i]) {                                                   // :376-379: replay, still in the far ring
                fr.far_from_stream = 1;
                fr.far_pos = (uint32_t)s.v[F_OLD_POS0 + i];
            }
            AECM_FLOW_MARK(FD_T_EST, (i == 0 && fs == 8000) || (i == 1 && fs == 16000));
            if ((i == 0 && fs == 8000) || (i == 1 && fs == 16000)) FlowEstBufDelay(s, mult);   // :384-387
            // WebRtcAecm_ProcessFrame (aecm_core.cc:501-572); the core's far delay line is a pass-through (knownDelay 0)
            fr.frm_pos = (uint32_t)s.v[F_FRM_POS];
            AECM_FLOW_MARK(FD_T_FROM_STREAM, fr.far_from_stream != 0);
            AECM_FLOW_MARK_IF(fr.far_from_stream != 0, FD_T_NEW_RUN, (int32_t)(fr.far_pos - fr.frm_pos) != s.v[F_RUN_DELTA]);
            if (fr.far_from_stream) {                       // does this frame continue the run of the far stream the previous one ended?
                const int32_t delta = (int32_t)(fr.far_pos - fr.frm_pos);
                if (delta != s.v[F_RUN_DELTA]) {
                    s.v[F_RUN_DELTA] = delta;
                    s.v[F_RUN_POS] = (int32_t)fr.frm_pos;
                }
            } else {
                s.v[F_RUN_POS] = (int32_t)(fr.frm_pos + (uint32_t)kFlowFrame);   // a replay row is no part of the far stream
            }
            p.near_base = near_pos + (uint32_t)(kFlowFrame * (c + i)) - fr.frm_pos;
            s.v[F_FRM_POS] = (int32_t)(fr.frm_pos + (uint32_t)kFlowFrame);
            int nb = 0;
            while ((int32_t)((uint32_t)s.v[F_FRM_POS] - (uint32_t)s.v[F_BLK_POS]) >= kFlowBlock) {
                s.v[F_BLK_POS] = (int32_t)((uint32_t)s.v[F_BLK_POS] + (uint32_t)kFlowBlock);
                ++nb;
            }
            AECM_FLOW_MARK(FD_T_TWO_BLOCKS, nb == 2);                                            // the loop's trip count: 1 or 2
            fr.n_blocks = nb;
            p.n_blocks += nb;
            const int32_t size = (int32_t)((uint32_t)s.v[F_BLK_POS] - (uint32_t)s.v[F_OUT_RP]);
            AECM_FLOW_MARK(FD_T_STUFF, size < kFlowFrame);
            if (size < kFlowFrame) s.v[F_OUT_RP] = (int32_t)((uint32_t)s.v[F_BLK_POS] - (uint32_t)kFlowFrame);   // stuffing (:559-562)
            fr.out_pos = (uint32_t)s.v[F_OUT_RP];
            s.v[F_OUT_RP] = (int32_t)(fr.out_pos + (uint32_t)kFlowFrame);
        }
    }
    for (int i = 0; i < 2; ++i) {
        AECM_FLOW_MARK(FD_T_SPILL_SET, p.spill[i] != 0);
        AECM_FLOW_MARK_IF(p.spill[i] != 0, FD_T_SPILL_NOT_REFRESHED, !refreshed[i]);
        if (p.spill[i] && !refreshed[i]) s.v[F_OLD_ROW0 + i] = 1;
    }
    AECM_FLOW_MARK(FD_T_ACTIVE0, p.frame[0].active != 0);
    AECM_FLOW_MARK_IF(!p.frame[0].active, FD_T_ACTIVE1, p.frame[1].active != 0);
    if (p.frame[0].active || p.frame[1].active) {          // every active frame completes at least one block
        AECM_FLOW_MARK(FD_T_DIRECT, (int32_t)((uint32_t)s.v[F_RUN_POS] - p.blk_pos0) <= 0);
        AECM_FLOW_MARK_IF(!((int32_t)((uint32_t)s.v[F_RUN_POS] - p.blk_pos0) <= 0), FD_T_FF_WAS_DIRECT, !s.v[F_FF_VALID]);
        AECM_FLOW_MARK_IF(!((int32_t)((uint32_t)s.v[F_RUN_POS] - p.blk_pos0) <= 0) && !s.v[F_FF_VALID], FD_T_LEFT_PENDING, frm_start != p.blk_pos0);
        if ((int32_t)((uint32_t)s.v[F_RUN_POS] - p.blk_pos0) <= 0) {
            p.direct = 1;
            p.far_delta = (uint32_t)s.v[F_RUN_DELTA];
            s.v[F_RUN_POS] = (int32_t)p.blk_pos0;           // any position of the run will do: keep it near (the counters wrap)
            s.v[F_FF_VALID] = 0;
        } else {
            if (!s.v[F_FF_VALID]) {                         // the ticks before were direct: their run covers what is pending
                p.left_count = (int32_t)(frm_start - p.blk_pos0);
                p.left_delta = run_delta_start;
            }
            s.v[F_FF_VALID] = 1;
        }
    }
}

// One tick of a session of an object of mixed rates and call sizes (aecm_flow_plan_mixed_kernel): fs is the SESSION's rate;
// with kFlowHalfCall (n = 160) the session makes one call pair of 80 samples on the first half of its rows -- the plan says one
// call, one frame -- and the 80 samples of the tick it did not consume are 80 samples the object's near position runs ahead
// of it: its lag, exactly as if it had sat out half a tick (FlowResync at its next call).  The tick kernel still appends all
// of the tick's near-end samples at the object's position; the second half lands ahead of the session's own position, where
// the next call's resync and append overwrite it before any block asks for it (tests/sim/sim_mixed.cpp).
AECM_FLOW_HD void FlowTickMixed(FlowRegs &s, int fs, int n, int ms, int flags, uint32_t near_pos, FlowPlan &p) {
    AECM_FLOW_MARK(FD_TM_HALF_FLAG, (flags & kFlowHalfCall) != 0);
    AECM_FLOW_MARK_IF((flags & kFlowHalfCall) != 0, FD_TM_HALF_N, n == 2 * kFlowFrame);
    const bool half = (flags & kFlowHalfCall) != 0 && n == 2 * kFlowFrame;
    FlowTick(s, fs, half ? kFlowFrame : n, ms, flags & (kFlowNoFarend | kFlowSplitCalls), near_pos, p);
    if (half) s.v[F_NEAR_LAG] = FlowIdleTick(s.v[F_NEAR_LAG], kFlowFrame);
}

// A tick of K call pairs of n samples (a 20 .. 60 ms packet interval on 10 ms calls; WebRtcAecmSessions_TickCalls): K times
// FlowTick, in order, the near position advancing n per call -- call c's samples are [c n, (c + 1) n) of every row and land at
// near-ring positions near_pos + c n.  One plan per call, handed to `sink(c, plan)` as it is made (on the device: packed and
// stored, so that only one plan is ever in registers).  No new arithmetic: every state between two calls is a state between two
// ordinary ticks, and the replay-row spill test is made per call, with its one-tick margin.  The session is in step
// (FlowResync ONCE, before the first call, otherwise); a session that sits the tick out falls calls * n samples behind
// (FlowIdleTick(lag, calls * n)).  flags: kFlowNoFarend (none of the K pairs has a BufferFarend) or 0.
constexpr int kFlowMaxTickCalls = 6;                // = AECM_SESSION_MAX_TICK_CALLS: 60 ms of 10 ms calls
template <class Sink>
AECM_FLOW_HD void FlowTickCalls(FlowRegs &s, int fs, int n, int calls, int ms, int flags, uint32_t near_pos, Sink &&sink) {
    for (int c = 0; c < calls; ++c) {
        FlowPlan p;
        FlowTick(s, fs, n, ms, flags & kFlowNoFarend, near_pos + (uint32_t)(c * n), p);
        sink(c, p);
    }
}
static_assert(kFlowMaxTickCalls * 2 * kFlowFrame < kFlowFarRing - kFlowJitterCapacity, "a K-call tick fits the rings");

// A packet tick (WebRtcAecmSessions_TickPackets): K call pairs per session, every session at its OWN rate (fs: the session's) and
// its own call size -- n_s = 80 with kFlowHalfCall in a 160-sample tick, else n -- on PACKED rows: call c's samples are
// [c n_s, (c + 1) n_s) of the session's rows and land at near-ring positions near_pos + c n_s, so the session's own near positions
// are contiguous across its K calls and nothing has to be brought back in step between them.  K times FlowTick of n_s samples
// (each plan carries the call size in n_frames); once, at the end, the samples of the tick the session did not consume become its
// lag: K * 80 for a session that made half calls, exactly as after K ordinary half-call ticks.  The session is in step at entry
// (FlowResync ONCE, before the first call, otherwise).  flags: kFlowNoFarend and kFlowHalfCall count.
AECM_FLOW_HD int FlowPacketCallSize(int n, int flags) {
    AECM_FLOW_MARK(FD_PK_HALF_FLAG, (flags & kFlowHalfCall) != 0);
    AECM_FLOW_MARK_IF((flags & kFlowHalfCall) != 0, FD_PK_HALF_N, n == 2 * kFlowFrame);
    return (flags & kFlowHalfCall) != 0 && n == 2 * kFlowFrame ? kFlowFrame : n;
}
template <class Sink>
AECM_FLOW_HD void FlowTickPackets(FlowRegs &s, int fs, int n, int calls, int ms, int flags, uint32_t near_pos, Sink &&sink) {
    const int n_s = FlowPacketCallSize(n, flags);
    for (int c = 0; c < calls; ++c) {
        FlowPlan p;
        FlowTick(s, fs, n_s, ms, flags & kFlowNoFarend, near_pos + (uint32_t)(c * n_s), p);
        sink(c, p);
    }
    s.v[F_NEAR_LAG] = FlowIdleTick(s.v[F_NEAR_LAG], calls * (n - n_s));
}

// The host's pass over a tick's flags (SessionBatch::Enqueue): FlowLiveBlockBases, and in the same pass what the sessions that
// call ask for -- *any = the OR of their bytes, *half_and_split = some session carries kFlowHalfCall and kFlowSplitCalls together.
inline int32_t FlowScanFlags(const uint8_t *flags, int32_t n_sessions, uint32_t *bases, uint8_t *any, bool *half_and_split) {
    int32_t live = 0;
    uint32_t any_bits = 0, both = 0;
    for (int32_t first = 0, b = 0; first < n_sessions; first += kFlowPlanBlock, ++b) {
        bases[b] = (uint32_t)live;
        const int32_t end = first + kFlowPlanBlock < n_sessions ? first + kFlowPlanBlock : n_sessions;
        int32_t idle = 0;
        for (int32_t s = first; s < end; ++s) {
            const uint32_t f = flags[s], is_idle = (f >> 2) & 1u, mine = f & (is_idle - 1u);     // an idle session's bits mean nothing
            idle += (int32_t)is_idle;
            any_bits |= mine;
            both |= mine & (mine >> 2);                                                          // bit 1: split (2) and half (8) together
        }
        live += (end - first) - idle;
    }
    *any = (uint8_t)any_bits;
    *half_and_split = (both & (uint32_t)kFlowSplitCalls) != 0;
    return live;
}
static_assert(kFlowHalfCall >> 2 == kFlowSplitCalls, "FlowScanFlags lines the two bits up");
// What a tick's flags may ask for: two calls of 80, or one call of 80 out of 160, need a tick of 160 samples, and exclude each other.
inline bool FlowTickFlagsValid(int n, uint8_t any, bool half_and_split) {
    return !(n != 2 * kFlowFrame && (any & (kFlowSplitCalls | kFlowHalfCall)) != 0) && !half_and_split;
}

// The plan as the kFlowPlanWords int32 the two kernels exchange.
constexpr int kFlowPlanWords = 16;
enum FlowPlanWord : int {
    P_FAR_COUNTS = 0,     // far[0].count | far[1].count << 16   (far[c].src = c * 80: a second piece only exists for two 80-sample calls)
    P_FAR_POS0, P_FAR_POS1,
    P_BITS,               // frame f at bits [4 f, 4 f + 4): active | far_from_stream << 1 | old_idx << 2 | spill[f] << 3;
                          // n_frames << 8, n_blocks << 12, direct << 16, left_count << 20
    P_FRAME_FAR_POS0, P_FRAME_FAR_POS1, P_FRM_POS0, P_FRM_POS1, P_OUT_POS0, P_OUT_POS1,
    P_BLK_POS0, P_NEAR_BASE, P_FAR_DELTA, P_LEFT_DELTA, P_SPILL_POS0, P_SPILL_POS1
};
AECM_FLOW_HD void FlowPackPlan(const FlowPlan &p, int32_t w[kFlowPlanWords]) {
    w[P_FAR_COUNTS] = p.far[0].count | (p.far[1].count << 16);
    w[P_FAR_POS0] = (int32_t)p.far[0].pos;
    w[P_FAR_POS1] = (int32_t)p.far[1].pos;
    int32_t bits = (p.n_frames << 8) | (p.n_blocks << 12) | (p.direct << 16) | (p.left_count << 20);
    for (int f = 0; f < 2; ++f)
        bits |= (p.frame[f].active | (p.frame[f].far_from_stream << 1) | (p.frame[f].old_idx << 2) | (p.spill[f] << 3)) << (4 * f);
    w[P_BITS] = bits;
    w[P_FRAME_FAR_POS0] = (int32_t)p.frame[0].far_pos;
    w[P_FRAME_FAR_POS1] = (int32_t)p.frame[1].far_pos;
    w[P_FRM_POS0] = (int32_t)p.frame[0].frm_pos;
    w[P_FRM_POS1] = (int32_t)p.frame[1].frm_pos;
    w[P_OUT_POS0] = (int32_t)p.frame[0].out_pos;
    w[P_OUT_POS1] = (int32_t)p.frame[1].out_pos;
    w[P_BLK_POS0] = (int32_t)p.blk_pos0;
    w[P_NEAR_BASE] = (int32_t)p.near_base;
    w[P_FAR_DELTA] = (int32_t)p.far_delta;
    w[P_LEFT_DELTA] = (int32_t)p.left_delta;
    w[P_SPILL_POS0] = (int32_t)p.spill_pos[0];
    w[P_SPILL_POS1] = (int32_t)p.spill_pos[1];
}
// far[1].src is the length of the first call: 80 whenever there is a second piece.  (Per-frame block counts do not travel.)
AECM_FLOW_HD void FlowUnpackPlan(const int32_t w[kFlowPlanWords], FlowPlan &p) {
    p.far[0] = FlowFarPiece{0, w[P_FAR_COUNTS] & 0xffff, (uint32_t)w[P_FAR_POS0]};
    p.far[1] = FlowFarPiece{kFlowFrame, (int32_t)((uint32_t)w[P_FAR_COUNTS] >> 16), (uint32_t)w[P_FAR_POS1]};
    const int32_t bits = w[P_BITS];
    p.n_calls = 0;
    p.n_frames = (bits >> 8) & 15;
    p.n_blocks = (bits >> 12) & 15;
    p.direct = (bits >> 16) & 1;
    p.left_count = (bits >> 20) & 127;
    for (int f = 0; f < 2; ++f) {
        const int32_t b = (bits >> (4 * f)) & 15;
        p.frame[f] = FlowFrame{b & 1, (b >> 1) & 1, (uint32_t)w[P_FRAME_FAR_POS0 + f], (b >> 2) & 1, (uint32_t)w[P_FRM_POS0 + f], 0,
                               (uint32_t)w[P_OUT_POS0 + f]};
        p.spill[f] = (b >> 3) & 1;
        p.spill_pos[f] = (uint32_t)w[P_SPILL_POS0 + f];
    }
    p.blk_pos0 = (uint32_t)w[P_BLK_POS0];
    p.near_base = (uint32_t)w[P_NEAR_BASE];
    p.far_delta = (uint32_t)w[P_FAR_DELTA];
    p.left_delta = (uint32_t)w[P_LEFT_DELTA];
}

}  // namespace aecm
#endif  // AECM_AMD_FLOW_PLAN_H_
