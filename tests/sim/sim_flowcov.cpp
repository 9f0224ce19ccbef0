// TEST INFRASTRUCTURE: the session wrapper's decision path (webrtc_aecm_amd/csrc/aecm_flow_plan.h: the Flow* functions) driven
// as the planning kernels drive it -- N sessions, one lane each, tick by tick, planned by the host's own planner (aecm_tick_plan.h):
// the dense, the sparse and the mixed planning kernel, the K-call and the packets planner, and far-end bursts -- with the
// header's decision markers switched on.  tools/flow_coverage.py builds this file with -O0 --coverage (branch counters) and reads
// the record of (decision, outcome) per tick and session the markers leave: from it, whether two sessions of one wavefront
// (64 consecutive ids) disagreed on a decision within one launch.  tests/test_gpu_flow_corpus.py builds it plainly and compares
// the wrapper words every tick leaves (regs_out) with the device's.
//
// The run is a parity run: every session is also a SessionFlow<T> (aecm_session_flow.h, the restatement of the reference's
// wrapper) on sample TAGS, as in sim_flow.cpp -- the tags that reach every block, every output sample and every return code of
// the plans executed the way aecm_tick_flow_kernel executes them (lags, resyncs and packed rows included) must be SessionFlow's.
#include <stdint.h>
#include <string.h>

#include <vector>

namespace {
thread_local uint8_t *g_marks = nullptr;        // the current (tick, session)'s row: bit 0 = went false, bit 1 = went true (runs may share a process)
inline void flowcov_mark(int id, bool outcome) {
    if (g_marks) g_marks[id] |= outcome ? 2 : 1;
}
}  // namespace
#define AECM_FLOW_MARK(id, outcome) flowcov_mark((int)(id), (outcome))
#define AECM_FLOW_MARK_IF(guard, id, outcome) \
    do {                                      \
        if (guard) flowcov_mark((int)(id), (outcome)); \
    } while (0)

#include "aecm_flow_plan.h"
#include "aecm_session_flow.h"
#include "aecm_tick_plan.h"

namespace {

using namespace aecm;

constexpr int32_t kRingLen = kFlowFarRing, kMask = kRingLen - 1, kNone = -1, kJunk = -2;
constexpr int32_t kNearTag = 1 << 28, kOutTag = 1 << 29;

struct Session {
    FlowRegs regs;
    int fs = 16000;
    std::vector<int32_t> far_ring, near_ring, out_ring, far_frames, far_old;
    int64_t blocks_done = 0, ref_blocks = 0, far_offered = 0, near_offered = 0;
    SessionFlow<int32_t> ref;
    Session() : far_ring(kRingLen, kNone), near_ring(kRingLen, kNone), out_ring(kRingLen, kNone), far_frames(kFlowFarFrameRing, kNone),
                far_old(2 * kFlowFrame, kNone), ref(kNone) {
        int32_t words[kFlowWords];
        FlowInit(words);
        for (int k = 0; k < kFlowFieldsUsed; ++k) regs.v[k] = words[k];
    }
    // aecm_buffer_farend_kernel: only the fields a burst may read, the spills first, then call by call
    void Burst(int len, int calls) {
        FlowRegs r;
        for (int k = 0; k < kFlowFieldsUsed; ++k) r.v[k] = 0x5a5a5a5a;
        FlowBurstReads([&](int f) { r.v[f] = regs.v[f]; });
        FlowBurst b;
        FlowBurstBegin(r, len, calls, b);
        for (int i = 0; i < 2; ++i)
            if (b.spill[i])
                for (int j = 0; j < kFlowFrame; ++j) far_old[i * kFlowFrame + j] = far_ring[(b.spill_pos[i] + (uint32_t)j) & kMask];
        std::vector<int32_t> in(len);
        for (int c = 0; c < calls; ++c) {
            for (int j = 0; j < len; ++j) in[j] = (int32_t)(far_offered + j);
            far_offered += len;
            const uint32_t pos = (uint32_t)r.v[F_FAR_WP];
            const int32_t accepted = FlowFarendCall(r, fs == 16000 ? 2 : 1, len);
            for (int j = 0; j < accepted; ++j) far_ring[(pos + (uint32_t)j) & kMask] = in[j];
            ref.BufferFarend(in.data(), (size_t)len);
        }
        FlowBurstWrites([&](int f) { regs.v[f] = r.v[f]; });
    }
    // One plan the way the tick kernels execute it (the near end is in the ring already): far pieces, spills, framing, blocks,
    // output frames.  far_in / near_in: the n_frames * 80 samples of this plan's calls.
    void Execute(const FlowPlan &planned, const int32_t *far_in, const int32_t *near_in, int32_t *out, std::vector<int32_t> *blk_far,
                 std::vector<int32_t> *blk_near) {
        FlowPlan p;
        int32_t words[kFlowPlanWords];
        FlowPackPlan(planned, words);
        FlowUnpackPlan(words, p);
        const int n = p.n_frames * kFlowFrame;
        for (int j = 0; j < n; ++j)
            for (int c = 0; c < 2; ++c)
                if (j >= p.far[c].src && j < p.far[c].src + p.far[c].count) far_ring[(p.far[c].pos + (uint32_t)(j - p.far[c].src)) & kMask] = far_in[j];
        for (int i = 0; i < 2; ++i)
            if (p.spill[i])
                for (int j = 0; j < kFlowFrame; ++j) far_old[i * kFlowFrame + j] = far_ring[(p.spill_pos[i] + (uint32_t)j) & kMask];
        if (!p.direct) {
            int32_t left[kFlowBlock], frames[2][kFlowFrame];
            for (int j = 0; j < p.left_count; ++j) left[j] = far_ring[(p.blk_pos0 + p.left_delta + (uint32_t)j) & kMask];
            for (int f = 0; f < p.n_frames; ++f) {
                const FlowFrame &q = p.frame[f];
                if (!q.active) continue;
                for (int j = 0; j < kFlowFrame; ++j)
                    frames[f][j] = q.far_from_stream ? far_ring[(q.far_pos + (uint32_t)j) & kMask] : far_old[q.old_idx * kFlowFrame + j];
            }
            for (int j = 0; j < p.left_count; ++j) far_frames[(p.blk_pos0 + (uint32_t)j) & (kFlowFarFrameRing - 1)] = left[j];
            for (int f = 0; f < p.n_frames; ++f) {
                const FlowFrame &q = p.frame[f];
                if (!q.active) continue;
                for (int j = 0; j < kFlowFrame; ++j) far_frames[(q.frm_pos + (uint32_t)j) & (kFlowFarFrameRing - 1)] = frames[f][j];
            }
        }
        for (int b = 0; b < p.n_blocks; ++b, ++blocks_done)
            for (int t = 0; t < kFlowBlock; ++t) {
                const uint32_t x = p.blk_pos0 + (uint32_t)(b * kFlowBlock + t);
                blk_far->push_back(p.direct ? far_ring[(x + p.far_delta) & kMask] : far_frames[x & (kFlowFarFrameRing - 1)]);
                blk_near->push_back(near_ring[(p.near_base + x) & kMask]);
                out_ring[x & kMask] = (int32_t)(kOutTag + blocks_done * kFlowBlock + t);
            }
        for (int f = 0; f < p.n_frames; ++f)
            for (int j = 0; j < kFlowFrame; ++j)
                out[f * kFlowFrame + j] = p.frame[f].active ? out_ring[(p.frame[f].out_pos + (uint32_t)j) & kMask] : near_in[f * kFlowFrame + j];
    }
    // The same call pairs on the reference side; returns the first non-zero code.
    int32_t RefCalls(int calls, int len, bool farend, int ms, const int32_t *far_in, const int32_t *near_in, int32_t *out, std::vector<int32_t> *blk_far,
                     std::vector<int32_t> *blk_near) {
        int32_t first = 0;
        for (int c = 0; c < calls; ++c) {
            if (farend) ref.BufferFarend(far_in + c * len, (size_t)len);
            const int32_t rc = ref.Process(near_in + c * len, nullptr, out + c * len, (size_t)len, (int16_t)ms,
                                           [&](const int32_t *fb, const int32_t *nb, const int32_t *, int32_t *ob, int nblk) {
                                               blk_far->insert(blk_far->end(), fb, fb + nblk * kFlowBlock);
                                               blk_near->insert(blk_near->end(), nb, nb + nblk * kFlowBlock);
                                               for (int j = 0; j < nblk * kFlowBlock; ++j) ob[j] = (int32_t)(kOutTag + ref_blocks * kFlowBlock + j);
                                               ref_blocks += nblk;
                                               return true;
                                           });
            if (rc != 0 && first == 0) first = rc;
        }
        return first;
    }
};

}  // namespace

extern "C" {

int flowcov_decisions(void) { return kFlowDecisions; }
int flowcov_fields(void) { return kFlowFieldsUsed; }
const char *flowcov_decision_name(int id) {
#define AECM_FLOW_DECISION_NAME(name) #name,
    static const char *const names[] = {AECM_FLOW_DECISIONS(AECM_FLOW_DECISION_NAME)};
    return id >= 0 && id < kFlowDecisions ? names[id] : "";
}

// A run of S sessions through T ticks of one object (rate object_fs; rates[S]: the sessions' own).
//   kind[T]       0 an ordinary tick of n_t samples (planned as SessionBatch::Enqueue plans it: dense, sparse or mixed planning kernel),
//                 1 a K-call tick (TickCalls), 2 a packet tick (TickPackets); calls_t[T] = K
//   flags[T * S], ms[T * S]      the tick's per-session arguments
//   burst[T * S], burst_len[T]   WebRtcAecm_BufferFarend calls of burst_len samples the session makes before the tick (a launch of
//                                aecm_buffer_farend_kernel of its own, one wavefront per session: its marks go to a row of their own)
//   preroll[S], preroll_ms[S]    Process calls of 80 samples without a far end the session has made before it was imported (16 kHz: the
//                                start-up counters run on and wrap); far_off[S], frm_off[S]: where its position counters stand
//   start_out[S * kFlowWords]    the wrapper words of that imported state (what the test patches into a snapshot)
//   regs_out[T * S * kFlowFieldsUsed]   the wrapper words after every tick
//   marks[T * 2 * S * kFlowDecisions]   the outcome record: [t][0] the tick's planning launch, [t][1] the burst launch before it;  kernel_out[T]: the tick's TickFamily (aecm_tick_plan.h)
//   continues[T * S]             calls of the tick the session's call loop left with `continue` (the start-up phase)
// Returns -1, or the first tick at which the two sides differed; detail[0] = what (1 block count, 2 far tags, 3 near tags, 4 output,
// 5 return code, 6 live list, 8 the host refuses the tick, 100 + field: FlowStateDefect refused the state), detail[1] = the session.
int64_t flowcov_run(int S, int T, int object_fs, int force_sparse, const int32_t *rates, const int32_t *kind, const int32_t *n_t, const int32_t *calls_t,
                    const uint8_t *flags, const int16_t *ms, const uint8_t *burst, const int32_t *burst_len, const int32_t *preroll,
                    const int16_t *preroll_ms, const uint32_t *far_off, const uint32_t *frm_off, int32_t *start_out, int32_t *regs_out, uint8_t *marks,
                    int32_t *kernel_out, uint8_t *continues, int64_t *detail) {
    std::vector<Session> sess((size_t)S);
    std::vector<int32_t> far_in, near_in, out_dev, out_ref, dfar, dnear, rfar, rnear;
    detail[0] = detail[1] = 0;
    g_marks = nullptr;
    TickObject obj;
    obj.Init(S, object_fs);
    obj.force_sparse = force_sparse != 0;
    for (int s = 0; s < S; ++s) {
        Session &x = sess[(size_t)s];
        x.fs = rates[s];
        obj.SetRate(s, rates[s]);
        x.ref.Init(x.fs);
        int32_t zeros[kFlowFrame], o[kFlowFrame];
        for (int c = 0; c < preroll[s]; ++c) {
            FlowPlan p;
            FlowTick(x.regs, x.fs, kFlowFrame, preroll_ms[s], kFlowNoFarend, 0u, p);
            for (int j = 0; j < kFlowFrame; ++j) zeros[j] = kJunk;
            x.ref.Process(zeros, nullptr, o, kFlowFrame, preroll_ms[s], [](const int32_t *, const int32_t *, const int32_t *, int32_t *, int) { return true; });
            if (!x.regs.v[F_EC_STARTUP] || x.ref.in_startup() == false) {
                detail[0] = 7;                  // a preroll must stay inside the start-up phase: nothing may have been framed
                detail[1] = s;
                return 0;
            }
        }
        for (int f : {F_FAR_RP, F_FAR_WP}) x.regs.v[f] = (int32_t)((uint32_t)x.regs.v[f] + far_off[s]);
        for (int f : {F_FRM_POS, F_BLK_POS, F_OUT_RP, F_RUN_POS}) x.regs.v[f] = (int32_t)((uint32_t)x.regs.v[f] + frm_off[s]);
        for (int k = 0; k < kFlowWords; ++k) start_out[(size_t)s * kFlowWords + k] = k < kFlowFieldsUsed ? x.regs.v[k] : 0;
        if (const int field = FlowStateDefect(start_out + (size_t)s * kFlowWords)) {
            detail[0] = 100 + field;
            detail[1] = s;
            return 0;
        }
    }
    const int n_groups = (S + kFlowPlanBlock - 1) / kFlowPlanBlock;
    std::vector<uint32_t> live_list((size_t)S);
    std::vector<int32_t> codes((size_t)S);
    for (int t = 0; t < T; ++t) {
        const int n = n_t[t], K = kind[t] == 0 ? 1 : calls_t[t], span = n * K;
        const uint8_t *fl = flags + (size_t)t * S;
        uint8_t *mrow = marks + (size_t)t * 2 * S * kFlowDecisions, *brow = mrow + (size_t)S * kFlowDecisions;
        // far-end bursts before the tick
        for (int s = 0; s < S; ++s)
            if (burst[(size_t)t * S + s]) {
                g_marks = brow + (size_t)s * kFlowDecisions;
                sess[(size_t)s].Burst(burst_len[t], burst[(size_t)t * S + s]);
                g_marks = nullptr;
            }
        // the host: check, plan, commit
        TickArgs args;
        args.flags_per_session = fl;
        args.n = n;
        args.calls = K;
        args.packets = kind[t] == 2;
        uint32_t near_pos;
        const TickPlan plan = obj.Tick(args, &near_pos);
        if (plan.code) {
            detail[0] = 8;
            detail[1] = plan.code;
            return t;
        }
        (void)TickCodes(ms + (size_t)t * S, 0, fl, S, codes.data());
        const TickFamily kernel = plan.family;
        kernel_out[t] = kernel;
        if (kernel != kTickFamily_nothing) {
            const FlowTickRoute &route = plan.route;
            const bool k_calls = plan.k_calls;
            const std::vector<uint32_t> &bases = obj.Bases(plan);
            const bool live_list_wanted = k_calls || (kernel != kTickFamily_dense && route.sparse_tick);
            if (live_list_wanted) {
                // the device half of the live list: ballots per wavefront, counts per workgroup, FlowLiveSlot per lane
                std::fill(live_list.begin(), live_list.end(), 0xffffffffu);
                for (int g = 0; g < n_groups; ++g) {
                    uint32_t wave_counts[kFlowPlanBlock / 64];
                    uint64_t ballots[kFlowPlanBlock / 64];
                    for (int w = 0; w < kFlowPlanBlock / 64; ++w) {
                        ballots[w] = 0;
                        for (int l = 0; l < 64; ++l) {
                            const int s = g * kFlowPlanBlock + w * 64 + l;
                            if (s < S && !(fl[s] & kFlowIdle)) ballots[w] |= uint64_t(1) << l;
                        }
                        wave_counts[w] = (uint32_t)__builtin_popcountll(ballots[w]);
                    }
                    for (int th = 0; th < kFlowPlanBlock; ++th) {
                        const int s = g * kFlowPlanBlock + th;
                        if (s < S) g_marks = mrow + (size_t)s * kFlowDecisions;
                        const uint32_t slot = FlowLiveSlot(bases[(size_t)g], wave_counts, th >> 6, ballots[th >> 6], th & 63);
                        g_marks = nullptr;
                        if (s < S && !(fl[s] & kFlowIdle) && slot < (uint32_t)S) live_list[slot] = (uint32_t)s;
                    }
                }
                int32_t at = 0;
                for (int s = 0; s < S; ++s)
                    if (!(fl[s] & kFlowIdle) && live_list[(size_t)at++] != (uint32_t)s) {
                        detail[0] = 6;
                        detail[1] = s;
                        return t;
                    }
            }
            for (int s = 0; s < S; ++s) {
                Session &x = sess[(size_t)s];
                g_marks = mrow + (size_t)s * kFlowDecisions;
                const int f = fl[s], m = ms[(size_t)t * S + s];
                if (kernel != kTickFamily_dense) {
                    const bool is_live = (f & kFlowIdle) == 0;
                    AECM_FLOW_MARK(FD_K_LIVE, is_live);
                    if (!is_live) {
                        x.regs.v[F_NEAR_LAG] = FlowIdleTick(FlowIdleTick(x.regs.v[F_NEAR_LAG], route.deferred_lag), span);
                        g_marks = nullptr;
                        continue;
                    }
                    x.regs.v[F_NEAR_LAG] = FlowIdleTick(x.regs.v[F_NEAR_LAG], route.deferred_lag);
                    AECM_FLOW_MARK(FD_K_RESYNC, x.regs.v[F_NEAR_LAG] != 0);
                    if (x.regs.v[F_NEAR_LAG] != 0) {
                        FlowNearMove mv;
                        FlowResync(x.regs, near_pos, mv);
                        FlowMoveNear(x.near_ring.data(), (uint32_t)kMask, mv);
                    }
                }
                // the session's own samples of the tick: K calls of n_s samples at the start of its rows, junk behind them
                const int session_fs = kernel == kTickFamily_dense || kernel == kTickFamily_sparse || kernel == kTickFamily_calls ? object_fs : x.fs;
                const bool half = (f & kFlowHalfCall) != 0 && n == 2 * kFlowFrame && (kernel == kTickFamily_mixed || kernel == kTickFamily_packets);
                const int n_s = half ? kFlowFrame : n, own = K * n_s;
                far_in.assign((size_t)span, kJunk);
                near_in.assign((size_t)span, kJunk);
                for (int j = 0; j < own; ++j) {
                    far_in[(size_t)j] = (int32_t)(x.far_offered + j);
                    near_in[(size_t)j] = (int32_t)(kNearTag + x.near_offered + j);
                }
                const bool farend = !(f & kFlowNoFarend);
                if (farend) x.far_offered += own;
                x.near_offered += own;
                for (int j = 0; j < span; ++j) x.near_ring[(near_pos + (uint32_t)j) & kMask] = near_in[(size_t)j];
                out_dev.assign((size_t)span, kNone);
                out_ref.assign((size_t)span, kNone);
                dfar.clear(), dnear.clear(), rfar.clear(), rnear.clear();
                int n_cont = 0;
                auto sink = [&](int c, const FlowPlan &p) {          // (two calls: frame c is call c's; else both frames are the one call's)
                    n_cont += p.n_calls == 2 ? !p.frame[0].active + !p.frame[1].active : !p.frame[0].active;
                    x.Execute(p, far_in.data() + c * n_s, near_in.data() + c * n_s, out_dev.data() + c * n_s, &dfar, &dnear);
                };
                if (kernel == kTickFamily_calls) {
                    FlowTickCalls(x.regs, session_fs, n, K, m, f, near_pos, sink);
                } else if (kernel == kTickFamily_packets) {
                    FlowTickPackets(x.regs, session_fs, n, K, m, f, near_pos, sink);
                } else {
                    FlowPlan p;
                    if (kernel == kTickFamily_mixed) FlowTickMixed(x.regs, session_fs, n, m, f, near_pos, p);
                    else FlowTick(x.regs, session_fs, n, m, f, near_pos, p);
                    sink(0, p);
                }
                g_marks = nullptr;
                continues[(size_t)t * S + s] = (uint8_t)n_cont;
                // the reference side: the same call pairs
                const bool split = (f & kFlowSplitCalls) != 0 && n_s == 2 * kFlowFrame && K == 1;
                const int ref_calls = split ? 2 : K, ref_len = split ? kFlowFrame : n_s;
                const int32_t rc_ref = x.RefCalls(ref_calls, ref_len, farend, m, far_in.data(), near_in.data(), out_ref.data(), &rfar, &rnear);
                const int32_t rc_dev = codes[(size_t)s];
                int what = 0;
                int32_t words[kFlowWords] = {0};
                for (int k = 0; k < kFlowFieldsUsed; ++k) words[k] = x.regs.v[k];
                if (const int field = FlowStateDefect(words)) what = 100 + field;
                else if (dfar.size() != rfar.size()) what = 1;
                else if (dfar != rfar) what = 2;
                else if (dnear != rnear) what = 3;
                else if (memcmp(out_dev.data(), out_ref.data(), sizeof(int32_t) * (size_t)own) != 0) what = 4;
                else if (rc_dev != rc_ref) what = 5;
                if (what) {
                    detail[0] = what;
                    detail[1] = s;
                    return t;
                }
            }
        }
        for (int s = 0; s < S; ++s)
            for (int k = 0; k < kFlowFieldsUsed; ++k) regs_out[((size_t)t * S + s) * kFlowFieldsUsed + k] = sess[(size_t)s].regs.v[k];
    }
    return -1;
}

}  // extern "C"
