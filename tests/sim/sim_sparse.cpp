// TEST INFRASTRUCTURE: sessions that sit out ticks (AECM_SESSION_IDLE) on sample TAGS -- the method of sim_flow.cpp.  The
// device side is what the host's tick planner (aecm_tick_plan.h), aecm_flow_plan_kernel / aecm_flow_plan_sparse_kernel and the tick kernels do for
// ONE session of an object whose other sessions may or may not call (webrtc_aecm_amd/csrc/aecm_flow_plan.h: FlowIdleTick,
// FlowResync, FlowMoveNear, FlowTick); the reference side is SessionFlow<T> (aecm_session_flow.h), which in an idle tick is
// simply not called.  Also: the live list of a tick (host half + device half) and FlowStateDefect's view of the lag.
#include <stdint.h>
#include <string.h>

#include <vector>

#include "aecm_flow_plan.h"
#include "aecm_ops.h"
#include "aecm_session_flow.h"
#include "aecm_tick_plan.h"

namespace {

using namespace aecm;

constexpr int64_t kRingLen = kFlowFarRing, kOutTagBase = int64_t(1) << 40, kNone = -1;

struct Rng {
    uint64_t s;
    uint32_t next() {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        return (uint32_t)(s >> 33);
    }
    int range(int lo, int hi) { return lo + (int)(next() % (uint32_t)(hi - lo + 1)); }
    bool chance(int percent) { return (int)(next() % 100u) < percent; }
};

// One session of an object, in the tag domain: the session's rows on the device + what the host keeps for the object.
struct DeviceSide {
    FlowRegs regs;
    std::vector<int64_t> far_ring, near_ring, out_ring, far_frames, far_old;
    TickObject obj;                        // what the host keeps for the object (its near position, its lags)
    int64_t blocks_done = 0, moves = 0, moved_samples = 0, dense_ticks = 0, deferred_ticks = 0;
    int fault = 0;                         // 1: a dense tick met a session that lags (the host's routing is wrong); 2: the host refused the
                                           // tick, or a K-call tick did not go by the live list
    DeviceSide() : far_ring(kRingLen, kNone), near_ring(kRingLen, kNone), out_ring(kRingLen, kNone), far_frames(kFlowFarFrameRing, kNone),
                   far_old(2 * kFlowFrame, kNone) {
        int32_t words[kFlowWords];
        FlowInit(words);
        for (int k = 0; k < kFlowFieldsUsed; ++k) regs.v[k] = words[k];
        obj.Init(3, 16000);
    }
    // The host's side of one tick -- check, plan, commit -- of an object of three sessions: this one, one that calls when the caller
    // says so (others_live) and one that sits out when the caller says so (others_idle); either of the two otherwise does as this
    // one does.  *tick_pos: the object's near position before the tick.
    TickPlan HostTick(int n, int calls, int flags, bool idle, bool others_live, bool others_idle, uint32_t *tick_pos) {
        const uint8_t follows = idle ? (uint8_t)kFlowIdle : (uint8_t)0;
        const uint8_t f[3] = {idle ? (uint8_t)kFlowIdle : (uint8_t)flags, others_live ? (uint8_t)0 : follows, others_idle ? (uint8_t)kFlowIdle : follows};
        TickArgs a;
        a.flags_per_session = f;
        a.n = n;
        a.calls = calls;
        const TickPlan plan = obj.Tick(a, tick_pos);
        if (plan.code) fault = 2;
        return plan;
    }
    // aecm_buffer_farend_kernel (as in sim_flow.cpp)
    void BufferFarend(int fs, int len, int calls, const int64_t *far_in) {
        const int64_t mask = kRingLen - 1;
        FlowRegs r;
        for (int k = 0; k < kFlowFieldsUsed; ++k) r.v[k] = 0x5a5a5a5a;
        FlowBurstReads([&](int f) { r.v[f] = regs.v[f]; });
        FlowBurst b;
        FlowBurstBegin(r, len, calls, b);
        for (int i = 0; i < 2; ++i)
            if (b.spill[i])
                for (int j = 0; j < kFlowFrame; ++j) far_old[i * kFlowFrame + j] = far_ring[(b.spill_pos[i] + (uint32_t)j) & mask];
        const int mult = fs == 16000 ? 2 : 1;
        for (int c = 0; c < calls; ++c) {
            const uint32_t pos = (uint32_t)r.v[F_FAR_WP];
            const int32_t accepted = FlowFarendCall(r, mult, len);
            for (int j = 0; j < accepted; ++j) far_ring[(pos + (uint32_t)j) & mask] = far_in[c * len + j];
        }
        FlowBurstWrites([&](int f) { regs.v[f] = r.v[f]; });
    }
    // One tick of the object.  idle: this session carries kFlowIdle; others_live: some other session calls; others_idle: some
    // other session is idle.  Returns false when the session made no call (out untouched).
    bool Tick(int fs, int n, int ms, int flags, bool idle, bool others_live, bool others_idle, const int64_t *far_in, const int64_t *near_in,
              int64_t *out, std::vector<int64_t> *blk_far, std::vector<int64_t> *blk_near) {
        const int64_t mask = kRingLen - 1;
        // which launches the tick takes is the host's own decision
        uint32_t near_pos;
        const TickPlan plan = HostTick(n, 1, flags, idle, others_live, others_idle, &near_pos);
        const FlowTickRoute &route = plan.route;
        if (!route.launch) {                                            // nobody calls: nothing is launched
            ++deferred_ticks;
            return false;
        }
        const int32_t deferred_lag = route.deferred_lag;
        FlowPlan planned, p;
        if (!route.sparse_plan) {                                       // aecm_flow_plan_kernel: knows no lags
            if (regs.v[F_NEAR_LAG] != 0 || obj.lag.deferred_lag != 0) fault = 1;
            FlowRegs r = regs;
            r.v[F_NEAR_LAG] = 0x5a5a5a5a;                               // (not loaded)
            FlowTick(r, fs, n, ms, flags, near_pos, planned);
            for (int k = 0; k < kFlowTickFields; ++k) regs.v[k] = r.v[k];
            ++dense_ticks;
        } else {                                                        // aecm_flow_plan_sparse_kernel
            if (idle) {
                regs.v[F_NEAR_LAG] = FlowIdleTick(FlowIdleTick(regs.v[F_NEAR_LAG], deferred_lag), n);
            } else {
                regs.v[F_NEAR_LAG] = FlowIdleTick(regs.v[F_NEAR_LAG], deferred_lag);
                if (regs.v[F_NEAR_LAG] != 0) {
                    FlowNearMove m;
                    FlowResync(regs, near_pos, m);
                    FlowMoveNear(near_ring.data(), (uint32_t)mask, m);
                    moves += m.count > 0;
                    moved_samples += m.count;
                }
                FlowTick(regs, fs, n, ms, flags, near_pos, planned);
            }
        }
        if (idle) return false;
        const uint32_t tick_pos = near_pos;
        // the tick kernel (dense or sparse: the same body)
        int32_t words[kFlowPlanWords];
        FlowPackPlan(planned, words);
        FlowUnpackPlan(words, p);
        for (int j = 0; j < n; ++j) {
            for (int c = 0; c < 2; ++c)
                if (j >= p.far[c].src && j < p.far[c].src + p.far[c].count) far_ring[(p.far[c].pos + (uint32_t)(j - p.far[c].src)) & mask] = far_in[j];
            near_ring[(tick_pos + (uint32_t)j) & mask] = near_in[j];
        }
        for (int i = 0; i < 2; ++i)
            if (p.spill[i])
                for (int j = 0; j < kFlowFrame; ++j) far_old[i * kFlowFrame + j] = far_ring[(p.spill_pos[i] + (uint32_t)j) & mask];
        if (!p.direct) {
            int64_t left[kFlowBlock], frames[2][kFlowFrame];
            for (int j = 0; j < p.left_count; ++j) left[j] = far_ring[(p.blk_pos0 + p.left_delta + (uint32_t)j) & mask];
            for (int f = 0; f < p.n_frames; ++f) {
                const FlowFrame &q = p.frame[f];
                if (!q.active) continue;
                for (int j = 0; j < kFlowFrame; ++j)
                    frames[f][j] = q.far_from_stream ? far_ring[(q.far_pos + (uint32_t)j) & mask] : far_old[q.old_idx * kFlowFrame + j];
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
                blk_far->push_back(p.direct ? far_ring[(x + p.far_delta) & mask] : far_frames[x & (kFlowFarFrameRing - 1)]);
                blk_near->push_back(near_ring[(p.near_base + x) & mask]);
                out_ring[x & mask] = kOutTagBase + blocks_done * kFlowBlock + t;
            }
        for (int f = 0; f < p.n_frames; ++f)
            for (int j = 0; j < kFlowFrame; ++j)
                out[f * kFlowFrame + j] = p.frame[f].active ? out_ring[(p.frame[f].out_pos + (uint32_t)j) & mask] : near_in[f * kFlowFrame + j];
        return true;
    }
};

}  // namespace

extern "C" {

// One session through n_ticks ticks of an object, idle with probability idle_percent per tick plus forced idle stretches
// (1, 2, 3 and >= 110 ticks; from the first ticks; from the first tick after the start-up phase).  pattern 0: the plain
// cadence (one call of 10 ms per tick); 1: 80 / 160 / split calls mixed, far-end underruns, out-of-range msInSndCardBuf,
// far-end bursts between ticks (also into idle ticks).  Returns -1 when every block input and output sample of every call
// agreed, else the first tick that differed; detail[0] = what (1 block count, 2 far block tags, 3 near block tags, 4 output,
// 6 a dense tick met a lagging session, 100 + field / 200 + field: FlowStateDefect refused the state after a tick / a burst),
// [1] blocks, [2] idle ticks, [3] longest idle stretch, [4] resyncs that moved samples, [5] samples moved, [6] dense ticks,
// [7] ticks nobody made, [8] idle ticks in the start-up phase, [9] idle stretches begun on the first tick after start-up,
// [10] idle ticks that replaced a two-block tick.
int64_t sim_sparse_fuzz(uint64_t seed, int fs, int n_ticks, int pattern, int idle_percent, uint32_t start_pos, int64_t *detail) {
    Rng rng{seed * 2654435761ull + 777};
    DeviceSide dev;
    dev.regs.v[F_FAR_RP] = dev.regs.v[F_FAR_WP] = (int32_t)start_pos;
    dev.regs.v[F_FRM_POS] = dev.regs.v[F_BLK_POS] = dev.regs.v[F_OUT_RP] = (int32_t)(start_pos * 3u);
    dev.obj.near_pos = start_pos * 80u;
    SessionFlow<int64_t> ref(kNone);
    ref.Init(fs);
    int64_t far_offered = 0, near_offered = 0, ref_blocks = 0;
    for (int i = 0; i < 11; ++i) detail[i] = 0;
    const auto state_defect = [&dev]() -> int {
        int32_t words[kFlowWords] = {0};
        for (int k = 0; k < kFlowFieldsUsed; ++k) words[k] = dev.regs.v[k];
        return FlowStateDefect(words);
    };
    int forced = seed % 4 == 1 ? rng.range(1, 3) : 0;                             // idle from the very first tick
    if (seed % 8 == 5) forced = rng.range(110, 130);
    int64_t stretch = 0;
    bool was_startup = true;
    for (int64_t tick = 0; tick < n_ticks; ++tick) {
        int n = fs == 16000 ? 160 : 80, ms = 40, flags = 0, extra = 0, extra_len = n;
        if (pattern == 1) {
            n = rng.chance(30) ? 80 : 160;
            ms = rng.range(0, 300);
            if (rng.chance(3)) ms = rng.chance(50) ? -300 : 700;
            if (rng.chance(25)) flags |= kFlowNoFarend;
            if (rng.chance(30)) flags |= kFlowSplitCalls;
            if (n != 160) flags &= ~kFlowSplitCalls;
            extra = rng.chance(20) ? rng.range(1, 4) : 0;
            extra_len = rng.chance(50) ? 80 : 160;
            if (rng.chance(1)) extra = rng.range(20, 60);
        }
        // who sits out
        if (forced == 0 && rng.chance(2)) {
            const int k = rng.range(0, 9);
            forced = k < 3 ? 1 : k < 5 ? 2 : k < 7 ? 3 : k < 9 ? rng.range(4, 12) : rng.range(110, 140);
        }
        const bool startup_now = dev.regs.v[F_EC_STARTUP] != 0;
        if (was_startup && !startup_now && forced == 0 && (seed & 1)) {         // the first tick after the start-up phase
            forced = rng.range(1, 3);
            detail[9]++;
        }
        was_startup = startup_now;
        bool idle = forced > 0 || rng.chance(idle_percent);
        if (forced > 0) --forced;
        const bool others_live = rng.chance(70), others_idle = rng.chance(50);
        if (extra > 0) {                                                        // far-end calls outside ticks: also ahead of an idle tick
            std::vector<int64_t> burst((size_t)extra * extra_len);
            for (size_t j = 0; j < burst.size(); ++j) burst[j] = far_offered + (int64_t)j;
            far_offered += (int64_t)burst.size();
            dev.BufferFarend(fs, extra_len, extra, burst.data());
            for (int c = 0; c < extra; ++c) ref.BufferFarend(burst.data() + (size_t)c * extra_len, (size_t)extra_len);
            if (const int field = state_defect()) {
                detail[0] = 200 + field;
                return tick;
            }
        }
        int64_t far_in[160], near_in[160], out_dev[160], out_ref[160];
        if (!idle) {
            for (int j = 0; j < n; ++j) { far_in[j] = far_offered + j; near_in[j] = (int64_t(1) << 32) + near_offered + j; }
            far_offered += n;
            near_offered += n;
        } else {                                                                // rows of an idle session hold anything
            for (int j = 0; j < n; ++j) far_in[j] = near_in[j] = -77;
            detail[2]++;
            detail[8] += startup_now;
            const uint32_t pending = (uint32_t)dev.regs.v[F_FRM_POS] - (uint32_t)dev.regs.v[F_BLK_POS];
            detail[10] += !startup_now && (int)pending + 80 * (n / 80) >= 2 * 64 + (n == 160 ? 64 : 0);
            ++stretch;
            if (stretch > detail[3]) detail[3] = stretch;
        }
        if (!idle) stretch = 0;
        std::vector<int64_t> dfar, dnear, rfar, rnear;
        for (int j = 0; j < 160; ++j) out_dev[j] = out_ref[j] = -5;
        const bool called = dev.Tick(fs, n, ms, flags, idle, others_live, others_idle, far_in, near_in, out_dev, &dfar, &dnear);
        if (const int field = state_defect()) {
            detail[0] = 100 + field;
            return tick;
        }
        if (dev.fault) {
            detail[0] = 6;
            return tick;
        }
        if (called != !idle) { detail[0] = 7; return tick; }
        if (!idle) {
            const int n_calls = (flags & kFlowSplitCalls) ? 2 : 1, len = n / n_calls;
            for (int c = 0; c < n_calls; ++c) {
                if (!(flags & kFlowNoFarend)) ref.BufferFarend(far_in + c * len, (size_t)len);
                (void)ref.Process(near_in + c * len, nullptr, out_ref + c * len, (size_t)len, (int16_t)ms,
                                  [&](const int64_t *fb, const int64_t *nb, const int64_t *, int64_t *ob, int nblk) {
                                      rfar.insert(rfar.end(), fb, fb + nblk * kFlowBlock);
                                      rnear.insert(rnear.end(), nb, nb + nblk * kFlowBlock);
                                      for (int j = 0; j < nblk * kFlowBlock; ++j) ob[j] = kOutTagBase + ref_blocks * kFlowBlock + j;
                                      ref_blocks += nblk;
                                      return true;
                                  });
            }
        }
        detail[1] = ref_blocks;
        detail[4] = dev.moves;
        detail[5] = dev.moved_samples;
        detail[6] = dev.dense_ticks;
        detail[7] = dev.deferred_ticks;
        int what = 0;
        if (dfar.size() != rfar.size()) what = 1;
        else if (dfar != rfar) what = 2;
        else if (dnear != rnear) what = 3;
        else if (memcmp(out_dev, out_ref, sizeof out_dev) != 0) what = 4;
        if (what) {
            detail[0] = what;
            return tick;
        }
    }
    return -1;
}

// FlowStateDefect of a freshly initialised session whose lag word is `lag`.
int sim_sparse_lag_defect(int32_t lag) {
    int32_t words[kFlowWords];
    FlowInit(words);
    words[F_NEAR_LAG] = lag;
    return FlowStateDefect(words);
}
int sim_sparse_lag_field(void) { return F_NEAR_LAG + 1; }
// n idle ticks of `n_samples` from lag 0.
int32_t sim_sparse_lag_after(int64_t ticks, int n_samples) {
    int32_t lag = 0;
    for (int64_t i = 0; i < ticks; ++i) lag = FlowIdleTick(lag, n_samples);
    return lag;
}

// FlowMoveNear on a ring of ring_len tags (tag = position before the move): count samples from [src, src + count) to
// [src + d, src + d + count).  Returns the number of destination samples that do not hold the tag of their source sample, plus
// the number of samples outside the destination that changed.
int sim_sparse_move_check(int ring_len, uint32_t src, uint32_t d, int count) {
    std::vector<int64_t> ring((size_t)ring_len), before;
    for (int i = 0; i < ring_len; ++i) ring[(size_t)i] = 1000 + i;
    before = ring;
    const uint32_t mask = (uint32_t)ring_len - 1u;
    const FlowNearMove m{count, src, src + d};
    FlowMoveNear(ring.data(), mask, m);
    int bad = 0;
    std::vector<char> is_dst((size_t)ring_len, 0);
    for (int k = 0; k < count; ++k) {
        const uint32_t to = (m.dst + (uint32_t)k) & mask;
        is_dst[to] = 1;
        bad += ring[to] != before[(m.src + (uint32_t)k) & mask];
    }
    for (int i = 0; i < ring_len; ++i) bad += !is_dst[(size_t)i] && ring[(size_t)i] != before[(size_t)i];
    return bad;
}

// The live list of a tick: the host half (FlowLiveBlockBases over the flags) and the device half as
// aecm_flow_plan_sparse_kernel runs it -- workgroups of kFlowPlanBlock lanes, wavefronts of 64, each live lane its own slot.
// list[n_sessions] is preset by the caller; returns the live count, or -1 - s when session s was given a slot outside the list.
int32_t sim_live_list(const uint8_t *flags, int32_t n_sessions, uint32_t *list) {
    const int blocks = (n_sessions + kFlowPlanBlock - 1) / kFlowPlanBlock;
    std::vector<uint32_t> bases((size_t)blocks);
    const int32_t live_count = FlowLiveBlockBases(flags, n_sessions, bases.data());
    for (int b = 0; b < blocks; ++b) {
        uint64_t ballots[kFlowPlanBlock / 64];
        uint32_t wave_counts[kFlowPlanBlock / 64];
        for (int w = 0; w < kFlowPlanBlock / 64; ++w) {
            ballots[w] = 0;
            for (int lane = 0; lane < 64; ++lane) {
                const int s = b * kFlowPlanBlock + w * 64 + lane;
                if (s < n_sessions && !(flags[s] & kFlowIdle)) ballots[w] |= uint64_t(1) << lane;
            }
            wave_counts[w] = (uint32_t)__builtin_popcountll(ballots[w]);
        }
        for (int w = 0; w < kFlowPlanBlock / 64; ++w)
            for (int lane = 0; lane < 64; ++lane) {
                if (!((ballots[w] >> lane) & 1)) continue;
                const uint32_t slot = FlowLiveSlot(bases[b], wave_counts, w, ballots[w], lane);
                if (slot >= (uint32_t)n_sessions) return -1 - (b * kFlowPlanBlock + w * 64 + lane);
                list[slot] = (uint32_t)(b * kFlowPlanBlock + w * 64 + lane);
            }
    }
    return live_count;
}

}  // extern "C"
