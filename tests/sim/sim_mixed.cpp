// TEST INFRASTRUCTURE: an OBJECT of sessions of both sampling rates and both call sizes (WebRtcAecmSessions_InitRates,
// AECM_SESSION_HALF_CALL) on sample TAGS -- the method of sim_sparse.cpp, with the whole object instead of one session of it.
// The device side is what the host's tick planner (aecm_tick_plan.h: check, plan, commit), the three planning
// kernels (aecm_flow_plan_kernel, aecm_flow_plan_sparse_kernel, aecm_flow_plan_mixed_kernel: FlowResync, FlowMoveNear, FlowTick,
// FlowTickMixed), the tick kernels' body (it appends ALL of a tick's near-end samples at the object's position, a half call's
// unconsumed second half included) and aecm_buffer_farend_kernel do; the reference side is one SessionFlow<T> per session
// (aecm_session_flow.h), initialised at that session's rate and called with that session's sizes.
// Built into tests/_build by tests/mixed_sim.py; with -DSIM_MIXED_MAIN a stand-alone program (for sanitizer runs).
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <memory>
#include <vector>

#include "aecm_flow_plan.h"
#include "aecm_ops.h"
#include "aecm_session_flow.h"
#include "aecm_tick_plan.h"

namespace {

using namespace aecm;

constexpr int64_t kRingLen = kFlowFarRing, kOutTagBase = int64_t(1) << 40, kNone = -1, kJunk = -77, kSentinel = -5;
constexpr int64_t kNearTagBase = int64_t(1) << 32, kCleanTagBase = int64_t(2) << 32;

struct Rng {
    uint64_t s;
    uint32_t next() {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        return (uint32_t)(s >> 33);
    }
    int range(int lo, int hi) { return lo + (int)(next() % (uint32_t)(hi - lo + 1)); }
    bool chance(int percent) { return (int)(next() % 100u) < percent; }
};

// One session's rows on the device, and its reference instance.
struct Session {
    int fs;
    FlowRegs regs;
    std::vector<int64_t> far_ring, near_ring, clean_ring, out_ring, far_frames, far_old;
    SessionFlow<int64_t> ref;
    int64_t far_offered = 0, near_offered = 0, blocks_done = 0, ref_blocks = 0;
    explicit Session(int rate)
        : fs(rate), far_ring(kRingLen, kNone), near_ring(kRingLen, kNone), clean_ring(kRingLen, kNone), out_ring(kRingLen, kNone),
          far_frames(kFlowFarFrameRing, kNone), far_old(2 * kFlowFrame, kNone), ref(kNone) {
        int32_t words[kFlowWords];
        FlowInit(words);
        for (int k = 0; k < kFlowFieldsUsed; ++k) regs.v[k] = words[k];
        ref.Init(rate);
    }
    int StateDefect() const {
        int32_t words[kFlowWords] = {0};
        for (int k = 0; k < kFlowFieldsUsed; ++k) words[k] = regs.v[k];
        return FlowStateDefect(words);
    }
    // aecm_buffer_farend_kernel: mult is the SESSION's
    void BufferFarend(int len, int calls, const int64_t *far_in) {
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
    // The tick kernels' body (aecm_tick_flow_body.inc) for this session: n = the OBJECT's tick, all of it appended.
    void TickBody(const FlowPlan &planned, bool has_clean, int n, uint32_t tick_pos, const int64_t *far_in, const int64_t *near_in, const int64_t *clean_in,
                  int64_t *out, std::vector<int64_t> *blk_far, std::vector<int64_t> *blk_near, std::vector<int64_t> *blk_clean) {
        const int64_t mask = kRingLen - 1;
        int32_t words[kFlowPlanWords];
        FlowPlan p;
        FlowPackPlan(planned, words);
        FlowUnpackPlan(words, p);
        for (int j = 0; j < n; ++j) {
            for (int c = 0; c < 2; ++c)
                if (j >= p.far[c].src && j < p.far[c].src + p.far[c].count) far_ring[(p.far[c].pos + (uint32_t)(j - p.far[c].src)) & mask] = far_in[j];
            near_ring[(tick_pos + (uint32_t)j) & mask] = near_in[j];
            if (has_clean) clean_ring[(tick_pos + (uint32_t)j) & mask] = clean_in[j];
        }
        for (int i = 0; i < 2; ++i)
            if (p.spill[i])
                for (int j = 0; j < kFlowFrame; ++j) far_old[i * kFlowFrame + j] = far_ring[(p.spill_pos[i] + (uint32_t)j) & mask];
        if (!p.direct && (p.frame[0].active | p.frame[1].active)) {
            int64_t left[kFlowBlock], frames[2][kFlowFrame];
            for (int j = 0; j < p.left_count; ++j) left[j] = far_ring[(p.blk_pos0 + p.left_delta + (uint32_t)j) & mask];
            for (int f = 0; f < 2; ++f) {
                const FlowFrame &q = p.frame[f];
                if (!q.active) continue;
                for (int j = 0; j < kFlowFrame; ++j)
                    frames[f][j] = q.far_from_stream ? far_ring[(q.far_pos + (uint32_t)j) & mask] : far_old[q.old_idx * kFlowFrame + j];
            }
            for (int j = 0; j < p.left_count; ++j) far_frames[(p.blk_pos0 + (uint32_t)j) & (kFlowFarFrameRing - 1)] = left[j];
            for (int f = 0; f < 2; ++f) {
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
                if (has_clean) blk_clean->push_back(clean_ring[(p.near_base + x) & mask]);
                out_ring[x & mask] = kOutTagBase + blocks_done * kFlowBlock + t;
            }
        const int64_t *pass = has_clean ? clean_in : near_in;
        for (int f = 0; f < p.n_frames; ++f)
            for (int j = 0; j < kFlowFrame; ++j)
                out[f * kFlowFrame + j] = p.frame[f].active ? out_ring[(p.frame[f].out_pos + (uint32_t)j) & mask] : pass[f * kFlowFrame + j];
    }
};

enum Detail : int {
    D_WHAT = 0, D_SESSION, D_BLOCKS, D_HALF_CALLS, D_RESYNCS, D_MOVED, D_MIXED_TICKS, D_SPARSE_TICKS, D_DENSE_TICKS, D_NOBODY_TICKS, D_IDLE, D_BURSTS,
    D_SPLIT_CALLS, D_FULL_8K, D_HALF_16K, D_WARNINGS, D_MAX_LAG, kDetail
};

}  // namespace

extern "C" {

int sim_mixed_detail_words(void) { return kDetail; }

// An object of n_sessions sessions through n_ticks ticks.  rates_mode 0: both rates at random (the object's own rate by seed);
// 1: every session at the object's rate AND nobody ever makes a half call (the uniform object: must route as before);
// 2: every session at the object's rate, half calls allowed.  Per tick the object's size is 160 (mostly) or 80; per session and
// tick at random: idle, NO_FAREND, a half call / a full call / (16 kHz) split calls, msInSndCardBuf anywhere, far-end bursts
// with per-session call counts before some ticks.  start_pos: the object's near position at the first tick.
// Returns -1 when everything agreed, else the first tick that did not; detail[D_WHAT]: 1 block count, 2 far block tags, 3 near
// block tags, 4 clean block tags, 5 output tags, 6 code, 7 out row written past the call, 8 a planning kernel met a session it
// cannot plan (the host's routing is wrong), 9 lag no multiple of 80 below the period, 10 the uniform object took a mixed
// planning launch, 100 + field / 200 + field: FlowStateDefect after a tick / a burst; detail[D_SESSION] = the session.
int64_t sim_mixed_fuzz(uint64_t seed, int n_sessions, int n_ticks, int rates_mode, int idle_percent, uint32_t start_pos, int64_t *detail) {
    Rng rng{seed * 2654435761ull + 4242};
    for (int i = 0; i < kDetail; ++i) detail[i] = 0;
    const int obj_fs = (seed & 1) ? 16000 : 8000;
    const bool has_clean = (seed & 2) != 0;
    std::vector<std::unique_ptr<Session>> ss;
    TickObject obj;                                                             // what the host keeps for the object
    obj.Init(n_sessions, obj_fs);
    for (int s = 0; s < n_sessions; ++s) {
        const int fs = rates_mode == 0 ? (rng.chance(50) ? 16000 : 8000) : obj_fs;
        obj.SetRate(s, fs);
        ss.emplace_back(new Session(fs));
        const uint32_t p0 = rng.chance(50) ? 0u : rng.next() * 7u;                 // positions that wrap
        ss[s]->regs.v[F_FAR_RP] = ss[s]->regs.v[F_FAR_WP] = (int32_t)p0;
        ss[s]->regs.v[F_FRM_POS] = ss[s]->regs.v[F_BLK_POS] = ss[s]->regs.v[F_OUT_RP] = (int32_t)(p0 * 3u);
    }
    obj.near_pos = start_pos;
    std::vector<uint8_t> flags((size_t)n_sessions), calls((size_t)n_sessions);
    std::vector<int> ms((size_t)n_sessions);
    std::vector<uint32_t> bases_ref(obj.live_bases.size());
    std::vector<int16_t> ms16((size_t)n_sessions);
    std::vector<int32_t> codes((size_t)n_sessions);
    const auto fail = [&](int what, int s) { detail[D_WHAT] = what; detail[D_SESSION] = s; };
    for (int64_t tick = 0; tick < n_ticks; ++tick) {
        const int n = rng.chance(85) ? 160 : 80;
        // ---- a far-end burst before the tick (WebRtcAecmSessions_BufferFarend with calls_host): one call size for the object
        if (rng.chance(15)) {
            const int len = rng.chance(50) ? 80 : 160, max_calls = rng.chance(5) ? rng.range(20, 60) : rng.range(1, 4);
            for (int s = 0; s < n_sessions; ++s) calls[s] = (uint8_t)(rng.chance(40) ? 0 : rng.range(1, max_calls));
            for (int s = 0; s < n_sessions; ++s) {
                if (!calls[s]) continue;
                Session &q = *ss[s];
                std::vector<int64_t> burst((size_t)calls[s] * len);
                for (size_t j = 0; j < burst.size(); ++j) burst[j] = q.far_offered + (int64_t)j;
                q.far_offered += (int64_t)burst.size();
                q.BufferFarend(len, calls[s], burst.data());
                for (int c = 0; c < calls[s]; ++c) q.ref.BufferFarend(burst.data() + (size_t)c * len, (size_t)len);
                if (const int field = q.StateDefect()) { fail(200 + field, s); return tick; }
                detail[D_BURSTS]++;
            }
        }
        // ---- the tick's flags
        const bool all_idle = rng.chance(3);
        for (int s = 0; s < n_sessions; ++s) {
            uint8_t f = 0;
            if (rng.chance(20)) f |= kFlowNoFarend;
            if (n == 160) {
                const int pick = rng.range(0, 99);
                if (rates_mode != 1 && pick < (ss[s]->fs == 8000 ? 70 : 30)) f |= kFlowHalfCall;
                else if (ss[s]->fs == 16000 && pick >= 75) f |= kFlowSplitCalls;
            }
            if (all_idle || rng.chance(idle_percent)) f = (uint8_t)(kFlowIdle | (rng.next() & 11u));      // an idle session's other bits mean nothing
            flags[s] = f;
            ms[s] = rng.range(0, 300);
            if (rng.chance(4)) ms[s] = rng.chance(50) ? -300 : 700;
        }
        // ---- the host (aecm_tick_plan.h): check, plan, commit
        TickArgs args;
        args.flags_per_session = flags.data();
        args.n = n;
        args.has_clean = has_clean;
        uint32_t tick_pos;
        const TickPlan plan = obj.Tick(args, &tick_pos);
        if (plan.code || plan.live != FlowLiveBlockBases(flags.data(), n_sessions, bases_ref.data()) || obj.live_bases != bases_ref) {
            fail(11, -1);
            return tick;
        }
        const bool mixed_plan = plan.mixed_plan;
        const FlowTickRoute route = plan.route;
        for (int s = 0; s < n_sessions; ++s) ms16[(size_t)s] = (int16_t)ms[s];
        (void)TickCodes(ms16.data(), 0, flags.data(), n_sessions, codes.data());
        if (!route.launch) {
            detail[D_NOBODY_TICKS]++;
            continue;
        }
        if (rates_mode == 1 && mixed_plan) { fail(10, -1); return tick; }
        detail[mixed_plan ? D_MIXED_TICKS : route.sparse_plan ? D_SPARSE_TICKS : D_DENSE_TICKS]++;
        // ---- the device: planning launch (a lane per session), tick launch (the sessions that call), per session
        for (int s = 0; s < n_sessions; ++s) {
            Session &q = *ss[s];
            const bool idle = (flags[s] & kFlowIdle) != 0, half = !idle && (flags[s] & kFlowHalfCall) != 0;
            FlowPlan planned;
            if (!route.sparse_plan) {                                       // aecm_flow_plan_kernel: no lags, no idle lanes, the object's rate
                if (q.regs.v[F_NEAR_LAG] != 0 || idle || half || q.fs != obj_fs) { fail(8, s); return tick; }
                FlowRegs r = q.regs;
                r.v[F_NEAR_LAG] = 0x5a5a5a5a;                               // (not loaded)
                FlowTick(r, obj_fs, n, ms[s], flags[s], tick_pos, planned);
                for (int k = 0; k < kFlowTickFields; ++k) q.regs.v[k] = r.v[k];
            } else if (idle) {                                              // an idle lane of the sparse / mixed planning kernel
                q.regs.v[F_NEAR_LAG] = FlowIdleTick(FlowIdleTick(q.regs.v[F_NEAR_LAG], route.deferred_lag), n);
            } else {
                if (!mixed_plan && (half || q.fs != obj_fs)) { fail(8, s); return tick; }
                q.regs.v[F_NEAR_LAG] = FlowIdleTick(q.regs.v[F_NEAR_LAG], route.deferred_lag);
                if (q.regs.v[F_NEAR_LAG] != 0) {
                    FlowNearMove m;
                    FlowResync(q.regs, tick_pos, m);
                    FlowMoveNear(q.near_ring.data(), (uint32_t)(kRingLen - 1), m);
                    if (has_clean) FlowMoveNear(q.clean_ring.data(), (uint32_t)(kRingLen - 1), m);
                    detail[D_RESYNCS] += m.count > 0;
                    detail[D_MOVED] += m.count;
                }
                if (mixed_plan) FlowTickMixed(q.regs, q.fs, n, ms[s], flags[s], tick_pos, planned);
                else FlowTick(q.regs, obj_fs, n, ms[s], flags[s], tick_pos, planned);
            }
            if (const int field = q.StateDefect()) { fail(100 + field, s); return tick; }
            const int32_t l = q.regs.v[F_NEAR_LAG];
            if (l < 0 || l >= kFlowLagPeriod || l % kFlowFrame != 0) { fail(9, s); return tick; }
            if (l > detail[D_MAX_LAG]) detail[D_MAX_LAG] = l;
            if (idle) {
                detail[D_IDLE]++;
                continue;
            }
            // the session's rows: what its call consumes carries tags, the rest of the tick's row junk that must never show
            const int n_eff = half ? 80 : n, n_calls = (flags[s] & kFlowSplitCalls) ? 2 : 1, len = n_eff / n_calls;
            int64_t far_in[160], near_in[160], clean_in[160], out_dev[160], out_ref[160];
            for (int j = 0; j < 160; ++j) {
                const bool mine = j < n_eff;
                far_in[j] = mine ? q.far_offered + j : kJunk;
                near_in[j] = mine ? kNearTagBase + q.near_offered + j : kJunk;
                clean_in[j] = mine ? kCleanTagBase + q.near_offered + j : kJunk;
                out_dev[j] = out_ref[j] = kSentinel;
            }
            q.far_offered += n_eff;                                         // (a NO_FAREND session's far row is never read: the tags are simply skipped)
            q.near_offered += n_eff;
            std::vector<int64_t> dfar, dnear, dclean, rfar, rnear, rclean;
            q.TickBody(planned, has_clean, n, tick_pos, far_in, near_in, clean_in, out_dev, &dfar, &dnear, &dclean);
            const int32_t dev_code = codes[(size_t)s];                      // the host's
            int32_t ref_code = 0;
            for (int c = 0; c < n_calls; ++c) {
                if (!(flags[s] & kFlowNoFarend)) q.ref.BufferFarend(far_in + c * len, (size_t)len);
                const int32_t rc = q.ref.Process(near_in + c * len, has_clean ? clean_in + c * len : nullptr, out_ref + c * len, (size_t)len, (int16_t)ms[s],
                                                 [&](const int64_t *fb, const int64_t *nb, const int64_t *cb, int64_t *ob, int nblk) {
                                                     rfar.insert(rfar.end(), fb, fb + nblk * kFlowBlock);
                                                     rnear.insert(rnear.end(), nb, nb + nblk * kFlowBlock);
                                                     if (cb) rclean.insert(rclean.end(), cb, cb + nblk * kFlowBlock);
                                                     for (int j = 0; j < nblk * kFlowBlock; ++j) ob[j] = kOutTagBase + q.ref_blocks * kFlowBlock + j;
                                                     q.ref_blocks += nblk;
                                                     return true;
                                                 });
                ref_code = ref_code ? ref_code : rc;
            }
            detail[D_BLOCKS] += (int64_t)rfar.size() / kFlowBlock;
            detail[D_HALF_CALLS] += half;
            detail[D_SPLIT_CALLS] += n_calls == 2;
            detail[D_FULL_8K] += q.fs == 8000 && n_eff == 160;
            detail[D_HALF_16K] += q.fs == 16000 && half;
            detail[D_WARNINGS] += dev_code != 0;
            int what = 0;
            if (dfar.size() != rfar.size()) what = 1;
            else if (dfar != rfar) what = 2;
            else if (dnear != rnear) what = 3;
            else if (dclean != rclean) what = 4;
            else if (memcmp(out_dev, out_ref, sizeof(int64_t) * (size_t)n_eff) != 0) what = 5;
            else if (dev_code != ref_code) what = 6;
            for (int j = n_eff; j < 160 && !what; ++j)
                if (out_dev[j] != kSentinel) what = 7;
            if (what) { fail(what, s); return tick; }
        }
    }
    return -1;
}

// FlowRouteTickMixed without half calls and without sessions of another rate against FlowRouteTick, on random ticks (live counts
// from nobody to everybody, both tick sizes, the diagnostics switch): the same route, field by field, the same object state after
// every tick, never the mixed planning launch.  Returns -1 or the first tick that differed.
int64_t sim_mixed_route_uniform(uint64_t seed, int n_sessions, int n_ticks) {
    Rng rng{seed * 0x9e3779b97f4a7c15ull + 1};
    FlowObjectLag a, b;
    for (int64_t tick = 0; tick < n_ticks; ++tick) {
        const int k = rng.range(0, 9);
        const int32_t live = k < 2 ? 0 : k < 6 ? n_sessions : rng.range(0, n_sessions);
        const int n = rng.chance(50) ? 80 : 160;
        const bool force = rng.chance(10);
        bool mixed = true;
        const FlowTickRoute ra = FlowRouteTick(a, live, n_sessions, n, force);
        const FlowTickRoute rb = FlowRouteTickMixed(b, live, n_sessions, n, force, false, false, &mixed);
        if (mixed || ra.launch != rb.launch || ra.sparse_plan != rb.sparse_plan || ra.sparse_tick != rb.sparse_tick || ra.deferred_lag != rb.deferred_lag ||
            a.deferred_lag != b.deferred_lag || a.may_lag != b.may_lag)
            return tick;
    }
    return -1;
}

// One tick of an object of n_sessions of which the first `live` call (half_calls: the first of them makes a half call; other_rates:
// session 0 runs at another rate than the object), through the host's planner: out[0..5] = launch, sparse_plan, sparse_tick,
// deferred_lag, mixed_plan, may_lag after; the object's lags go in and out through lag_state[2] = {deferred_lag, may_lag}.
void sim_mixed_route(int32_t *lag_state, int32_t live, int32_t n_sessions, int n, int force_sparse, int half_calls, int other_rates, int32_t *out) {
    TickObject o;
    o.Init(n_sessions, 16000);
    o.lag.deferred_lag = lag_state[0];
    o.lag.may_lag = lag_state[1] != 0;
    o.force_sparse = force_sparse != 0;
    if (other_rates) o.SetRate(0, 8000);
    std::vector<uint8_t> flags((size_t)n_sessions, (uint8_t)kFlowIdle);
    for (int32_t s = 0; s < live; ++s) flags[(size_t)s] = s == 0 && half_calls ? kFlowHalfCall : 0;
    TickArgs a;
    a.flags_per_session = flags.data();
    a.n = n;
    const TickPlan p = o.Tick(a);
    out[0] = p.route.launch; out[1] = p.route.sparse_plan; out[2] = p.route.sparse_tick; out[3] = p.route.deferred_lag; out[4] = p.mixed_plan; out[5] = o.lag.may_lag;
    lag_state[0] = o.lag.deferred_lag;
    lag_state[1] = o.lag.may_lag;
}

// The host's check of a tick's flags (aecm_tick_plan.h): 0 = accepted, 1 = AECM_BAD_PARAMETER_ERROR.  Also hands back what the pass
// found: result[0] = live sessions, [1] = OR of the calling sessions' bytes, [2] = FlowLiveBlockBases agrees (count and every base).
int sim_mixed_check_flags(const uint8_t *flags, int32_t n_sessions, int n, int32_t *result) {
    TickObject o;
    o.Init(n_sessions, 16000);
    std::vector<uint32_t> ref(o.live_bases.size());
    TickArgs a;
    a.flags_per_session = flags;
    a.n = n;
    const TickPlan p = o.Plan(a);
    result[0] = p.live;
    result[1] = p.any;
    result[2] = p.live == FlowLiveBlockBases(flags, n_sessions, ref.data()) && o.live_bases == ref;
    return p.code ? 1 : 0;
}

}  // extern "C"

#if defined(SIM_MIXED_MAIN)
// Stand-alone: the fuzz and the routing check over a few seeds (what tests/test_mixed_sessions.py runs through the shared library).
int main() {
    int64_t detail[kDetail];
    const uint32_t starts[3] = {0u, 0xffffffffu - 0xffffffffu % 80u - 800u, (uint32_t)kFlowLagPeriod * 1000u - 400u};
    // tests/mixed_sim.py: FUZZ_PLAN -- 24 seeds with both rates, 12 uniform with half calls, 12 uniform without; every mode from
    // every start position
    const int plan[3][3] = {{0, 0, 24}, {2, 24, 12}, {1, 36, 12}};
    for (const auto &m : plan)
        for (uint64_t seed = (uint64_t)m[1]; seed < (uint64_t)(m[1] + m[2]); ++seed) {
            const int64_t t = sim_mixed_fuzz(seed, 6, 600, m[0], seed % 4 == 3 ? 30 : 10, starts[((seed - (uint64_t)m[1]) / 4) % 3], detail);
            if (t != -1) {
                printf("seed %llu: tick %lld what %lld session %lld\n", (unsigned long long)seed, (long long)t, (long long)detail[0], (long long)detail[1]);
                return 1;
            }
            if (sim_mixed_route_uniform(seed, 9, 5000) != -1) return 2;
        }
    printf("ok\n");
    return 0;
}
#endif
