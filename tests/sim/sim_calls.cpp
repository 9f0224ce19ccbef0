// TEST INFRASTRUCTURE: ticks of K call pairs (WebRtcAecmSessions_TickCalls) on sample TAGS -- the method of sim_flow.cpp and
// sim_sparse.cpp.  The device side is what the host's tick planner (calls > 1), aecm_flow_plan_calls_kernel and
// aecm_tick_calls_kernel (webrtc_aecm_amd/csrc/aecm_tick_calls_kernels.hip) do for ONE session of an object, in the kernel's own
// order per call -- spill, far framing (fresh samples from call c's piece of the input row, everything older from the ring),
// append, blocks, output frames -- on the rows of sim_sparse.cpp's device model, so that K-call ticks, ordinary ticks, bursts
// and idle ticks mix on one object.  It is compared with
//   - the reference side, SessionFlow<T> (aecm_session_flow.h) called K times: every block input and every output sample;
//   - the existing device model (sim_sparse.cpp: DeviceSide) ticked K times with ordinary ticks: the state words after every tick.
// Stand-alone too (main below): g++ -fsanitize=address,undefined tests/sim/sim_calls.cpp -Iwebrtc_aecm_amd/csrc && ./a.out
#include "sim_sparse.cpp"      // the device model of ordinary / sparse ticks and bursts (its anonymous namespace: this unit's too)

#include <stdio.h>

namespace {

struct CallsCounters {
    int64_t calls_ticks = 0, nondirect_later = 0, spill_later = 0, startup_end_later = 0, stuffing_later = 0, no_block_calls = 0, resyncs = 0,
            spill_first = 0;
    int state_defect = 0;          // FlowStateDefect of a state between two calls (1-based field), 0: none
    int last_spill_call = -1, last_spill_row = -1;
};

struct CallsSide : DeviceSide {
    // One tick of K call pairs.  far_in / near_in: calls * n tags; out: calls * n.  Returns false when the session made no call.
    bool TickCalls(int fs, int n, int calls, int ms, int flags, bool idle, bool others_live, bool others_idle, const int64_t *far_in,
                   const int64_t *near_in, int64_t *out, std::vector<int64_t> *blk_far, std::vector<int64_t> *blk_near, CallsCounters &cnt) {
        const int64_t mask = kRingLen - 1;
        const int span = calls * n;
        uint32_t tick_pos;
        const TickPlan plan = HostTick(n, calls, flags, idle, others_live, others_idle, &tick_pos);
        const FlowTickRoute &route = plan.route;
        if (!route.launch) {
            ++deferred_ticks;
            return false;
        }
        // the host is told the whole tick's samples, and a K-call tick always goes by the live list
        if (plan.span != span || plan.family != kTickFamily_calls || !route.sparse_plan || !route.sparse_tick) fault = 2;
        // aecm_flow_plan_calls_kernel
        if (idle) {
            regs.v[F_NEAR_LAG] = FlowIdleTick(FlowIdleTick(regs.v[F_NEAR_LAG], route.deferred_lag), span);
            return false;
        }
        regs.v[F_NEAR_LAG] = FlowIdleTick(regs.v[F_NEAR_LAG], route.deferred_lag);
        if (regs.v[F_NEAR_LAG] != 0) {
            FlowNearMove m;
            FlowResync(regs, tick_pos, m);
            FlowMoveNear(near_ring.data(), (uint32_t)mask, m);
            moves += m.count > 0;
            moved_samples += m.count;
            ++cnt.resyncs;
        }
        int32_t words[kFlowMaxTickCalls][kFlowPlanWords];
        bool startup_before = regs.v[F_EC_STARTUP] != 0;
        uint32_t out_rp = (uint32_t)regs.v[F_OUT_RP];
        FlowTickCalls(regs, fs, n, calls, ms, flags, tick_pos, [&](int c, const FlowPlan &p) {
            FlowPackPlan(p, words[c]);
            int32_t w[kFlowWords] = {0};
            for (int k = 0; k < kFlowFieldsUsed; ++k) w[k] = regs.v[k];
            if (const int field = FlowStateDefect(w)) cnt.state_defect = cnt.state_defect ? cnt.state_defect : field;
            const bool startup_now = regs.v[F_EC_STARTUP] != 0;
            if (c > 0 && startup_before && !startup_now) ++cnt.startup_end_later;
            startup_before = startup_now;
            for (int f = 0; f < p.n_frames; ++f) {
                if (!p.frame[f].active) continue;
                if (c > 0 && p.frame[f].out_pos != out_rp) ++cnt.stuffing_later;
                out_rp = p.frame[f].out_pos + (uint32_t)kFlowFrame;
            }
        });
        ++cnt.calls_ticks;
        // aecm_tick_calls_kernel
        for (int c = 0; c < calls; ++c) {
            FlowPlan p;
            FlowUnpackPlan(words[c], p);
            const int64_t *fin = far_in + c * n, *nin = near_in + c * n;
            const uint32_t npos = tick_pos + (uint32_t)(c * n);
            if (p.spill[0] | p.spill[1]) {
                if (c > 0) ++cnt.spill_later; else ++cnt.spill_first;
                cnt.last_spill_call = c;
                cnt.last_spill_row = p.spill[1] ? 1 : 0;
            }
            for (int i = 0; i < 2; ++i)
                if (p.spill[i])
                    for (int j = 0; j < kFlowFrame; ++j) far_old[i * kFlowFrame + j] = far_ring[(p.spill_pos[i] + (uint32_t)j) & mask];
            const bool active = p.frame[0].active | p.frame[1].active;
            if (c > 0 && active && !p.direct) ++cnt.nondirect_later;
            if (!p.direct && active) {
                const auto far_stream = [&](uint32_t q) -> int64_t {
                    const int r0 = (int)(q - p.far[0].pos);
                    return r0 >= 0 && r0 < p.far[0].count ? fin[r0] : far_ring[q & mask];
                };
                int64_t left[kFlowBlock], frames[2][kFlowFrame];
                for (int j = 0; j < p.left_count; ++j) left[j] = far_ring[(p.blk_pos0 + p.left_delta + (uint32_t)j) & mask];
                for (int f = 0; f < 2; ++f) {
                    const FlowFrame &q = p.frame[f];
                    if (!q.active) continue;
                    for (int j = 0; j < kFlowFrame; ++j) frames[f][j] = q.far_from_stream ? far_stream(q.far_pos + (uint32_t)j) : far_old[q.old_idx * kFlowFrame + j];
                }
                for (int j = 0; j < p.left_count; ++j) far_frames[(p.blk_pos0 + (uint32_t)j) & (kFlowFarFrameRing - 1)] = left[j];
                for (int f = 0; f < 2; ++f) {
                    const FlowFrame &q = p.frame[f];
                    if (!q.active) continue;
                    for (int j = 0; j < kFlowFrame; ++j) far_frames[(q.frm_pos + (uint32_t)j) & (kFlowFarFrameRing - 1)] = frames[f][j];
                }
            }
            // append (TickBlockIo::ready, or the branch of a call without blocks)
            for (int j = 0; j < n; ++j) {
                if (j < p.far[0].count) far_ring[(p.far[0].pos + (uint32_t)j) & mask] = fin[j];
                near_ring[(npos + (uint32_t)j) & mask] = nin[j];
            }
            if (p.n_blocks == 0) ++cnt.no_block_calls;
            for (int b = 0; b < p.n_blocks; ++b, ++blocks_done)
                for (int t = 0; t < kFlowBlock; ++t) {
                    const uint32_t x = p.blk_pos0 + (uint32_t)(b * kFlowBlock + t);
                    blk_far->push_back(p.direct ? far_ring[(x + p.far_delta) & mask] : far_frames[x & (kFlowFarFrameRing - 1)]);
                    blk_near->push_back(near_ring[(p.near_base + x) & mask]);
                    out_ring[x & mask] = kOutTagBase + blocks_done * kFlowBlock + t;
                }
            for (int f = 0; f < p.n_frames; ++f)
                for (int j = 0; j < kFlowFrame; ++j)
                    out[c * n + f * kFlowFrame + j] = p.frame[f].active ? out_ring[(p.frame[f].out_pos + (uint32_t)j) & mask] : nin[f * kFlowFrame + j];
        }
        return true;
    }
};

template <class D>
void StartAt(D &dev, uint32_t start_pos) {
    dev.regs.v[F_FAR_RP] = dev.regs.v[F_FAR_WP] = (int32_t)start_pos;
    dev.regs.v[F_FRM_POS] = dev.regs.v[F_BLK_POS] = dev.regs.v[F_OUT_RP] = (int32_t)(start_pos * 3u);
    dev.obj.near_pos = start_pos * 80u;
}

}  // namespace

extern "C" {

// One session through n_ticks ticks of an object on which K-call ticks (K drawn per tick from 1 .. 6; K == 1 is the ordinary
// tick, as on the host), ordinary ticks (80 / 160 / split calls), far-end bursts (also into idle ticks), underruns, idle ticks
// and stretches (some longer than the ring), ticks nobody makes and msInSndCardBuf jumps mix; the call size n changes in
// stretches, so that runs of more than 98 calls of 80 samples occur.  Returns -1 when everything agreed, else the first tick that
// did not; detail[0] = what (1 block count, 2 far block tags, 3 near block tags, 4 output, 5 the state words differ from the twin's
// (detail[12] = field), 6 a dense tick met a lagging session, 7 called / idle mismatch, 100 + field: FlowStateDefect refused a
// state, also one BETWEEN two calls), [1] blocks, [2] K-call ticks, [3] non-direct calls at c > 0, [4] spills at c > 0, [5]
// start-up phases that ended at c > 0, [6] stuffing frames at c > 0, [7] calls without blocks, [8] idle ticks, [9] longest idle
// stretch in samples, [10] ticks nobody made, [11] resyncs in K-call ticks, [12] see 5, [13] ordinary ticks, [14] bursts.
int64_t sim_calls_fuzz(uint64_t seed, int fs, int n_ticks, uint32_t start_pos, int64_t *detail) {
    Rng rng{seed * 2654435761ull + 4242};
    CallsSide dev;
    DeviceSide twin;
    StartAt(dev, start_pos);
    StartAt(twin, start_pos);
    SessionFlow<int64_t> ref(kNone);
    ref.Init(fs);
    CallsCounters cnt;
    int64_t far_offered = 0, near_offered = 0, ref_blocks = 0, stretch_samples = 0;
    for (int i = 0; i < 15; ++i) detail[i] = 0;
    const auto state_defect = [](const DeviceSide &d) -> int {
        int32_t words[kFlowWords] = {0};
        for (int k = 0; k < kFlowFieldsUsed; ++k) words[k] = d.regs.v[k];
        return FlowStateDefect(words);
    };
    int forced = seed % 4 == 1 ? rng.range(1, 3) : 0, n = rng.chance(50) ? 80 : 160, n_left = 0, ms = 40;
    for (int64_t tick = 0; tick < n_ticks; ++tick) {
        if (n_left-- <= 0) {                                                    // the call size changes in stretches
            n = rng.chance(50) ? 80 : 160;
            n_left = rng.range(5, 60);
        }
        const int calls = rng.range(1, kFlowMaxTickCalls);
        const bool ordinary = calls == 1 || rng.chance(20);                     // an ordinary tick (on the host: calls == 1 IS one)
        int flags = 0, extra = 0, extra_len = n;
        if (rng.chance(10)) ms = rng.chance(50) ? rng.range(0, 60) : rng.range(250, 400);      // jumps that move the read pointer
        else if (rng.chance(30)) ms += rng.range(-10, 10);
        int ms_now = ms;
        if (rng.chance(3)) ms_now = rng.chance(50) ? -300 : 700;
        if (rng.chance(20)) flags |= kFlowNoFarend;
        if (ordinary && n == 160 && rng.chance(30)) flags |= kFlowSplitCalls;
        if (rng.chance(15)) { extra = rng.range(1, 4); extra_len = rng.chance(50) ? 80 : 160; }
        if (rng.chance(1)) extra = rng.range(20, 60);
        if (forced == 0 && rng.chance(2)) {
            const int k = rng.range(0, 9);
            forced = k < 3 ? 1 : k < 5 ? 2 : k < 7 ? 3 : k < 9 ? rng.range(4, 12) : rng.range(20, 40);      // (x up to 960 samples: longer than the ring)
        }
        const bool idle = forced > 0 || rng.chance(10);
        if (forced > 0) --forced;
        const bool others_live = rng.chance(70), others_idle = rng.chance(50);
        if (extra > 0) {
            std::vector<int64_t> burst((size_t)extra * extra_len);
            for (size_t j = 0; j < burst.size(); ++j) burst[j] = far_offered + (int64_t)j;
            far_offered += (int64_t)burst.size();
            dev.BufferFarend(fs, extra_len, extra, burst.data());
            twin.BufferFarend(fs, extra_len, extra, burst.data());
            for (int c = 0; c < extra; ++c) ref.BufferFarend(burst.data() + (size_t)c * extra_len, (size_t)extra_len);
            detail[14]++;
        }
        const int k_calls = ordinary ? 1 : calls, span = k_calls * n;
        int64_t far_in[kFlowMaxTickCalls * 160], near_in[kFlowMaxTickCalls * 160], out_dev[kFlowMaxTickCalls * 160], out_twin[kFlowMaxTickCalls * 160],
            out_ref[kFlowMaxTickCalls * 160];
        if (!idle) {
            for (int j = 0; j < span; ++j) { far_in[j] = far_offered + j; near_in[j] = (int64_t(1) << 32) + near_offered + j; }
            far_offered += span;
            near_offered += span;
            stretch_samples = 0;
        } else {
            for (int j = 0; j < span; ++j) far_in[j] = near_in[j] = -77;
            detail[8]++;
            stretch_samples += span;
            if (stretch_samples > detail[9]) detail[9] = stretch_samples;
        }
        if (idle && !others_live) detail[10]++;
        std::vector<int64_t> dfar, dnear, tfar, tnear, rfar, rnear;
        for (int j = 0; j < kFlowMaxTickCalls * 160; ++j) out_dev[j] = out_twin[j] = out_ref[j] = -5;
        bool called;
        if (ordinary) {
            called = dev.Tick(fs, n, ms_now, flags, idle, others_live, others_idle, far_in, near_in, out_dev, &dfar, &dnear);
            detail[13]++;
        } else {
            called = dev.TickCalls(fs, n, calls, ms_now, flags, idle, others_live, others_idle, far_in, near_in, out_dev, &dfar, &dnear, cnt);
        }
        for (int c = 0; c < k_calls; ++c)      // the twin: K ordinary ticks on the same rows
            (void)twin.Tick(fs, n, ms_now, flags, idle, others_live, others_idle, far_in + c * n, near_in + c * n, out_twin + c * n, &tfar, &tnear);
        detail[1] = ref_blocks;
        detail[2] = cnt.calls_ticks;
        detail[3] = cnt.nondirect_later;
        detail[4] = cnt.spill_later;
        detail[5] = cnt.startup_end_later;
        detail[6] = cnt.stuffing_later;
        detail[7] = cnt.no_block_calls;
        detail[11] = cnt.resyncs;
        int what = 0;
        if (const int field = cnt.state_defect ? cnt.state_defect : state_defect(dev)) what = 100 + field;
        else if (dev.fault || twin.fault) what = 6;
        else if (called != !idle) what = 7;
        if (!what) {
            // the lag words: the twin's object defers what nobody ticked tick by tick, this one once -- the same sum
            const int32_t own = FlowIdleTick(dev.regs.v[F_NEAR_LAG], dev.obj.lag.deferred_lag), other = FlowIdleTick(twin.regs.v[F_NEAR_LAG], twin.obj.lag.deferred_lag);
            for (int k = 0; k < kFlowTickFields && !what; ++k)
                if (dev.regs.v[k] != twin.regs.v[k]) { what = 5; detail[12] = k + 1; }
            if (!what && (own != other || dev.obj.near_pos != twin.obj.near_pos)) { what = 5; detail[12] = F_NEAR_LAG + 1; }
        }
        if (what) { detail[0] = what; return tick; }
        if (!idle) {
            const int n_calls = ordinary ? ((flags & kFlowSplitCalls) ? 2 : 1) : calls, len = span / n_calls;
            for (int c = 0; c < n_calls; ++c) {
                if (!(flags & kFlowNoFarend)) ref.BufferFarend(far_in + c * len, (size_t)len);
                (void)ref.Process(near_in + c * len, nullptr, out_ref + c * len, (size_t)len, (int16_t)ms_now,
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
        if (dfar.size() != rfar.size()) what = 1;
        else if (dfar != rfar) what = 2;
        else if (dnear != rnear) what = 3;
        else if (memcmp(out_dev, out_ref, sizeof out_dev) != 0) what = 4;
        if (what) { detail[0] = what; return tick; }
    }
    return -1;
}

// The recipe of the GPU test of a replay-row spill inside a K-call tick: a session at fs with msInSndCardBuf 40 makes pre_ticks
// ordinary ticks of 160 samples, then ticks of `calls` calls of 80 samples until a plan spills a replay row (at most max_ticks).
// result = {K-call tick of the spill (0-based), call c of the spill, replay row, calls of 80 made before that tick}; returns 0, or
// -1 when no spill happened.
int sim_calls_spill_recipe(int fs, int pre_ticks, int calls, int max_ticks, int32_t *result) {
    FlowRegs r;
    int32_t words[kFlowWords];
    FlowInit(words);
    for (int k = 0; k < kFlowFieldsUsed; ++k) r.v[k] = words[k];
    uint32_t near_pos = 0;
    for (int t = 0; t < pre_ticks; ++t, near_pos += 160) {
        FlowPlan p;
        FlowTick(r, fs, 160, 40, 0, near_pos, p);
    }
    for (int t = 0; t < max_ticks; ++t, near_pos += (uint32_t)(calls * 80)) {
        int at = -1, row = -1;
        FlowTickCalls(r, fs, 80, calls, 40, 0, near_pos, [&](int c, const FlowPlan &p) {
            if (at < 0 && (p.spill[0] | p.spill[1])) { at = c; row = p.spill[1] ? 1 : 0; }
        });
        if (at >= 0) {
            result[0] = t; result[1] = at; result[2] = row; result[3] = t * calls;
            return 0;
        }
    }
    return -1;
}

// The lag of a session after `ticks` idle K-call ticks of calls * n samples from lag 0, and after the same samples as idle ordinary ticks.
int32_t sim_calls_lag_after(int64_t ticks, int calls, int n, int32_t *as_single_ticks) {
    int32_t lag = 0, single = 0;
    for (int64_t i = 0; i < ticks; ++i) {
        lag = FlowIdleTick(lag, calls * n);
        for (int c = 0; c < calls; ++c) single = FlowIdleTick(single, n);
    }
    *as_single_ticks = single;
    return lag;
}

}  // extern "C"

#if !defined(AECM_SIM_CALLS_NO_MAIN)
int main() {
    int64_t detail[15];
    for (uint64_t seed = 0; seed < 8; ++seed)
        for (int fs : {8000, 16000}) {
            const int64_t tick = sim_calls_fuzz(seed, fs, 600, seed % 3 == 2 ? 0xffffff00u : 0u, detail);
            if (tick != -1) {
                printf("seed %llu fs %d: tick %lld what %lld\n", (unsigned long long)seed, fs, (long long)tick, (long long)detail[0]);
                return 1;
            }
        }
    int32_t res[4];
    if (sim_calls_spill_recipe(16000, 12, 6, 40, res) != 0) return 2;
    printf("ok\n");
    return 0;
}
#endif
