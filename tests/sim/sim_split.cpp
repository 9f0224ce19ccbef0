// TEST INFRASTRUCTURE: the host side of AECM_SESSION_NO_CLEAN (webrtc_aecm_amd/csrc/aecm_flow_clean.h) without a device.
//   - the two live lists of a split tick: the host's pass over the flags (FlowScanFlagsClean) and the planning kernel's half,
//     simulated lane by lane -- ballots per wavefront of 64, counts per workgroup of 256, FlowSplitSlot, the kernel's store guard
//     (aecm_tick_split_plan_kernels.hip);
//   - the history rule as the host's planner applies it (aecm_tick_plan.h: the object and the ticks are the product's own).
// Built as a library for tests/split_sim.py, or (-DSIM_SPLIT_MAIN) as a program of its own, the only form built with sanitizers.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "aecm_tick_plan.h"

using namespace aecm;

namespace {

// list: FlowSplitListEntries(S) entries the caller has preset; res = {clean_count, plain_count, plain_start, stores out of range}.
void Lists(const uint8_t *flags, int32_t S, uint32_t *list, int32_t res[4]) {
    const int32_t blocks = (S + kFlowPlanBlock - 1) / kFlowPlanBlock;
    std::vector<uint32_t> clean_bases((size_t)blocks), plain_bases((size_t)blocks);
    int32_t clean_count, plain_count;
    FlowScanFlagsClean(flags, S, clean_bases.data(), plain_bases.data(), &clean_count, &plain_count);
    const uint32_t plain_start = FlowPlainListStart((uint32_t)clean_count);
    int32_t dropped = 0;
    for (int32_t b = 0; b < blocks; ++b) {
        uint32_t wave_counts[2][kFlowPlanBlock / 64];
        uint64_t ballots[2][kFlowPlanBlock / 64];
        auto flag_of = [&](int t) { const int32_t s = b * kFlowPlanBlock + t; return s < S ? (int)flags[s] : kFlowIdle; };
        for (int w = 0; w < kFlowPlanBlock / 64; ++w) {
            ballots[0][w] = ballots[1][w] = 0;
            for (int lane = 0; lane < 64; ++lane) {
                const int f = flag_of(w * 64 + lane);
                const bool live = (f & kFlowIdle) == 0, no_clean = (f & kFlowNoClean) != 0;
                if (live && !no_clean) ballots[0][w] |= uint64_t(1) << lane;
                if (live && no_clean) ballots[1][w] |= uint64_t(1) << lane;
            }
            wave_counts[0][w] = (uint32_t)__builtin_popcountll(ballots[0][w]);
            wave_counts[1][w] = (uint32_t)__builtin_popcountll(ballots[1][w]);
        }
        for (int t = 0; t < kFlowPlanBlock; ++t) {
            const int f = flag_of(t), w = t >> 6, lane = t & 63;
            const bool live = (f & kFlowIdle) == 0, no_clean = (f & kFlowNoClean) != 0;
            const uint32_t slot = FlowSplitSlot(no_clean, clean_bases[(size_t)b], plain_bases[(size_t)b], plain_start, wave_counts, w, ballots[0][w], ballots[1][w], lane);
            const uint32_t end = no_clean ? plain_start + (uint32_t)plain_count : (uint32_t)clean_count;
            if (!live) continue;
            if (slot < end && slot < FlowSplitListEntries((uint32_t)S)) list[slot] = (uint32_t)(b * kFlowPlanBlock + t);
            else ++dropped;
        }
    }
    res[0] = clean_count;
    res[1] = plain_count;
    res[2] = (int32_t)plain_start;
    res[3] = dropped;
}

// A tick of SessionBatch::Enqueue's as far as the host goes -- check, plan, commit: 0 accepted, 1 AECM_BAD_PARAMETER_ERROR,
// 2 AECM_UNSUPPORTED_FUNCTION_ERROR.
int Tick(TickObject &o, const uint8_t *flags, int has_clean, int calls, int n, int32_t route[3]) {
    TickArgs a;
    a.flags_per_session = flags;
    a.n = n;
    a.calls = calls;
    a.has_clean = has_clean != 0;
    const TickPlan plan = o.Tick(a);
    if (plan.code) return plan.code == kTickUnsupported ? 2 : 1;
    route[0] = plan.split_tick;                  // the split launches
    route[1] = plan.clean_plane;                 // the tick's kernels take a clean input
    route[2] = plan.clean_tick.checked;
    return 0;
}

uint64_t Next(uint64_t &x) {
    x ^= x << 13; x ^= x >> 7; x ^= x << 17;
    return x;
}

// Random flag bytes against a plain partition; returns 0 or the line that failed.
int SelfCheck() {
    uint64_t rng = 0x9e3779b97f4a7c15ull;
    for (int S : {1, 63, 64, 65, 255, 256, 257, 300, 1000}) {
        for (int round = 0; round < 20; ++round) {
            std::vector<uint8_t> flags((size_t)S);
            for (auto &f : flags) f = (uint8_t)(((Next(rng) & 31u) | (round % 5 == 1 ? kFlowNoClean : 0)) & (round % 5 == 2 ? ~(unsigned)kFlowNoClean : ~0u));   // (nobody clean / nobody plain)
            std::vector<uint32_t> list(FlowSplitListEntries((uint32_t)S), 0xffffffffu), want_clean, want_plain;
            int32_t res[4];
            Lists(flags.data(), S, list.data(), res);
            for (int s = 0; s < S; ++s)
                if (!(flags[(size_t)s] & kFlowIdle)) ((flags[(size_t)s] & kFlowNoClean) ? want_plain : want_clean).push_back((uint32_t)s);
            if (res[0] != (int32_t)want_clean.size() || res[1] != (int32_t)want_plain.size() || res[2] % kFlowSplitGroup != 0 || res[3] != 0) return __LINE__;
            for (size_t i = 0; i < want_clean.size(); ++i)
                if (list[i] != want_clean[i]) return __LINE__;
            for (size_t i = 0; i < want_plain.size(); ++i)
                if (list[(size_t)res[2] + i] != want_plain[i]) return __LINE__;
        }
    }
    TickObject o;
    o.Init(8, 16000);
    const FlowCleanHistory &h = o.history;
    int32_t route[3];
    const uint8_t mixed[8] = {0, 16, 0, 16, 4, 4 | 16, 0, 16}, swapped[8] = {16, 0, 4, 4, 4, 4, 4, 4};
    if (Tick(o, nullptr, 1, 1, 160, route) != 0 || h.Get(1) != kCleanAlways) return __LINE__;
    if (Tick(o, mixed, 1, 1, 160, route) != 1 || o.near_pos != 160 || h.split_used) return __LINE__;
    o.Init(8, 16000);
    if (Tick(o, mixed, 1, 1, 160, route) != 0 || !route[0] || h.Get(1) != kCleanNever || h.Get(4) != kCleanNone) return __LINE__;
    if (Tick(o, swapped, 1, 1, 160, route) != 1 || Tick(o, nullptr, 1, 1, 160, route) != 1 || Tick(o, mixed, 1, 2, 160, route) != 2) return __LINE__;
    o.InitSession(1, 16000);
    if (h.Get(1) != kCleanNone || h.Get(3) != kCleanNever) return __LINE__;
    return 0;
}

}  // namespace

extern "C" {

void sim_split_lists(const uint8_t *flags, int32_t n_sessions, uint32_t *list, int32_t *res) { Lists(flags, n_sessions, list, res); }
int32_t sim_split_list_entries(int32_t n_sessions) { return (int32_t)FlowSplitListEntries((uint32_t)n_sessions); }

void *sim_split_object_new(int32_t n_sessions) {
    TickObject *o = new TickObject();
    o->Init(n_sessions, 16000);
    return o;
}
void sim_split_object_free(void *o) { delete static_cast<TickObject *>(o); }
void sim_split_object_init(void *o) {
    TickObject *p = static_cast<TickObject *>(o);
    p->Init(p->n_sessions, p->fs);
}
int32_t sim_split_object_tick(void *o, const uint8_t *flags, int32_t has_clean, int32_t calls, int32_t n, int32_t *route) {
    return Tick(*static_cast<TickObject *>(o), flags, has_clean, calls, n, route);
}
void sim_split_object_reset_session(void *o, int32_t session) {
    TickObject *p = static_cast<TickObject *>(o);
    p->InitSession(session, p->fs);
}
// modes[S], then what else an observer could see: {position, split_used}
void sim_split_object_state(void *o, uint8_t *modes, int64_t *rest) {
    TickObject *p = static_cast<TickObject *>(o);
    for (int32_t s = 0; s < p->n_sessions; ++s) modes[s] = p->history.Get(s);
    rest[0] = p->near_pos;
    rest[1] = p->history.split_used;
}
int32_t sim_split_self_check(void) { return SelfCheck(); }

}  // extern "C"

#if defined(SIM_SPLIT_MAIN)
int main() {
    const int line = SelfCheck();
    if (line) {
        printf("sim_split.cpp:%d\n", line);
        return 1;
    }
    printf("ok\n");
    return 0;
}
#endif
