// A clean near-end input PER SESSION (AECM_SESSION_NO_CLEAN): in one tick that carries a clean plane, some sessions'
// WebRtcAecm_Process gets its clean row and the others' gets nearendClean = NULL.  What that needs beyond aecm_flow_plan.h, for host
// and device alike:
//   - the two live lists of such a SPLIT tick: the ids of the calling sessions that take their clean row, ascending, then -- from the
//     next workgroup boundary of the tick kernel on -- those that take none, ascending.  Built like the one live list
//     (aecm_flow_plan.h: FlowLiveBlockBases / FlowLiveSlot), without atomics, in two halves: the host's pass over the flags counts per
//     planning workgroup the sessions of either kind before it (FlowScanFlagsClean), the planning kernel adds ballot + popcount
//     within the wavefront and LDS counts across the workgroup's wavefronts, once per list (FlowSplitSlot);
//   - the rule by which the host keeps a session from changing its kind within its life (FlowCleanHistory): the reference's clean
//     frame buffer under-runs when the clean pointer comes and goes (aecm_core.cc:501-572), so a session is "always" or "never"
//     between two initialisations, and an object that has once taken a split tick checks that on every tick.
// tests/sim/sim_split.cpp drives every function of this header on the CPU.
#ifndef AECM_AMD_FLOW_CLEAN_H_
#define AECM_AMD_FLOW_CLEAN_H_

#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "aecm_flow_plan.h"

namespace aecm {

constexpr int kFlowNoClean = 16;                    // = SessionBatch::kNoClean = AECM_SESSION_NO_CLEAN
constexpr int kFlowSplitGroup = 4;                  // sessions per workgroup of the tick kernels (aecm_tick_unit.h: kTickFlowWaves)

// Where the list of the sessions without a clean input starts behind clean_count entries of the other: the next multiple of
// kFlowSplitGroup, so that no workgroup of the tick kernel serves sessions of both kinds.
AECM_FLOW_HD uint32_t FlowPlainListStart(uint32_t clean_count) {
    return (clean_count + (uint32_t)kFlowSplitGroup - 1u) / (uint32_t)kFlowSplitGroup * (uint32_t)kFlowSplitGroup;
}
// Entries the device list of an object of n_sessions has to hold: both lists and the gap between them.
AECM_FLOW_HD uint32_t FlowSplitListEntries(uint32_t n_sessions) { return n_sessions + (uint32_t)kFlowSplitGroup; }

// The host half: clean_bases[b] / plain_bases[b] = calling sessions with / without a clean input among the first
// kFlowPlanBlock * b; the totals in *clean_count / *plain_count.  An idle session's bits mean nothing.
inline void FlowScanFlagsClean(const uint8_t *flags, int32_t n_sessions, uint32_t *clean_bases, uint32_t *plain_bases, int32_t *clean_count,
                               int32_t *plain_count) {
    int32_t with = 0, without = 0;
    for (int32_t first = 0, b = 0; first < n_sessions; first += kFlowPlanBlock, ++b) {
        clean_bases[b] = (uint32_t)with;
        plain_bases[b] = (uint32_t)without;
        const int32_t end = first + kFlowPlanBlock < n_sessions ? first + kFlowPlanBlock : n_sessions;
        for (int32_t s = first; s < end; ++s) {
            const uint32_t f = flags[s], calls = ((f >> 2) & 1u) ^ 1u, no_clean = (f >> 4) & 1u;
            without += (int32_t)(calls & no_clean);
            with += (int32_t)(calls & (no_clean ^ 1u));
        }
    }
    *clean_count = with;
    *plain_count = without;
}
static_assert(kFlowIdle == 4 && kFlowNoClean == 16, "FlowScanFlagsClean reads bits 2 and 4");

// The device half: this lane's slot in the device list.  wave_counts[0][w] / [1][w] = calling lanes with / without a clean input of
// wavefront w of the workgroup, ballot_clean / ballot_plain = those lanes of this lane's wavefront, plain_start =
// FlowPlainListStart(clean_count).  Only a calling lane's result means anything.
AECM_FLOW_HD uint32_t FlowSplitSlot(bool no_clean, uint32_t clean_base, uint32_t plain_base, uint32_t plain_start,
                                    const uint32_t wave_counts[2][kFlowPlanBlock / 64], int wave, uint64_t ballot_clean, uint64_t ballot_plain, int lane) {
    const uint32_t in_clean = FlowLiveSlot(clean_base, wave_counts[0], wave, ballot_clean, lane);
    const uint32_t in_plain = FlowLiveSlot(plain_start + plain_base, wave_counts[1], wave, ballot_plain, lane);
    return no_clean ? in_plain : in_clean;
}

// ---- the history rule (host only) -------------------------------------------------------------------------------------------------
// One byte per session: what its WebRtcAecm_Process calls since its last initialisation carried.
enum FlowCleanMode : uint8_t { kCleanNone = 0, kCleanAlways = 1, kCleanNever = 2, kCleanBoth = 3 };
enum FlowCleanVerdict : int { kCleanAccepted = 0, kCleanRefused = 1, kCleanUnsupported = 2 };

struct FlowCleanTick {
    bool split;          // some calling session carries kFlowNoClean in a tick that has a clean plane
    bool checked;        // the tick was held against the sessions' histories (split, or the object has taken a split tick before)
};

struct FlowCleanHistory {
    // (mode and pending are mutable for Fold alone: bringing the one up to date with the other changes nothing Get can tell)
    mutable std::vector<uint8_t> mode;      // [S] FlowCleanMode
    mutable uint8_t pending = 0;            // what ticks WITHOUT a flags array gave every session since `mode` was last brought up to date:
                                    // such a tick must not cost a pass over the sessions, so it leaves its mark here
    bool split_used = false;        // the object has accepted a split tick since its last Init: every tick is checked from then on

    void Reset(size_t n_sessions) {
        mode.assign(n_sessions, (uint8_t)kCleanNone);
        pending = 0;
        split_used = false;
    }
    void Fold() const {
        if (!pending) return;
        for (uint8_t &m : mode) m |= pending;
        pending = 0;
    }
    // WebRtcAecm_Init of one session / a session that arrives by a snapshot: it starts at "none".
    void ResetSession(int session) {
        Fold();
        mode[(size_t)session] = (uint8_t)kCleanNone;
    }
    uint8_t Get(int session) const { return (uint8_t)(mode[(size_t)session] | pending); }

    // What a tick gives session s: flags = its byte (the tick's one byte without a flags array), has_clean = the tick has a clean plane.
    static uint8_t Gives(uint32_t flags, bool has_clean) { return has_clean && !(flags & (uint32_t)kFlowNoClean) ? (uint8_t)kCleanAlways : (uint8_t)kCleanNever; }

    // May the tick be made?  flags: the per-session bytes or null (then everybody calls with no bit of interest set), any = the OR of
    // the calling sessions' bytes (FlowScanFlags), calls = call pairs per session.  Changes nothing that can be observed (it may bring
    // `mode` up to date with `pending`).  split_calls: the object takes split ticks of several calls (TickObject::split_call_ticks,
    // and no call trace attached) -- such a tick gives a session the same kind for all of its calls, so the rule is the one below;
    // without it a split tick of calls > 1 is unsupported, before its histories are looked at.
    FlowCleanVerdict Check(const uint8_t *flags, uint8_t any, bool has_clean, int32_t calls, FlowCleanTick *tick, bool split_calls = false) const {
        tick->split = has_clean && flags != nullptr && (any & (uint8_t)kFlowNoClean) != 0;
        tick->checked = tick->split || split_used;
        if (tick->split && calls > 1 && !split_calls) return kCleanUnsupported;
        if (!tick->checked) return kCleanAccepted;
        Fold();
        const size_t S = mode.size();
        uint32_t bad = 0;
        if (flags) {
            for (size_t s = 0; s < S; ++s) {
                const uint32_t f = flags[s], gives = Gives(f, has_clean), m = mode[s];
                bad |= (uint32_t)(!(f & (uint32_t)kFlowIdle) && m != 0 && m != gives);
            }
        } else {
            const uint32_t gives = Gives(0, has_clean);
            for (size_t s = 0; s < S; ++s) bad |= (uint32_t)(mode[s] != 0 && mode[s] != gives);
        }
        return bad ? kCleanRefused : kCleanAccepted;
    }
    // The tick is made (it has passed Check and is certain to be enqueued; somebody calls).
    void Commit(const uint8_t *flags, bool has_clean, const FlowCleanTick &tick) {
        if (tick.split) split_used = true;
        if (!flags) {
            pending |= Gives(0, has_clean);
            return;
        }
        const size_t S = mode.size();
        const uint8_t fold = pending;
        pending = 0;
        for (size_t s = 0; s < S; ++s) {
            const uint32_t f = flags[s];
            mode[s] = (uint8_t)(mode[s] | fold | ((f & (uint32_t)kFlowIdle) ? 0u : (uint32_t)Gives(f, has_clean)));
        }
    }
};

}  // namespace aecm
#endif  // AECM_AMD_FLOW_CLEAN_H_
