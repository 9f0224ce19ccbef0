// What the HOST decides about a tick of an object of sessions, without a device: the state the object keeps between ticks
// (TickObject), the check of a tick's arguments (CheckArgs), the plan of a tick (Plan: one pass over the flags, then who calls,
// the clean-history verdict, the launches the tick takes and what the object looks like afterwards) and the one place that
// moves the object (Commit).  SessionBatch::Enqueue (aecm_sessions.cpp) is CheckArgs -> Plan -> prepare -> Commit -> launch;
// the simulators under tests/sim/ tick their objects through the same three functions, so that what they simulate is routed
// as the product routes it.  A refused tick changes nothing: CheckArgs and Plan are const, and nothing but Commit writes.
// tests/sim/sim_tickplan.cpp holds the one restatement of Plan from the primitives (aecm_flow_plan.h, aecm_flow_clean.h).
#ifndef AECM_AMD_TICK_PLAN_H_
#define AECM_AMD_TICK_PLAN_H_

#include "aecm_flow_clean.h"

namespace aecm {

// The AECM_* codes (include/echo_control_mobile.h; aecm_sessions.cpp asserts the values) a tick can be refused with.
constexpr int32_t kTickUnspecified = 12000, kTickUnsupported = 12001, kTickUninitialized = 12002, kTickNullPointer = 12003,
                  kTickBadParameter = 12004, kTickWarning = 12100;

// The kernels a tick is made by -- the one numbering, for the product's launch switch and the tests alike.
#define AECM_TICK_FAMILIES(X) X(nothing) X(dense) X(sparse) X(mixed) X(calls) X(packets) X(split)
enum TickFamily : int {
#define AECM_TICK_FAMILY_ENUM(name) kTickFamily_##name,
    AECM_TICK_FAMILIES(AECM_TICK_FAMILY_ENUM) kTickFamilies
#undef AECM_TICK_FAMILY_ENUM
};
inline const char *TickFamilyName(int family) {
#define AECM_TICK_FAMILY_NAME(name) #name,
    static const char *const names[] = {AECM_TICK_FAMILIES(AECM_TICK_FAMILY_NAME)};
#undef AECM_TICK_FAMILY_NAME
    return family >= 0 && family < kTickFamilies ? names[family] : "";
}

// A tick's arguments as far as its plan goes (SessionBatch::Tick: aecm_sessions.h).
struct TickArgs {
    const uint8_t *flags_per_session = nullptr;      // [S] or null
    int flags = 0;                                   // everybody's byte when flags_per_session is null
    int n = 160;                                     // samples per call: 80 or 160 (CheckArgs)
    int32_t calls = 1;
    bool packets = false, has_clean = false, host_pointers = false, ms_per_session = false;
};

struct TickPlan {
    int32_t code = 0;                  // 0, kTickBadParameter or kTickUnsupported; refused: only `code` means anything
    int32_t live = 0;                  // sessions that call
    int32_t span = 0;                  // the samples of the tick in every row: n * calls
    int32_t calls = 1;                 // the tick's argument: the call slots a call trace counts for it
    uint8_t any = 0;                   // the OR of the calling sessions' flag bytes
    bool half_calls = false;           // some session that calls makes a half call
    bool k_calls = false;              // calls > 1
    bool split_tick = false;           // callers with and without a clean input: the two lists (aecm_flow_clean.h)
    int32_t clean_count = 0, plain_count = 0;      // a split tick's callers of either kind
    bool clean_plane = false;          // the kernels take the clean plane (not when every caller carries kNoClean)
    bool need_slot = false;            // a pinned argument slot is written: ms, flags or the bases of the live list(s)
    bool zero_out = false;             // host output: rows or half rows no kernel writes travel back as zeros
    FlowTickRoute route{false, false, false, 0};
    bool mixed_plan = false;
    TickFamily family = kTickFamily_nothing;
    // what Commit gives the object
    FlowObjectLag lag_after;
    FlowCleanTick clean_tick{false, false};
    const uint8_t *flags_per_session = nullptr;      // (the caller's array, as FlowCleanHistory::Commit reads it)
    bool had_clean = false;
};

struct TickObject {
    int32_t n_sessions = 0;
    int32_t fs = 0;                          // the object's rate; 0: not initialised
    std::vector<int32_t> rates;              // [S] every session's own rate
    int32_t other_rates = 0;                 // sessions whose rate is not fs
    bool force_sparse = false;               // diagnostics: every tick by the live list
    // WebRtcAecmSessions_SetSplitCallTicks: K-call and packet ticks with callers of both kinds are planned (family split with
    // k_calls; mixed_plan: the packed layout) instead of refused.  The caller's switch, like force_sparse: no Init touches it.
    bool split_call_ticks = false;
    int64_t near_pos = 0;                    // near-end samples ticked so far = ring position of the next tick's first one
    FlowObjectLag lag;                       // aecm_flow_plan.h: FlowRouteTick
    FlowCleanHistory history;                // what every session's Process calls carried (kNoClean)
    // The session trace (include/aecm_batch.h: WebRtcAecmSessions_SetSessionTrace), the per-TICK mode: whether one is attached -- the
    // caller's switch, like force_sparse, which no Init touches -- and the ticks accepted since it was (AttachTrace zeroes the count;
    // only Commit moves it).
    // The call trace (WebRtcAecmSessions_SetCallTrace), the per-CALL mode: a switch of its own, under which ticks of several calls
    // are accepted and the count is of call slots: an accepted tick of `calls` call pairs moves it by `calls` (Commit).
    // At most one of the two is on: switching one on while the other is on is refused (false) and changes nothing; switching off
    // touches only its own kind.
    bool trace_attached = false, call_trace_attached = false;
    int64_t trace_ticks = 0, call_trace_calls = 0;
    bool AttachTrace(bool on) {
        if (on && call_trace_attached) return false;
        trace_attached = on;
        trace_ticks = 0;
        return true;
    }
    bool AttachCallTrace(bool on) {
        if (on && trace_attached) return false;
        call_trace_attached = on;
        call_trace_calls = 0;
        return true;
    }
    // scratch of Plan, read by whoever launches that plan: FlowLiveBlockBases of the tick's flags [ceil(S / kFlowPlanBlock)], and
    // FlowScanFlagsClean of a split tick's [2][the same]
    mutable std::vector<uint32_t> live_bases, split_bases;

    // WebRtcAecm_Init of every session at samp_freq (force_sparse is the caller's switch, not the sessions' state).
    void Init(int32_t sessions, int32_t samp_freq) {
        n_sessions = sessions;
        fs = samp_freq;
        rates.assign((size_t)sessions, samp_freq);
        other_rates = 0;
        near_pos = 0;
        lag = FlowObjectLag();
        history.Reset((size_t)sessions);
        const size_t blocks = ((size_t)sessions + kFlowPlanBlock - 1) / kFlowPlanBlock;
        live_bases.assign(blocks, 0u);
        split_bases.assign(2 * blocks, 0u);
    }
    // An Init that did not get through: the object is as one that was never initialised.
    void Forget() { fs = 0; }
    void SetRate(int session, int32_t samp_freq) {
        other_rates += (samp_freq != fs) - (rates[(size_t)session] != fs);
        rates[(size_t)session] = samp_freq;
    }
    // WebRtcAecm_Init of one session, or a session that arrives by a snapshot: its rate, and no Process call so far.
    void InitSession(int session, int32_t samp_freq) {
        SetRate(session, samp_freq);
        history.ResetSession(session);
    }

    // Everything about a tick's arguments that needs neither the device nor the flags' meaning, in the order of the reference's
    // own checks (echo_control_mobile.cc:236-265) and then this object's.  far may be null only when nobody buffers a far frame.
    int32_t CheckArgs(bool has_far, bool has_near_and_out, const uint8_t *flags_per_session, int flags, size_t n_samples, int32_t calls, int64_t stride,
                      bool packets, bool poisoned, bool fast_variant) const {
        if (!has_near_and_out) return kTickNullPointer;
        if (!has_far) {
            bool nobody = flags_per_session ? true : (flags & kFlowNoFarend) != 0;
            if (flags_per_session && fs != 0)
                for (int32_t s = 0; s < n_sessions && nobody; ++s) nobody = (flags_per_session[s] & (kFlowNoFarend | kFlowIdle)) != 0;
            if (!nobody) return kTickNullPointer;
        }
        if (fs == 0) return kTickUninitialized;
        if (n_samples != 80 && n_samples != 160) return kTickBadParameter;       // compared as size_t: 2^32 + 80 is not 80
        if (calls < 1 || calls > kFlowMaxTickCalls) return kTickBadParameter;
        if (stride < (int64_t)n_samples * calls) return kTickBadParameter;
        if (poisoned) return kTickUnspecified;
        // the tick kernels exist for the fast cross-lane primitives only: a batch switched to the safe variant is told so (and
        // stays usable after switching back)
        if (!fast_variant) return kTickUnsupported;
        // K calls per row of a session of the other rate is a layout of its own: the packed rows of a packet tick
        if (calls > 1 && other_rates > 0 && !packets) return kTickUnsupported;
        // a session trace has one record per tick of ONE call pair (the per-tick mode); a record per call of a K-call or packet tick
        // is the call trace's, the per-call mode, which this refusal does not touch
        if (calls > 1 && trace_attached) return kTickUnsupported;
        return 0;
    }

    // The tick that CheckArgs has passed.  Writes nothing an observer can see (the scratch vectors; FlowCleanHistory::Fold).
    TickPlan Plan(const TickArgs &a) const {
        TickPlan p;
        const int32_t S = n_sessions;
        p.span = a.n * a.calls;
        p.calls = a.calls;
        p.k_calls = a.calls > 1;
        // Who calls (kIdle: neither call; the other bits of an idle session's byte mean nothing).  One pass over the flags: the
        // live count, and per planning workgroup the live sessions before it (what the device needs for the live list).
        p.live = S;
        p.any = a.flags_per_session ? 0 : (uint8_t)a.flags;
        bool half_and_split = false;
        if (a.flags_per_session) p.live = FlowScanFlags(a.flags_per_session, S, live_bases.data(), &p.any, &half_and_split);
        const auto refused = [&p](int32_t code) { p.code = code; return p; };
        if (!FlowTickFlagsValid(a.n, p.any, half_and_split)) return refused(kTickBadParameter);      // two 80-sample calls, or 80 of 160, need 160 samples
        // a K-call tick's calls are whole calls of n samples; a packet tick's are whole calls of the session's own size (80 with kHalfCall)
        if (p.k_calls && (p.any & (a.packets ? kFlowSplitCalls : kFlowSplitCalls | kFlowHalfCall)) != 0) return refused(kTickBadParameter);
        p.half_calls = a.flags_per_session && (p.any & kFlowHalfCall) != 0;
        // kNoClean: a tick that gives a calling session another kind of Process call than it has had is refused
        // (callers of both kinds in a tick of several calls: only with the object's switch, and never under a call trace)
        if (const FlowCleanVerdict v = history.Check(a.flags_per_session, p.any, a.has_clean, a.calls, &p.clean_tick, split_call_ticks && !call_trace_attached))
            return refused(v == kCleanUnsupported ? kTickUnsupported : kTickBadParameter);
        p.flags_per_session = a.flags_per_session;
        p.had_clean = a.has_clean;
        if (p.clean_tick.split)
            FlowScanFlagsClean(a.flags_per_session, S, split_bases.data(), split_bases.data() + live_bases.size(), &p.clean_count, &p.plain_count);
        // all callers flagged: the tick without a clean input, by its launches; some: the two lists
        p.clean_plane = a.has_clean && !(p.clean_tick.split && p.clean_count == 0);
        p.split_tick = p.clean_tick.split && p.clean_count > 0;
        // (a K-call tick and a split tick always go by the live list; a K-call tick is told the whole tick's samples; half calls
        // leave their sessions behind, the object out of step.  Nobody calls: the position moves on, the lag is deferred.)
        p.lag_after = lag;
        p.route = FlowRouteTickMixed(p.lag_after, p.live, S, p.span, force_sparse || p.k_calls || p.split_tick, p.half_calls, other_rates > 0, &p.mixed_plan);
        p.zero_out = a.host_pointers && (p.live < S || p.half_calls);
        if (!p.route.launch) return p;
        p.need_slot = a.ms_per_session || a.flags_per_session || p.route.sparse_tick;
        if (p.route.sparse_tick && !a.flags_per_session)
            for (size_t b = 0; b < live_bases.size(); ++b) live_bases[b] = (uint32_t)(b * kFlowPlanBlock);
        // (mixed_plan with K calls: a packet tick in which somebody makes half calls or runs at another rate; a packet tick of a
        // uniform object without half calls IS the K-call tick)
        p.family = p.split_tick ? kTickFamily_split
                   : p.k_calls ? (p.mixed_plan ? kTickFamily_packets : kTickFamily_calls)
                   : !p.route.sparse_plan ? kTickFamily_dense
                   : p.mixed_plan ? kTickFamily_mixed
                                  : kTickFamily_sparse;
        return p;
    }
    // The bases the planning launch of `p` reads: both lists' of a split tick, one behind the other, else the live list's.
    const std::vector<uint32_t> &Bases(const TickPlan &p) const { return p.split_tick ? split_bases : live_bases; }

    // The planned tick is certain to be made: the only place that moves near_pos, lag, the clean history, the session trace's
    // tick count and the call trace's count of call slots.  (A tick nobody makes gives no session a Process call: the history stays;
    // it writes no record and still counts.)
    void Commit(const TickPlan &p) {
        near_pos += p.span;
        lag = p.lag_after;
        if (trace_attached) ++trace_ticks;
        if (call_trace_attached) call_trace_calls += p.calls;
        if (p.route.launch) history.Commit(p.flags_per_session, p.had_clean, p.clean_tick);
    }
    // Check, plan and -- accepted -- commit in one, for a caller with nothing between the steps (the simulators under tests/sim/:
    // every pointer there, rows of n * calls samples, a healthy object).  *tick_pos: the near position before the tick.
    TickPlan Tick(const TickArgs &a, uint32_t *tick_pos = nullptr) {
        TickPlan p;
        p.code = CheckArgs(true, true, a.flags_per_session, a.flags, (size_t)a.n, a.calls, (int64_t)a.n * a.calls, a.packets, false, true);
        if (!p.code) p = Plan(a);
        if (tick_pos) *tick_pos = (uint32_t)near_pos;
        if (!p.code) Commit(p);
        return p;
    }
};

// The codes of a tick's Process calls, which need no device: the only thing a call of an initialised session with valid
// arguments can return is the warning for an out-of-range msInSndCardBuf (echo_control_mobile.cc:258-265).  codes ([S], may be
// null) gets every session's, an idle session's is 0; returns the first non-zero one (without ms_per_session: ms's).
inline int32_t TickCodes(const int16_t *ms_per_session, int16_t ms, const uint8_t *flags_per_session, int32_t n_sessions, int32_t *codes) {
    const auto idle = [&](int32_t s) { return flags_per_session && (flags_per_session[s] & kFlowIdle) != 0; };
    const auto code_of = [](int16_t v) -> int32_t { return (v < 0 || v > 500) ? kTickWarning : 0; };
    int32_t first = 0;
    if (!ms_per_session) {
        first = code_of(ms);
        if (codes)
            for (int32_t s = 0; s < n_sessions; ++s) codes[s] = idle(s) ? 0 : first;
        return first;
    }
    int lo = ms_per_session[0], hi = lo;                                    // one vectorisable pass; the per-session codes
    for (int32_t s = 1; s < n_sessions; ++s) {                              // only need a second one when somebody is out of range
        lo = lo < ms_per_session[s] ? lo : ms_per_session[s];
        hi = hi > ms_per_session[s] ? hi : ms_per_session[s];
    }
    if (lo < 0 || hi > 500) {
        for (int32_t s = 0; s < n_sessions; ++s) {
            const int32_t rc = idle(s) ? 0 : code_of(ms_per_session[s]);    // an idle session makes no call: no code
            if (codes) codes[s] = rc;
            if (rc != 0 && first == 0) first = rc;
        }
    } else if (codes) {
        for (int32_t s = 0; s < n_sessions; ++s) codes[s] = 0;
    }
    return first;
}

}  // namespace aecm
#endif  // AECM_AMD_TICK_PLAN_H_
