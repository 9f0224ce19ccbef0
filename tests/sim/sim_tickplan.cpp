// TEST INFRASTRUCTURE: the host's tick planner (webrtc_aecm_amd/csrc/aecm_tick_plan.h: TickObject::CheckArgs / Plan / Commit, TickCodes)
// without a device.  tests/test_tick_plan.py drives single ticks through it (a hand-written table of cases) and runs Fuzz(): random
// ticks against RefTick below -- the ONE restatement of the planner in the tree, written straight from the primitives it is made of
// (FlowScanFlags, FlowTickFlagsValid, FlowCleanHistory, FlowScanFlagsClean, FlowRouteTick[Mixed]) in the order the contract of
// SessionBatch::Tick (aecm_sessions.h) gives them.
// Built as a library, or (-DSIM_TICKPLAN_MAIN) as a program of its own, the only form built with sanitizers.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "aecm_tick_plan.h"

using namespace aecm;

namespace {

// ---- the restatement ------------------------------------------------------------------------------------------------------------
struct RefObject {
    int32_t S = 0, fs = 0;
    std::vector<int32_t> rates;
    bool force_sparse = false;
    int64_t near_pos = 0;
    FlowObjectLag lag;
    FlowCleanHistory h;
    int32_t OtherRates() const {
        int32_t k = 0;
        for (int32_t r : rates) k += r != fs;
        return k;
    }
    void Init(int32_t sessions, int32_t samp_freq) {
        S = sessions;
        fs = samp_freq;
        rates.assign((size_t)S, fs);
        near_pos = 0;
        lag = FlowObjectLag();
        h.Reset((size_t)S);
    }
};

struct RefResult {
    int32_t code = 0, live = 0, span = 0, clean_count = 0, plain_count = 0, family = 0;
    uint8_t any = 0;
    bool half_calls = false, k_calls = false, split_tick = false, clean_plane = false, need_slot = false, zero_out = false, mixed_plan = false;
    FlowTickRoute route{false, false, false, 0};
    std::vector<uint32_t> bases;      // what the planning launch reads (sparse tick)
};

// A tick as SessionBatch::Tick documents it; commits when accepted.
RefResult RefTick(RefObject &o, const TickArgs &a, bool has_far, bool has_near_and_out, size_t n_samples, int64_t stride, bool poisoned, bool fast) {
    RefResult r;
    const size_t blocks = ((size_t)o.S + kFlowPlanBlock - 1) / kFlowPlanBlock;
    const auto refuse = [&](int32_t code) { r = RefResult(); r.code = code; return r; };
    if (!has_near_and_out) return refuse(kTickNullPointer);
    if (!has_far) {
        bool somebody = a.flags_per_session ? false : !(a.flags & kFlowNoFarend);
        for (int32_t s = 0; a.flags_per_session && o.fs != 0 && s < o.S; ++s) somebody = somebody || !(a.flags_per_session[s] & (kFlowNoFarend | kFlowIdle));
        if (somebody) return refuse(kTickNullPointer);
    }
    if (o.fs == 0) return refuse(kTickUninitialized);
    if ((n_samples != 80 && n_samples != 160) || a.calls < 1 || a.calls > kFlowMaxTickCalls || stride < (int64_t)n_samples * a.calls) return refuse(kTickBadParameter);
    if (poisoned) return refuse(kTickUnspecified);
    if (!fast || (a.calls > 1 && o.OtherRates() > 0 && !a.packets)) return refuse(kTickUnsupported);
    std::vector<uint32_t> live_bases(blocks), split_bases(2 * blocks);
    bool both = false;
    r.live = o.S;
    r.any = (uint8_t)a.flags;
    if (a.flags_per_session) r.live = FlowScanFlags(a.flags_per_session, o.S, live_bases.data(), &r.any, &both);
    if (!FlowTickFlagsValid(a.n, r.any, both)) return refuse(kTickBadParameter);
    if (a.calls > 1 && (r.any & (kFlowSplitCalls | (a.packets ? 0 : kFlowHalfCall)))) return refuse(kTickBadParameter);
    FlowCleanTick ct;
    const FlowCleanVerdict v = o.h.Check(a.flags_per_session, r.any, a.has_clean, a.calls, &ct);
    if (v == kCleanUnsupported) return refuse(kTickUnsupported);
    if (v == kCleanRefused) return refuse(kTickBadParameter);
    r.span = a.n * a.calls;
    r.k_calls = a.calls > 1;
    r.half_calls = a.flags_per_session && (r.any & kFlowHalfCall);
    if (ct.split) FlowScanFlagsClean(a.flags_per_session, o.S, split_bases.data(), split_bases.data() + blocks, &r.clean_count, &r.plain_count);
    r.split_tick = ct.split && r.clean_count > 0;
    r.clean_plane = a.has_clean && (!ct.split || r.clean_count > 0);
    r.zero_out = a.host_pointers && (r.live < o.S || r.half_calls);
    o.near_pos += r.span;
    if (r.live == 0) {
        r.route = FlowRouteTick(o.lag, 0, o.S, r.span, o.force_sparse);
        return r;
    }
    r.route = FlowRouteTickMixed(o.lag, r.live, o.S, r.span, o.force_sparse || r.k_calls || r.split_tick, r.half_calls, o.OtherRates() > 0, &r.mixed_plan);
    o.h.Commit(a.flags_per_session, a.has_clean, ct);
    r.need_slot = a.ms_per_session || a.flags_per_session || r.route.sparse_tick;
    r.family = r.split_tick ? kTickFamily_split : r.k_calls ? (r.mixed_plan ? kTickFamily_packets : kTickFamily_calls)
               : !r.route.sparse_plan ? kTickFamily_dense : r.mixed_plan ? kTickFamily_mixed : kTickFamily_sparse;
    if (r.route.sparse_tick) {
        if (!a.flags_per_session)
            for (size_t b = 0; b < blocks; ++b) live_bases[b] = (uint32_t)(b * kFlowPlanBlock);
        r.bases = r.split_tick ? split_bases : live_bases;
    }
    return r;
}

// ---- the planner under test ------------------------------------------------------------------------------------------------------
struct Tick {
    TickArgs a;
    bool has_far = true, has_near_and_out = true, poisoned = false, fast = true;
    size_t n_samples = 160;
    int64_t stride = 160;
};

// CheckArgs, Plan and (accepted, commit) Commit; the code the tick returns.
int32_t Run(TickObject &o, const Tick &t, bool commit, TickPlan *plan) {
    *plan = TickPlan();
    if (const int32_t rc = o.CheckArgs(t.has_far, t.has_near_and_out, t.a.flags_per_session, t.a.flags, t.n_samples, t.a.calls, t.stride, t.a.packets, t.poisoned, t.fast))
        return rc;
    *plan = o.Plan(t.a);
    if (plan->code == 0 && commit) o.Commit(*plan);
    return plan->code;
}

bool SamePlan(const TickPlan &x, const TickPlan &y) {
    return x.code == y.code && x.live == y.live && x.span == y.span && x.any == y.any && x.half_calls == y.half_calls && x.k_calls == y.k_calls &&
           x.split_tick == y.split_tick && x.clean_count == y.clean_count && x.plain_count == y.plain_count && x.clean_plane == y.clean_plane &&
           x.need_slot == y.need_slot && x.zero_out == y.zero_out && x.route.launch == y.route.launch && x.route.sparse_plan == y.route.sparse_plan &&
           x.route.sparse_tick == y.route.sparse_tick && x.route.deferred_lag == y.route.deferred_lag && x.mixed_plan == y.mixed_plan &&
           x.family == y.family && x.lag_after.deferred_lag == y.lag_after.deferred_lag && x.lag_after.may_lag == y.lag_after.may_lag &&
           x.clean_tick.split == y.clean_tick.split && x.clean_tick.checked == y.clean_tick.checked && x.flags_per_session == y.flags_per_session &&
           x.had_clean == y.had_clean;
}

// Everything the object keeps, the history as an observer sees it (Get).
struct Seen {
    int32_t n_sessions, fs, other_rates;
    bool force_sparse, may_lag, split_used;
    int64_t near_pos;
    int32_t deferred_lag;
    std::vector<int32_t> rates;
    std::vector<uint8_t> modes;
    bool operator==(const Seen &b) const {
        return n_sessions == b.n_sessions && fs == b.fs && other_rates == b.other_rates && force_sparse == b.force_sparse && may_lag == b.may_lag &&
               split_used == b.split_used && near_pos == b.near_pos && deferred_lag == b.deferred_lag && rates == b.rates && modes == b.modes;
    }
};
Seen See(const TickObject &o) {
    Seen s{o.n_sessions, o.fs, o.other_rates, o.force_sparse, o.lag.may_lag, o.history.split_used, o.near_pos, o.lag.deferred_lag, o.rates, {}};
    for (int32_t k = 0; k < o.n_sessions; ++k) s.modes.push_back(o.history.Get(k));
    return s;
}
Seen See(const RefObject &o) {
    Seen s{o.S, o.fs, o.OtherRates(), o.force_sparse, o.lag.may_lag, o.h.split_used, o.near_pos, o.lag.deferred_lag, o.rates, {}};
    for (int32_t k = 0; k < o.S; ++k) s.modes.push_back(o.h.Get(k));
    return s;
}

uint64_t Next(uint64_t &x) {
    x ^= x << 13; x ^= x >> 7; x ^= x << 17;
    return x;
}

// Random ticks (and now and then a session initialised anew, at either rate) through the planner and through RefTick.  Returns -1,
// or the tick at which they differed; *what = 1 the code, 2 a plan field, 3 the bases, 4 the object after the tick, 5 a refused tick
// changed the object, 6 planning twice gave two plans, 7 the per-session codes.  seen[family] = accepted ticks of that family,
// seen[kTickFamilies] = refused ticks.
int64_t Fuzz(uint64_t seed, int32_t S, int64_t ticks, int32_t *what, int64_t *seen) {
    uint64_t rng = seed * 0x9e3779b97f4a7c15ull + 0x2545f4914f6cdd1dull;
    TickObject o;
    RefObject ref;
    o.Init(S, 16000);
    ref.Init(S, 16000);
    std::vector<uint8_t> flags((size_t)S);
    std::vector<int16_t> ms((size_t)S);
    std::vector<int32_t> codes((size_t)S), want_codes((size_t)S);
    // per Init: most ticks carry a clean plane or most do not, and (era_split) the same third of the sessions goes without theirs --
    // the callers keep their kind, so that ticks of every family are accepted and not only the first of each era
    bool era_clean = false, era_split = false;
    for (int64_t t = 0; t < ticks; ++t) {
        const uint64_t r = Next(rng);
        if (r % 97 == 0) {                                        // Init: everything anew
            const int32_t fs = (r >> 8) & 1 ? 8000 : 16000;
            o.Init(S, fs);
            ref.Init(S, fs);
            era_clean = ((r >> 10) & 1) != 0;
            era_split = ((r >> 11) & 1) != 0;
        }
        if (r % 11 == 0) {                                        // a session initialised at a rate of its own (a snapshot arriving)
            const int32_t s = (int32_t)((r >> 16) % (uint64_t)S), fs = (r >> 12) % 4 == 0 ? 24000 - ref.fs : ref.fs;
            o.InitSession(s, fs);
            ref.rates[(size_t)s] = fs;
            ref.h.ResetSession(s);
        }
        if (r % 53 == 0) o.force_sparse = ref.force_sparse = ((r >> 9) & 1) != 0;
        Tick k;
        // flag bytes: a regime per tick (nobody idle, most idle, everybody idle; no other bit, few bits, any bits), so that every
        // family and every refusal comes up often
        const int regime = (int)((r >> 20) % 8), idle_in = (int)((r >> 24) % 4), per_session = (r >> 28) % 4 != 0;
        const uint8_t bits = regime < 3 ? 0 : regime == 3 ? kFlowNoFarend : regime == 4 ? kFlowNoClean : regime == 5 ? (kFlowNoFarend | kFlowHalfCall | kFlowNoClean) : 0xff;
        for (int32_t s = 0; s < S; ++s) {
            const uint64_t q = Next(rng);
            uint8_t f = (uint8_t)(q & bits & ~(uint64_t)kFlowIdle);
            if (regime == 4 && (r >> 30) % 3 == 0) f = kFlowNoClean;                             // (everybody without)
            if (regime != 4 && regime != 7) f = (uint8_t)((f & ~kFlowNoClean) | (era_split && s % 3 == 1 ? kFlowNoClean : 0));
            const bool idle = idle_in == 0 ? false : idle_in == 1 ? (q >> 8) % 4 == 0 : idle_in == 2 ? (q >> 8) % 16 != 0 : true;
            flags[(size_t)s] = idle ? (uint8_t)(kFlowIdle | (q >> 16)) : f;                      // an idle session's other bits are junk
            ms[(size_t)s] = (int16_t)((q >> 32) % 64 == 0 ? (int)((q >> 40) % 2000) - 700 : (int)((q >> 40) % 500));
        }
        k.a.flags_per_session = per_session ? flags.data() : nullptr;
        k.a.flags = per_session ? 0 : (int)((r >> 32) % 8 == 0 ? (r >> 36) & 31 : (r >> 36) & (kFlowNoFarend | kFlowSplitCalls));
        k.n_samples = (r >> 42) % 64 == 0 ? 81 : (r >> 41) & 1 ? 80 : 160;
        k.a.n = (int)k.n_samples;
        k.a.calls = (r >> 44) % 3 != 0 ? 1 : (int32_t)((r >> 46) % 8);                             // (0 and 7: out of range)
        k.stride = (int64_t)k.n_samples * (k.a.calls > 0 ? k.a.calls : 1) - ((r >> 50) % 64 == 0);
        k.a.packets = ((r >> 51) & 1) != 0;
        k.a.has_clean = era_clean != ((r >> 52) % 16 == 0);
        k.a.host_pointers = ((r >> 53) & 1) != 0;
        k.a.ms_per_session = ((r >> 54) & 1) != 0;
        k.has_far = (r >> 55) % 8 != 0;
        k.has_near_and_out = (r >> 58) % 64 != 0;
        k.poisoned = (r >> 40) % 128 == 1;
        k.fast = (r >> 33) % 128 != 1;
        const Seen before = See(o);
        TickPlan dry, again, plan;
        const int32_t dry_rc = Run(o, k, false, &dry);
        if (!(See(o) == before)) { *what = 5; return t; }
        if (Run(o, k, false, &again) != dry_rc || !SamePlan(dry, again)) { *what = 6; return t; }
        const int32_t rc = Run(o, k, true, &plan);
        if (rc != dry_rc || (rc == 0 && !SamePlan(dry, plan))) { *what = 6; return t; }
        if (rc != 0 && !(See(o) == before)) { *what = 5; return t; }
        const RefResult w = RefTick(ref, k.a, k.has_far, k.has_near_and_out, k.n_samples, k.stride, k.poisoned, k.fast);
        if (rc != w.code) { *what = 1; return t; }
        ++seen[rc == 0 ? (int)plan.family : (int)kTickFamilies];
        if (rc == 0) {
            if (plan.live != w.live || plan.span != w.span || plan.any != w.any || plan.half_calls != w.half_calls || plan.k_calls != w.k_calls ||
                plan.split_tick != w.split_tick || plan.clean_count != w.clean_count || plan.plain_count != w.plain_count || plan.clean_plane != w.clean_plane ||
                plan.need_slot != w.need_slot || plan.zero_out != w.zero_out || plan.mixed_plan != w.mixed_plan || (int32_t)plan.family != w.family ||
                plan.route.launch != w.route.launch || plan.route.sparse_plan != w.route.sparse_plan || plan.route.sparse_tick != w.route.sparse_tick ||
                plan.route.deferred_lag != w.route.deferred_lag || plan.lag_after.deferred_lag != ref.lag.deferred_lag || plan.lag_after.may_lag != ref.lag.may_lag) {
                *what = 2;
                return t;
            }
            if (plan.route.sparse_tick && o.Bases(plan) != w.bases) { *what = 3; return t; }
            // the codes: the warning for an msInSndCardBuf out of range, 0 for a session that sits out
            const int16_t one = ms[0];
            const int32_t first = TickCodes(k.a.ms_per_session ? ms.data() : nullptr, one, k.a.flags_per_session, S, codes.data());
            int32_t want_first = k.a.ms_per_session ? 0 : (one < 0 || one > 500 ? kTickWarning : 0);
            for (int32_t s = 0; s < S; ++s) {
                const int16_t m = k.a.ms_per_session ? ms[(size_t)s] : one;
                const bool idle = k.a.flags_per_session && (flags[(size_t)s] & kFlowIdle);
                want_codes[(size_t)s] = !idle && (m < 0 || m > 500) ? kTickWarning : 0;
                if (k.a.ms_per_session && want_first == 0) want_first = want_codes[(size_t)s];
            }
            if (first != want_first || codes != want_codes) { *what = 7; return t; }
        }
        if (!(See(o) == See(ref))) { *what = 4; return t; }
    }
    return -1;
}

}  // namespace

extern "C" {

int32_t tickplan_families(void) { return kTickFamilies; }
const char *tickplan_family_name(int32_t family) { return TickFamilyName(family); }

void *tickplan_new(int32_t n_sessions, int32_t fs) {
    TickObject *o = new TickObject();
    o->Init(n_sessions, fs ? fs : 16000);
    o->fs = fs;                                   // (0: as an object that was never initialised)
    return o;
}
void tickplan_free(void *o) { delete static_cast<TickObject *>(o); }
void tickplan_init_session(void *o, int32_t session, int32_t fs) { static_cast<TickObject *>(o)->InitSession(session, fs); }
void tickplan_force_sparse(void *o, int32_t on) { static_cast<TickObject *>(o)->force_sparse = on != 0; }
// The object's other switches that a plan reads: WebRtcAecmSessions_SetSplitCallTicks, and the two traces (which = 0 the session
// trace, 1 the call trace; returns 0 where the planner refuses the attachment: the other kind is attached).
void tickplan_split_call_ticks(void *o, int32_t on) { static_cast<TickObject *>(o)->split_call_ticks = on != 0; }
int32_t tickplan_attach_trace(void *o, int32_t which, int32_t on) {
    TickObject *t = static_cast<TickObject *>(o);
    return which ? t->AttachCallTrace(on != 0) : t->AttachTrace(on != 0);
}
// counts = {ticks of the session trace, call slots of the call trace}
void tickplan_trace_counts(void *o, int64_t *counts) {
    const TickObject *t = static_cast<TickObject *>(o);
    counts[0] = t->trace_ticks;
    counts[1] = t->call_trace_calls;
}

// One tick.  args = {flags, n_samples, calls, stride, packets, has_clean, host_pointers, ms_per_session, has_far, has_near_and_out, poisoned,
// fast, commit}; out = {family, live, span, sparse_plan, sparse_tick, deferred_lag handed over, mixed_plan, need_slot, zero_out, clean_plane,
// split_tick, clean_count, plain_count, half_calls, checked}.  Returns the code.
int32_t tickplan_tick(void *obj, const uint8_t *flags_per_session, const int64_t *args, int32_t *out) {
    Tick k;
    k.a.flags_per_session = flags_per_session;
    k.a.flags = (int)args[0];
    k.n_samples = (size_t)args[1];
    k.a.n = (int)args[1];
    k.a.calls = (int32_t)args[2];
    k.stride = args[3];
    k.a.packets = args[4] != 0;
    k.a.has_clean = args[5] != 0;
    k.a.host_pointers = args[6] != 0;
    k.a.ms_per_session = args[7] != 0;
    k.has_far = args[8] != 0;
    k.has_near_and_out = args[9] != 0;
    k.poisoned = args[10] != 0;
    k.fast = args[11] != 0;
    TickPlan p;
    const int32_t rc = Run(*static_cast<TickObject *>(obj), k, args[12] != 0, &p);
    const int32_t fields[15] = {(int32_t)p.family, p.live, p.span, p.route.sparse_plan, p.route.sparse_tick, p.route.deferred_lag, p.mixed_plan, p.need_slot,
                                p.zero_out, p.clean_plane, p.split_tick, p.clean_count, p.plain_count, p.half_calls, p.clean_tick.checked};
    memcpy(out, fields, sizeof fields);
    return rc;
}
// rest = {near_pos, deferred_lag, may_lag, split_used, other_rates}; modes[S] as GetSessionCleanMode gives them
void tickplan_state(void *obj, int64_t *rest, uint8_t *modes) {
    const Seen s = See(*static_cast<TickObject *>(obj));
    const int64_t fields[5] = {s.near_pos, s.deferred_lag, s.may_lag, s.split_used, s.other_rates};
    memcpy(rest, fields, sizeof fields);
    memcpy(modes, s.modes.data(), s.modes.size());
}
int32_t tickplan_codes(const int16_t *ms_per_session, int32_t ms, const uint8_t *flags_per_session, int32_t n_sessions, int32_t *codes) {
    return TickCodes(ms_per_session, (int16_t)ms, flags_per_session, n_sessions, codes);
}
int64_t tickplan_fuzz(uint64_t seed, int32_t n_sessions, int64_t ticks, int32_t *what, int64_t *seen) { return Fuzz(seed, n_sessions, ticks, what, seen); }

}  // extern "C"

#if defined(SIM_TICKPLAN_MAIN)
int main() {
    for (int32_t S : {1, 5, 256, 257, 600}) {
        int32_t what = 0;
        int64_t seen[kTickFamilies + 1] = {0};
        const int64_t at = Fuzz(7u + (uint64_t)S, S, 10000, &what, seen);
        if (at >= 0) {
            printf("S %d: tick %lld, what %d\n", S, (long long)at, what);
            return 1;
        }
        printf("S %d:", S);
        for (int f = 0; f <= kTickFamilies; ++f) printf(" %s %lld", f < kTickFamilies ? TickFamilyName(f) : "refused", (long long)seen[f]);
        printf("\n");
    }
    printf("ok\n");
    return 0;
}
#endif
