// The planning lane of a tick in which sessions may sit out (kFlowIdle) or may have done so before (aecm_flow_plan.h: F_NEAR_LAG),
// one lane per session, as TEXT: included between the braces of every planning kernel but the dense one (aecm_flow_plan_kernel) --
// aecm_flow_plan_sparse_kernel and FlowPlanMixedBody (aecm_kernels.hip), aecm_flow_plan_calls_kernel, aecm_flow_plan_packets_kernel,
// aecm_flow_plan_split_kernel -- behind the lines that name the lane's session and fill the live list (aecm_flow_plan_list.inc; the
// split kernel has its own, for two lists).  A text rather than a function for the reason aecm_tick_flow_body.inc gives: every one
// of those kernels stays, instruction for instruction, what it was (as a __forceinline__ function template that takes the planning
// step as a lambda, aecm_flow_plan_calls_kernel came out 161 assembly lines shorter).
//
// An idle lane adds the tick to its session's lag and touches nothing else.  A live lane brings its session back in step first
// (FlowResync: the pending near-end samples, fewer than one block, move behind the object's position -- rare, and at most 63
// samples per ring), once, before its first call, then plans the tick and stores the session's fields and its plan(s).
//
// In scope: fio, sp, n, near_pos, n_streams (the kernel's arguments); s, in_range, live, flags (the lines before).  The hooks, which
// this text undefines again:
//   AECM_FLOW_PLAN_IDLE_SAMPLES   the samples an idle lane adds to its lag, the WHOLE tick: `n`, or `calls * n` in a tick of K calls
// and ONE of the two planning steps, a statement each, with r (FlowRegs) and ms in scope:
//   AECM_FLOW_PLAN_TICK(p)        plans one call pair into `FlowPlan p` (FlowTick, FlowTickMixed); the plan goes to
//                                 fio.plans[s][kFlowPlanWords]
//   AECM_FLOW_PLAN_CALLS(emit)    plans `calls` (in scope) call pairs, handing every one to emit(c, plan) (FlowTickCalls,
//                                 FlowTickPackets); the plans go to fio.plans[s][calls][kFlowPlanWords]
// and, with AECM_FLOW_PLAN_CALLS only, an optional statement at the end of emit, with c, p and -- directly behind call c's FlowTick
// -- r in scope (nothing where the includer defines none: every kernel without it keeps its tokens):
//   AECM_FLOW_PLAN_CALL_RECORD    the call trace's planning kernels (aecm_call_trace_plan_kernels.hip) store the wrapper half of
//                                 call c's record here
#if !defined(AECM_FLOW_PLAN_CALL_RECORD)
#define AECM_FLOW_PLAN_CALL_RECORD
#endif
    if (!in_range) return;
    int32_t *lag = fio.state + (size_t)F_NEAR_LAG * n_streams + s;
    if (!live) {
        *lag = FlowIdleTick(FlowIdleTick(*lag, sp.deferred_lag), AECM_FLOW_PLAN_IDLE_SAMPLES);
        return;
    }
    FlowRegs r;
    for (int k = 0; k < kFlowFieldsUsed; ++k) r.v[k] = fio.state[(size_t)k * n_streams + s];
    r.v[F_NEAR_LAG] = FlowIdleTick(r.v[F_NEAR_LAG], sp.deferred_lag);
    if (r.v[F_NEAR_LAG] != 0) {
        FlowNearMove m;
        FlowResync(r, near_pos, m);
        const uint32_t mask = (uint32_t)sp.ring_len - 1u;
        FlowMoveNear(sp.near_ring + (size_t)s * sp.ring_len, mask, m);
        if (sp.clean_ring) FlowMoveNear(sp.clean_ring + (size_t)s * sp.ring_len, mask, m);
    }
    const int ms = fio.ms_per_session ? (int)fio.ms_per_session[s] : fio.ms;
#if defined(AECM_FLOW_PLAN_TICK)
    FlowPlan p;
    AECM_FLOW_PLAN_TICK(p);
    for (int k = 0; k < kFlowFieldsUsed; ++k) fio.state[(size_t)k * n_streams + s] = r.v[k];
    int32_t w[kFlowPlanWords];
    FlowPackPlan(p, w);
    int4 *dst = reinterpret_cast<int4 *>(fio.plans + (size_t)s * kFlowPlanWords);
    for (int q = 0; q < kFlowPlanWords / 4; ++q) dst[q] = make_int4(w[4 * q], w[4 * q + 1], w[4 * q + 2], w[4 * q + 3]);
#undef AECM_FLOW_PLAN_TICK
#else
    int4 *dst = reinterpret_cast<int4 *>(fio.plans + (size_t)s * calls * kFlowPlanWords);
    AECM_FLOW_PLAN_CALLS(([&](int c, const FlowPlan &p) {
        int32_t w[kFlowPlanWords];
        FlowPackPlan(p, w);
        for (int q = 0; q < kFlowPlanWords / 4; ++q) dst[c * (kFlowPlanWords / 4) + q] = make_int4(w[4 * q], w[4 * q + 1], w[4 * q + 2], w[4 * q + 3]);
        AECM_FLOW_PLAN_CALL_RECORD
    }));
    for (int k = 0; k < kFlowFieldsUsed; ++k) fio.state[(size_t)k * n_streams + s] = r.v[k];
#undef AECM_FLOW_PLAN_CALLS
#endif
#undef AECM_FLOW_PLAN_CALL_RECORD
#undef AECM_FLOW_PLAN_IDLE_SAMPLES
