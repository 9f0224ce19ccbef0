// The first lines of a planning kernel with ONE live list, as TEXT (aecm_flow_plan_lane.inc follows and says why a text): the lane's
// session s, whether it calls in this tick (live), and the session's id into its slot of the list -- wave ballot + mbcnt within the
// wavefront, LDS across the workgroup's four wavefronts, the host's prefix count (sp.block_base) across workgroups: ascending ids,
// no atomics.  Lanes past the last session take part as idle ones (the barrier).
//
// In scope: fio, sp, n_streams (the kernel's arguments) and wave_counts (uint32_t[kFlowPlanBlock / 64], in LDS).  The hook, which
// this text undefines again:
//   AECM_FLOW_PLAN_LIST_GUARD   `if (sp.live)` where the list is optional (the sparse and the mixed tick: nobody idles in this tick,
//                               the dense tick kernel follows -- uniform, a kernel argument); empty where the launcher insists on
//                               a list (K-call and packet ticks)
    const int s = blockIdx.x * 256 + threadIdx.x;
    const bool in_range = s < n_streams;
    const int flags = !in_range ? kFlowIdle : fio.flags_per_session ? (int)fio.flags_per_session[s] : fio.flags;
    const bool live = (flags & kFlowIdle) == 0;
    AECM_FLOW_PLAN_LIST_GUARD {
        const uint64_t ballot = __ballot(live);
        const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
        if (lane == 0) wave_counts[wave] = (uint32_t)__builtin_popcountll(ballot);
        __syncthreads();
        const uint32_t slot = FlowLiveSlot(sp.block_base[blockIdx.x], wave_counts, wave, ballot, lane);
        if (live && slot < (uint32_t)n_streams) sp.live[slot] = (uint32_t)s;      // (the list holds n_streams entries)
    }
#undef AECM_FLOW_PLAN_LIST_GUARD
