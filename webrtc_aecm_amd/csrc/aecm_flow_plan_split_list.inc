// The first lines of a planning kernel with TWO live lists, as TEXT (aecm_flow_plan_list.inc has the one-list form,
// aecm_flow_plan_lane.inc follows and says why a text): the lane's session s, whether it calls in this tick (live) and of which kind
// it is (no_clean: kFlowNoClean in its flag byte), and the session's id into its slot of the list of its kind -- each list ascending,
// the second starting at split.plain_start (aecm_flow_clean.h: FlowSplitSlot).  Lanes past the last session take part as idle ones
// (the barrier).  Included by aecm_flow_plan_split_kernel (aecm_tick_split_plan_kernels.hip) and by the planning kernels of the split
// K-call and packet ticks (aecm_tick_split_calls_plan_kernels.hip).
//
// In scope: fio, sp, split, n_streams (the kernel's arguments) and wave_counts (uint32_t[2][kFlowPlanBlock / 64], in LDS).
    const int s = blockIdx.x * 256 + threadIdx.x;
    const bool in_range = s < n_streams;
    const int flags = !in_range ? kFlowIdle : (int)fio.flags_per_session[s];
    const bool live = (flags & kFlowIdle) == 0, no_clean = (flags & kFlowNoClean) != 0;
    {
        const uint64_t ballot_clean = __ballot(live && !no_clean), ballot_plain = __ballot(live && no_clean);
        const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
        if (lane == 0) {
            wave_counts[0][wave] = (uint32_t)__builtin_popcountll(ballot_clean);
            wave_counts[1][wave] = (uint32_t)__builtin_popcountll(ballot_plain);
        }
        __syncthreads();
        const uint32_t slot = FlowSplitSlot(no_clean, sp.block_base[blockIdx.x], split.plain_base[blockIdx.x], split.plain_start, wave_counts, wave,
                                            ballot_clean, ballot_plain, lane);
        // (the list holds FlowSplitListEntries(n_streams); either list ends where the host counted it to end)
        const uint32_t end = no_clean ? split.plain_start + (uint32_t)split.plain_count : (uint32_t)split.clean_count;
        if (live && slot < end && slot < FlowSplitListEntries((uint32_t)n_streams)) sp.live[slot] = (uint32_t)s;
    }
