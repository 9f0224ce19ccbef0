// The planning kernels of the split K-call and the split packet tick (aecm_tick_split_calls_kernels.hip has the tick kernels and the
// whole picture; aecm_flow_clean.h the two lists).  A unit of its own for the reason aecm_tick_calls_plan_kernels.hip gives: these
// kernels run one LANE per session, every branch of FlowTick diverges, and the unit is built without
// -structurizecfg-skip-uniform-regions (with it, that unit's loop over the calls cleared F_FF_VALID of start-up sessions on the
// device) -- and apart from the other planning units, so that their kernels stay, instruction for instruction, what they were.
#include <initializer_list>

#include <hip/hip_runtime.h>

#include "aecm_flow_clean.h"
#include "aecm_kernels.h"

namespace aecm {

// One lane per session: the two-list first lines of aecm_flow_plan_split_kernel (aecm_flow_plan_split_list.inc), then the planning
// lane of the K-call tick -- K plans per session (FlowTickCalls), an idle lane falls calls * n samples behind.
static_assert(kFlowPlanBlock == 256, "the planning kernels run 256 lanes per workgroup");
__global__ __launch_bounds__(256)
void aecm_flow_plan_split_calls_kernel(TickFlowIo fio, TickSparseIo sp, TickSplitIo split, int n, int calls, unsigned near_pos, int n_streams) {
    __shared__ uint32_t wave_counts[2][kFlowPlanBlock / 64];
#include "aecm_flow_plan_split_list.inc"
#define AECM_FLOW_PLAN_IDLE_SAMPLES calls * n
#define AECM_FLOW_PLAN_CALLS(emit) FlowTickCalls(r, fio.fs, n, calls, ms, flags, near_pos, emit)
#include "aecm_flow_plan_lane.inc"
}

// The same with the planning lane of the packet tick: the lane's rate is its session's (the core state's S_MULT), its call size 80
// where its flag byte carries kFlowHalfCall in a 160-sample tick (FlowTickPackets).
__global__ __launch_bounds__(256)
void aecm_flow_plan_split_packets_kernel(TickFlowIo fio, TickSparseIo sp, TickSplitIo split, const int32_t *__restrict__ scal, int n, int calls,
                                         unsigned near_pos, int n_streams) {
    __shared__ uint32_t wave_counts[2][kFlowPlanBlock / 64];
#include "aecm_flow_plan_split_list.inc"
#define AECM_FLOW_PLAN_IDLE_SAMPLES calls * n
#define AECM_FLOW_PLAN_CALLS(emit) \
    FlowTickPackets(r, scal[(size_t)s * kNumScal + S_MULT] == 2 ? 16000 : 8000, n, calls, ms, flags, near_pos, emit)
#include "aecm_flow_plan_lane.inc"
}

// What both planning launches ask of their arguments: both lists, the host's counts per planning workgroup, per-session flags (only
// they can name a kind), the counts within the object and the second list where FlowPlainListStart puts it.
static bool SplitCallsPlanArgsValid(const TickFlowIo &fio, const TickSparseIo &sp, const TickSplitIo &split, int n_streams, int calls) {
    return sp.live && sp.block_base && split.plain_base && fio.flags_per_session && fio.plans && split.clean_count >= 0 && split.plain_count >= 0 &&
           split.clean_count + split.plain_count <= n_streams && split.plain_start == FlowPlainListStart((uint32_t)split.clean_count) && calls >= 1 &&
           calls <= kFlowMaxTickCalls;
}

hipError_t LaunchPlanSplitCalls(const TickIo &io, const TickFlowIo &fio, const TickSparseIo &sp, const TickSplitIo &split, int n_streams, int calls,
                                hipStream_t stream) {
    if (n_streams <= 0) return hipSuccess;
    if (!SplitCallsPlanArgsValid(fio, sp, split, n_streams, calls)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(aecm_flow_plan_split_calls_kernel, dim3((n_streams + 255) / 256), dim3(256), 0, stream, fio, sp, split, io.n, calls,
                       (unsigned)io.near_pos, n_streams);
    return hipGetLastError();
}

hipError_t LaunchPlanSplitPackets(const StatePtrs &st, const TickIo &io, const TickFlowIo &fio, const TickSparseIo &sp, const TickSplitIo &split,
                                  int n_streams, int calls, hipStream_t stream) {
    if (n_streams <= 0) return hipSuccess;
    if (!SplitCallsPlanArgsValid(fio, sp, split, n_streams, calls) || !st.scal) return hipErrorInvalidValue;
    hipLaunchKernelGGL(aecm_flow_plan_split_packets_kernel, dim3((n_streams + 255) / 256), dim3(256), 0, stream, fio, sp, split, st.scal, io.n, calls,
                       (unsigned)io.near_pos, n_streams);
    return hipGetLastError();
}

}  // namespace aecm
