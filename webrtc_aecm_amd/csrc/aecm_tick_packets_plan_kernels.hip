// The planning kernel of the packet tick (aecm_tick_packets_kernels.hip has the tick kernel and the whole picture).  A unit of its
// own for the reason aecm_tick_calls_plan_kernels.hip gives: one LANE per session, every branch of FlowTick diverges, so it is built
// WITHOUT -structurizecfg-skip-uniform-regions -- and apart from that unit, so that aecm_flow_plan_calls_kernel stays, instruction
// for instruction, what it was (tests/golden/tick_calls_fingerprints.json).
#include <initializer_list>

#include <hip/hip_runtime.h>

#include "aecm_kernels.h"

namespace aecm {

// One lane per session: aecm_flow_plan_calls_kernel's text (aecm_flow_plan_list.inc, aecm_flow_plan_lane.inc) with two differences.
// The lane's rate is its session's (the core state's S_MULT, what the block engine itself goes by -- as aecm_flow_plan_mixed_kernel),
// and the planning is FlowTickPackets: the lane's call size is 80 where its flag byte carries kFlowHalfCall in a 160-sample tick,
// and what it did not consume of the tick becomes its lag.
static_assert(kFlowPlanBlock == 256, "the planning kernels run 256 lanes per workgroup");
__global__ __launch_bounds__(256)
void aecm_flow_plan_packets_kernel(TickFlowIo fio, TickSparseIo sp, const int32_t *__restrict__ scal, int n, int calls, unsigned near_pos, int n_streams) {
    __shared__ uint32_t wave_counts[kFlowPlanBlock / 64];
#define AECM_FLOW_PLAN_LIST_GUARD
#include "aecm_flow_plan_list.inc"
#define AECM_FLOW_PLAN_IDLE_SAMPLES calls * n
#define AECM_FLOW_PLAN_CALLS(emit) \
    FlowTickPackets(r, scal[(size_t)s * kNumScal + S_MULT] == 2 ? 16000 : 8000, n, calls, ms, flags, near_pos, emit)
#include "aecm_flow_plan_lane.inc"
}

hipError_t LaunchPlanPackets(const StatePtrs &st, const TickIo &io, const TickFlowIo &fio, const TickSparseIo &sp, int n_streams, int calls,
                             hipStream_t stream) {
    if (n_streams <= 0) return hipSuccess;
    if (!sp.live || !sp.block_base || !st.scal || calls < 1 || calls > kFlowMaxTickCalls) return hipErrorInvalidValue;
    hipLaunchKernelGGL(aecm_flow_plan_packets_kernel, dim3((n_streams + 255) / 256), dim3(256), 0, stream, fio, sp, st.scal, io.n, calls,
                       (unsigned)io.near_pos, n_streams);
    return hipGetLastError();
}

}  // namespace aecm
