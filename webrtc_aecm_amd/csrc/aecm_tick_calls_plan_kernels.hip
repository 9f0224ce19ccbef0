// The planning kernel of the K-call tick (aecm_tick_calls_kernels.hip has the tick kernel and the whole picture).  A unit of its
// own because it is built WITHOUT the flags of the tick kernels' units: -structurizecfg-skip-uniform-regions is for kernels whose
// branches are wave-uniform, and this kernel runs one LANE per session -- every branch of FlowTick diverges.  Built with that flag,
// the loop over the calls came out wrong on the MI355X: lanes that skip a call's frames (a session in its start-up phase) were
// taken for lanes with active frames at the end of FlowTick, and their F_FF_VALID was cleared (found by the 4 100-session test:
// the snapshot of a session that had not left the start-up phase differed from its twin's in that one word).
#include <initializer_list>

#include <hip/hip_runtime.h>

#include "aecm_kernels.h"

namespace aecm {

// One lane per session: the planning lane of the sparse tick (aecm_flow_plan_list.inc, aecm_flow_plan_lane.inc) with the list
// always filled and K plans per session (FlowTickCalls).
static_assert(kFlowPlanBlock == 256, "the planning kernels run 256 lanes per workgroup");
__global__ __launch_bounds__(256)
void aecm_flow_plan_calls_kernel(TickFlowIo fio, TickSparseIo sp, int n, int calls, unsigned near_pos, int n_streams) {
    __shared__ uint32_t wave_counts[kFlowPlanBlock / 64];
#define AECM_FLOW_PLAN_LIST_GUARD
#include "aecm_flow_plan_list.inc"
#define AECM_FLOW_PLAN_IDLE_SAMPLES calls * n
#define AECM_FLOW_PLAN_CALLS(emit) FlowTickCalls(r, fio.fs, n, calls, ms, flags, near_pos, emit)
#include "aecm_flow_plan_lane.inc"
}

hipError_t LaunchPlanCalls(const TickIo &io, const TickFlowIo &fio, const TickSparseIo &sp, int n_streams, int calls, hipStream_t stream) {
    if (n_streams <= 0) return hipSuccess;
    if (!sp.live || !sp.block_base || calls < 1 || calls > kFlowMaxTickCalls) return hipErrorInvalidValue;
    hipLaunchKernelGGL(aecm_flow_plan_calls_kernel, dim3((n_streams + 255) / 256), dim3(256), 0, stream, fio, sp, io.n, calls, (unsigned)io.near_pos, n_streams);
    return hipGetLastError();
}

}  // namespace aecm
