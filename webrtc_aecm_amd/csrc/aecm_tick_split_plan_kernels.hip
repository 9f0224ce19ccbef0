// The planning kernels of a split tick (aecm_tick_split_kernels.hip has the tick kernel and the whole picture; aecm_flow_clean.h the
// two lists).  A unit of its own for the reason aecm_tick_calls_plan_kernels.hip gives: these kernels run one LANE per session, every
// branch of FlowTick diverges, and the unit is built without -structurizecfg-skip-uniform-regions.
#include <initializer_list>

#include <hip/hip_runtime.h>

#include "aecm_flow_clean.h"
#include "aecm_kernels.h"

namespace aecm {

// One lane per session: the planning lane of the sparse tick (kMixed: of the mixed tick -- the lane takes its session's rate from
// the core state and plans with FlowTickMixed; aecm_flow_plan_lane.inc), behind first lines for two live lists in place of one
// (aecm_flow_plan_split_list.inc): a calling lane's id goes to the list of its kind (kFlowNoClean in its flag byte: the sessions whose Process gets no clean
// pointer), each list ascending, the second starting at split.plain_start.  A session without a clean input keeps a clean ring row
// all the same; nothing reads it, so the resync may move it along with the near ring like everybody's.
static_assert(kFlowPlanBlock == 256, "the planning kernels run 256 lanes per workgroup");
template <bool kMixed>
__global__ __launch_bounds__(256)
void aecm_flow_plan_split_kernel(TickFlowIo fio, TickSparseIo sp, TickSplitIo split, const int32_t *__restrict__ scal, int n, unsigned near_pos, int n_streams) {
    __shared__ uint32_t wave_counts[2][kFlowPlanBlock / 64];
#include "aecm_flow_plan_split_list.inc"
#define AECM_FLOW_PLAN_IDLE_SAMPLES n
#define AECM_FLOW_PLAN_TICK(p)                                                                                      \
    if (kMixed) FlowTickMixed(r, scal[(size_t)s * kNumScal + S_MULT] == 2 ? 16000 : 8000, n, ms, flags, near_pos, p); \
    else FlowTick(r, fio.fs, n, ms, flags, near_pos, p)
#include "aecm_flow_plan_lane.inc"
}

hipError_t LaunchPlanSplit(const StatePtrs &st, const TickIo &io, const TickFlowIo &fio, const TickSparseIo &sp, const TickSplitIo &split, int n_streams,
                           bool mixed_plan, hipStream_t stream) {
    if (n_streams <= 0) return hipSuccess;
    if (!sp.live || !sp.block_base || !split.plain_base || !fio.flags_per_session || split.clean_count < 0 || split.plain_count < 0 ||
        split.clean_count + split.plain_count > n_streams || split.plain_start != FlowPlainListStart((uint32_t)split.clean_count))
        return hipErrorInvalidValue;
    const dim3 grid((n_streams + 255) / 256), block(256);
    if (mixed_plan) hipLaunchKernelGGL((aecm_flow_plan_split_kernel<true>), grid, block, 0, stream, fio, sp, split, st.scal, io.n, (unsigned)io.near_pos, n_streams);
    else hipLaunchKernelGGL((aecm_flow_plan_split_kernel<false>), grid, block, 0, stream, fio, sp, split, st.scal, io.n, (unsigned)io.near_pos, n_streams);
    return hipGetLastError();
}

}  // namespace aecm
