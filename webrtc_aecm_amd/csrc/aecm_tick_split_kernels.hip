// The split tick of the streaming sessions (AECM_SESSION_NO_CLEAN): one tick that carries a clean near-end plane, in which some of
// the calling sessions' WebRtcAecm_Process gets its clean row and the others' gets nearendClean = NULL -- calls behind a noise
// suppressor and calls without one on one 10 ms clock, in ONE planning launch and ONE tick launch.
//   aecm_flow_plan_split_kernel   one LANE per session: what the sparse / mixed planning kernels do, with two live lists
//                                 (aecm_tick_split_plan_kernels.hip; aecm_flow_clean.h)
//   aecm_tick_split_kernel        one WAVEFRONT per calling session: workgroups [0, clean_groups) serve the list of the sessions with a
//                                 clean input by the tick body with a clean input, the rest serve the other list by the body without
// A session without a clean input runs two forward transforms per block instead of three; its clean row and its clean ring row are
// never touched.  A unit of its own: the tick kernels of aecm_kernels.hip stay, instruction for instruction, what they were.
// Compiled with that unit's flags (build.py: SOURCE_FLAGS).
#define AECM_TABLE_ATTR __device__
#define AECM_CHECK_UNIT tick_split      // (aecm_kernel_common.h: the unit's pair of audit counters)
#include "aecm_kernel_common.h"

#include "aecm_flow_clean.h"      // (behind the HIP headers: aecm_flow_plan.h takes __forceinline__ from them)

namespace aecm {

// This unit's share of the audit counters of the -DAECM_CHECKED build (aecm_ops.h); hipErrorNotSupported in the shipped build.
AECM_DEFINE_CHECK_COUNTERS(ReadTickSplitCheckCounters)

// What aecm_tick_flow_body.inc expects of the unit that includes it: the blocks' view of the session's rings and the build's choices
// for the tick kernels, those of aecm_kernels.hip (LaunchTickSplit checks the workgroup size against TickWorkgroupWaves() of that unit).
#include "aecm_tick_unit.h"
static_assert(kTickFlowWaves == kFlowSplitGroup, "the second list starts at a workgroup boundary of the tick kernel");

// Workgroups [0, clean_groups) serve live[0 .. clean_count), the others live[4 clean_groups .. + plain_count): the branch is on
// blockIdx.x against a kernel argument -- uniform over the workgroup, so the barrier of the table fill inside either copy of the body
// is taken by all of a workgroup's wavefronts or by none.  A wavefront finds its session as in aecm_tick_flow_sparse_kernel
// (AECM_TICK_LIVE_SESSION, aecm_tick_unit.h).  The body is the one text of the other tick kernels, once per kind, each in a
// scope of its own.
__global__ __launch_bounds__(64 * kTickFlowWaves) __attribute__((amdgpu_waves_per_eu(AECM_TICK_FLOW_WAVES_PER_EU, 8)))
void aecm_tick_split_kernel(StatePtrs st, TickIo io, TickFlowIo fio, int n_streams, const uint32_t *__restrict__ live, int clean_count, int clean_groups,
                            int plain_count) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if ((int)blockIdx.x < clean_groups) {
        constexpr bool kHasClean = true;
        const int64_t wave_id = (int64_t)blockIdx.x * kTickFlowWaves + wave;
        AECM_TICK_LIVE_SESSION(live, clean_count, wave_id)
#include "aecm_tick_flow_body.inc"
    } else {
        constexpr bool kHasClean = false;
        const uint32_t *__restrict__ plain = live + (int64_t)clean_groups * kTickFlowWaves;
        const int64_t wave_id = ((int64_t)blockIdx.x - clean_groups) * kTickFlowWaves + wave;
        AECM_TICK_LIVE_SESSION(plain, plain_count, wave_id)
#include "aecm_tick_flow_body.inc"
    }
}

// The same tick as two launches, one per list: aecm_tick_flow_sparse_kernel's text under a name of this unit (that kernel has no
// launcher of its own).  Either body alone keeps the scalar spills of the sparse tick kernel (69 and 53 scalar registers) where the
// fused kernel, one function holding both, has 551: per session this is the faster code, at the price of a second dispatch.  Large
// ticks take this form, ticks the device holds at once the fused one (SessionBatch::SplitTickTwoLaunches;
// profiles/r24_split_clean_ticks.txt has the measurement).  Results are the same.
template <bool kHasClean>
__global__ __launch_bounds__(64 * kTickFlowWaves) __attribute__((amdgpu_waves_per_eu(AECM_TICK_FLOW_WAVES_PER_EU, 8)))
void aecm_tick_split_list_kernel(StatePtrs st, TickIo io, TickFlowIo fio, int n_streams, const uint32_t *__restrict__ live, int live_count) {
    const int64_t wave_id = (int64_t)blockIdx.x * kTickFlowWaves + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    AECM_TICK_LIVE_SESSION(live, live_count, wave_id)
    const int lane = threadIdx.x & 63;
#include "aecm_tick_flow_body.inc"
}

hipError_t LaunchTickSplit(const StatePtrs &st, const TickIo &io, const TickFlowIo &fio, const TickSparseIo &sp, const TickSplitIo &split, int n_streams,
                           bool mixed_plan, bool two_launches, hipStream_t stream) {
    if (n_streams <= 0) return hipSuccess;
    // a split tick has sessions of both kinds and a clean plane (all of one kind: the caller takes the tick of that kind)
    if (split.clean_count <= 0 || split.plain_count <= 0 || !io.clean_in || !io.clean_ring || TickWorkgroupWaves() != kTickFlowWaves) return hipErrorInvalidValue;
    // the planning launch runs over ALL sessions (the idle ones count their lag); the tick launch over the calling ones only
    if (const hipError_t e = LaunchPlanSplit(st, io, fio, sp, split, n_streams, mixed_plan, stream)) return e;
    const int clean_groups = (int)(split.plain_start / (uint32_t)kTickFlowWaves), plain_groups = (split.plain_count + kTickFlowWaves - 1) / kTickFlowWaves;
    const dim3 block(64 * kTickFlowWaves);
    const size_t lds = sizeof(LdsTables);
    if (!two_launches) {
        hipLaunchKernelGGL(aecm_tick_split_kernel, dim3(clean_groups + plain_groups), block, lds, stream, st, io, fio, n_streams, sp.live, split.clean_count,
                           clean_groups, split.plain_count);
    } else {
        hipLaunchKernelGGL((aecm_tick_split_list_kernel<true>), dim3(clean_groups), block, lds, stream, st, io, fio, n_streams, sp.live, split.clean_count);
        hipLaunchKernelGGL((aecm_tick_split_list_kernel<false>), dim3(plain_groups), block, lds, stream, st, io, fio, n_streams, sp.live + split.plain_start,
                           split.plain_count);
    }
    return hipGetLastError();
}

}  // namespace aecm
