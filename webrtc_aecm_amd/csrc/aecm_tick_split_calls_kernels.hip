// The split K-call and the split packet tick of the streaming sessions (WebRtcAecmSessions_SetSplitCallTicks): a tick of K = 2 .. 6
// call pairs per session that carries a clean near-end plane, in which some of the calling sessions' WebRtcAecm_Process calls get
// their clean rows and the others' get nearendClean = NULL (AECM_SESSION_NO_CLEAN) -- the 20 / 40 / 60 ms packet clock of a server
// with legs behind a noise suppressor and legs without one, in ONE planning launch and one tick launch PER KIND.
//   aecm_flow_plan_split_calls_kernel / aecm_flow_plan_split_packets_kernel
//                                     one LANE per session: what aecm_flow_plan_calls_kernel / aecm_flow_plan_packets_kernel do, with
//                                     the two live lists of the split tick (aecm_tick_split_calls_plan_kernels.hip; aecm_flow_clean.h)
//   aecm_tick_split_calls_kernel<kHasClean> / aecm_tick_split_packets_kernel<kHasClean>
//                                     one WAVEFRONT per calling session of ONE list: the loop-form tick body
//                                     (aecm_tick_calls_body.inc) under a name of this unit, <true> over live[0 .. clean_count),
//                                     <false> over live[plain_start .. + plain_count)
// A session without a clean input runs two forward transforms per block instead of three; neither its clean rows (all K pieces) nor
// its clean ring row are touched: the <false> body names io.clean_in and io.clean_ring nowhere.  One launch per list, not a fused
// kernel: the one-call fused kernel (aecm_tick_split_kernels.hip) already spills several hundred scalars, and the loop body fills
// its vector registers.  A unit of its own: the kernels of aecm_tick_calls_kernels.hip and aecm_tick_packets_kernels.hip stay,
// instruction for instruction, what they were (tests/golden/tick_calls_fingerprints.json).  Compiled with those units' flags
// (build.py: SOURCE_FLAGS).
#define AECM_TABLE_ATTR __device__
#define AECM_CHECK_UNIT tick_split_calls      // (aecm_kernel_common.h: the unit's pair of audit counters)
#include "aecm_kernel_common.h"

#include "aecm_flow_clean.h"      // (behind the HIP headers: aecm_flow_plan.h takes __forceinline__ from them)

namespace aecm {

// This unit's share of the audit counters of the -DAECM_CHECKED build (aecm_ops.h); hipErrorNotSupported in the shipped build.
AECM_DEFINE_CHECK_COUNTERS(ReadTickSplitCallsCheckCounters)

#include "aecm_tick_unit.h"
static_assert(kTickCallsWaves == kFlowSplitGroup, "the second list starts at a workgroup boundary of the tick kernel");

// Wavefront w of the grid serves session live[w], w < live_count, of the list the launch was given: aecm_tick_calls_kernel's text.
template <bool kHasClean>
__global__ __launch_bounds__(64 * kTickCallsWaves) __attribute__((amdgpu_waves_per_eu(AECM_TICK_CALLS_WAVES_PER_EU, 8)))
void aecm_tick_split_calls_kernel(StatePtrs st, TickIo io, TickFlowIo fio, int n_streams, const uint32_t *__restrict__ live, int live_count, int calls) {
#define AECM_TICK_CALLS_SIZE_OF_LAUNCH const int n = io.n;
#define AECM_TICK_CALLS_SIZE_OF_PLAN
#include "aecm_tick_calls_body.inc"
#undef AECM_TICK_CALLS_SIZE_OF_LAUNCH
#undef AECM_TICK_CALLS_SIZE_OF_PLAN
}

// The same with every session's call size taken from its own plans: aecm_tick_packets_kernel's text.
template <bool kHasClean>
__global__ __launch_bounds__(64 * kTickCallsWaves) __attribute__((amdgpu_waves_per_eu(AECM_TICK_CALLS_WAVES_PER_EU, 8)))
void aecm_tick_split_packets_kernel(StatePtrs st, TickIo io, TickFlowIo fio, int n_streams, const uint32_t *__restrict__ live, int live_count, int calls) {
#define AECM_TICK_CALLS_SIZE_OF_LAUNCH
#define AECM_TICK_CALLS_SIZE_OF_PLAN const int n = p.n_frames * kFlowFrame;
#include "aecm_tick_calls_body.inc"
#undef AECM_TICK_CALLS_SIZE_OF_LAUNCH
#undef AECM_TICK_CALLS_SIZE_OF_PLAN
}

// A split tick has sessions of both kinds and a clean plane (all of one kind: the caller takes the K-call / packet tick of that kind).
static bool SplitCallsTickArgsValid(const TickIo &io, const TickFlowIo &fio, const TickSparseIo &sp, const TickSplitIo &split, int n_streams, int calls) {
    return split.clean_count > 0 && split.plain_count > 0 && split.clean_count + split.plain_count <= n_streams && io.clean_in && io.clean_ring && sp.live &&
           fio.plans && calls >= 1 && calls <= kFlowMaxTickCalls && split.plain_start == FlowPlainListStart((uint32_t)split.clean_count) &&
           io.io_stride >= (int64_t)calls * io.n;
}

hipError_t LaunchTickSplitCalls(const StatePtrs &st, const TickIo &io, const TickFlowIo &fio, const TickSparseIo &sp, const TickSplitIo &split, int n_streams,
                                int calls, hipStream_t stream) {
    if (n_streams <= 0) return hipSuccess;
    if (!SplitCallsTickArgsValid(io, fio, sp, split, n_streams, calls)) return hipErrorInvalidValue;
    // the planning launch runs over ALL sessions (the idle ones count their lag); the tick launches over the calling ones only
    if (const hipError_t e = LaunchPlanSplitCalls(io, fio, sp, split, n_streams, calls, stream)) return e;
    const dim3 clean_grid((split.clean_count + kTickCallsWaves - 1) / kTickCallsWaves), plain_grid((split.plain_count + kTickCallsWaves - 1) / kTickCallsWaves);
    const dim3 block(64 * kTickCallsWaves);
    const size_t lds = sizeof(LdsTables);
    hipLaunchKernelGGL((aecm_tick_split_calls_kernel<true>), clean_grid, block, lds, stream, st, io, fio, n_streams, sp.live, split.clean_count, calls);
    hipLaunchKernelGGL((aecm_tick_split_calls_kernel<false>), plain_grid, block, lds, stream, st, io, fio, n_streams, sp.live + split.plain_start,
                       split.plain_count, calls);
    return hipGetLastError();
}

hipError_t LaunchTickSplitPackets(const StatePtrs &st, const TickIo &io, const TickFlowIo &fio, const TickSparseIo &sp, const TickSplitIo &split, int n_streams,
                                  int calls, hipStream_t stream) {
    if (n_streams <= 0) return hipSuccess;
    if (!SplitCallsTickArgsValid(io, fio, sp, split, n_streams, calls)) return hipErrorInvalidValue;
    if (const hipError_t e = LaunchPlanSplitPackets(st, io, fio, sp, split, n_streams, calls, stream)) return e;
    const dim3 clean_grid((split.clean_count + kTickCallsWaves - 1) / kTickCallsWaves), plain_grid((split.plain_count + kTickCallsWaves - 1) / kTickCallsWaves);
    const dim3 block(64 * kTickCallsWaves);
    const size_t lds = sizeof(LdsTables);
    hipLaunchKernelGGL((aecm_tick_split_packets_kernel<true>), clean_grid, block, lds, stream, st, io, fio, n_streams, sp.live, split.clean_count, calls);
    hipLaunchKernelGGL((aecm_tick_split_packets_kernel<false>), plain_grid, block, lds, stream, st, io, fio, n_streams, sp.live + split.plain_start,
                       split.plain_count, calls);
    return hipGetLastError();
}

}  // namespace aecm
