// The K-call tick of the streaming sessions (WebRtcAecmSessions_TickCalls): K = 2 .. 6 [BufferFarend] + Process call pairs
// of n samples per session in ONE planning launch and ONE tick launch -- the 20 / 40 / 60 ms packet interval of a media
// server on 10 ms calls.  K ordinary ticks load and store a session's core state K times; here it is loaded once, stays in
// registers across the K call pairs, and is stored once.
//   aecm_flow_plan_calls_kernel   one LANE per session: what aecm_flow_plan_sparse_kernel does (idle lanes, resync, the live
//                                 list), then FlowTickCalls -> K packed plans per session (aecm_tick_calls_plan_kernels.hip)
//   aecm_tick_calls_kernel        one WAVEFRONT per live session: for c = 0 .. K - 1 the five steps of a tick (append, spill,
//                                 far framing, blocks, output frames) with plan c and the rows offset by c * n
// A unit of its own: the tick kernels of aecm_kernels.hip stay, instruction for instruction, what they were.  Compiled with
// that unit's flags (build.py: SOURCE_FLAGS).
#define AECM_TABLE_ATTR __device__
#define AECM_CHECK_UNIT tick_calls      // (aecm_kernel_common.h: the unit's pair of audit counters)
#include "aecm_kernel_common.h"

namespace aecm {

// This unit's share of the audit counters of the -DAECM_CHECKED build (aecm_ops.h); hipErrorNotSupported in the shipped build.
AECM_DEFINE_CHECK_COUNTERS(ReadTickCallsCheckCounters)

#include "aecm_tick_unit.h"

// Wavefront w of the grid serves session live[w], w < live_count (ascending ids; the id wave-uniform and in a scalar register
// before anything is addressed by it).  The state loads are issued once, ahead of the table fill -- and ahead of every fence
// and every wide store of the kernel, so that the scalar half of the state arrives through scalar loads; the state stores
// happen once, behind the last call (not at all for a session whose K calls ran no block: still in its start-up phase).
template <bool kHasClean>
__global__ __launch_bounds__(64 * kTickCallsWaves) __attribute__((amdgpu_waves_per_eu(AECM_TICK_CALLS_WAVES_PER_EU, 8)))
void aecm_tick_calls_kernel(StatePtrs st, TickIo io, TickFlowIo fio, int n_streams, const uint32_t *__restrict__ live, int live_count, int calls) {
#define AECM_TICK_CALLS_SIZE_OF_LAUNCH const int n = io.n;
#define AECM_TICK_CALLS_SIZE_OF_PLAN
#include "aecm_tick_calls_body.inc"
}

hipError_t LaunchTickCalls(const StatePtrs &st, const TickIo &io, const TickFlowIo &fio, const TickSparseIo &sp, int n_streams, int live_count,
                           int calls, hipStream_t stream) {
    if (n_streams <= 0) return hipSuccess;
    if (live_count < 0 || live_count > n_streams || !sp.live || !sp.block_base || calls < 1 || calls > kFlowMaxTickCalls) return hipErrorInvalidValue;
    // the planning launch runs over ALL sessions (the idle ones count their lag); the tick launch over the live ones only
    if (const hipError_t e = LaunchPlanCalls(io, fio, sp, n_streams, calls, stream)) return e;
    if (live_count > 0) {
        const dim3 grid((live_count + kTickCallsWaves - 1) / kTickCallsWaves), block(64 * kTickCallsWaves);
        const size_t lds = sizeof(LdsTables);
        if (io.clean_in) hipLaunchKernelGGL((aecm_tick_calls_kernel<true>), grid, block, lds, stream, st, io, fio, n_streams, sp.live, live_count, calls);
        else hipLaunchKernelGGL((aecm_tick_calls_kernel<false>), grid, block, lds, stream, st, io, fio, n_streams, sp.live, live_count, calls);
    }
    return hipGetLastError();
}

}  // namespace aecm
