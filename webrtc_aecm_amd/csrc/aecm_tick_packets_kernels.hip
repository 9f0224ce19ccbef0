// The packet tick of the streaming sessions (WebRtcAecmSessions_TickPackets): one tick is one PACKET of K = 2 .. 6 10 ms calls per
// session, in an object that holds sessions of both rates and both call sizes.  A session's samples are packed: a decoded 20 ms
// G.711 packet is 160 contiguous samples at the start of its row -- two calls of n_s = 80 -- next to a wideband session's 320.
//   aecm_flow_plan_packets_kernel   one LANE per session: what aecm_flow_plan_calls_kernel does, at the lane's own rate and call
//                                   size (FlowTickPackets) -> K packed plans per session (aecm_tick_packets_plan_kernels.hip)
//   aecm_tick_packets_kernel        one WAVEFRONT per live session: aecm_tick_calls_kernel's text (aecm_tick_calls_body.inc) with the
//                                   call's sample count and the row step read from the session's plans (n_frames * 80, wave-uniform)
//                                   instead of the launch: call c appends n_s samples at near position near_pos + c n_s and uses
//                                   the rows at c n_s; c * 80 samples are still 8-byte aligned, so the four-samples-per-lane path stays
// It serves full-size and half-call sessions alike; the samples [K n_s, K n) of a half-call session's rows are neither read nor
// written.  A unit of its own: the kernels of aecm_tick_calls_kernels.hip stay, instruction for instruction, what they were
// (tests/golden/tick_calls_fingerprints.json).  Compiled with that unit's flags (build.py: SOURCE_FLAGS).
#define AECM_TABLE_ATTR __device__
#define AECM_CHECK_UNIT tick_packets      // (aecm_kernel_common.h: the unit's pair of audit counters)
#include "aecm_kernel_common.h"

namespace aecm {

// This unit's share of the audit counters of the -DAECM_CHECKED build (aecm_ops.h); hipErrorNotSupported in the shipped build.
AECM_DEFINE_CHECK_COUNTERS(ReadTickPacketsCheckCounters)

#include "aecm_tick_unit.h"

// Wavefront w of the grid serves session live[w], w < live_count: the K-call tick kernel, but every session with the call size its
// own plans name (the planning kernel gave every one of a session's K plans the same n_frames).
template <bool kHasClean>
__global__ __launch_bounds__(64 * kTickCallsWaves) __attribute__((amdgpu_waves_per_eu(AECM_TICK_CALLS_WAVES_PER_EU, 8)))
void aecm_tick_packets_kernel(StatePtrs st, TickIo io, TickFlowIo fio, int n_streams, const uint32_t *__restrict__ live, int live_count, int calls) {
#define AECM_TICK_CALLS_SIZE_OF_LAUNCH
#define AECM_TICK_CALLS_SIZE_OF_PLAN const int n = p.n_frames * kFlowFrame;
#include "aecm_tick_calls_body.inc"
}

hipError_t LaunchTickPackets(const StatePtrs &st, const TickIo &io, const TickFlowIo &fio, const TickSparseIo &sp, int n_streams, int live_count,
                             int calls, hipStream_t stream) {
    if (n_streams <= 0) return hipSuccess;
    if (live_count < 0 || live_count > n_streams || !sp.live || !sp.block_base || calls < 1 || calls > kFlowMaxTickCalls) return hipErrorInvalidValue;
    // the planning launch runs over ALL sessions (the idle ones count their lag); the tick launch over the live ones only
    if (const hipError_t e = LaunchPlanPackets(st, io, fio, sp, n_streams, calls, stream)) return e;
    if (live_count > 0) {
        const dim3 grid((live_count + kTickCallsWaves - 1) / kTickCallsWaves), block(64 * kTickCallsWaves);
        const size_t lds = sizeof(LdsTables);
        if (io.clean_in) hipLaunchKernelGGL((aecm_tick_packets_kernel<true>), grid, block, lds, stream, st, io, fio, n_streams, sp.live, live_count, calls);
        else hipLaunchKernelGGL((aecm_tick_packets_kernel<false>), grid, block, lds, stream, st, io, fio, n_streams, sp.live, live_count, calls);
    }
    return hipGetLastError();
}

}  // namespace aecm
