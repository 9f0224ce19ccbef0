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
#if defined(AECM_CHECKED)
#define g_aecm_check_fail g_aecm_check_fail_tick_split      // device symbols are per translation unit (no relocatable device code)
#endif
#include "aecm_kernel_common.h"

#include "aecm_flow_clean.h"      // (behind the HIP headers: aecm_flow_plan.h takes __forceinline__ from them)

namespace aecm {

#if defined(AECM_CHECKED)
__device__ unsigned long long g_aecm_check_fail_tick_split[2];
#endif
// This unit's share of the audit counters of the -DAECM_CHECKED build (aecm_ops.h); hipErrorNotSupported in the shipped build.
hipError_t ReadTickSplitCheckCounters(uint64_t counters[2], bool reset) {
#if defined(AECM_CHECKED)
    unsigned long long host[2] = {0, 0};
    hipError_t e = hipMemcpyFromSymbol(host, HIP_SYMBOL(g_aecm_check_fail_tick_split), sizeof host);
    if (e != hipSuccess) return e;
    counters[0] = host[0];
    counters[1] = host[1];
    if (reset) {
        const unsigned long long zero[2] = {0, 0};
        e = hipMemcpyToSymbol(HIP_SYMBOL(g_aecm_check_fail_tick_split), zero, sizeof zero);
    }
    return e;
#else
    (void)counters;
    (void)reset;
    return hipErrorNotSupported;
#endif
}

// What aecm_tick_flow_body.inc expects of the unit that includes it, as aecm_kernels.hip has it: the blocks' view of the session's
// rings, and the build's choices for the tick kernels (the same defaults; LaunchTickSplit checks the workgroup size against
// TickWorkgroupWaves() of that unit).
template <bool kHasClean, class Append>
struct TickFlowBlockIo {
    using E = BlockEngine<Gfx950Wave<true, true, true>, kHasClean>;
    using Regs = typename E::Regs;
    const int16_t *far_src;          // the far ring itself (direct ticks) or the framed far stream
    const int16_t *nr, *cr;          // near / clean rings of this session
    int16_t *out_row;                // output stream ring
    int far_mask, mask;
    unsigned far_pos, near_pos, out_pos;      // positions of the tick's first block in far_src / the near rings / the output ring
    const Append &append;            // the tick's samples -> rings
    __device__ __forceinline__ int far(const Regs &r, int b) const { return far_src[(far_pos + b * kBlock + r.lane) & far_mask]; }
    __device__ __forceinline__ int near(const Regs &r, int b) const { return nr[(near_pos + b * kBlock + r.lane) & mask]; }
    __device__ __forceinline__ int clean(const Regs &r, int b) const { return cr[(near_pos + b * kBlock + r.lane) & mask]; }
    __device__ __forceinline__ void out(const Regs &r, int b, int v) const { out_row[(out_pos + b * kBlock + r.brev) & mask] = (int16_t)v; }
    // (aecm_kernels.hip: the tick's samples go into the rings behind the engine's state loads, then this wave's fetches see them)
    __device__ __forceinline__ void ready() const {
        append();
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    }
};
#ifndef AECM_TICK_FLOW_WAVES
#define AECM_TICK_FLOW_WAVES 4
#endif
#ifndef AECM_TICK_EARLY_STATE_LOAD
#define AECM_TICK_EARLY_STATE_LOAD 1
#endif
#ifndef AECM_TICK_SPLIT_PLAN_WORDS
#define AECM_TICK_SPLIT_PLAN_WORDS 1
#endif
#ifndef AECM_TICK_FLOW_WAVES_PER_EU
#if defined(AECM_CHECKED)
#define AECM_TICK_FLOW_WAVES_PER_EU 4
#else
#define AECM_TICK_FLOW_WAVES_PER_EU 7      // (aecm_kernels.hip: the scalar budget of 8 waves per SIMD costs the body hundreds of scalar spills)
#endif
#endif
constexpr int kTickFlowWaves = AECM_TICK_FLOW_WAVES;
static_assert(kTickFlowWaves == kFlowSplitGroup, "the second list starts at a workgroup boundary of the tick kernel");

// Workgroups [0, clean_groups) serve live[0 .. clean_count), the others live[4 clean_groups .. + plain_count): the branch is on
// blockIdx.x against a kernel argument -- uniform over the workgroup, so the barrier of the table fill inside either copy of the body
// is taken by all of a workgroup's wavefronts or by none.  As in aecm_tick_flow_sparse_kernel the session's id is wave-uniform and in
// a scalar register before anything is addressed by it, and a wavefront past its list's end serves nobody but still takes the
// barrier (s = n_streams makes it leave behind it).  The body is the one text of the other tick kernels, once per kind, each in a
// scope of its own.
__global__ __launch_bounds__(64 * kTickFlowWaves) __attribute__((amdgpu_waves_per_eu(AECM_TICK_FLOW_WAVES_PER_EU, 8)))
void aecm_tick_split_kernel(StatePtrs st, TickIo io, TickFlowIo fio, int n_streams, const uint32_t *__restrict__ live, int clean_count, int clean_groups,
                            int plain_count) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if ((int)blockIdx.x < clean_groups) {
        constexpr bool kHasClean = true;
        const int64_t wave_id = (int64_t)blockIdx.x * kTickFlowWaves + wave;
        const uint32_t id = (uint32_t)__builtin_amdgcn_readfirstlane((int)live[wave_id < clean_count ? wave_id : 0]);
        const int64_t s = wave_id < clean_count && id < (uint32_t)n_streams ? (int64_t)id : (int64_t)n_streams;
#include "aecm_tick_flow_body.inc"
    } else {
        constexpr bool kHasClean = false;
        const uint32_t *__restrict__ plain = live + (int64_t)clean_groups * kTickFlowWaves;
        const int64_t wave_id = ((int64_t)blockIdx.x - clean_groups) * kTickFlowWaves + wave;
        const uint32_t id = (uint32_t)__builtin_amdgcn_readfirstlane((int)plain[wave_id < plain_count ? wave_id : 0]);
        const int64_t s = wave_id < plain_count && id < (uint32_t)n_streams ? (int64_t)id : (int64_t)n_streams;
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
    const uint32_t id = (uint32_t)__builtin_amdgcn_readfirstlane((int)live[wave_id < live_count ? wave_id : 0]);
    const int64_t s = wave_id < live_count && id < (uint32_t)n_streams ? (int64_t)id : (int64_t)n_streams;
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
