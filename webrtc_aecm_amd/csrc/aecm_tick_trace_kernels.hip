// The traced twins of the tick kernels of one call pair per session (aecm_kernels.hip: aecm_tick_flow_kernel,
// aecm_tick_flow_sparse_kernel; aecm_tick_split_kernels.hip: aecm_tick_split_kernel, aecm_tick_split_list_kernel): the same ticks
// with a session trace attached (include/aecm_batch.h: AecmSessionTrace, WebRtcAecmSessions_SetSessionTrace).  Besides its output
// frames every session that calls writes one 64-byte record of where it stands behind the tick -- start-up, the delay the wrapper
// steers by, the jitter buffer's fill, and the core's AecmBlockTrace after the tick's last block:
//   aecm_tick_traced_dense_kernel        one wavefront per session
//   aecm_tick_traced_live_kernel         wavefront w serves session live[w]
//   aecm_tick_traced_split_kernel        the fused split tick (both bodies, by workgroup)
//   aecm_tick_traced_split_list_kernel   the split tick, one launch per list
// (no name contains the dense kernel's: tests find that one by its name and expect one match per instantiation).
//
// A unit of its own: the untraced kernels' instruction streams stay what they are, and a tick without a trace runs what it always
// ran.  A twin is the body's text (aecm_tick_flow_body.inc) unchanged, followed by the record.  The body hands its registers to
// run_stream_loaded by reference, so behind it early_r holds the core's uniform state as store_state wrote it -- for a session
// that ran no block (start-up) the state as loaded --, and p, s, lane and fio are still in scope.  The planning launch of the
// same tick has written the wrapper words, so the record reads them where ExportSession would: fio.state, eleven wave-uniform
// loads brought to the scalar side by readfirstlane.
//
// The record (aecm_session_trace.h: the one text of the wrapper half): eight words packed on the scalar side go into lanes 0..7
// with v_writelane, BlockEngine::block_trace_row is moved to lanes 8..15, and lanes 0..15 store one 64-byte row -- a plain vector
// store, like the audio's.  Compiled with the tick units' flags (build.py: SOURCE_FLAGS).
#define AECM_TABLE_ATTR __device__
#define AECM_CHECK_UNIT tick_trace      // (aecm_kernel_common.h: the unit's pair of audit counters)
#include "aecm_kernel_common.h"

#include "aecm_flow_clean.h"      // (behind the HIP headers: aecm_flow_plan.h takes __forceinline__ from them)
#include "aecm_session_trace.h"

namespace aecm {

// This unit's share of the audit counters (see ReadCheckCounters in aecm_kernels.hip).
AECM_DEFINE_CHECK_COUNTERS(ReadTickTraceCheckCounters)

#include "aecm_tick_unit.h"
static_assert(AECM_TICK_EARLY_STATE_LOAD, "the record reads the registers the body loaded ahead of its table fill (early_r)");
static_assert(kTickFlowWaves == kFlowSplitGroup, "the second list starts at a workgroup boundary of the tick kernel");
static_assert(kSessionTraceWords == kSessionTraceHeaderWords + kTraceWords && kSessionTraceWords == 16, "a record is one row of sixteen lanes");

// The record of session s behind its tick, word k in lane k (lanes 16..63: nothing a store takes).  r: the body's early_r;
// n_blocks: the plan's.
template <class E>
__device__ __forceinline__ int SessionTraceRow(const typename E::Regs &r, int n_blocks, const TickFlowIo &fio, int n_streams, int64_t s,
                                               const SessionTraceView &tv) {
    using W = Gfx950Wave<true, true, true>;
    int32_t flow[kFlowFieldsUsed] = {};
#define AECM_SESSION_TRACE_LOAD(f) flow[f] = __builtin_amdgcn_readfirstlane(fio.state[(size_t)(f) * n_streams + s]);
    AECM_SESSION_TRACE_FIELDS(AECM_SESSION_TRACE_LOAD)
#undef AECM_SESSION_TRACE_LOAD
    uint32_t w[kSessionTraceHeaderWords];
    SessionTraceHeaderWords(flow, tv.tick, n_blocks, r.u.mult == 2 ? 16 : 8, w);
    // the core half: words 0..7 in lanes 0..7 -> lanes 8..15 (row_shr:8 inside the row of sixteen; lanes 0..7 read 0)
    int row = __builtin_amdgcn_update_dpp(0, E::block_trace_row(r), 0x118, 0xf, 0xf, true);
    for (int k = 0; k < kSessionTraceHeaderWords; ++k) row = W::writelane(row, (int)w[k], k);
    return row;
}
// Lanes 0..15 store it as one 64-byte row.  Only called for s < n_streams, so the address is inside the caller's records.
__device__ __forceinline__ void StoreSessionTraceRow(const SessionTraceView &tv, int64_t s, int lane, int row) {
    Gfx950Wave<true, true, true>::store_out_u32_if(lane < kSessionTraceWords, tv.records + (s * tv.session_stride + tv.tick_slot_offset) * kSessionTraceWords,
                                                   lane, row);
}

// In every twin the body and the row stand in a lambda (always inlined) and the store behind it, under s < n_streams.  The body
// leaves by `return` where its wavefront serves nobody; in the kernel's own scope that edge would run past the record to the
// kernel's end, the body would no longer be a region with one exit, and the compiler would structurize the whole kernel --
// in the fused split kernel it then lays one copy of the body behind the other, takes the second copy's plan words for
// clobbered by the first copy's stores, fetches them with vector loads, and the body's scalar constraints on them cannot be
// met.  From the lambda a `return` lands in front of the store's test: one exit, and the uniform regions stay unstructurized
// as they are in the untraced kernels.
template <bool kHasClean>
__global__ __launch_bounds__(64 * kTickFlowWaves) __attribute__((amdgpu_waves_per_eu(AECM_TICK_FLOW_WAVES_PER_EU, 8)))
void aecm_tick_traced_dense_kernel(StatePtrs st, TickIo io, TickFlowIo fio, int n_streams, SessionTraceView tv) {
    const int64_t s = (int64_t)blockIdx.x * kTickFlowWaves + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int lane = threadIdx.x & 63;
    int row = 0;
    [&]() __attribute__((always_inline)) {
#include "aecm_tick_flow_body.inc"
        row = SessionTraceRow<EarlyE>(early_r, nb, fio, n_streams, s, tv);
    }();
    if (s < n_streams) StoreSessionTraceRow(tv, s, lane, row);
}

template <bool kHasClean>
__global__ __launch_bounds__(64 * kTickFlowWaves) __attribute__((amdgpu_waves_per_eu(AECM_TICK_FLOW_WAVES_PER_EU, 8)))
void aecm_tick_traced_live_kernel(StatePtrs st, TickIo io, TickFlowIo fio, int n_streams, const uint32_t *__restrict__ live, int live_count,
                                  SessionTraceView tv) {
    const int64_t wave_id = (int64_t)blockIdx.x * kTickFlowWaves + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    AECM_TICK_LIVE_SESSION(live, live_count, wave_id)
    const int lane = threadIdx.x & 63;
    int row = 0;
    [&]() __attribute__((always_inline)) {
#include "aecm_tick_flow_body.inc"
        row = SessionTraceRow<EarlyE>(early_r, nb, fio, n_streams, s, tv);
    }();
    if (s < n_streams) StoreSessionTraceRow(tv, s, lane, row);
}

// (aecm_tick_split_kernel's text: the branch is uniform over the workgroup, either copy of the body takes the table fill's barrier
// with all of a workgroup's wavefronts or with none.)
__global__ __launch_bounds__(64 * kTickFlowWaves) __attribute__((amdgpu_waves_per_eu(AECM_TICK_FLOW_WAVES_PER_EU, 8)))
void aecm_tick_traced_split_kernel(StatePtrs st, TickIo io, TickFlowIo fio, int n_streams, const uint32_t *__restrict__ live, int clean_count,
                                   int clean_groups, int plain_count, SessionTraceView tv) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    int row = 0;
    int64_t session = n_streams;
    if ((int)blockIdx.x < clean_groups) {
        [&]() __attribute__((always_inline)) {
            constexpr bool kHasClean = true;
            const int64_t wave_id = (int64_t)blockIdx.x * kTickFlowWaves + wave;
            AECM_TICK_LIVE_SESSION(live, clean_count, wave_id)
            session = s;
#include "aecm_tick_flow_body.inc"
            row = SessionTraceRow<EarlyE>(early_r, nb, fio, n_streams, s, tv);
        }();
    } else {
        [&]() __attribute__((always_inline)) {
            constexpr bool kHasClean = false;
            const uint32_t *__restrict__ plain = live + (int64_t)clean_groups * kTickFlowWaves;
            const int64_t wave_id = ((int64_t)blockIdx.x - clean_groups) * kTickFlowWaves + wave;
            AECM_TICK_LIVE_SESSION(plain, plain_count, wave_id)
            session = s;
#include "aecm_tick_flow_body.inc"
            row = SessionTraceRow<EarlyE>(early_r, nb, fio, n_streams, s, tv);
        }();
    }
    if (session < n_streams) StoreSessionTraceRow(tv, session, lane, row);
}

template <bool kHasClean>
__global__ __launch_bounds__(64 * kTickFlowWaves) __attribute__((amdgpu_waves_per_eu(AECM_TICK_FLOW_WAVES_PER_EU, 8)))
void aecm_tick_traced_split_list_kernel(StatePtrs st, TickIo io, TickFlowIo fio, int n_streams, const uint32_t *__restrict__ live, int live_count,
                                        SessionTraceView tv) {
    const int64_t wave_id = (int64_t)blockIdx.x * kTickFlowWaves + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    AECM_TICK_LIVE_SESSION(live, live_count, wave_id)
    const int lane = threadIdx.x & 63;
    int row = 0;
    [&]() __attribute__((always_inline)) {
#include "aecm_tick_flow_body.inc"
        row = SessionTraceRow<EarlyE>(early_r, nb, fio, n_streams, s, tv);
    }();
    if (s < n_streams) StoreSessionTraceRow(tv, s, lane, row);
}

// ---- launchers: the untraced ones' (aecm_kernels.hip, aecm_tick_split_kernels.hip), by the SAME planning launches, with the trace
// view as one more argument of the tick launch ---------------------------------------------------------------------------------
static bool TraceViewUsable(const SessionTraceView &tv) {
    return tv.records && !(reinterpret_cast<uintptr_t>(tv.records) & 3) && tv.session_stride > 0 && tv.tick_slot_offset >= 0;
}

hipError_t LaunchTickFlowTraced(const StatePtrs &st, const TickIo &io, const TickFlowIo &fio, const SessionTraceView &tv, int n_streams, hipStream_t stream) {
    if (n_streams <= 0) return hipSuccess;
    if (!TraceViewUsable(tv) || TickWorkgroupWaves() != kTickFlowWaves) return hipErrorInvalidValue;
    if (const hipError_t e = LaunchPlanFlow(st, io, fio, nullptr, n_streams, false, stream)) return e;
    const dim3 grid((n_streams + kTickFlowWaves - 1) / kTickFlowWaves), block(64 * kTickFlowWaves);
    const size_t lds = sizeof(LdsTables);
    if (io.clean_in) hipLaunchKernelGGL((aecm_tick_traced_dense_kernel<true>), grid, block, lds, stream, st, io, fio, n_streams, tv);
    else hipLaunchKernelGGL((aecm_tick_traced_dense_kernel<false>), grid, block, lds, stream, st, io, fio, n_streams, tv);
    return hipGetLastError();
}

hipError_t LaunchTickFlowSparseTraced(const StatePtrs &st, const TickIo &io, const TickFlowIo &fio, const TickSparseIo &sp, const SessionTraceView &tv,
                                      int n_streams, int live_count, hipStream_t stream, bool mixed_plan) {
    if (n_streams <= 0) return hipSuccess;
    if (live_count < 0 || live_count > n_streams || (sp.live && !sp.block_base)) return hipErrorInvalidValue;
    if (!TraceViewUsable(tv) || TickWorkgroupWaves() != kTickFlowWaves) return hipErrorInvalidValue;
    if (const hipError_t e = LaunchPlanFlow(st, io, fio, &sp, n_streams, mixed_plan, stream)) return e;
    const dim3 block(64 * kTickFlowWaves);
    const size_t lds = sizeof(LdsTables);
    if (!sp.live) {                        // nobody idles in this tick: everybody is live, the dense tick
        const dim3 grid((n_streams + kTickFlowWaves - 1) / kTickFlowWaves);
        if (io.clean_in) hipLaunchKernelGGL((aecm_tick_traced_dense_kernel<true>), grid, block, lds, stream, st, io, fio, n_streams, tv);
        else hipLaunchKernelGGL((aecm_tick_traced_dense_kernel<false>), grid, block, lds, stream, st, io, fio, n_streams, tv);
    } else if (live_count > 0) {
        const dim3 grid((live_count + kTickFlowWaves - 1) / kTickFlowWaves);
        if (io.clean_in) hipLaunchKernelGGL((aecm_tick_traced_live_kernel<true>), grid, block, lds, stream, st, io, fio, n_streams, sp.live, live_count, tv);
        else hipLaunchKernelGGL((aecm_tick_traced_live_kernel<false>), grid, block, lds, stream, st, io, fio, n_streams, sp.live, live_count, tv);
    }
    return hipGetLastError();
}

hipError_t LaunchTickSplitTraced(const StatePtrs &st, const TickIo &io, const TickFlowIo &fio, const TickSparseIo &sp, const TickSplitIo &split,
                                 const SessionTraceView &tv, int n_streams, bool mixed_plan, bool two_launches, hipStream_t stream) {
    if (n_streams <= 0) return hipSuccess;
    if (split.clean_count <= 0 || split.plain_count <= 0 || !io.clean_in || !io.clean_ring || TickWorkgroupWaves() != kTickFlowWaves) return hipErrorInvalidValue;
    if (!TraceViewUsable(tv)) return hipErrorInvalidValue;
    if (const hipError_t e = LaunchPlanSplit(st, io, fio, sp, split, n_streams, mixed_plan, stream)) return e;
    const int clean_groups = (int)(split.plain_start / (uint32_t)kTickFlowWaves), plain_groups = (split.plain_count + kTickFlowWaves - 1) / kTickFlowWaves;
    const dim3 block(64 * kTickFlowWaves);
    const size_t lds = sizeof(LdsTables);
    if (!two_launches) {
        hipLaunchKernelGGL(aecm_tick_traced_split_kernel, dim3(clean_groups + plain_groups), block, lds, stream, st, io, fio, n_streams, sp.live, split.clean_count,
                           clean_groups, split.plain_count, tv);
    } else {
        hipLaunchKernelGGL((aecm_tick_traced_split_list_kernel<true>), dim3(clean_groups), block, lds, stream, st, io, fio, n_streams, sp.live, split.clean_count, tv);
        hipLaunchKernelGGL((aecm_tick_traced_split_list_kernel<false>), dim3(plain_groups), block, lds, stream, st, io, fio, n_streams, sp.live + split.plain_start,
                           split.plain_count, tv);
    }
    return hipGetLastError();
}

}  // namespace aecm
