// The K-call and the packet tick with a call trace attached (include/aecm_batch.h: WebRtcAecmSessions_SetCallTrace): one 64-byte
// AecmSessionTrace record per session and CALL from the ticks that keep the core state in registers across their calls -- byte for
// byte the records that K ordinary ticks under a session trace write.  The two halves of a record come from the two launches of
// the tick, each where its half is at hand:
//   aecm_plan_calls_traced_kernel / aecm_plan_packets_traced_kernel   (aecm_call_trace_plan_kernels.hip) one LANE per session:
//                                     words 0..7, the wrapper half, from the planning lane's registers behind call c's FlowTick
//   aecm_calls_traced_tick_kernel / aecm_packets_traced_tick_kernel   one WAVEFRONT per live session: the text of
//                                     aecm_tick_calls_kernel / aecm_tick_packets_kernel (aecm_tick_calls_body.inc) with the body's
//                                     one hook filled in -- behind step 4 of call c, lanes 0..7 store BlockEngine::block_trace_row
//                                     of the registers to words 8..15 of call c's record: the core state behind the call's last
//                                     block, or, for a call that ran none, the state as it is held (as loaded, or as the calls
//                                     before left it)
// (no name contains an untraced kernel's: tests find those by their names and expect one match per instantiation).  The store is a
// plain vector store, like the audio's and the block trace's (TracedIo::trace); nothing reads a record inside the launch.  The
// record sits inside the loop, in front of the call's fence, so the body's early `return` -- ahead of the loop -- leaves the loop
// the region it was (aecm_tick_trace_kernels.hip tells what an exit past a record did to the one-call twins).  Where the record
// lies is walked call by call on the scalar side (CallTraceNextSlot: no division); a ring shorter than the tick stores only the
// last call of every slot (CallTraceStored), as the planning kernels do.
//
// A unit of its own: the untraced kernels' instruction streams stay what they are, and a tick without a trace runs what it always
// ran.  Compiled with the tick units' flags (build.py: SOURCE_FLAGS).
#define AECM_TABLE_ATTR __device__
#define AECM_CHECK_UNIT call_trace      // (aecm_kernel_common.h: the unit's pair of audit counters)
#include "aecm_kernel_common.h"

namespace aecm {

// This unit's share of the audit counters (see ReadCheckCounters in aecm_kernels.hip).
AECM_DEFINE_CHECK_COUNTERS(ReadCallTraceCheckCounters)

#include "aecm_tick_unit.h"
static_assert(kSessionTraceWords == kSessionTraceHeaderWords + kTraceWords, "the core half is the block trace's row");

// Words 8..15 of session s's record in ring slot `slot`: word k of the row is in lane k.  Only called for s < n_streams (the body
// has returned otherwise), so the address is inside the caller's records.
template <class E>
__device__ __forceinline__ void StoreCallTraceCore(const typename E::Regs &r, const CallTraceView &cv, int64_t s, int slot) {
    Gfx950Wave<true, true, true>::store_out_u32_if(r.lane < kTraceWords, cv.records + CallTraceRecord(cv, s, slot) * kSessionTraceWords + kSessionTraceHeaderWords,
                                                   r.lane, E::block_trace_row(r));
}
// (the hook of aecm_tick_calls_body.inc is aecm_session_trace.h's AECM_CALL_TRACE_TICK_RECORD: c, calls, r, s, E in scope;
// trace_slot declared ahead of the text)

template <bool kHasClean>
__global__ __launch_bounds__(64 * kTickCallsWaves) __attribute__((amdgpu_waves_per_eu(AECM_TICK_CALLS_WAVES_PER_EU, 8)))
void aecm_calls_traced_tick_kernel(StatePtrs st, TickIo io, TickFlowIo fio, int n_streams, const uint32_t *__restrict__ live, int live_count, int calls,
                                   CallTraceView cv) {
    int trace_slot = cv.first_slot;
#define AECM_TICK_CALLS_SIZE_OF_LAUNCH const int n = io.n;
#define AECM_TICK_CALLS_SIZE_OF_PLAN
#define AECM_TICK_CALLS_AFTER_BLOCKS AECM_CALL_TRACE_TICK_RECORD
#include "aecm_tick_calls_body.inc"
#undef AECM_TICK_CALLS_SIZE_OF_LAUNCH
#undef AECM_TICK_CALLS_SIZE_OF_PLAN
}

template <bool kHasClean>
__global__ __launch_bounds__(64 * kTickCallsWaves) __attribute__((amdgpu_waves_per_eu(AECM_TICK_CALLS_WAVES_PER_EU, 8)))
void aecm_packets_traced_tick_kernel(StatePtrs st, TickIo io, TickFlowIo fio, int n_streams, const uint32_t *__restrict__ live, int live_count, int calls,
                                     CallTraceView cv) {
    int trace_slot = cv.first_slot;
#define AECM_TICK_CALLS_SIZE_OF_LAUNCH
#define AECM_TICK_CALLS_SIZE_OF_PLAN const int n = p.n_frames * kFlowFrame;
#define AECM_TICK_CALLS_AFTER_BLOCKS AECM_CALL_TRACE_TICK_RECORD
#include "aecm_tick_calls_body.inc"
#undef AECM_TICK_CALLS_SIZE_OF_LAUNCH
#undef AECM_TICK_CALLS_SIZE_OF_PLAN
}

// ---- launchers: the untraced ones' (aecm_tick_calls_kernels.hip, aecm_tick_packets_kernels.hip), by the traced planning launches,
// with the trace view as one more argument of both launches -------------------------------------------------------------------
hipError_t LaunchTickCallsTraced(const StatePtrs &st, const TickIo &io, const TickFlowIo &fio, const TickSparseIo &sp, const CallTraceView &cv, int n_streams,
                                 int live_count, int calls, hipStream_t stream) {
    if (n_streams <= 0) return hipSuccess;
    if (live_count < 0 || live_count > n_streams || !sp.live || !sp.block_base || calls < 1 || calls > kFlowMaxTickCalls) return hipErrorInvalidValue;
    // the planning launch runs over ALL sessions (the idle ones count their lag); the tick launch over the live ones only
    if (const hipError_t e = LaunchPlanCallsTraced(io, fio, sp, cv, n_streams, calls, stream)) return e;      // (refuses a view nothing can be written by)
    if (live_count > 0) {
        const dim3 grid((live_count + kTickCallsWaves - 1) / kTickCallsWaves), block(64 * kTickCallsWaves);
        const size_t lds = sizeof(LdsTables);
        if (io.clean_in) hipLaunchKernelGGL((aecm_calls_traced_tick_kernel<true>), grid, block, lds, stream, st, io, fio, n_streams, sp.live, live_count, calls, cv);
        else hipLaunchKernelGGL((aecm_calls_traced_tick_kernel<false>), grid, block, lds, stream, st, io, fio, n_streams, sp.live, live_count, calls, cv);
    }
    return hipGetLastError();
}

hipError_t LaunchTickPacketsTraced(const StatePtrs &st, const TickIo &io, const TickFlowIo &fio, const TickSparseIo &sp, const CallTraceView &cv, int n_streams,
                                   int live_count, int calls, hipStream_t stream) {
    if (n_streams <= 0) return hipSuccess;
    if (live_count < 0 || live_count > n_streams || !sp.live || !sp.block_base || calls < 1 || calls > kFlowMaxTickCalls) return hipErrorInvalidValue;
    if (const hipError_t e = LaunchPlanPacketsTraced(st, io, fio, sp, cv, n_streams, calls, stream)) return e;
    if (live_count > 0) {
        const dim3 grid((live_count + kTickCallsWaves - 1) / kTickCallsWaves), block(64 * kTickCallsWaves);
        const size_t lds = sizeof(LdsTables);
        if (io.clean_in) hipLaunchKernelGGL((aecm_packets_traced_tick_kernel<true>), grid, block, lds, stream, st, io, fio, n_streams, sp.live, live_count, calls, cv);
        else hipLaunchKernelGGL((aecm_packets_traced_tick_kernel<false>), grid, block, lds, stream, st, io, fio, n_streams, sp.live, live_count, calls, cv);
    }
    return hipGetLastError();
}

}  // namespace aecm
