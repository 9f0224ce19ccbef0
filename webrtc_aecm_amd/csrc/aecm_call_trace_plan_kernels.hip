// The planning kernels of the K-call and the packet tick with a call trace attached (include/aecm_batch.h:
// WebRtcAecmSessions_SetCallTrace; aecm_call_trace_kernels.hip has the tick kernels and the whole picture): twins of
// aecm_flow_plan_calls_kernel and aecm_flow_plan_packets_kernel -- the same texts (aecm_flow_plan_list.inc, aecm_flow_plan_lane.inc)
// with the lane's one hook filled in.  The planning lane hands every call's plan to its sink while it still holds that call's
// wrapper words in registers: directly behind call c's FlowTick they are what ExportSession would show directly after that call
// pair.  So the sink also writes the wrapper half of call c's record -- the eight words of SessionTraceHeaderWords
// (aecm_session_trace.h, the one text of the layout) with the call's slot number, its n_blocks and the session's own rate -- straight
// into the caller's buffer, as two 16-byte stores per call.  The tick kernel then has no wrapper word to fetch (the per-tick twins
// of aecm_tick_trace_kernels.hip pay eleven loads and readfirstlanes for them) and adds only the core half.
//   aecm_plan_calls_traced_kernel     every session at the object's rate (fio.fs)
//   aecm_plan_packets_traced_kernel   every session at its own rate (the core state's S_MULT)
// (no name contains an untraced kernel's: tests find those by their names and expect one match each).  Idle lanes and lanes past
// the last session return before any record (aecm_flow_plan_lane.inc).  A record's address is the caller's geometry, 4-byte
// aligned like the buffer: the two stores are 16 bytes wide and 4-byte aligned, which global memory takes.
//
// A unit of its own, so that the untraced planning kernels stay what they were, and built WITHOUT the flags of the tick units for
// the reason aecm_tick_calls_plan_kernels.hip gives: one LANE per session, every branch of FlowTick diverges.
#include <initializer_list>

#include <hip/hip_runtime.h>

#include "aecm_kernels.h"

namespace aecm {

static_assert(kFlowPlanBlock == 256, "the planning kernels run 256 lanes per workgroup");
static_assert(kSessionTraceHeaderWords == 8, "the wrapper half is two 16-byte stores");

// Call c's wrapper half into the record in ring slot `slot` of session s.  r: the lane's registers behind call c's FlowTick.
typedef uint32_t CallTraceQuad __attribute__((ext_vector_type(4), aligned(4)));
__device__ __forceinline__ void StoreCallTraceHeader(const CallTraceView &cv, int s, int slot, const FlowRegs &r, int c, int blocks, int khz) {
    uint32_t w[kSessionTraceHeaderWords];
    CallTraceHeaderWords(cv, r.v, c, blocks, khz, w);
    CallTraceQuad *dst = reinterpret_cast<CallTraceQuad *>(cv.records + CallTraceRecord(cv, s, slot) * kSessionTraceWords);
    dst[0] = CallTraceQuad{w[0], w[1], w[2], w[3]};
    dst[1] = CallTraceQuad{w[4], w[5], w[6], w[7]};
}
// (the hook of aecm_flow_plan_lane.inc's sink is aecm_session_trace.h's AECM_CALL_TRACE_PLAN_RECORD: c, p, r, s, calls in scope;
// trace_slot, trace_khz declared ahead of the text)

__global__ __launch_bounds__(256)
void aecm_plan_calls_traced_kernel(TickFlowIo fio, TickSparseIo sp, CallTraceView cv, int n, int calls, unsigned near_pos, int n_streams) {
    __shared__ uint32_t wave_counts[kFlowPlanBlock / 64];
#define AECM_FLOW_PLAN_LIST_GUARD
#include "aecm_flow_plan_list.inc"
    int trace_slot = cv.first_slot;
    const int trace_khz = fio.fs == 16000 ? 16 : 8;
#define AECM_FLOW_PLAN_IDLE_SAMPLES calls * n
#define AECM_FLOW_PLAN_CALLS(emit) FlowTickCalls(r, fio.fs, n, calls, ms, flags, near_pos, emit)
#define AECM_FLOW_PLAN_CALL_RECORD AECM_CALL_TRACE_PLAN_RECORD
#include "aecm_flow_plan_lane.inc"
}

__global__ __launch_bounds__(256)
void aecm_plan_packets_traced_kernel(TickFlowIo fio, TickSparseIo sp, const int32_t *__restrict__ scal, CallTraceView cv, int n, int calls, unsigned near_pos,
                                     int n_streams) {
    __shared__ uint32_t wave_counts[kFlowPlanBlock / 64];
#define AECM_FLOW_PLAN_LIST_GUARD
#include "aecm_flow_plan_list.inc"
    int trace_slot = cv.first_slot;
    const bool wideband = in_range && scal[(size_t)s * kNumScal + S_MULT] == 2;
    const int trace_khz = wideband ? 16 : 8;
#define AECM_FLOW_PLAN_IDLE_SAMPLES calls * n
#define AECM_FLOW_PLAN_CALLS(emit) FlowTickPackets(r, wideband ? 16000 : 8000, n, calls, ms, flags, near_pos, emit)
#define AECM_FLOW_PLAN_CALL_RECORD AECM_CALL_TRACE_PLAN_RECORD
#include "aecm_flow_plan_lane.inc"
}

static bool CallTraceViewUsable(const CallTraceView &cv) {
    return cv.records && !(reinterpret_cast<uintptr_t>(cv.records) & 3) && cv.session_stride > 0 && cv.call_stride > 0 && cv.ring_calls > 0 && cv.first_slot >= 0 &&
           cv.first_slot < cv.ring_calls;
}

hipError_t LaunchPlanCallsTraced(const TickIo &io, const TickFlowIo &fio, const TickSparseIo &sp, const CallTraceView &cv, int n_streams, int calls,
                                 hipStream_t stream) {
    if (n_streams <= 0) return hipSuccess;
    if (!sp.live || !sp.block_base || calls < 1 || calls > kFlowMaxTickCalls || !CallTraceViewUsable(cv)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(aecm_plan_calls_traced_kernel, dim3((n_streams + 255) / 256), dim3(256), 0, stream, fio, sp, cv, io.n, calls, (unsigned)io.near_pos,
                       n_streams);
    return hipGetLastError();
}

hipError_t LaunchPlanPacketsTraced(const StatePtrs &st, const TickIo &io, const TickFlowIo &fio, const TickSparseIo &sp, const CallTraceView &cv, int n_streams,
                                   int calls, hipStream_t stream) {
    if (n_streams <= 0) return hipSuccess;
    if (!sp.live || !sp.block_base || !st.scal || calls < 1 || calls > kFlowMaxTickCalls || !CallTraceViewUsable(cv)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(aecm_plan_packets_traced_kernel, dim3((n_streams + 255) / 256), dim3(256), 0, stream, fio, sp, st.scal, cv, io.n, calls,
                       (unsigned)io.near_pos, n_streams);
    return hipGetLastError();
}

}  // namespace aecm
