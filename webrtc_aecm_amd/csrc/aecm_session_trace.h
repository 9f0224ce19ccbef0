// The session trace (include/aecm_batch.h: AecmSessionTrace, WebRtcAecmSessions_SetSessionTrace): the 64-byte record a session
// writes at the end of a tick of one call pair -- sixteen words, the first eight from the wrapper state (FlowField) and the
// tick's plan, the last eight the core's AecmBlockTrace (BlockEngine::block_trace_row, aecm_wave.h).  This header is the ONE
// text of the wrapper half's layout: the traced tick kernels (aecm_tick_trace_kernels.hip) pack it on the scalar side, the host
// (aecm_capi.cpp asserts the struct against it) and the simulator (tests/sim/sim_session_trace.cpp) call the same function.
// The call trace (WebRtcAecmSessions_SetCallTrace: the same record per CALL of a K-call or packet tick) has its view, its walk of
// the ring and its two hooks at the end of this header.  HIP-free.
#ifndef AECM_AMD_SESSION_TRACE_H_
#define AECM_AMD_SESSION_TRACE_H_

#include <stdint.h>

#include "aecm_flow_plan.h"

namespace aecm {

constexpr int kSessionTraceHeaderWords = 8;                             // the wrapper half
constexpr int kSessionTraceWords = kSessionTraceHeaderWords + 8;        // + AecmBlockTrace (aecm_state.h: kTraceWords)

// Where the records of ONE tick go, computed on the host (SessionBatch::Enqueue): session s writes its sixteen words at
// records + kSessionTraceWords * (s * session_stride + tick_slot_offset), tick_slot_offset = (tick % ring_ticks) * tick_stride.
struct SessionTraceView {
    uint32_t *records;           // nullptr: no trace attached
    int64_t session_stride;      // in records
    int64_t tick_slot_offset;    // in records
    uint32_t tick;               // number of this tick, counted from 0 at attachment
};

// The FlowField values the record reads (the kernels load exactly these).
#define AECM_SESSION_TRACE_FIELDS(X)                                                                                                \
    X(F_MS) X(F_KNOWN_DELAY) X(F_FILT_DELAY) X(F_BUF_SIZE_START) X(F_EC_STARTUP) X(F_CHECK_BUFF_SIZE) X(F_DELAY_CHANGE) X(F_LAST_DELAY_DIFF) \
    X(F_FAR_WP) X(F_FAR_RP) X(F_TIME_FOR_DELAY_CHANGE)

AECM_FLOW_HD uint32_t SessionTracePack(int32_t lo, int32_t hi) { return ((uint32_t)lo & 0xffffu) | ((uint32_t)hi << 16); }

// Words 0..7 of the record.  flow: the session's wrapper words after the tick, indexed by FlowField (only the fields named above
// are read); blocks: FlowPlan::n_blocks of the tick; khz: 8 or 16, the session's own rate.  The 16-bit fields are the low halves
// of their words (the reference's short members: FlowStateDefect keeps them in range).
//   0 tick   1 blocks | khz << 16   2 ms | known_delay << 16   3 filt_delay | buf_size_start << 16   4 ec_startup | check_buff_size << 16
//   5 delay_change | last_delay_diff << 16   6 far_wp - far_rp   7 time_for_delay_change
AECM_FLOW_HD void SessionTraceHeaderWords(const int32_t flow[], uint32_t tick, int blocks, int khz, uint32_t out[kSessionTraceHeaderWords]) {
    out[0] = tick;
    out[1] = SessionTracePack(blocks, khz);
    out[2] = SessionTracePack(flow[F_MS], flow[F_KNOWN_DELAY]);
    out[3] = SessionTracePack(flow[F_FILT_DELAY], flow[F_BUF_SIZE_START]);
    out[4] = SessionTracePack(flow[F_EC_STARTUP], flow[F_CHECK_BUFF_SIZE]);
    out[5] = SessionTracePack(flow[F_DELAY_CHANGE], flow[F_LAST_DELAY_DIFF]);
    out[6] = (uint32_t)flow[F_FAR_WP] - (uint32_t)flow[F_FAR_RP];
    out[7] = (uint32_t)flow[F_TIME_FOR_DELAY_CHANGE];
}

// ---- the call trace (include/aecm_batch.h: WebRtcAecmSessions_SetCallTrace): the same record, one per CALL SLOT -----------------
// Where the records of ONE tick of `calls` call pairs go, computed on the host (SessionBatch::Enqueue): the tick starts at call
// slot number first_call, and call c of session s writes its sixteen words at
// records + kSessionTraceWords * (s * session_stride + ((first_slot + c) % ring_calls) * call_stride), first_slot = first_call % ring_calls.
// The two halves of a record come from two launches of the tick: the planning lane stores words 0..7 as it plans call c
// (CallTraceHeaderWords below, from the lane's own registers), the tick kernel words 8..15 behind call c's blocks.
struct CallTraceView {
    uint32_t *records;           // nullptr: no trace attached
    int64_t session_stride;      // in records
    int64_t call_stride;         // in records
    int32_t ring_calls;          // > 0
    int32_t first_slot;          // first_call % ring_calls
    uint32_t first_call;         // slot number of call 0 of this tick, counted from 0 at attachment
};

// A ring shorter than the tick: call c + ring_calls of the same tick takes call c's slot.  What in-order writing leaves is the LAST
// call of every slot, so only those are stored -- by both launches, by this one test (no order between two stores is relied on).
AECM_FLOW_HD bool CallTraceStored(const CallTraceView &cv, int c, int calls) { return calls - c <= cv.ring_calls; }

// The ring slot of call c + 1 from call c's (call 0: cv.first_slot): both launches walk the ring call by call, without a division.
// (slot < ring_calls <= INT32_MAX: the sum does not overflow.)
AECM_FLOW_HD int32_t CallTraceNextSlot(const CallTraceView &cv, int32_t slot) { return slot + 1 >= cv.ring_calls ? 0 : slot + 1; }
// The index, in records, of session s's record in ring slot `slot`.
AECM_FLOW_HD int64_t CallTraceRecord(const CallTraceView &cv, int64_t s, int32_t slot) { return s * cv.session_stride + (int64_t)slot * cv.call_stride; }

// Words 0..7 of call c's record from the planning lane: flow = the lane's wrapper words directly behind call c's FlowTick.
AECM_FLOW_HD void CallTraceHeaderWords(const CallTraceView &cv, const int32_t flow[], int c, int blocks, int khz, uint32_t out[kSessionTraceHeaderWords]) {
    SessionTraceHeaderWords(flow, cv.first_call + (uint32_t)c, blocks, khz, out);
}

}  // namespace aecm

// The two hooks as TEXT, one for either launch, the same in the kernels and in the simulator (tests/sim/sim_call_trace.cpp).  Both
// stand inside a loop over the calls c = 0 .. calls - 1 of one session s and walk `int trace_slot`, which the includer declares
// ahead of the loop as cv.first_slot; the includer also provides the two stores (16-byte vector stores on the device).
//   the planning lane's sink (aecm_flow_plan_lane.inc: AECM_FLOW_PLAN_CALL_RECORD), r = the lane's registers behind call c's FlowTick,
//   p = call c's plan, trace_khz = the session's own rate: StoreCallTraceHeader(cv, s, slot, r, c, blocks, khz)
#define AECM_CALL_TRACE_PLAN_RECORD                                                                          \
    if (CallTraceStored(cv, c, calls)) StoreCallTraceHeader(cv, s, trace_slot, r, c, p.n_blocks, trace_khz); \
    trace_slot = CallTraceNextSlot(cv, trace_slot);
//   the tick kernel's loop (aecm_tick_calls_body.inc: AECM_TICK_CALLS_AFTER_BLOCKS), r = the core state's registers behind call c's
//   blocks, E = the block engine: StoreCallTraceCore<E>(r, cv, s, slot)
#define AECM_CALL_TRACE_TICK_RECORD                                                   \
    if (CallTraceStored(cv, c, calls)) StoreCallTraceCore<E>(r, cv, s, trace_slot);  \
    trace_slot = CallTraceNextSlot(cv, trace_slot);

#endif  // AECM_AMD_SESSION_TRACE_H_
