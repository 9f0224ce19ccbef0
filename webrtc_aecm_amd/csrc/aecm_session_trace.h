// The session trace (include/aecm_batch.h: AecmSessionTrace, WebRtcAecmSessions_SetSessionTrace): the 64-byte record a session
// writes at the end of a tick of one call pair -- sixteen words, the first eight from the wrapper state (FlowField) and the
// tick's plan, the last eight the core's AecmBlockTrace (BlockEngine::block_trace_row, aecm_wave.h).  This header is the ONE
// text of the wrapper half's layout: the traced tick kernels (aecm_tick_trace_kernels.hip) pack it on the scalar side, the host
// (aecm_capi.cpp asserts the struct against it) and the simulator (tests/sim/sim_session_trace.cpp) call the same function.
// HIP-free.
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

}  // namespace aecm
#endif  // AECM_AMD_SESSION_TRACE_H_
