// TEST INFRASTRUCTURE: the host compile of what the session trace shares between kernel, host and simulator
// (webrtc_aecm_amd/csrc/aecm_session_trace.h: SessionTraceHeaderWords -- the wrapper half of the 64-byte record) and the session
// trace's rules on the tick planner (aecm_tick_plan.h: TickObject::trace_attached / trace_ticks -- the refusal of ticks of several
// calls sits in CheckArgs, the count moves in Commit).  Bound by tests/session_trace_helpers.py; tests/test_session_trace.py holds
// the first against a Python restatement of include/aecm_batch.h's table and states the second.
#include <stdint.h>

#include <string_view>

#include "aecm_session_trace.h"
#include "aecm_tick_plan.h"

using namespace aecm;

extern "C" {

int strace_words() { return kSessionTraceWords; }
int strace_header_words_count() { return kSessionTraceHeaderWords; }

// flow: kFlowWords wrapper words, indexed by FlowField
void strace_header_words(const int32_t *flow, uint32_t tick, int blocks, int khz, uint32_t *out) { SessionTraceHeaderWords(flow, tick, blocks, khz, out); }

// FlowField indices by name, for the Python side: -1 for a name the record does not read
int strace_field(const char *name) {
#define STRACE_FIELD(f) \
    if (std::string_view(name) == #f) return f;
    AECM_SESSION_TRACE_FIELDS(STRACE_FIELD)
#undef STRACE_FIELD
    return -1;
}

// ---- the planner with a trace
void *strace_object_new(int sessions, int fs) {
    TickObject *o = new TickObject();
    o->Init(sessions, fs);
    return o;
}
void strace_object_free(void *o) { delete static_cast<TickObject *>(o); }
void strace_object_attach(void *o, int on) { static_cast<TickObject *>(o)->AttachTrace(on != 0); }
int64_t strace_object_ticks(void *o) { return static_cast<TickObject *>(o)->trace_ticks; }
int64_t strace_object_near_pos(void *o) { return static_cast<TickObject *>(o)->near_pos; }
// One tick through TickObject::Tick (check, plan, commit when accepted): flags [S] or null; returns the code; *family gets the plan's.
int32_t strace_object_tick(void *o, const uint8_t *flags, int all_flags, int n, int calls, int packets, int has_clean, int32_t *family) {
    TickArgs a;
    a.flags_per_session = flags;
    a.flags = all_flags;
    a.n = n;
    a.calls = calls;
    a.packets = packets != 0;
    a.has_clean = has_clean != 0;
    a.ms_per_session = flags != nullptr;
    const TickPlan p = static_cast<TickObject *>(o)->Tick(a);
    if (family) *family = p.code ? -1 : (int32_t)p.family;
    return p.code;
}

}  // extern "C"
