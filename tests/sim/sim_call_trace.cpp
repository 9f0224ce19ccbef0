// TEST INFRASTRUCTURE -- the CPU double of the call trace (include/aecm_batch.h: WebRtcAecmSessions_SetCallTrace), built into
// tests/_build/libaecm_sim_call_trace.so on top of libaecm_sim.so (tests/call_trace_sim.py).  An object of S sessions -- the host's
// tick planner (aecm_tick_plan.h: TickObject, with both trace switches), every session's wrapper words, its plans, and its core state
// as a SimStream on the 64-lane simulator -- makes ticks the way the product's two launches make them:
//   the planning launch   one call of PlanLane per session: the TEXT of the planning kernels, aecm_flow_plan_lane.inc, compiled for
//                         the host -- for a tick of several calls with the call trace's sink (AECM_CALL_TRACE_PLAN_RECORD) and the
//                         header store of this file in place of the device's two 16-byte stores
//   the tick launch       per session the loop over the calls of aecm_tick_calls_body.inc as far as the record goes -- the plan of
//                         call c unpacked, its n_blocks blocks by BlockEngine::run_blocks_loaded on registers that stay loaded
//                         across the calls, the body's hook (AECM_CALL_TRACE_TICK_RECORD) behind them, one store_state at the end;
//                         a tick of one call pair loads, runs, takes the per-tick record (the restatement of
//                         aecm_tick_trace_kernels.hip: SessionTraceRow) and stores
// The wrapper's sample movement is not part of it (sim_calls.cpp, sim_packets.cpp have that, on tags): the blocks of a session take
// their far and near samples from the session's own streams of 64-sample blocks, in order.  What a record shows does not depend on
// which samples a block ate, as long as both forms of a tick feed it the same ones -- and the plans decide that, not the audio.
#include <stdint.h>
#include <string.h>

#include <vector>

#include "wave_sim.h"
#include "sim_stream.h"
#include "aecm_wave.h"
#include "aecm_kernels.h"
#include "aecm_tick_plan.h"

extern "C" {
void *sim_create(int fs, int cng_mode, int echo_mode);      // sim_lib.cpp
void sim_free(void *h);
void sim_digest(void *h, uint32_t *digest);
}

namespace ctsim {
using namespace aecm;

// what the planning lane's text stores its plans by (HIP's on the device)
struct int4 { int x, y, z, w; };
inline int4 make_int4(int x, int y, int z, int w) { return int4{x, y, z, w}; }

struct TraceSimWave : SimWave {
    static void store_out_u32_if(const VecB &m, uint32_t *p, const vi &idx, const vi &val) { store_u32_if(m, p, idx, val); }
};
using E = BlockEngine<TraceSimWave, false>;
using vi = E::vi;

// The two stores the hooks call (aecm_session_trace.h), as the kernels' units define them for the device.
inline void StoreCallTraceHeader(const CallTraceView &cv, int s, int slot, const FlowRegs &r, int c, int blocks, int khz) {
    uint32_t w[kSessionTraceHeaderWords];
    CallTraceHeaderWords(cv, r.v, c, blocks, khz, w);
    memcpy(cv.records + CallTraceRecord(cv, s, slot) * kSessionTraceWords, w, sizeof w);
}
template <class Engine>
inline void StoreCallTraceCore(const typename Engine::Regs &r, const CallTraceView &cv, int64_t s, int slot) {
    TraceSimWave::store_out_u32_if(r.lane < kTraceWords, cv.records + CallTraceRecord(cv, s, slot) * kSessionTraceWords + kSessionTraceHeaderWords, r.lane,
                                   Engine::block_trace_row(r));
}

// ---- the planning launch, one lane: the kernels' text.  flags: the lane's byte as aecm_flow_plan_list.inc reads it.
void PlanLaneCalls(const TickFlowIo &fio, const TickSparseIo &sp, const CallTraceView &cv, bool traced, bool packets, int rate, int n, int calls,
                   unsigned near_pos, int n_streams, int s) {
    const bool in_range = s < n_streams;
    const int flags = !in_range ? kFlowIdle : fio.flags_per_session ? (int)fio.flags_per_session[s] : fio.flags;
    const bool live = (flags & kFlowIdle) == 0;
    int trace_slot = cv.first_slot;
    const int trace_khz = rate == 16000 ? 16 : 8;
    if (traced) {
#define AECM_FLOW_PLAN_IDLE_SAMPLES calls * n
#define AECM_FLOW_PLAN_CALLS(emit)                                                      \
    if (packets) FlowTickPackets(r, rate, n, calls, ms, flags, near_pos, emit);         \
    else FlowTickCalls(r, rate, n, calls, ms, flags, near_pos, emit)
#define AECM_FLOW_PLAN_CALL_RECORD AECM_CALL_TRACE_PLAN_RECORD
#include "aecm_flow_plan_lane.inc"
    } else {
#define AECM_FLOW_PLAN_IDLE_SAMPLES calls * n
#define AECM_FLOW_PLAN_CALLS(emit)                                                      \
    if (packets) FlowTickPackets(r, rate, n, calls, ms, flags, near_pos, emit);         \
    else FlowTickCalls(r, rate, n, calls, ms, flags, near_pos, emit)
#include "aecm_flow_plan_lane.inc"
    }
}
void PlanLaneTick(const TickFlowIo &fio, const TickSparseIo &sp, int rate, int n, unsigned near_pos, int n_streams, int s) {
    const bool in_range = s < n_streams;
    const int flags = !in_range ? kFlowIdle : fio.flags_per_session ? (int)fio.flags_per_session[s] : fio.flags;
    const bool live = (flags & kFlowIdle) == 0;
#define AECM_FLOW_PLAN_IDLE_SAMPLES n
#define AECM_FLOW_PLAN_TICK(p) FlowTickMixed(r, rate, n, ms, flags, near_pos, p)
#include "aecm_flow_plan_lane.inc"
}

// ---- the tick launch, one session
struct BlockStreamIo {      // block b of this run: the session's next blocks
    const int16_t *far_s, *near_s;
    int16_t *out_s;
    vi far(const E::Regs &r, int b) const { return TraceSimWave::load_i16(far_s + (int64_t)b * kBlock, r.lane); }
    vi near(const E::Regs &r, int b) const { return TraceSimWave::load_i16(near_s + (int64_t)b * kBlock, r.lane); }
    vi clean(const E::Regs &, int) const { return vi(0); }
    void out(const E::Regs &r, int b, vi val) const { TraceSimWave::store_i16(out_s + (int64_t)b * kBlock, r.brev, val); }
    void ready() const {}
};

struct Object {
    int S = 0;
    TickObject plan;
    std::vector<void *> core;                 // [S] SimStream
    std::vector<int32_t> rates, state, plans; // [S]; [kFlowFieldsUsed][S]; [S][kFlowMaxTickCalls][kFlowPlanWords]
    std::vector<int16_t> near_ring;           // [S][kFlowFarRing] (only FlowResync's moves touch it)
    std::vector<int64_t> block_pos;           // [S] blocks run so far = the next block of the session's streams
    // the attached trace: kind 0 none, 1 per tick, 2 per call
    int kind = 0;
    uint32_t *records = nullptr;
    int64_t session_stride = 0, slot_stride = 0;
    int32_t ring = 1;
    ~Object() {
        for (void *h : core) sim_free(h);
    }
};

StatePtrs StateOf(Object &o, int s) {
    SimStream *x = (SimStream *)o.core[(size_t)s];
    return StatePtrs{x->img.vec.data(), x->img.scal.data(), x->hist.data(), nullptr};
}

// aecm_tick_calls_body.inc, as far as the record goes.  Returns the blocks run.
int TickLaneCalls(Object &o, int s, const CallTraceView &cv, bool traced, int calls, const int16_t *far_s, const int16_t *near_s, int16_t *out_s) {
    const StatePtrs st = StateOf(o, s);
    E::Regs r;
    E::init_lane_constants(r, st.consts);
    E::load_state(r, st.vec, st.scal);
    const int32_t *plans = o.plans.data() + (size_t)s * calls * kFlowPlanWords;
    int trace_slot = cv.first_slot, done = 0;
    bool ran = false;
    for (int c = 0; c < calls; ++c) {
        FlowPlan p;
        FlowUnpackPlan(plans + c * kFlowPlanWords, p);
        const int nb = p.n_blocks;
        if (nb > 0) {
            BlockStreamIo bio{far_s + (int64_t)done * kBlock, near_s + (int64_t)done * kBlock, out_s + (int64_t)done * kBlock};
            E::run_blocks_loaded(r, st, bio, 0, nb);
            ran = true;
            done += nb;
        }
        if (traced) {
            AECM_CALL_TRACE_TICK_RECORD
        }
    }
    if (ran) E::store_state(r, st.vec, st.scal);
    return done;
}

// A tick of one call pair: aecm_tick_flow_body.inc as far as the record goes, and -- traced -- SessionTraceRow + StoreSessionTraceRow.
int TickLaneOne(Object &o, int s, const SessionTraceView &tv, bool traced, const int16_t *far_s, const int16_t *near_s, int16_t *out_s) {
    const StatePtrs st = StateOf(o, s);
    E::Regs r;
    E::init_lane_constants(r, st.consts);
    E::load_state(r, st.vec, st.scal);
    FlowPlan p;
    FlowUnpackPlan(o.plans.data() + (size_t)s * kFlowPlanWords, p);
    const int nb = p.n_blocks;
    if (nb > 0) {
        BlockStreamIo bio{far_s, near_s, out_s};
        E::run_blocks_loaded(r, st, bio, 0, nb);
        E::store_state(r, st.vec, st.scal);
    }
    if (traced) {
        int32_t flow[kFlowFieldsUsed] = {};
#define CTSIM_LOAD(f) flow[f] = o.state[(size_t)(f) * o.S + s];
        AECM_SESSION_TRACE_FIELDS(CTSIM_LOAD)
#undef CTSIM_LOAD
        uint32_t w[kSessionTraceWords];
        SessionTraceHeaderWords(flow, tv.tick, nb, st.scal[S_MULT] == 2 ? 16 : 8, w);
        const vi row = E::block_trace_row(r);
        for (int k = 0; k < kTraceWords; ++k) w[kSessionTraceHeaderWords + k] = (uint32_t)row.v[k];
        memcpy(tv.records + (s * tv.session_stride + tv.tick_slot_offset) * kSessionTraceWords, w, sizeof w);
    }
    return nb;
}

}  // namespace ctsim

using namespace ctsim;

extern "C" {

int ctsim_flow_words() { return kFlowWords; }
int ctsim_max_calls() { return kFlowMaxTickCalls; }

// S sessions of an object at fs; rates[S]: every session's own (8000 / 16000).
void *ctsim_new(int sessions, int fs, const int32_t *rates) {
    Object *o = new Object();
    o->S = sessions;
    o->plan.Init(sessions, fs);
    o->rates.assign(rates, rates + sessions);
    o->state.assign((size_t)kFlowFieldsUsed * sessions, 0);
    o->plans.assign((size_t)sessions * kFlowMaxTickCalls * kFlowPlanWords, 0);
    o->near_ring.assign((size_t)sessions * kFlowFarRing, 0);
    o->block_pos.assign((size_t)sessions, 0);
    int32_t words[kFlowWords];
    FlowInit(words);
    for (int s = 0; s < sessions; ++s) {
        o->plan.SetRate(s, rates[s]);
        o->core.push_back(sim_create(rates[s], 1, 3));
        for (int k = 0; k < kFlowFieldsUsed; ++k) o->state[(size_t)k * sessions + s] = words[k];
    }
    return o;
}
void ctsim_free(void *h) { delete (Object *)h; }

// kind 1: SetSessionTrace, 2: SetCallTrace, with SessionBatch's checks (aecm_sessions.cpp): records == null detaches that kind only.
int32_t ctsim_attach(void *h, int kind, uint32_t *records, int64_t session_stride, int64_t slot_stride, int32_t ring) {
    Object &o = *(Object *)h;
    if (!records) {
        if (kind == 1) o.plan.AttachTrace(false); else o.plan.AttachCallTrace(false);
        if (o.kind == kind) o.kind = 0;
        return 0;
    }
    if ((reinterpret_cast<uintptr_t>(records) & 3) || session_stride <= 0 || slot_stride <= 0 || ring <= 0) return kTickBadParameter;
    if (!(kind == 1 ? o.plan.AttachTrace(true) : o.plan.AttachCallTrace(true))) return kTickBadParameter;
    o.kind = kind;
    o.records = records;
    o.session_stride = session_stride;
    o.slot_stride = slot_stride;
    o.ring = ring;
    return 0;
}
int64_t ctsim_count(void *h, int kind) { return kind == 1 ? ((Object *)h)->plan.trace_ticks : ((Object *)h)->plan.call_trace_calls; }
int64_t ctsim_near_pos(void *h) { return ((Object *)h)->plan.near_pos; }
int64_t ctsim_blocks_run(void *h, int s) { return ((Object *)h)->block_pos[(size_t)s]; }
void ctsim_digest(void *h, int s, uint32_t *digest) { sim_digest(((Object *)h)->core[(size_t)s], digest); }
// the wrapper words of session s, kFlowWords of them (those past the used fields: 0)
void ctsim_flow(void *h, int s, int32_t *words) {
    Object &o = *(Object *)h;
    for (int k = 0; k < kFlowWords; ++k) words[k] = k < kFlowFieldsUsed ? o.state[(size_t)k * o.S + s] : 0;
}

// One tick through TickObject::Tick and, accepted, the two launches.  flags [S] or null (all_flags then); ms [S]; far / near / out:
// every session's streams of 64-sample blocks, [S][stream_blocks * 64] -- session s's blocks of this tick are those from
// ctsim_blocks_run(s) on.  blocks_out [S][calls] (may be null): the n_blocks of every call of every session that called, else -1.
// Returns the tick's code; *family gets the plan's family (-1 refused).  -2: a session's streams are too short.
int32_t ctsim_tick(void *h, const uint8_t *flags, int all_flags, const int16_t *ms, int n, int calls, int packets, const int16_t *far_s,
                   const int16_t *near_s, int16_t *out_s, int64_t stream_blocks, int32_t *blocks_out, int32_t *family) {
    Object &o = *(Object *)h;
    const int S = o.S;
    TickArgs a;
    a.flags_per_session = flags;
    a.flags = all_flags;
    a.n = n;
    a.calls = calls;
    a.packets = packets != 0;
    a.ms_per_session = true;
    // the numbers of this tick's records: the counts before Commit moves them (SessionBatch::Enqueue)
    const int64_t first_call = o.plan.call_trace_calls, first_slot = first_call % o.ring, tick_no = o.plan.trace_ticks;
    uint32_t tick_pos = 0;
    const TickPlan plan = o.plan.Tick(a, &tick_pos);
    if (family) *family = plan.code ? -1 : (int32_t)plan.family;
    if (blocks_out)
        for (int i = 0; i < S * (calls > 0 ? calls : 1); ++i) blocks_out[i] = -1;
    if (plan.code || plan.family == kTickFamily_nothing) return plan.code;
    const bool traced = o.kind != 0;
    const CallTraceView cv{o.records, o.session_stride, o.slot_stride, o.ring, (int32_t)first_slot, (uint32_t)first_call};
    const SessionTraceView tv = o.kind == 2 ? SessionTraceView{o.records, o.session_stride, first_slot * o.slot_stride, (uint32_t)first_call}
                                            : SessionTraceView{o.records, o.session_stride, (tick_no % o.ring) * o.slot_stride, (uint32_t)tick_no};
    TickFlowIo fio{o.state.data(), o.plans.data(), nullptr, nullptr, ms, flags, 0, all_flags, o.plan.fs};
    const TickSparseIo sp{o.near_ring.data(), nullptr, kFlowFarRing, nullptr, nullptr, plan.route.deferred_lag};
    const bool k_calls = plan.family == kTickFamily_calls || plan.family == kTickFamily_packets;
    for (int s = 0; s < S; ++s) {
        const int rate = plan.family == kTickFamily_packets || plan.mixed_plan ? o.rates[(size_t)s] : o.plan.fs;
        if (k_calls) PlanLaneCalls(fio, sp, cv, traced, plan.family == kTickFamily_packets, rate, n, calls, tick_pos, S, s);
        else PlanLaneTick(fio, sp, rate, n, tick_pos, S, s);
    }
    for (int s = 0; s < S; ++s) {
        if (((flags ? flags[s] : all_flags) & kFlowIdle) != 0) continue;
        const int64_t at = o.block_pos[(size_t)s];
        int want = 0;
        for (int c = 0; c < (k_calls ? calls : 1); ++c) {
            FlowPlan p;
            FlowUnpackPlan(o.plans.data() + ((size_t)s * (k_calls ? calls : 1) + c) * kFlowPlanWords, p);
            if (blocks_out) blocks_out[s * calls + c] = p.n_blocks;
            want += p.n_blocks;
        }
        if (at + want > stream_blocks) return -2;
        const int64_t off = ((int64_t)s * stream_blocks + at) * kBlock;
        o.block_pos[(size_t)s] += k_calls ? TickLaneCalls(o, s, cv, traced, calls, far_s + off, near_s + off, out_s + off)
                                          : TickLaneOne(o, s, tv, traced, far_s + off, near_s + off, out_s + off);
    }
    return 0;
}

}  // extern "C"
