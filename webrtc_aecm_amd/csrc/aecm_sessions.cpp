#include "aecm_sessions.h"

#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/echo_control_mobile.h"
#include "aecm_session_snapshot.h"
#include "aecm_state_check.h"

namespace aecm {

#define AECM_HIP_OK(expr) ((expr) == hipSuccess)

static_assert(kTickUnspecified == AECM_UNSPECIFIED_ERROR && kTickUnsupported == AECM_UNSUPPORTED_FUNCTION_ERROR &&
                  kTickUninitialized == AECM_UNINITIALIZED_ERROR && kTickNullPointer == AECM_NULL_POINTER_ERROR &&
                  kTickBadParameter == AECM_BAD_PARAMETER_ERROR && kTickWarning == AECM_BAD_PARAMETER_WARNING,
              "aecm_tick_plan.h returns the AECM_* codes");

SessionBatch *SessionBatch::Create(int num_streams, int device_id) {
    BatchEngine *e = BatchEngine::Create(num_streams, device_id);
    if (!e) return nullptr;
    SessionBatch *b = new SessionBatch();
    b->engine_.reset(e);
    b->device_ = device_id;
    const size_t S = (size_t)num_streams;
    const bool ok = AECM_HIP_OK(hipMalloc((void **)&b->far_ring_, S * kRing * 2)) &&
                    AECM_HIP_OK(hipMalloc((void **)&b->near_ring_, S * kRing * 2)) &&
                    AECM_HIP_OK(hipMalloc((void **)&b->out_ring_, S * kRing * 2)) &&
                    AECM_HIP_OK(hipMalloc((void **)&b->io_dev_, 4 * S * 160 * 2)) &&
                    AECM_HIP_OK(hipMalloc((void **)&b->flow_state_, S * kFlowFieldsUsed * sizeof(int32_t))) &&
                    AECM_HIP_OK(hipMalloc((void **)&b->flow_plans_, S * kFlowPlanWords * sizeof(int32_t))) &&
                    AECM_HIP_OK(hipMalloc((void **)&b->far_frames_, S * kFlowFarFrameRing * 2)) &&
                    AECM_HIP_OK(hipMalloc((void **)&b->live_dev_, S * sizeof(uint32_t))) &&
                    // (the per-session msInSndCardBuf / flags slots: pinned host arrays the planning kernel reads in place, below)
                    AECM_HIP_OK(hipMalloc((void **)&b->far_old_, S * 2 * kFlowFrame * 2));
    bool slots = ok;
    const size_t plan_blocks = (S + kFlowPlanBlock - 1) / kFlowPlanBlock;
    for (int k = 0; k < kArgSlots && slots; ++k)
        slots = AECM_HIP_OK(hipHostMalloc((void **)&b->ms_host_[k], S * sizeof(int16_t), hipHostMallocMapped)) &&
                AECM_HIP_OK(hipHostMalloc((void **)&b->flags_host_[k], S, hipHostMallocMapped)) &&
                AECM_HIP_OK(hipHostMalloc((void **)&b->bases_host_[k], 2 * plan_blocks * sizeof(uint32_t), hipHostMallocMapped)) &&
                AECM_HIP_OK(hipHostGetDevicePointer((void **)&b->ms_dev_[k], b->ms_host_[k], 0)) &&
                AECM_HIP_OK(hipHostGetDevicePointer((void **)&b->flags_dev_[k], b->flags_host_[k], 0)) &&
                AECM_HIP_OK(hipHostGetDevicePointer((void **)&b->bases_dev_[k], b->bases_host_[k], 0)) &&
                AECM_HIP_OK(hipEventCreateWithFlags(&b->slot_read_[k], hipEventDisableTiming));
    if (!slots) {
        delete b;
        return nullptr;
    }
    return b;
}

SessionBatch::~SessionBatch() {
    (void)hipSetDevice(device_);
    if (engine_) (void)engine_->Synchronize();
    (void)hipFree(far_ring_);
    (void)hipFree(near_ring_);
    (void)hipFree(out_ring_);
    (void)hipFree(clean_ring_);
    (void)hipFree(io_dev_);
    (void)hipFree(flow_state_);
    (void)hipFree(flow_plans_);
    (void)hipFree(calls_plans_);
    (void)hipFree(far_frames_);
    (void)hipFree(far_old_);
    (void)hipFree(live_dev_);
    (void)hipFree(split_live_dev_);
    (void)hipFree(snap_list_);
    (void)hipFree(snap_stage_);
    (void)hipFree(snap_verdict_);
    for (int k = 0; k < kArgSlots; ++k) {
        if (bases_host_[k]) (void)hipHostFree(bases_host_[k]);
        if (ms_host_[k]) (void)hipHostFree(ms_host_[k]);
        if (flags_host_[k]) (void)hipHostFree(flags_host_[k]);
        if (slot_read_[k]) (void)hipEventDestroy(slot_read_[k]);
    }
}

// WebRtcAecm_Init of the wrapper side of sessions [first, first + count): one launch (aecm_kernels.h).
bool SessionBatch::ResetFlowRows(int first, int count) {
    TickIo tio{nullptr, nullptr, nullptr, nullptr, 0, 0, far_ring_, near_ring_, clean_ring_, out_ring_, kRing, 0};
    TickFlowIo fio{flow_state_, flow_plans_, far_frames_, far_old_, nullptr, nullptr, 0, 0, tick_.fs};
    return AECM_HIP_OK(LaunchResetSessions(tio, fio, engine_->num_streams(), first, count, engine_->stream()));
}

int32_t SessionBatch::Init(int32_t samp_freq) {
    if (samp_freq != 8000 && samp_freq != 16000) return AECM_BAD_PARAMETER_ERROR;
    if (!engine_->Init(samp_freq)) return AECM_UNSPECIFIED_ERROR;
    const int S = engine_->num_streams();
    const size_t bytes = (size_t)S * kRing * 2;
    if (!AECM_HIP_OK(hipMemsetAsync(near_ring_, 0, bytes, engine_->stream())) ||
        (clean_ring_ && !AECM_HIP_OK(hipMemsetAsync(clean_ring_, 0, bytes, engine_->stream()))) || !ResetFlowRows(0, S))
        return AECM_UNSPECIFIED_ERROR;
    tick_.Init(S, samp_freq);
    poisoned_ = false;
    return 0;
}

int32_t SessionBatch::InitRates(int32_t samp_freq, const int32_t *rates) {
    if (rates == nullptr) return AECM_NULL_POINTER_ERROR;
    if (samp_freq != 8000 && samp_freq != 16000) return AECM_BAD_PARAMETER_ERROR;
    const int S = engine_->num_streams();
    for (int s = 0; s < S; ++s)
        if (rates[s] != 8000 && rates[s] != 16000) return AECM_BAD_PARAMETER_ERROR;
    if (int32_t rc = Init(samp_freq)) return rc;
    if (!engine_->InitStreamsOfOtherRate(rates)) { tick_.Forget(); return AECM_UNSPECIFIED_ERROR; }      // (the wrapper state knows no rate)
    for (int s = 0; s < S; ++s) tick_.SetRate(s, rates[s]);
    return 0;
}

int32_t SessionBatch::GetSessionRate(int session, int32_t *samp_freq) const {
    if (samp_freq == nullptr) return AECM_NULL_POINTER_ERROR;
    if (int32_t rc = CheckSession(session)) return rc;
    *samp_freq = tick_.rates[(size_t)session];
    return 0;
}

int32_t SessionBatch::GetSessionCleanMode(int session, int32_t *mode) const {
    if (mode == nullptr) return AECM_NULL_POINTER_ERROR;
    if (int32_t rc = CheckSession(session)) return rc;
    *mode = tick_.history.Get(session);
    return 0;
}

// One launch or two for a split tick of `calling` sessions (profiles/r24_split_clean_ticks.txt).  The fused kernel holds both tick
// bodies in one function and comes out with several times the scalar spills of either body alone: per session it is the slower code
// (about a tenth more kernel time), but it is ONE dispatch; the second of two dependent launches costs 6 .. 12 us of ramp-down and
// ramp-up whatever the size.  Measured at half the sessions flagged, fused against two launches, ms per tick: 4 096 sessions 0.0354 /
// 0.0417, 8 192: 0.0538 / 0.0558, 16 384: 0.0832 / 0.0897, 32 768: 0.1442 / 0.1379, 65 536: 0.2653 / 0.2425.  The two lines cross
// between 16 384 and 32 768 sessions, interpolated linearly at about 25 000 = 3.5 times what the device holds at once (7 168 on 256
// CUs): the fused launch up to four residency rounds -- at that threshold the two forms differ by less than 2 us --, two beyond.
constexpr int kSplitFusedRounds = 4;
bool SessionBatch::SplitTickTwoLaunches(int calling) const {
    if (split_two_launches_ >= 0) return split_two_launches_ > 0;
    const int64_t resident = (int64_t)TickWorkgroupsPerCu() * TickWorkgroupWaves() * engine_->launch_policy().compute_units;
    return calling > kSplitFusedRounds * resident;
}

// Host state only: every tick launch takes its view as a kernel argument, so the ticks already enqueued keep theirs.
int32_t SessionBatch::SetSessionTrace(void *trace_dev, int64_t session_stride, int64_t tick_stride, int32_t ring_ticks) {
    if (!trace_dev) {      // (detaches its own kind only: a call trace stays)
        trace_records_ = nullptr;
        tick_.AttachTrace(false);
        return 0;
    }
    // the kernels store the records as 32-bit words: a pointer that is not a multiple of 4 would fault on the GPU
    if ((reinterpret_cast<uintptr_t>(trace_dev) & 3) || session_stride <= 0 || tick_stride <= 0 || ring_ticks <= 0) return AECM_BAD_PARAMETER_ERROR;
    if (!tick_.AttachTrace(true)) return AECM_BAD_PARAMETER_ERROR;       // at most one of the two traces: a call trace is attached
    trace_records_ = static_cast<uint32_t *>(trace_dev);
    trace_session_stride_ = session_stride;
    trace_tick_stride_ = tick_stride;
    trace_ring_ticks_ = ring_ticks;
    return 0;
}

// Host state only, as SetSessionTrace.
int32_t SessionBatch::SetCallTrace(void *trace_dev, int64_t session_stride, int64_t call_stride, int32_t ring_calls) {
    if (!trace_dev) {      // (detaches its own kind only: a session trace stays)
        call_trace_records_ = nullptr;
        tick_.AttachCallTrace(false);
        return 0;
    }
    if ((reinterpret_cast<uintptr_t>(trace_dev) & 3) || session_stride <= 0 || call_stride <= 0 || ring_calls <= 0) return AECM_BAD_PARAMETER_ERROR;
    if (!tick_.AttachCallTrace(true)) return AECM_BAD_PARAMETER_ERROR;   // at most one of the two traces: a session trace is attached
    call_trace_records_ = static_cast<uint32_t *>(trace_dev);
    call_trace_session_stride_ = session_stride;
    call_trace_call_stride_ = call_stride;
    call_trace_ring_calls_ = ring_calls;
    return 0;
}

int32_t SessionBatch::CheckSession(int session) const {
    if (tick_.fs == 0) return AECM_UNINITIALIZED_ERROR;
    if (poisoned_) return AECM_UNSPECIFIED_ERROR;
    if (session < 0 || session >= engine_->num_streams()) return AECM_BAD_PARAMETER_ERROR;
    return 0;
}

// WebRtcAecm_Init of ONE session (same sampling rate as the batch): fresh core state, fresh wrapper state, and rings
// that read as never written (a fresh jitter buffer's read pointer can be moved back over never-written memory, the
// output ring is stuffed from it: ring_buffer.c:75-82).
int32_t SessionBatch::InitSession(int session) { return InitSessionRate(session, tick_.fs); }

// The same at a rate of the caller's choice; the slot then runs at that rate (InitSession: back at the object's own).
int32_t SessionBatch::InitSessionRate(int session, int32_t samp_freq) {
    if (int32_t rc = CheckSession(session)) return rc;              // (an uninitialised object: tick_.fs == 0 never gets further)
    if (samp_freq != 8000 && samp_freq != 16000) return AECM_BAD_PARAMETER_ERROR;
    // two launches, ordered before the next tick on the object's stream: no synchronisation with the host
    const bool ok = AECM_HIP_OK(hipSetDevice(device_)) && engine_->InitStreamsAtRate(session, 1, samp_freq) && ResetFlowRows(session, 1);
    if (!ok) { poisoned_ = true; return AECM_UNSPECIFIED_ERROR; }
    tick_.InitSession(session, samp_freq);
    return 0;
}

int32_t SessionBatch::SetConfigSession(int session, int16_t cng_mode, int16_t echo_mode) {
    if (int32_t rc = CheckSession(session)) return rc;
    if (cng_mode != AecmFalse && cng_mode != AecmTrue) return AECM_BAD_PARAMETER_ERROR;
    if (echo_mode < 0 || echo_mode > 4) {                    // the reference commits cngMode before it rejects echoMode (:421-428)
        if (!engine_->SetCngMode(cng_mode, session, 1)) return AECM_UNSPECIFIED_ERROR;
        return AECM_BAD_PARAMETER_ERROR;
    }
    return engine_->SetConfig(cng_mode, echo_mode, session, 1) ? 0 : AECM_UNSPECIFIED_ERROR;
}

int32_t SessionBatch::InitEchoPathSession(int session, const void *path, size_t size_bytes) {
    if (path == nullptr) return AECM_NULL_POINTER_ERROR;
    if (size_bytes != kBins * sizeof(int16_t)) return AECM_BAD_PARAMETER_ERROR;
    if (int32_t rc = CheckSession(session)) return rc;
    int16_t tmp[kBins];
    memcpy(tmp, path, sizeof tmp);
    return engine_->SetEchoPath(session, tmp) ? 0 : AECM_UNSPECIFIED_ERROR;
}

int32_t SessionBatch::GetEchoPathSession(int session, void *path, size_t size_bytes) {
    if (path == nullptr) return AECM_NULL_POINTER_ERROR;
    if (size_bytes != kBins * sizeof(int16_t)) return AECM_BAD_PARAMETER_ERROR;
    if (int32_t rc = CheckSession(session)) return rc;
    int16_t tmp[kBins];
    if (!engine_->GetEchoPath(session, tmp)) return AECM_UNSPECIFIED_ERROR;
    memcpy(path, tmp, sizeof tmp);
    return 0;
}

int32_t SessionBatch::SetConfig(int16_t cng_mode, int16_t echo_mode) {
    if (tick_.fs == 0) return AECM_UNINITIALIZED_ERROR;
    if (poisoned_) return AECM_UNSPECIFIED_ERROR;
    if (cng_mode != AecmFalse && cng_mode != AecmTrue) return AECM_BAD_PARAMETER_ERROR;
    if (echo_mode < 0 || echo_mode > 4) {
        if (!engine_->SetCngMode(cng_mode, 0, -1)) return AECM_UNSPECIFIED_ERROR;
        return AECM_BAD_PARAMETER_ERROR;
    }
    return engine_->SetConfig(cng_mode, echo_mode, 0, -1) ? 0 : AECM_UNSPECIFIED_ERROR;
}

// One tick: a planning launch (one lane per session) and a tick launch (one wavefront per session); nothing per session
// happens on the host beyond handing over the tick's msInSndCardBuf / flags.  The return codes need no device either:
// the only thing a call of an initialised session with valid arguments can return is the warning for an out-of-range
// msInSndCardBuf (echo_control_mobile.cc:258-265).
int32_t SessionBatch::Fail() {
    poisoned_ = true;
    (void)hipStreamSynchronize(engine_->stream());      // async copies from caller / pinned memory may still be in flight
    return AECM_UNSPECIFIED_ERROR;
}

// The caller's events are parameters: a stale or foreign handle is refused before anything is touched (a query of a
// live event answers "done" or "not ready", never anything else), and refused without consequences for the sessions.
bool SessionBatch::EventUsable(void *ev) const {
    if (!ev) return true;
    const hipError_t q = hipEventQuery(static_cast<hipEvent_t>(ev));
    if (q == hipSuccess || q == hipErrorNotReady) return true;
    (void)hipGetLastError();
    return false;
}

// The next of the pinned per-session argument slots; when it is going to be written (needed), wait -- normally not at all --
// until the launch that last read it has run.
int SessionBatch::AcquireArgSlot(bool needed, bool *ok) {
    const int slot = slot_;
    slot_ = (slot_ + 1) % kArgSlots;
    *ok = true;
    if (needed && slot_busy_[slot]) {
        *ok = AECM_HIP_OK(hipEventSynchronize(slot_read_[slot]));
        slot_busy_[slot] = false;
    }
    return slot;
}

int32_t SessionBatch::BufferFarend(const int16_t *far, int64_t stride, size_t n_samples, int32_t calls, const uint8_t *calls_per_session,
                                   bool host_pointers, bool wait, void *wait_event, void *done_event) {
    if (far == nullptr) return AECM_NULL_POINTER_ERROR;                                  // the order of WebRtcAecm_GetBufferFarendError (:195-213)
    if (tick_.fs == 0) return AECM_UNINITIALIZED_ERROR;
    if (n_samples != 80 && n_samples != 160) return AECM_BAD_PARAMETER_ERROR;
    if (calls < 0 || calls > 255 || stride < (int64_t)n_samples * calls) return AECM_BAD_PARAMETER_ERROR;
    if (poisoned_) return AECM_UNSPECIFIED_ERROR;
    const int S = engine_->num_streams(), n = (int)n_samples;
    if (calls_per_session)
        for (int s = 0; s < S; ++s)
            if (calls_per_session[s] > calls) return AECM_BAD_PARAMETER_ERROR;
    if (!AECM_HIP_OK(hipSetDevice(device_))) return AECM_UNSPECIFIED_ERROR;
    if (!EventUsable(wait_event) || !EventUsable(done_event)) return AECM_BAD_PARAMETER_ERROR;
    hipStream_t st = engine_->stream();
    if (calls > 0) {
        bool slot_ok;
        const int slot = AcquireArgSlot(calls_per_session != nullptr, &slot_ok);
        if (!slot_ok) return Fail();
        if (calls_per_session) memcpy(flags_host_[slot], calls_per_session, (size_t)S);     // pinned + mapped: the kernel reads it in place
        if (!WaitForCallerEvent(wait_event)) return AECM_BAD_PARAMETER_ERROR;             // nothing has been enqueued: no poison
        TickFlowIo fio{flow_state_, flow_plans_, far_frames_, far_old_, nullptr, nullptr, 0, 0, tick_.fs};
        const uint8_t *calls_dev = calls_per_session ? flags_dev_[slot] : nullptr;
        bool ok = true;
        if (!host_pointers) {
            TickIo tio{far, nullptr, nullptr, nullptr, stride, n, far_ring_, nullptr, nullptr, nullptr, kRing, 0};
            ok = AECM_HIP_OK(LaunchBufferFarend(engine_->state_ptrs(), tio, fio, calls_dev, 0, calls, S, st));
        } else {
            // host audio: staged through the ticks' device rows, as many calls per round as they hold
            const int per_round = (4 * 160) / n;
            for (int base = 0; base < calls && ok; base += per_round) {
                const int round = std::min(per_round, calls - base);
                const size_t width = (size_t)round * n * 2;
                ok = AECM_HIP_OK(hipMemcpy2DAsync(io_dev_, width, far + (size_t)base * n, (size_t)stride * 2, width, S, hipMemcpyHostToDevice, st));
                TickIo tio{io_dev_, nullptr, nullptr, nullptr, (int64_t)round * n, n, far_ring_, nullptr, nullptr, nullptr, kRing, 0};
                ok = ok && AECM_HIP_OK(LaunchBufferFarend(engine_->state_ptrs(), tio, fio, calls_dev, base, round, S, st));
            }
        }
        if (!ok) return Fail();
        if (calls_per_session) {
            if (!AECM_HIP_OK(hipEventRecord(slot_read_[slot], st))) return Fail();
            slot_busy_[slot] = true;
        }
    }
    if (done_event && !AECM_HIP_OK(hipEventRecord(static_cast<hipEvent_t>(done_event), st))) return Fail();
    if ((wait || host_pointers) && !AECM_HIP_OK(hipStreamSynchronize(st))) return Fail();
    return 0;
}

// The kernels wait for the caller's event first.  False: the handle was refused -- nothing has been enqueued for it, no poison.
bool SessionBatch::WaitForCallerEvent(void *wait_event) {
    if (!wait_event || AECM_HIP_OK(hipStreamWaitEvent(engine_->stream(), static_cast<hipEvent_t>(wait_event), 0))) return true;
    (void)hipGetLastError();
    return false;
}

// A grow-only device buffer of `*have` units: at least `need` afterwards, contents not kept (aecm_engine.h: GrowDeviceBuffer).
// A stream that could not be synchronised poisons the object; no memory does not.
int32_t SessionBatch::Grow(void **buf, size_t *have, size_t need, size_t unit) {
    if (GrowDeviceBuffer(buf, have, need, unit, engine_->stream())) return 0;
    return *buf ? Fail() : AECM_UNSPECIFIED_ERROR;
}
// The same for a buffer of one size, allocated by the first call that needs it.
int32_t SessionBatch::GrowOnce(void **buf, size_t bytes) {
    size_t have = *buf ? bytes : 0;
    return Grow(buf, &have, bytes, 1);
}

// The clean near-end ring, allocated and zeroed (a ring that may hold anything is no ring) by the first call that needs it.
int32_t SessionBatch::EnsureCleanRing() {
    if (clean_ring_) return 0;
    const size_t bytes = (size_t)engine_->num_streams() * kRing * 2;
    if (!AECM_HIP_OK(hipMalloc((void **)&clean_ring_, bytes))) { clean_ring_ = nullptr; return AECM_UNSPECIFIED_ERROR; }
    if (AECM_HIP_OK(hipMemsetAsync(clean_ring_, 0, bytes, engine_->stream()))) return 0;
    (void)hipFree(clean_ring_);
    clean_ring_ = nullptr;
    return Fail();
}

// Check -> plan -> prepare -> commit -> launch.  The first two are host logic without a device (aecm_tick_plan.h) on either side
// of the one device call between them; a tick refused by either has changed nothing.
int32_t SessionBatch::Enqueue(const int16_t *far, const int16_t *near, const int16_t *clean, int16_t *out, int64_t stride, size_t n_samples,
                              int16_t ms, const int16_t *ms_per_session, const uint8_t *flags_per_session, int32_t *codes,
                              bool host_pointers, void *wait_event, void *done_event, int flags, int32_t calls, bool packets) {
    // ---- check
    if (const int32_t rc = tick_.CheckArgs(far != nullptr, near != nullptr && out != nullptr, flags_per_session, flags, n_samples, calls, stride, packets,
                                           poisoned_, engine_->variant() == kVariantFast))
        return rc;
    if (!AECM_HIP_OK(hipSetDevice(device_))) return AECM_UNSPECIFIED_ERROR;
    if (!EventUsable(wait_event) || !EventUsable(done_event)) return AECM_BAD_PARAMETER_ERROR;
    // ---- plan
    TickArgs args;
    args.flags_per_session = flags_per_session;
    args.flags = flags;
    args.n = (int)n_samples;
    args.calls = calls;
    args.packets = packets;
    args.has_clean = clean != nullptr;
    args.host_pointers = host_pointers;
    args.ms_per_session = ms_per_session != nullptr;
    const TickPlan plan = tick_.Plan(args);
    if (plan.code) return plan.code;
    const int S = engine_->num_streams(), n = args.n, span = plan.span;
    hipStream_t st = engine_->stream();
    if (plan.family == kTickFamily_nothing) {
        // Nobody calls: nothing is launched and no slot rotates, but the caller's events are honoured, and the object's position
        // moves on all the same; the sessions learn of it with the next tick somebody makes (aecm_flow_plan.h: FlowRouteTick).
        if (!WaitForCallerEvent(wait_event)) return AECM_BAD_PARAMETER_ERROR;
        tick_.Commit(plan);
        if (codes) memset(codes, 0, (size_t)S * sizeof(int32_t));
        if (plan.zero_out)
            for (int s = 0; s < S; ++s) memset(out + (size_t)s * stride, 0, (size_t)span * 2);
        if (done_event && !AECM_HIP_OK(hipEventRecord(static_cast<hipEvent_t>(done_event), st))) return Fail();
        return 0;
    }
    // ---- prepare.  What the tick's kind needs for the first time is allocated first: a failure here returns before anything is
    // committed and before the slot rotates.
    if (plan.split_tick)
        if (const int32_t rc = GrowOnce((void **)&split_live_dev_, FlowSplitListEntries((uint32_t)S) * sizeof(uint32_t))) return rc;
    if (plan.k_calls)
        if (const int32_t rc = GrowOnce((void **)&calls_plans_, (size_t)S * kFlowMaxTickCalls * kFlowPlanWords * sizeof(int32_t))) return rc;
    if (host_pointers)      // host audio of a K-call tick: the staging planes grow to calls * n samples per row
        if (const int32_t rc = Grow((void **)&io_dev_, &io_row_, (size_t)span, 4 * (size_t)S * 2)) return rc;
    if (!plan.clean_plane) clean = nullptr;      // (every caller carries kNoClean: the tick without a clean input)
    if (clean)
        if (const int32_t rc = EnsureCleanRing()) return rc;
    // This tick's argument slot, acquired before the caller's event is waited for.
    bool slot_ok;
    const int slot = AcquireArgSlot(plan.need_slot, &slot_ok);
    if (!slot_ok) return Fail();
    const int32_t first_rc = TickCodes(ms_per_session, ms, flags_per_session, S, codes);
    if (ms_per_session) memcpy(ms_host_[slot], ms_per_session, (size_t)S * sizeof(int16_t));      // pinned + mapped
    if (flags_per_session) memcpy(flags_host_[slot], flags_per_session, (size_t)S);
    if (plan.route.sparse_tick) memcpy(bases_host_[slot], tick_.Bases(plan).data(), tick_.Bases(plan).size() * sizeof(uint32_t));
    // without far rows (nobody buffers a far frame in this tick) the kernel's far row pointer is never used for a sample that
    // counts; it still has to be an address: the near rows
    if (far == nullptr) far = near;
    const int16_t *dfar = far, *dnear = near, *dclean = clean;
    int16_t *dout = out;
    int64_t dstride = stride;
    // Host audio: staged in device rows of n (K calls: calls * n) samples; rows that are dense on the host too travel as one copy each way.
    auto copy_rows = [&](void *dst, size_t dpitch, const void *src, size_t spitch, hipMemcpyKind kind) {
        const size_t width = (size_t)span * 2;
        if (dpitch == width && spitch == width) return AECM_HIP_OK(hipMemcpyAsync(dst, src, width * S, kind, st));
        return AECM_HIP_OK(hipMemcpy2DAsync(dst, dpitch, src, spitch, width, S, kind, st));
    };
    if (host_pointers) {
        dstride = span;
        const size_t plane = (size_t)S * io_row_;
        int16_t *f = io_dev_, *d = io_dev_ + plane, *c = io_dev_ + 3 * plane;
        if (!copy_rows(f, (size_t)span * 2, far, (size_t)stride * 2, hipMemcpyHostToDevice) ||
            !copy_rows(d, (size_t)span * 2, near, (size_t)stride * 2, hipMemcpyHostToDevice) ||
            (clean && !copy_rows(c, (size_t)span * 2, clean, (size_t)stride * 2, hipMemcpyHostToDevice)))
            return Fail();
        dfar = f;
        dnear = d;
        dout = io_dev_ + 2 * plane;
        if (clean) dclean = c;
        // whole planes travel back: the rows of sessions that sit out, which no kernel writes, as zeros
        // (and the second halves of the rows of sessions that make a half call)
        if (plan.zero_out && !AECM_HIP_OK(hipMemsetAsync(dout, 0, (size_t)S * span * 2, st))) return Fail();
    }
    TickIo tio{dfar, dnear, dclean, dout, dstride, n, far_ring_, near_ring_, clean_ring_, out_ring_, kRing, tick_.near_pos};
    TickFlowIo fio{flow_state_, flow_plans_, far_frames_, far_old_, ms_per_session ? ms_dev_[slot] : nullptr,
                   flags_per_session ? flags_dev_[slot] : nullptr, ms, flags & (kNoFarend | kSplitCalls), tick_.fs};      // (fs: the object's; mixed planning goes by the session's)
    // nothing of this tick has been enqueued (device pointers: no staging copies): a refused event leaves no poison
    if (!WaitForCallerEvent(wait_event)) return AECM_BAD_PARAMETER_ERROR;
    // the records of this tick, by its number: the count before Commit moves it (a session trace is attached: calls == 1, CheckArgs).
    // With a call trace the numbers are call slots: the first slot of this tick for the K-call and packet families (cv); a tick of
    // one call pair is the session trace's tick with its slot as the tick number (tv).
    const bool call_traced = tick_.call_trace_attached, traced = tick_.trace_attached || call_traced;
    const int64_t first_call = tick_.call_trace_calls, first_slot = first_call % call_trace_ring_calls_;
    const CallTraceView cv{call_trace_records_, call_trace_session_stride_, call_trace_call_stride_, call_trace_ring_calls_, (int32_t)first_slot, (uint32_t)first_call};
    const SessionTraceView tv = call_traced ? SessionTraceView{call_trace_records_, call_trace_session_stride_, first_slot * call_trace_call_stride_, (uint32_t)first_call}
                                            : SessionTraceView{trace_records_, trace_session_stride_, (tick_.trace_ticks % trace_ring_ticks_) * trace_tick_stride_,
                                                               (uint32_t)tick_.trace_ticks};
    // ---- commit: the tick is certain to be enqueued.  Behind the accepted wait, before the first launch: the position has moved
    // even when a launch fails (the object is then poisoned).
    tick_.Commit(plan);
    // ---- launch
    const FlowTickRoute &route = plan.route;
    const TickSparseIo sp{near_ring_, clean_ring_, kRing, live_dev_, bases_dev_[slot], route.deferred_lag};
    bool ok = false;
    switch (plan.family) {
    case kTickFamily_dense:
        ok = traced ? AECM_HIP_OK(LaunchTickFlowTraced(engine_->state_ptrs(), tio, fio, tv, S, st)) : AECM_HIP_OK(LaunchTickFlow(engine_->state_ptrs(), tio, fio, S, st));
        break;
    case kTickFamily_sparse:
    case kTickFamily_mixed: {
        // (a sparse plan for a tick everybody makes -- the lags are brought up to date --: the dense tick kernel, no live list)
        const TickSparseIo dense_tick{near_ring_, clean_ring_, kRing, nullptr, nullptr, route.deferred_lag};
        const TickSparseIo &lists = route.sparse_tick ? sp : dense_tick;
        ok = traced ? AECM_HIP_OK(LaunchTickFlowSparseTraced(engine_->state_ptrs(), tio, fio, lists, tv, S, plan.live, st, plan.mixed_plan))
                    : AECM_HIP_OK(LaunchTickFlowSparse(engine_->state_ptrs(), tio, fio, lists, S, plan.live, st, plan.mixed_plan));
        break;
    }
    case kTickFamily_calls:
        fio.plans = calls_plans_;
        ok = call_traced ? AECM_HIP_OK(LaunchTickCallsTraced(engine_->state_ptrs(), tio, fio, sp, cv, S, plan.live, calls, st))
                         : AECM_HIP_OK(LaunchTickCalls(engine_->state_ptrs(), tio, fio, sp, S, plan.live, calls, st));
        break;
    case kTickFamily_packets:      // the packed layout and its kernels
        fio.plans = calls_plans_;
        fio.flags = flags & kNoFarend;
        ok = call_traced ? AECM_HIP_OK(LaunchTickPacketsTraced(engine_->state_ptrs(), tio, fio, sp, cv, S, plan.live, calls, st))
                         : AECM_HIP_OK(LaunchTickPackets(engine_->state_ptrs(), tio, fio, sp, S, plan.live, calls, st));
        break;
    case kTickFamily_split: {
        TickSparseIo lists = sp;
        lists.live = split_live_dev_;
        const TickSplitIo split{bases_dev_[slot] + tick_.live_bases.size(), plan.clean_count, plan.plain_count, FlowPlainListStart((uint32_t)plan.clean_count)};
        if (plan.k_calls) {
            // several call pairs per session (SetSplitCallTicks; no trace of either kind: CheckArgs, Plan): the K plans per session
            // of the K-call tick, or -- half calls, sessions of another rate -- the packed layout of the packet tick; always one
            // tick launch per list
            fio.plans = calls_plans_;
            if (plan.mixed_plan) fio.flags = flags & kNoFarend;
            ok = plan.mixed_plan ? AECM_HIP_OK(LaunchTickSplitPackets(engine_->state_ptrs(), tio, fio, lists, split, S, calls, st))
                                 : AECM_HIP_OK(LaunchTickSplitCalls(engine_->state_ptrs(), tio, fio, lists, split, S, calls, st));
            break;
        }
        ok = traced ? AECM_HIP_OK(LaunchTickSplitTraced(engine_->state_ptrs(), tio, fio, lists, split, tv, S, plan.mixed_plan, SplitTickTwoLaunches(plan.live), st))
                    : AECM_HIP_OK(LaunchTickSplit(engine_->state_ptrs(), tio, fio, lists, split, S, plan.mixed_plan, SplitTickTwoLaunches(plan.live), st));
        break;
    }
    default: break;      // (kTickFamily_nothing has returned above)
    }
    if (!ok) return Fail();
    if (plan.need_slot) {            // both launches of the tick are behind this event; only the first reads the slot
        if (!AECM_HIP_OK(hipEventRecord(slot_read_[slot], st))) return Fail();
        slot_busy_[slot] = true;
    }
    if (host_pointers && !copy_rows(out, (size_t)stride * 2, dout, (size_t)span * 2, hipMemcpyDeviceToHost)) return Fail();
    if (done_event && !AECM_HIP_OK(hipEventRecord(static_cast<hipEvent_t>(done_event), st))) return Fail();
    return first_rc;
}

int32_t SessionBatch::Tick(const int16_t *far, const int16_t *near, const int16_t *clean, int16_t *out, int64_t stride, size_t n_samples,
                           int16_t ms, const int16_t *ms_per_session, const uint8_t *flags_per_session, int32_t *codes,
                           bool host_pointers, int flags, int32_t calls, bool packets) {
    const int32_t rc = Enqueue(far, near, clean, out, stride, n_samples, ms, ms_per_session, flags_per_session, codes, host_pointers,
                               nullptr, nullptr, flags, calls, packets);
    if (rc != 0 && rc != AECM_BAD_PARAMETER_WARNING) return rc;            // nothing was enqueued (or the object is poisoned)
    if (!AECM_HIP_OK(hipStreamSynchronize(engine_->stream()))) return Fail();
    return rc;
}

int32_t SessionBatch::TickAsync(const int16_t *far, const int16_t *near, const int16_t *clean, int16_t *out, int64_t stride,
                                size_t n_samples, int16_t ms, const int16_t *ms_per_session, const uint8_t *flags_per_session,
                                int32_t *codes, void *wait_event, void *done_event, int flags, int32_t calls, bool packets) {
    return Enqueue(far, near, clean, out, stride, n_samples, ms, ms_per_session, flags_per_session, codes, false, wait_event, done_event, flags, calls,
                   packets);
}

// ---- session snapshots ---------------------------------------------------------------------------------
// The layout (header, offsets of the parts) and its one statement for host and device: aecm_session_snapshot.h.
static_assert(kSessionHeaderBytes == SessionBatch::kSessionHeaderBytes && kSessionBytes == SessionBatch::kSessionBytes &&
                  kSessionOutTail == SessionBatch::kOutTail && kSessionNearTail == SessionBatch::kNearTail && kStateBlobBytes == BatchEngine::kStateBytes,
              "session snapshot size");

int32_t SessionBatch::ExportSession(int session, void *buf) {
    if (buf == nullptr) return AECM_NULL_POINTER_ERROR;
    if (int32_t rc = CheckSession(session)) return rc;
    if (!AECM_HIP_OK(hipSetDevice(device_)) || !engine_->Synchronize()) return Fail();
    const int S = engine_->num_streams();
    const SessionOffsets at;
    uint8_t *p = static_cast<uint8_t *>(buf);
    const SessionSnapshotHeader h{kSessionMagic, kSessionVersion, (uint32_t)tick_.rates[(size_t)session], clean_ring_ ? 1u : 0u, (uint32_t)kFlowWords, (uint32_t)kRing,
                                  (uint32_t)kOutTail, (uint32_t)kNearTail};
    memcpy(p, &h, sizeof h);
    if (!engine_->ExportState(session, p + at.state)) return Fail();
    int32_t flow[kFlowWords] = {0};
    std::vector<int16_t> row(kRing);
    auto tail = [&](const int16_t *ring_row, uint32_t end_pos, int n, uint8_t *dst) -> bool {      // ring positions [end_pos - n, end_pos)
        if (!AECM_HIP_OK(hipMemcpy(row.data(), ring_row, kRing * 2, hipMemcpyDeviceToHost))) return false;
        int16_t *d = reinterpret_cast<int16_t *>(dst);
        for (int k = 0; k < n; ++k) d[k] = row[(end_pos - (uint32_t)n + (uint32_t)k) & (uint32_t)(kRing - 1)];
        return true;
    };
    bool ok = AECM_HIP_OK(hipMemcpy2D(flow, sizeof(int32_t), flow_state_ + session, (size_t)S * sizeof(int32_t), sizeof(int32_t), kFlowFieldsUsed,
                                      hipMemcpyDeviceToHost));
    // The session's own near position: the object's, less what the session has sat out (its lag on the device + the all-idle
    // ticks not yet added to it).  The snapshot itself is in step -- lag 0, as every snapshot before there were idle ticks.
    const uint32_t own_near_pos = (uint32_t)tick_.near_pos - (uint32_t)flow[F_NEAR_LAG] - (uint32_t)tick_.lag.deferred_lag;
    flow[F_NEAR_LAG] = 0;
    memcpy(p + at.flow, flow, sizeof flow);
    ok = ok && AECM_HIP_OK(hipMemcpy(p + at.far, far_ring_ + (size_t)session * kRing, kRing * 2, hipMemcpyDeviceToHost)) &&
         tail(out_ring_ + (size_t)session * kRing, (uint32_t)flow[F_BLK_POS], kOutTail, p + at.out) &&
         tail(near_ring_ + (size_t)session * kRing, own_near_pos, kNearTail, p + at.near);
    if (ok && clean_ring_) ok = tail(clean_ring_ + (size_t)session * kRing, own_near_pos, kNearTail, p + at.clean);
    else memset(p + at.clean, 0, kNearTail * 2);
    ok = ok && AECM_HIP_OK(hipMemcpy(p + at.frames, far_frames_ + (size_t)session * kFlowFarFrameRing, kFlowFarFrameRing * 2, hipMemcpyDeviceToHost)) &&
         AECM_HIP_OK(hipMemcpy(p + at.old, far_old_ + (size_t)session * 2 * kFlowFrame, 2 * kFlowFrame * 2, hipMemcpyDeviceToHost));
    return ok ? 0 : Fail();
}

int32_t SessionBatch::ImportSession(int session, const void *buf, bool any_rate) {
    if (buf == nullptr) return AECM_NULL_POINTER_ERROR;
    if (int32_t rc = CheckSession(session)) return rc;
    const SessionOffsets at;
    const uint8_t *p = static_cast<const uint8_t *>(buf);
    SessionSnapshotHeader h;
    memcpy(&h, p, sizeof h);
    if (h.magic != kSessionMagic || h.version != kSessionVersion || (any_rate ? h.fs != 8000u && h.fs != 16000u : h.fs != (uint32_t)tick_.fs) || h.has_clean > 1u || h.flow_words != (uint32_t)kFlowWords ||
        h.far_ring != (uint32_t)kRing || h.out_tail != (uint32_t)kOutTail || h.near_tail != (uint32_t)kNearTail)
        return AECM_BAD_PARAMETER_ERROR;
    int32_t flow[kFlowWords];
    memcpy(flow, p + at.flow, sizeof flow);
    if (FlowStateDefect(flow) != 0) return AECM_BAD_PARAMETER_ERROR;
    SnapshotHeader core;                                     // the core state must be of the session's rate
    memcpy(&core, p + at.state, sizeof core);
    if (!SnapshotHeaderOk(core) || core.fs != h.fs) return AECM_BAD_PARAMETER_ERROR;
    {   // the block-stream blob: the same rules ImportState applies, BEFORE anything is allocated or written (a refused snapshot changes nothing)
        std::vector<uint32_t> vec(kVecWordsPerStream);
        int32_t scal[kNumScal];
        memcpy(vec.data(), p + at.state + BatchEngine::kStateHeaderBytes, kVecWordsPerStream * 4);
        memcpy(scal, p + at.state + BatchEngine::kStateHeaderBytes + kVecWordsPerStream * 4, sizeof scal);
        if (ValidateStateImage(vec.data(), scal, (int)core.fs) != nullptr) return AECM_BAD_PARAMETER_ERROR;
    }
    if (!AECM_HIP_OK(hipSetDevice(device_))) return AECM_UNSPECIFIED_ERROR;
    const int S = engine_->num_streams();
    hipStream_t st = engine_->stream();
    if (h.has_clean)                                        // as the first tick that carries a clean near end would
        if (const int32_t rc = EnsureCleanRing()) return rc;
    // (ImportState validates the blob once more and is the first thing that writes)
    if (const int32_t rc = engine_->ImportState(session, p + at.state)) return rc;
    tick_.InitSession(session, (int32_t)h.fs);      // (its clean history starts anew: the caller continues the session as it was exported)
    // The session arrives in step with this object: its tail goes behind the object's near position, its lag is 0 -- behind
    // the position the device takes for the object's while all-idle ticks are still to be added to the lags, that is.
    flow[F_NEAR_LAG] = 0;
    const uint32_t own_near_pos = (uint32_t)tick_.near_pos - (uint32_t)tick_.lag.deferred_lag;
    std::vector<int16_t> row(kRing, 0);
    auto place_tail = [&](int16_t *ring_row, uint32_t end_pos, int n, const uint8_t *src, bool zero_rest) -> bool {
        if (!zero_rest && !AECM_HIP_OK(hipMemcpy(row.data(), ring_row, kRing * 2, hipMemcpyDeviceToHost))) return false;
        if (zero_rest) std::fill(row.begin(), row.end(), (int16_t)0);
        const int16_t *s = reinterpret_cast<const int16_t *>(src);
        for (int k = 0; k < n; ++k) row[(end_pos - (uint32_t)n + (uint32_t)k) & (uint32_t)(kRing - 1)] = s[k];
        return AECM_HIP_OK(hipMemcpy(ring_row, row.data(), kRing * 2, hipMemcpyHostToDevice));
    };
    bool ok = AECM_HIP_OK(hipStreamSynchronize(st)) &&
              AECM_HIP_OK(hipMemcpy2D(flow_state_ + session, (size_t)S * sizeof(int32_t), flow, sizeof(int32_t), sizeof(int32_t), kFlowFieldsUsed,
                                      hipMemcpyHostToDevice)) &&
              AECM_HIP_OK(hipMemcpy(far_ring_ + (size_t)session * kRing, p + at.far, kRing * 2, hipMemcpyHostToDevice)) &&
              place_tail(out_ring_ + (size_t)session * kRing, (uint32_t)flow[F_BLK_POS], kOutTail, p + at.out, true) &&
              place_tail(near_ring_ + (size_t)session * kRing, own_near_pos, kNearTail, p + at.near, false);
    if (ok && clean_ring_) ok = place_tail(clean_ring_ + (size_t)session * kRing, own_near_pos, kNearTail, p + at.clean, false);
    ok = ok && AECM_HIP_OK(hipMemcpy(far_frames_ + (size_t)session * kFlowFarFrameRing, p + at.frames, kFlowFarFrameRing * 2, hipMemcpyHostToDevice)) &&
         AECM_HIP_OK(hipMemcpy(far_old_ + (size_t)session * 2 * kFlowFrame, p + at.old, 2 * kFlowFrame * 2, hipMemcpyHostToDevice));
    return ok ? 0 : Fail();           // a session half written is not a session: the object is poisoned
}

// ---- bulk session snapshots: a list of sessions, one or two launches, no per-session host work ---------------
SessionView SessionBatch::View() const {
    return SessionView{engine_->state_ptrs(), flow_state_, (int64_t)engine_->num_streams(), far_ring_, near_ring_, clean_ring_, out_ring_,
                       far_frames_, far_old_, (uint32_t)tick_.near_pos, tick_.lag.deferred_lag};
}

// In range and distinct, or nothing is touched.
int32_t SessionBatch::CheckSessionList(const int32_t *sessions, int count) const {
    const int S = engine_->num_streams();
    if (count > S) return AECM_BAD_PARAMETER_ERROR;          // (more entries than sessions: out of range without a list, a duplicate with one)
    if (!sessions) return 0;
    std::vector<uint8_t> seen((size_t)S, 0);
    for (int i = 0; i < count; ++i) {
        if (sessions[i] < 0 || sessions[i] >= S || seen[(size_t)sessions[i]]) return AECM_BAD_PARAMETER_ERROR;
        seen[(size_t)sessions[i]] = 1;
    }
    return 0;
}

int32_t SessionBatch::EnsureSnapshotBuffers(int list_entries, int stage_sessions, int info_words) {
    if (const int32_t rc = Grow((void **)&snap_list_, &snap_list_entries_, (size_t)list_entries, sizeof(int32_t))) return rc;
    if (const int32_t rc = Grow((void **)&snap_stage_, &snap_stage_bytes_, (size_t)std::min(stage_sessions, kSnapshotStageSessions) * kSessionBytes, 1)) return rc;
    return Grow((void **)&snap_verdict_, &snap_verdict_words_, info_words > 0 ? (size_t)info_words + 1 : 0, sizeof(uint32_t));
}

int32_t SessionBatch::ExportSessions(const int32_t *sessions, int count, void *snapshots, bool device) {
    if (count < 0) return AECM_BAD_PARAMETER_ERROR;
    if (count == 0) return 0;
    if (snapshots == nullptr) return AECM_NULL_POINTER_ERROR;
    if (tick_.fs == 0) return AECM_UNINITIALIZED_ERROR;
    if (poisoned_) return AECM_UNSPECIFIED_ERROR;
    if (int32_t rc = CheckSessionList(sessions, count)) return rc;
    if (device && (reinterpret_cast<uintptr_t>(snapshots) & 3)) return AECM_BAD_PARAMETER_ERROR;      // the kernels move 32-bit words at least
    if (!AECM_HIP_OK(hipSetDevice(device_))) return AECM_UNSPECIFIED_ERROR;
    if (const int32_t rc = EnsureSnapshotBuffers(sessions ? count : 0, device ? 0 : count, 0)) return rc;
    hipStream_t st = engine_->stream();
    if (sessions && !AECM_HIP_OK(hipMemcpyAsync(snap_list_, sessions, (size_t)count * sizeof(int32_t), hipMemcpyHostToDevice, st))) return Fail();
    const SessionView view = View();
    bool ok = true;
    if (device) {
        ok = AECM_HIP_OK(LaunchGatherSessions(view, sessions ? snap_list_ : nullptr, 0, count, snapshots, (reinterpret_cast<uintptr_t>(snapshots) & 15) == 0, st));
    } else {
        uint8_t *dst = static_cast<uint8_t *>(snapshots);
        for (int s0 = 0; s0 < count && ok; s0 += kSnapshotStageSessions) {            // the copy of a chunk is ordered before the next gather
            const int n = std::min(kSnapshotStageSessions, count - s0);
            ok = AECM_HIP_OK(LaunchGatherSessions(view, sessions ? snap_list_ + s0 : nullptr, s0, n, snap_stage_, true, st)) &&
                 AECM_HIP_OK(hipMemcpyAsync(dst + (size_t)s0 * kSessionBytes, snap_stage_, (size_t)n * kSessionBytes, hipMemcpyDeviceToHost, st));
        }
    }
    if (!ok || !AECM_HIP_OK(hipStreamSynchronize(st))) return Fail();
    return 0;
}

int32_t SessionBatch::ImportSessions(const int32_t *sessions, int count, const void *snapshots, bool device, bool any_rate) {
    if (count < 0) return AECM_BAD_PARAMETER_ERROR;
    if (count == 0) return 0;
    if (snapshots == nullptr) return AECM_NULL_POINTER_ERROR;
    if (tick_.fs == 0) return AECM_UNINITIALIZED_ERROR;
    if (poisoned_) return AECM_UNSPECIFIED_ERROR;
    if (int32_t rc = CheckSessionList(sessions, count)) return rc;
    if (device && (reinterpret_cast<uintptr_t>(snapshots) & 3)) return AECM_BAD_PARAMETER_ERROR;
    if (!AECM_HIP_OK(hipSetDevice(device_))) return AECM_UNSPECIFIED_ERROR;
    if (const int32_t rc = EnsureSnapshotBuffers(sessions ? count : 0, device ? 0 : count, device ? count : 0)) return rc;
    hipStream_t st = engine_->stream();
    const bool wide = (reinterpret_cast<uintptr_t>(snapshots) & 15) == 0;
    const uint8_t *src = static_cast<const uint8_t *>(snapshots);
    // All or nothing: every snapshot before any slot.  info[i] = rate | has_clean << 31 of snapshot i.
    std::vector<uint32_t> info((size_t)count + 1);
    if (device) {
        static const uint32_t preset = 0xffffffffu;           // the verdict word; the info words follow it
        if (!AECM_HIP_OK(hipMemcpyAsync(snap_verdict_, &preset, sizeof preset, hipMemcpyHostToDevice, st)) ||
            !AECM_HIP_OK(LaunchValidateSessions(snapshots, count, tick_.fs, any_rate, snap_verdict_, snap_verdict_ + 1, st)) ||
            !AECM_HIP_OK(hipMemcpyAsync(info.data(), snap_verdict_, ((size_t)count + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost, st)) ||
            !AECM_HIP_OK(hipStreamSynchronize(st))) {
            (void)hipStreamSynchronize(st);                   // (the read-back into `info` may still be in flight)
            return AECM_UNSPECIFIED_ERROR;                    // nothing of the object has been written: no poison
        }
        if (info[0] != 0xffffffffu) return AECM_BAD_PARAMETER_ERROR;
    } else {
        for (int i = 0; i < count; ++i) {
            const uint8_t *blob = src + (size_t)i * kSessionBytes;
            for (int t = 0; t < kLanes; ++t)
                if (SessionBlobDefect(blob, tick_.fs, any_rate, t) != 0) return AECM_BAD_PARAMETER_ERROR;
            info[(size_t)i + 1] = SessionBlobWord(blob, 0, 2) | (SessionBlobWord(blob, 0, 3) << 31);
        }
    }
    bool has_clean = false, other_rate = false;
    for (int i = 0; i < count; ++i) {
        has_clean = has_clean || (info[(size_t)i + 1] >> 31) != 0;
        other_rate = other_rate || (int32_t)(info[(size_t)i + 1] & 0x7fffffffu) != tick_.fs;
    }
    if (has_clean)                                          // as the first tick that carries a clean near end would
        if (const int32_t rc = EnsureCleanRing()) return rc;
    if (sessions && !AECM_HIP_OK(hipMemcpyAsync(snap_list_, sessions, (size_t)count * sizeof(int32_t), hipMemcpyHostToDevice, st))) return Fail();
    const SessionView view = View();
    bool ok = true;
    if (device) {
        ok = AECM_HIP_OK(LaunchScatterSessions(view, sessions ? snap_list_ : nullptr, 0, count, snapshots, wide, st));
    } else {
        for (int s0 = 0; s0 < count && ok; s0 += kSnapshotStageSessions) {            // the scatter of a chunk is ordered before the next copy
            const int n = std::min(kSnapshotStageSessions, count - s0);
            ok = AECM_HIP_OK(hipMemcpyAsync(snap_stage_, src + (size_t)s0 * kSessionBytes, (size_t)n * kSessionBytes, hipMemcpyHostToDevice, st)) &&
                 AECM_HIP_OK(LaunchScatterSessions(view, sessions ? snap_list_ + s0 : nullptr, s0, n, snap_stage_, true, st));
        }
    }
    if (!ok || !AECM_HIP_OK(hipStreamSynchronize(st))) return Fail();      // sessions half written are no sessions: the object is poisoned
    for (int i = 0; i < count; ++i) tick_.InitSession(sessions ? sessions[i] : i, (int32_t)(info[(size_t)i + 1] & 0x7fffffffu));
    if (other_rate) engine_->NoteStreamOfOtherRate();
    return 0;
}

int32_t SessionBatch::Synchronize() {
    if (tick_.fs == 0) return AECM_UNINITIALIZED_ERROR;
    if (poisoned_) return AECM_UNSPECIFIED_ERROR;
    if (!AECM_HIP_OK(hipSetDevice(device_)) || !AECM_HIP_OK(hipStreamSynchronize(engine_->stream()))) return Fail();
    return 0;
}

}  // namespace aecm
