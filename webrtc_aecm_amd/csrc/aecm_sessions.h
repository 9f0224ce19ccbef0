// Streaming batch of sessions: S independent WebRtcAecm_* sessions ticking together (one BufferFarend + one
// Process of n samples per tick each, or two of 80 for a session flagged so) -- the shape of a media server mixing
// many calls on a 10 ms clock.  msInSndCardBuf and the call flags are per tick for everybody or per session.
//
// The session wrapper and the frame adapter of the reference (echo_control_mobile.cc, aecm_core.cc:501-572) run ON THE
// DEVICE, per session, as position arithmetic on per-session state (aecm_flow_plan.h): a planning kernel with one lane
// per session, then a tick kernel with one wavefront per session (aecm_kernels.h: TickFlowIo).  The audio lives in
// per-session rings in HBM.  The host does nothing per session; sessions share nothing but the tick.
#ifndef AECM_AMD_SESSIONS_H_
#define AECM_AMD_SESSIONS_H_

#include <stdint.h>

#include <memory>
#include <vector>

#include "aecm_engine.h"
#include "aecm_kernels.h"
#include "aecm_tick_plan.h"

namespace aecm {

struct SessionView;      // aecm_session_snapshot.h

class SessionBatch {
public:
    static SessionBatch *Create(int num_streams, int device_id);
    ~SessionBatch();
    int num_streams() const { return engine_->num_streams(); }
    BatchEngine *engine() { return engine_.get(); }

    int32_t Init(int32_t samp_freq);
    // Sessions of both rates in one object.  samp_freq stays the OBJECT's rate (what InitSession and ImportSession mean by "the
    // same rate"); every session runs at its own: on the device that is its core state's S_MULT (what the block engine, the
    // mixed planning kernel and the burst kernel read), the host keeps a mirror for argument checks, snapshot headers and the
    // launch routing (aecm_tick_plan.h: TickObject::Plan -- an object that holds a session of another rate plans every tick per session).
    int32_t InitRates(int32_t samp_freq, const int32_t *rates);          // Init, then WebRtcAecm_Init(inst_k, rates[k]) where rates[k] differs: one launch
    int32_t InitSessionRate(int session, int32_t samp_freq);             // InitSession at that rate
    int32_t GetSessionRate(int session, int32_t *samp_freq) const;
    int32_t SetConfig(int16_t cng_mode, int16_t echo_mode);
    // Per-session control (a media server recycling one slot while the others keep running), reference
    // echo_control_mobile.cc:142-191 (WebRtcAecm_Init), :410-479 (set_config), :481-532 (Init/GetEchoPath).
    int32_t InitSession(int session);
    int32_t SetConfigSession(int session, int16_t cng_mode, int16_t echo_mode);
    int32_t InitEchoPathSession(int session, const void *path, size_t size_bytes);
    int32_t GetEchoPathSession(int session, void *path, size_t size_bytes);
    // One tick for every session; far/near/clean/out are [S][>= n] with the given stream stride, device
    // or host pointers; clean (WebRtcAecm_Process's nearendClean) may be null.
    //   ms_per_session == nullptr: every session gets `ms`; the return value is the code each session's
    //     WebRtcAecm_Process would return.
    //   ms_per_session != nullptr (host array, S entries): session s gets ms_per_session[s]; codes (host,
    //     S entries, may be null) receives each session's code, the return value is 0 or the first
    //     non-zero code.
    //   flags_per_session (host array, S entries, may be null):
    //     bit 0 (kNoFarend) = this session gets NO WebRtcAecm_BufferFarend call in this tick (far-end underrun: its
    //     Process replays the last far frame, reference echo_control_mobile.cc:369-380); its far row is ignored.
    //     bit 1 (kSplitCalls, 160-sample ticks only) = this session makes TWO BufferFarend + Process call pairs of 80
    //     samples in this tick instead of one of 160 (the reference treats the two cadences differently:
    //     echo_control_mobile.cc:282-283, 384-385).
    //     bit 2 (kIdle) = this session makes NO call in this tick (a reference instance that is not called: nothing of it
    //     changes, what is pending stays pending); its other bits and its far / near / clean / ms / out entries mean nothing,
    //     its code is 0, its out row is not written (host pointers: zeros).  The tick's device work is by the sessions that call;
    //     a tick nobody makes launches nothing.
    //   flags: the same bits for every session when flags_per_session is null (kNoFarend / kSplitCalls).
    //   far may be null when no session makes a BufferFarend call in this tick (kNoFarend or kIdle for everybody).
    int32_t Tick(const int16_t *far, const int16_t *near, const int16_t *clean, int16_t *out, int64_t stream_stride, size_t n,
                 int16_t ms, const int16_t *ms_per_session, const uint8_t *flags_per_session, int32_t *codes, bool host_pointers, int flags = 0,
                 int32_t calls = 1, bool packets = false);
    // calls (1 .. kFlowMaxTickCalls; WebRtcAecmSessions_TickCalls): every session that calls makes `calls` [BufferFarend] + Process
    // call pairs of n samples in this tick, in order, call c on samples [c n, (c + 1) n) of its rows (stream_stride >= calls * n),
    // all with the session's one ms -- the 20 .. 60 ms packet interval of a server on 10 ms calls, bit for bit `calls` ordinary
    // ticks on the same rows, in ONE planning and ONE tick launch that keeps the core state in registers across the calls
    // (aecm_tick_calls_kernels.hip).  calls == 1 is the tick above: the same launches, the same kernels.  With calls > 1:
    // kSplitCalls / kHalfCall on a session that calls are refused (bad parameter), kNoFarend means none of the pairs has a
    // BufferFarend, an idle session falls calls * n samples behind; an object that holds a session of another rate than its own
    // is refused (unsupported function: K half calls per row is a layout of its own, the packet tick's).  A refused tick changes nothing.
    // packets (WebRtcAecmSessions_TickPackets): the tick is one PACKET of `calls` 10 ms calls per session, every session at its own
    // rate and its own call size n_s -- 80 with kHalfCall (n == 160), else n -- on packed rows: call c on samples [c n_s, (c + 1) n_s)
    // of its rows (a decoded 20 ms G.711 packet: 160 contiguous samples).  Objects holding both rates and kHalfCall are accepted
    // with calls > 1; the samples [calls * 80, calls * n) of a half-call session's rows are neither read nor written (host pointers:
    // out zeros), and the session ends calls * 80 samples behind the object.  calls == 1: the ordinary tick; calls > 1 in a uniform
    // object with no half call among the sessions that call: the K-call tick above, by its launches and kernels.  Otherwise
    // aecm_tick_packets_kernels.hip.  kSplitCalls with calls > 1 stays refused.
    // The same tick, enqueued on the object's stream without waiting for it (device pointers, or host memory the device
    // can address: see RegisterHostAudio): the two launches of tick t + 1 may be issued while tick t still runs.
    // wait_event (hipEvent_t, may be null): the tick's kernels wait for it first (the caller's producer of far / near);
    // done_event (hipEvent_t, may be null): recorded behind the tick (the caller's consumer of out waits for it).
    int32_t TickAsync(const int16_t *far, const int16_t *near, const int16_t *clean, int16_t *out, int64_t stream_stride, size_t n,
                      int16_t ms, const int16_t *ms_per_session, const uint8_t *flags_per_session, int32_t *codes, void *wait_event,
                      void *done_event, int flags = 0, int32_t calls = 1, bool packets = false);
    // Far-end bursts: WebRtcAecm_BufferFarend calls that come without a WebRtcAecm_Process (reference
    // echo_control_mobile.cc:215-234) -- session s makes calls_per_session[s] (host array, S entries <= calls; null:
    // everybody makes `calls`) consecutive calls of n samples on far[s][c * n .. + n).  Together with ticks whose sessions are
    // flagged kNoFarend (far may then be null) any interleaving of the two reference calls can be expressed per session.
    // Enqueued on the object's stream like a tick (device pointers; host pointers are staged and the call waits).
    int32_t BufferFarend(const int16_t *far, int64_t stream_stride, size_t n, int32_t calls, const uint8_t *calls_per_session, bool host_pointers,
                         bool wait, void *wait_event, void *done_event);
    int32_t Synchronize();
    //     bit 3 (kHalfCall, 160-sample ticks only, not with kSplitCalls) = this session makes ONE call pair of 80 samples, on the
    //     first half of its rows; out[s][80..160) is not written (host pointers: zeros).  Its near-end position then lies 80
    //     samples behind the object's: F_NEAR_LAG, as after half an idle tick (aecm_flow_plan.h: FlowTickMixed).
    //     bit 4 (kNoClean; a tick that passes `clean`, calls == 1) = this session's WebRtcAecm_Process gets nearendClean = NULL: its clean
    //     row is not read, its clean ring row neither written nor read, its start-up output is the copy of its noisy near end.  A
    //     session is of one kind between two initialisations (aecm_flow_clean.h: FlowCleanHistory); a tick that would change a calling
    //     session's kind is refused (bad parameter) and changes nothing, and so is every later tick or Process of an object that has
    //     accepted a tick with the bit, an object that never uses it is never refused for it.  Nobody flagged among the callers: the
    //     tick without the bit, by its launches; everybody: the launches of the tick without `clean`; else aecm_tick_split_kernels.hip,
    //     always by the live lists (which of them: aecm_tick_plan.h, TickPlan::family).  Ignored without `clean` and in an idle session's byte; with calls > 1: unsupported function
    //     unless SetSplitCallTicks is on (and no call trace is attached): then the same rules for all K calls of the tick.
    static constexpr uint8_t kNoFarend = kFlowNoFarend, kSplitCalls = kFlowSplitCalls, kIdle = kFlowIdle, kHalfCall = kFlowHalfCall, kNoClean = kFlowNoClean;
    // 0 no Process call since the session's last initialisation, 1 every one carried a clean input, 2 none did, 3 both
    int32_t GetSessionCleanMode(int session, int32_t *mode) const;
    // The tick launch of a split tick: the fused kernel, or one launch per list -- by the size of the tick (SplitTickTwoLaunches below;
    // mode < 0, the default), or as the caller says (diagnostics, tools/bench_split_clean.py: 0 fused, > 0 two).  Results do not change.
    void SplitCleanTwoLaunches(int mode) { split_two_launches_ = mode < 0 ? -1 : mode > 0 ? 1 : 0; }
    // K-call and packet ticks (calls > 1) with callers of both kinds: refused (unsupported function) while off, the default; on, they
    // are planned like every split tick (TickObject::Plan: family split with k_calls, and mixed_plan for the packed layout) and made by
    // aecm_tick_split_calls_kernels.hip -- always one tick launch per list, SplitCleanTwoLaunches does not apply.  The caller's
    // switch, like ForceSparseTicks: host state only, so it is ordered behind the ticks already enqueued, and no Init touches it.
    // With a call trace attached such ticks stay refused whatever the switch says.
    void SetSplitCallTicks(bool on) { tick_.split_call_ticks = on; }
    // Diagnostics (tools/bench_sessions.py): every tick through the live list and the sparse tick kernel, idle sessions or
    // not -- what the indirection itself costs.
    void ForceSparseTicks(bool on) { tick_.force_sparse = on; }
    // The session trace (include/aecm_batch.h: AecmSessionTrace has the contract).  While one is attached every tick of one call
    // pair runs the traced twin of its tick launch (aecm_tick_trace_kernels.hip) behind the same planning launch, and tick j since
    // attachment has session s write its record at trace_dev + 64 * (s * session_stride + (j % ring_ticks) * tick_stride); ticks of
    // several calls are refused (TickObject::CheckArgs), the count moves in TickObject::Commit.  The view travels as a kernel
    // argument, so attaching and detaching are ordered behind the ticks already enqueued.  nullptr detaches.
    int32_t SetSessionTrace(void *trace_dev, int64_t session_stride, int64_t tick_stride, int32_t ring_ticks);
    int64_t session_trace_ticks() const { return tick_.trace_ticks; }
    // The call trace (include/aecm_batch.h: WebRtcAecmSessions_SetCallTrace has the contract): the same record per CALL SLOT.  While
    // one is attached the object counts call slots (TickObject::Commit: a tick of K call pairs moves the count by K), a tick of one
    // call pair runs the session trace's twins with the slot number as its tick, and a K-call or packet tick runs the traced twins
    // of both of its launches (aecm_call_trace_plan_kernels.hip, aecm_call_trace_kernels.hip).  At most one of the two traces is
    // attached: either call refuses while the other kind is.  The view travels as a kernel argument, as the session trace's.
    int32_t SetCallTrace(void *trace_dev, int64_t session_stride, int64_t call_stride, int32_t ring_calls);
    int64_t call_trace_calls() const { return tick_.call_trace_calls; }

    // Snapshot of ONE live session (checkpoint; migration into another object, on another GPU): everything the reference
    // keeps per instance -- AecMobile's wrapper members and jitter buffer (echo_control_mobile.cc:42-79), the core's frame
    // buffers (aecm_core.h:41-60) and the core state proper (the block stream's snapshot, aecm_engine.h) -- in a form that
    // does not depend on the object it came from:
    //   header (32 B) | block-stream blob (BatchEngine::kStateBytes) | wrapper state kFlowWords int32 | far ring kRing int16
    //   (indexed by the session's own far-stream positions) | the last kOutTail block-output samples before F_BLK_POS |
    //   the last kNearTail near-end (and clean near-end) samples ticked (the only ones a later block can still ask for:
    //   fewer than one block is ever pending) | framed-far ring | the two replay rows.
    // The near-end rings are indexed by the OBJECT's tick position, so their tails are re-placed at the importing object's
    // (and cut at the session's own position, which lies behind the object's while the session sits out ticks: kIdle; the
    // snapshot itself is always in step, lag word 0, and the session arrives in step with the importing object).
    // ImportSession validates everything FlowTick / the tick kernel turn into a count or an index (aecm_flow_plan.h:
    // FlowStateDefect) and the block-stream blob like ImportState does; a refused blob changes nothing.  The session's rate
    // must be the object's.  Both calls wait for the ticks enqueued so far.
    static constexpr int kOutTail = 256, kNearTail = 64;
    static constexpr size_t kSessionHeaderBytes = 32;
    static constexpr size_t kSessionBytes = kSessionHeaderBytes + BatchEngine::kStateBytes + kFlowWords * 4 + kFlowFarRing * 2 + kOutTail * 2 +
                                            2 * kNearTail * 2 + kFlowFarFrameRing * 2 + 2 * kFlowFrame * 2;
    int32_t ExportSession(int session, void *buf);
    // any_rate: a snapshot of the other rate is taken too (ImportSessionAnyRate); the slot then runs at the snapshot's rate.
    int32_t ImportSession(int session, const void *buf, bool any_rate = false);
    // The same for a LIST of sessions (draining or rebalancing a GPU, checkpointing an object): `sessions` = count distinct
    // indices in any order (host array; null: 0 .. count - 1), `snapshots` = count snapshots of kSessionBytes back to back in list
    // order -- host memory, or (device = true) anything the device can address, 4-byte aligned (16-byte aligned: the kernels move
    // 16 bytes per lane).  One gather (scatter) launch for the whole list instead of about ten blocking copies per session
    // (aecm_session_snapshot.h); the host forms stage through a grow-only device buffer of at most kSnapshotStageSessions
    // snapshots, one copy per chunk.  Every snapshot is byte for byte ExportSession's.  ImportSessions is all or nothing: every
    // snapshot is validated by ImportSession's rules (host memory: on the host; device memory: by a validation launch and one
    // read-back) before any slot, mirror or ring is touched; afterwards the object is what count ImportSession calls would have
    // left.  Both wait for what is enqueued on the object's stream and return when their work is done.
    static constexpr int kSnapshotStageSessions = 256;
    int32_t ExportSessions(const int32_t *sessions, int count, void *snapshots, bool device);
    int32_t ImportSessions(const int32_t *sessions, int count, const void *snapshots, bool device, bool any_rate);

private:
    SessionBatch() {}
    int32_t CheckSession(int session) const;
    bool ResetFlowRows(int first, int count);
    static constexpr int64_t kRing = kFlowFarRing;   // >= 4000 (jitter buffer) + a tick + the window a replayed frame may age in
    std::unique_ptr<BatchEngine> engine_;
    // What the host keeps per object and decides a tick by -- the rates (mirror of the core states' S_MULT; fs == 0: not initialised),
    // the near position, the lags, the clean history -- and the planner of a tick: aecm_tick_plan.h.  Only TickObject's own
    // methods write it.
    TickObject tick_;
    // what SetSessionTrace attached (tick_.trace_attached says whether; tick_.trace_ticks is the count): the base, the strides, the ring
    uint32_t *trace_records_ = nullptr;
    int64_t trace_session_stride_ = 0, trace_tick_stride_ = 0;
    int32_t trace_ring_ticks_ = 1;
    // what SetCallTrace attached (tick_.call_trace_attached says whether; tick_.call_trace_calls is the count)
    uint32_t *call_trace_records_ = nullptr;
    int64_t call_trace_session_stride_ = 0, call_trace_call_stride_ = 0;
    int32_t call_trace_ring_calls_ = 1;
    int split_two_launches_ = -1;
    bool SplitTickTwoLaunches(int calling) const;
    uint32_t *split_live_dev_ = nullptr;       // [FlowSplitListEntries(S)] the two lists of a split tick; allocated by the first one
    // A tick that failed on the device leaves the rings and the wrapper state out of step: every later call is refused
    // (AECM_UNSPECIFIED_ERROR) until Init.
    bool poisoned_ = false;
    uint32_t *live_dev_ = nullptr;             // [S] the tick's live sessions, ascending (written by the planning launch)
    int16_t *far_ring_ = nullptr, *near_ring_ = nullptr, *out_ring_ = nullptr;   // [S][kRing]
    int16_t *clean_ring_ = nullptr;            // [S][kRing], allocated by the first tick that carries a clean near-end
    int16_t *io_dev_ = nullptr;                // [4][S][io_row_] staging when the caller passes host pointers
    size_t io_row_ = 160;                      // samples per staged row: grows (only) with the host form of a K-call tick, to calls * n
    int32_t *calls_plans_ = nullptr;           // [S][kFlowMaxTickCalls][kFlowPlanWords]: the plans of a K-call tick; allocated by the first one
    int32_t *flow_state_ = nullptr;            // [kFlowFieldsUsed][S] wrapper state, field-major
    int32_t *flow_plans_ = nullptr;            // [S][kFlowPlanWords]: this tick's plan of every session
    int16_t *far_frames_ = nullptr;            // [S][kFlowFarFrameRing]
    int16_t *far_old_ = nullptr;               // [S][2 * 80]
    // Per-session msInSndCardBuf / flags of a tick: pinned host memory the planning kernel reads in place.  Two slots used
    // alternately, each guarded by an event recorded behind the planning launch that reads it, so that an asynchronous
    // tick can fill the other slot while the previous tick is still in flight.
    static constexpr int kArgSlots = 2;
    int16_t *ms_host_[kArgSlots] = {nullptr, nullptr}, *ms_dev_[kArgSlots] = {nullptr, nullptr};          // [S] each
    uint8_t *flags_host_[kArgSlots] = {nullptr, nullptr}, *flags_dev_[kArgSlots] = {nullptr, nullptr};    // [S] each
    uint32_t *bases_host_[kArgSlots] = {nullptr, nullptr}, *bases_dev_[kArgSlots] = {nullptr, nullptr};    // [ceil(S / 256)] each
    hipEvent_t slot_read_[kArgSlots] = {nullptr, nullptr};
    bool slot_busy_[kArgSlots] = {false, false};
    int slot_ = 0;
    int32_t Enqueue(const int16_t *far, const int16_t *near, const int16_t *clean, int16_t *out, int64_t stream_stride, size_t n,
                    int16_t ms, const int16_t *ms_per_session, const uint8_t *flags_per_session, int32_t *codes, bool host_pointers,
                    void *wait_event, void *done_event, int flags, int32_t calls = 1, bool packets = false);
    bool EventUsable(void *ev) const;
    bool WaitForCallerEvent(void *wait_event);
    int32_t Grow(void **buf, size_t *have, size_t need, size_t unit);
    int32_t GrowOnce(void **buf, size_t bytes);
    int32_t EnsureCleanRing();
    int AcquireArgSlot(bool needed, bool *ok);
    int32_t Fail();
    // bulk snapshots: the list on the device, the host forms' stage, the validation verdict (word 0) + info words; all grow-only
    int32_t CheckSessionList(const int32_t *sessions, int count) const;
    int32_t EnsureSnapshotBuffers(int list_entries, int stage_sessions, int info_words);
    SessionView View() const;
    int32_t *snap_list_ = nullptr;
    size_t snap_list_entries_ = 0;
    uint8_t *snap_stage_ = nullptr;
    size_t snap_stage_bytes_ = 0;
    uint32_t *snap_verdict_ = nullptr;
    size_t snap_verdict_words_ = 0;
    int device_ = 0;
};

}  // namespace aecm
#endif  // AECM_AMD_SESSIONS_H_
