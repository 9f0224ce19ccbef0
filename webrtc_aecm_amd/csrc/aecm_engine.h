// Host-side owner of the device state of S AECM streams and of the HIP stream they run on.
#ifndef AECM_AMD_ENGINE_H_
#define AECM_AMD_ENGINE_H_

#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include <vector>

#include "aecm_host_state.h"
#include "aecm_kernels.h"
#include "aecm_state.h"

namespace aecm {

constexpr int kDefaultQueueChunk = 128;

// How ProcessBlocks launches are scheduled on a device (results never depend on it): the thresholds between the launch forms and
// the wishes for the pipelined form's shape.  One value type, set through the C ABI (include/aecm_batch.h: AecmLaunchPolicy mirrors
// it field by field); DefaultLaunchPolicy derives it from the device's compute units alone.  The environment is consulted only by
// an -DAECM_EXPERIMENTS build (ApplyEnvironmentWishes).
struct LaunchPolicy {
    int compute_units = 0;
    int queue_chunk_blocks = kDefaultQueueChunk;   // chunk queue: blocks per item; 0 = every launch keeps one wavefront per stream
    bool queue_chunk_explicit = false;             // set by the caller: taken as it is (else quartered while every stream's wave is resident)
    int queue_min_streams = -1;                    // the queue above this many streams; < 0: above pipelined_max_streams
    int pipelined_min_streams = 2;                 // a single stream (the drop-in ABI's 10 ms calls) keeps its one-wave launch; > num_streams: never
    // launches of one or two blocks keep one wave per stream: the pipelined kernel's fill and drain steps (up to five with the sixteen-wave
    // shape) cost more than they save there -- 1 024 streams x 1 / 2 / 3 / 4 blocks: 10.8 / 12.4 / 14.3 / 15.9 us against 8.7 / 11.7 / 15.1 / 18.2 us
    int pipelined_min_blocks = 3;
    int pipelined_max_streams = 0;                 // what the chip holds of the pipelined form's widest shape (16 streams per CU)
    int resident_waves = 0;                        // waves of the one-wave-per-stream kernels the chip holds (28 per CU)
    int rotation_stream_limit = 0;                 // launches of at most this many streams take the kernel variants built for full residency
    PipeWishes pipe;
};
LaunchPolicy DefaultLaunchPolicy(int compute_units);
bool LaunchPolicyValid(const LaunchPolicy &p);
// What a ProcessBlocks launch looks like on the device (WebRtcAecmBatch_DescribeLaunchDetail; capacity planning).
struct LaunchDescription {
    int form = 0;                   // AECM_LAUNCH_*
    int chunk_blocks = 0;           // chunk queue: blocks per item
    int shape = 0;                  // pipelined: the shape bits of WebRtcAecmBatch_DescribeLaunch
    int workgroups = 0, waves_per_workgroup = 0;
    int workgroups_per_cu = 0;      // of this kernel a CU holds at once
    int rounds_x1000 = 0;           // 1000 x workgroups / (CUs x workgroups_per_cu): 1000 = the chip exactly full once; 9140 = nine full rounds and one 14 % full
    int cu_load_evenness_x1000 = 1000;   // pipelined: 1000 x (streams / CUs) / streams on the fullest CU
    int detail() const { return form == 2 ? chunk_blocks : form == 3 ? shape : 0; }      // what WebRtcAecmBatch_DescribeLaunch returns beside the form
};
LaunchDescription DescribeTickLaunch(int num_sessions, int compute_units);
LaunchDescription DescribeTickLaunchLive(int num_sessions, int live_sessions, int compute_units);

// A ragged launch: stream s runs len[s] blocks.  Pure host logic (no device), so that it can be tested and used for planning.
// The streams sorted by length, longest first (stable: equal lengths keep their stream order), make the streams live in chunk c --
// those with more than c x chunk_blocks blocks -- the ranks [0, live[c]); the queue's items are chunk-major, those of chunk c the
// numbers first_item[c] .. first_item[c] + live[c], item first_item[c] + r = (chunk c, stream order[r]).
struct RaggedPlan {
    int num_streams = 0, chunk_blocks = 0, n_chunks = 0;
    int live_streams = 0;             // streams of non-zero length (live[0])
    int max_blocks = 0;               // the longest stream: the launch's critical path
    int64_t sum_blocks = 0;           // the useful work
    int64_t items = 0;                // sum over the streams of ceil(len / chunk_blocks)
    // what the kernel reads (aecm_kernels.h: RaggedPlanOffsetWords): len[S], order[S], first_item[n_chunks + 1]
    // (first_item only when the items fit 31 bits; without a chunk -- chunk_blocks <= 0 -- n_chunks = 0 and first_item = {0})
    std::vector<uint32_t> words;
    const uint32_t *len() const { return words.data(); }
    const uint32_t *order() const { return words.data() + num_streams; }
    const uint32_t *first_item() const { return words.data() + 2 * (size_t)num_streams; }
};
// false: a length outside [0, num_blocks] (the plan is then not usable).
bool BuildRaggedPlan(const int32_t *blocks_per_stream, int num_streams, int num_blocks, int chunk_blocks, RaggedPlan *plan);
// The plan of a ragged PIPELINED launch (aecm_process_pipelined_ragged_kernel, _ragged_clean_kernel): which stream sits in which of the four slots
// of which workgroup.  Pure host logic.  Workgroups i, i + cus, ... share a compute unit (the dispatcher deals them out in turn);
// a stream stays on its unit for the whole launch, so the launch ends when the unit with the most blocks does.  The live streams
// (len > 0), longest first, each go to the unit with the fewest blocks so far that still has a free slot (longest processing time
// first); a unit's streams, in that order, are cut into its workgroups in consecutive runs of as equal a size as can be (lock-step
// partners have similar lengths); in a workgroup the longest takes slot 0, the next slot 2, then 1, then 3 (the two longest on
// different two-slot front / tail / delay waves; 1 / 2 / 3 streams use the slots of the equal-length kernel's table).
struct RaggedPipePlan {
    int num_streams = 0, live_streams = 0, max_blocks = 0;
    int workgroups = 0;               // of the launch: up to the last one that has a stream
    int used_cus = 0;                 // compute units that carry a workgroup
    int64_t sum_blocks = 0;
    int64_t fullest_cu_blocks = 0;    // blocks on the unit that carries the most: the launch's critical path in blocks of one unit
    PipeShape shape{};
    std::vector<uint32_t> words;      // what the kernel reads: slot_stream[workgroups][4] (-1 = empty), then len[num_streams]
    const int32_t *slot_stream() const { return reinterpret_cast<const int32_t *>(words.data()); }
    // 1000 x (mean blocks per compute unit) / (blocks on the fullest unit)
    int evenness_x1000() const {
        return fullest_cu_blocks > 0 && used_cus > 0 ? (int)((1000 * sum_blocks / used_cus) / fullest_cu_blocks) : 1000;
    }
};
// The shape a ragged pipelined launch of `live` streams, the longest of max_blocks blocks, takes: PipelinedShapeFor without the
// progress-feedback balance (its "slowest workgroup" rule assumes equal work; a launch whose size would pick it takes the plain
// six-wave shape).
PipeShape RaggedPipeShapeFor(int live, int max_blocks, int compute_units, const PipeWishes &wishes);
// false: a negative length, no live stream, a balanced shape, or more live streams than the shape's workgroups have slots.
bool BuildRaggedPipePlan(const int32_t *blocks_per_stream, int num_streams, const PipeShape &shape, int compute_units, RaggedPipePlan *plan);
// The switches of a batch that the launch rule reads besides the policy.
struct LaunchSwitches {
    int variant = kVariantFast;
    bool ragged_pipelining = false;   // BatchEngine::set_ragged_pipelining: ragged launches the chip holds at once are pipelined
    bool clean_pipelining = false;    // BatchEngine::set_clean_pipelining: equal-length launches WITH a clean input are pipelined too
    bool ragged_clean_pipelining = false;      // BatchEngine::set_ragged_clean_pipelining: ragged launches WITH a clean input are pipelined too
    // BatchEngine::SetBlockTrace: a block trace is attached.  The launch runs the traced kernels (aecm_trace_kernels.hip) and never takes
    // the pipelined form -- there the traced values live in four role waves: a size that would be pipelined runs one wavefront per stream
    bool trace = false;
};
// Everything one launch of the block kernels runs by.  PlanLaunch and PlanRaggedLaunch (pure host logic) are the only places that
// decide it; BatchEngine launches a plan as it stands and DescribePlan reports it, so what is reported is what runs.
struct LaunchPlan {
    int form = 0;                     // AECM_LAUNCH_*; < 0: a length outside [0, num_blocks] (nothing else is set)
    int variant = kVariantFast;
    int count = 0, num_blocks = 0;    // streams of the launch; blocks of each (ragged: of the longest; 0: nothing to launch)
    bool has_clean = false;
    bool trace = false;               // the traced twin of the form's kernel (never form 3); LaunchBlocks writes the records by the engine's TraceView
    int chunk_blocks = 0;             // form 2: blocks per item of the queue
    PipeShape shape{};                // form 3
    bool is_ragged = false;           // the lengths differ: forms 0 to 2 run by `ragged`, form 3 by `pipe`
    RaggedPlan ragged;                // PlanRaggedLaunch always fills in the sums (equal lengths too: items = the queue's, if it is form 2)
    RaggedPipePlan pipe;
    const std::vector<uint32_t> &words() const { return form == 3 ? pipe.words : ragged.words; }      // (is_ragged) what is uploaded
};
// An equal-length launch (the rules of INTEGRATION.md's table; aecm_engine.cpp has the reasons).
LaunchPlan PlanLaunch(const LaunchPolicy &policy, const LaunchSwitches &sw, int num_streams, int num_blocks, bool has_clean);
// A ragged launch.  Every length equal: exactly PlanLaunch of that length.  Otherwise the chunk queue when the fast variant is
// selected, more than queue_min_streams streams are live, the longest stream has at least two chunks and the items fit 31 bits;
// else -- only with sw.ragged_pipelining, or with a clean input only with sw.ragged_clean_pipelining (then in the shapes of
// PipelinedCleanShapeFor) -- pipelined when the fast variant is selected, the LIVE streams are within
// [pipelined_min_streams, pipelined_max_streams] and the longest has at least pipelined_min_blocks blocks; else one
// wavefront per stream, each with its own block count.
LaunchPlan PlanRaggedLaunch(const LaunchPolicy &policy, const LaunchSwitches &sw, int num_streams, int num_blocks, const int32_t *blocks_per_stream,
                            bool has_clean);
// The reporting arithmetic (grid, residency, rounds, evenness): O(workgroups) for a pipelined plan, so never on the launch path.
LaunchDescription DescribePlan(const LaunchPolicy &policy, const LaunchPlan &plan);

// A grow-only device allocation (the recording scratch, ProcessBlocksRaggedHost's stage, SessionBatch::Grow): a buffer of `*have` units of `unit` bytes has at least `need` afterwards, contents not
// kept.  Work enqueued on `stream` may still use the old buffer, so the stream is synchronised before a non-null one is freed.
// false: the stream failed (the old buffer stays: *buf is not null) or there is no memory (*buf is null, *have 0).
bool GrowDeviceBuffer(void **buf, size_t *have, size_t need, size_t unit, hipStream_t stream);

class BatchEngine {
public:
    // Returns nullptr if the device cannot be used or memory cannot be allocated.
    static BatchEngine *Create(int num_streams, int device_id);
    ~BatchEngine();

    int num_streams() const { return num_streams_; }
    bool initialized() const { return initialized_; }
    hipStream_t stream() const { return stream_; }

    // All methods return a hipError_t-free status: true on success.
    bool Init(int fs);
    // Re-initialise streams [first, first + count) only (same rate as the last Init; default config): WebRtcAecm_InitCore
    // + default set_config for those streams, asynchronous on stream().
    bool InitStreams(int first, int count);
    // The same at a rate of the caller's choice (8000 / 16000: Init keeps the initial image of both rates on the device), and
    // for the streams with rates_host[s] != fs() among all of them (one launch; rates_host: num_streams() entries, validated
    // by the caller).  Streams of another rate than fs() make the engine one of mixed rates (ImportState).
    bool InitStreamsAtRate(int first, int count, int fs);
    bool InitStreamsOfOtherRate(const int32_t *rates_host);
    bool SetConfig(int cng_mode, int echo_mode, int first, int count);
    bool SetCngMode(int cng_mode, int first, int count);
    bool Control(int fixed_delay, int nlp_flag, int first, int count);
    // async.  The third parameter is retired (ragged launches go through ProcessBlocksRagged): anything but null is refused.  It stays
    // in the signature because the engine's CPU double (tests/sim/sim_engine.cpp) defines this member as it has always been declared.
    bool ProcessBlocks(const IoView &io_dev, int num_blocks, const int32_t *retired = nullptr);
    bool ProcessBlocksRange(const IoView &io_dev, int num_blocks, int first, int count);
    // sync.  One of three paths (aecm_engine.cpp): buffers that fit kMappedBytes through the mapped buffer;
    // else dense rows of at least 2 x kHostChunkStreams streams through the chunked pipeline; else staged.
    bool ProcessBlocksHost(const IoView &io_host, int num_blocks);
    // Ragged launches: stream s runs its first blocks_per_stream_host[s] blocks only (host array, read before the call returns;
    // the Range form's array and io are indexed from `first`).  Its state afterwards is the state after exactly that many blocks,
    // its out blocks beyond that are not written.  Every length equal to num_blocks: exactly ProcessBlocks.  async like ProcessBlocks.
    // Returns 0, kErrBadParameter (a length outside [0, num_blocks] or a bad range: nothing changed) or kErrUnspecified (HIP).
    int32_t ProcessBlocksRagged(const IoView &io_dev, int num_blocks, const int32_t *blocks_per_stream_host);
    int32_t ProcessBlocksRaggedRange(const IoView &io_dev, int num_blocks, int first, int count, const int32_t *blocks_per_stream_host);
    int32_t ProcessBlocksRaggedHost(const IoView &io_host, int num_blocks, const int32_t *blocks_per_stream_host);     // sync; stages the live blocks
    // ProcessRecordings with one call count per stream (host array, entries in [0, n_calls]): stream s is a session of
    // calls_per_stream_host[s] call pairs; its out samples from calls x frame to n_calls x frame are written as 0.
    // codes_host (may be null): what each session's calls returned (first non-zero); *rc = the first non-zero of them.
    bool ProcessRecordingsRagged(const int16_t *far, const int16_t *near, const int16_t *clean, int16_t *out, int64_t stream_stride, int frame,
                                 int n_calls, const int32_t *calls_per_stream_host, int16_t ms, bool host_pointers, int32_t *rc, int32_t *codes_host);
    // *plan receives the plan described: its `ragged` carries items, sum_blocks and max_blocks.
    LaunchDescription DescribeRaggedLaunch(int num_blocks, const int32_t *blocks_per_stream_host, bool has_clean, LaunchPlan *plan) const {
        *plan = PlanRaggedLaunch(policy_, switches_, num_streams_, num_blocks, blocks_per_stream_host, has_clean);
        return DescribePlan(policy_, *plan);
    }
    // Ragged launches the chip holds at once take the pipelined form (PlanRaggedLaunch's rule).  Off by default.
    void set_ragged_pipelining(bool on) { switches_.ragged_pipelining = on; }
    bool ragged_pipelining() const { return switches_.ragged_pipelining; }
    // Equal-length launches with a clean near-end input that the chip holds at once take the pipelined form (PlanLaunch's rule).
    // Off by default.  Ragged launches with a clean input are not pipelined by either switch (set_ragged_clean_pipelining, below).
    void set_clean_pipelining(bool on) { switches_.clean_pipelining = on; }
    bool clean_pipelining() const { return switches_.clean_pipelining; }
    // Ragged launches with a clean near-end input that the chip holds at once take the pipelined form (PlanRaggedLaunch's rule).
    // Off by default; with it off the other two switches leave such a launch exactly as it is.
    void set_ragged_clean_pipelining(bool on) { switches_.ragged_clean_pipelining = on; }
    bool ragged_clean_pipelining() const { return switches_.ragged_clean_pipelining; }
    // Whole recordings as sessions: every stream is driven like a fresh WebRtcAecm_* session by
    // n_calls x (BufferFarend, Process) of `frame` samples with a constant msInSndCardBuf
    // (aecm_session_flow.h).  far/near/clean/out: [S][>= n_calls*frame], device (or host) pointers; clean
    // (WebRtcAecm_Process's nearendClean) may be null.
    // *rc receives the ABI return code a single session would have produced (0 or 12100).
    bool ProcessRecordings(const int16_t *far, const int16_t *near, const int16_t *clean, int16_t *out, int64_t stream_stride,
                           int frame, int n_calls, int16_t ms, bool host_pointers, int32_t *rc);
    int fs() const { return fs_; }
    bool Synchronize();
    bool LastLaunchMs(float *ms);
    bool Timers(double *total_ms, int64_t *launches);
    void ResetTimers();
    bool SetEchoPath(int stream, const int16_t path[kBins]);
    bool GetEchoPath(int stream, int16_t path[kBins]);
    bool Digest(int stream, uint32_t digest[kDigestWords]);
    static constexpr size_t kStateHeaderBytes = 32;
    static constexpr size_t kStateBytes = kStateHeaderBytes + kVecWordsPerStream * 4 + kNumScal * 4 + kHistWordsPerStream * 2;
    bool ExportState(int stream, void *buf);
    int32_t ImportState(int stream, const void *buf);       // 0 / AECM_BAD_PARAMETER_ERROR / AECM_UNSPECIFIED_ERROR
    // The same for streams [first, first + count) at once: `states` = count blobs of kStateBytes, host memory or (device =
    // true) anything the device can address -- device memory, or the alias of a registered host buffer.  One gather /
    // scatter launch (+ one copy per chunk of streams for host memory) instead of three blocking copies per stream.
    // ImportStates is all or nothing: every blob is validated like ImportState validates one (on the device for device
    // blobs) before any stream is touched.
    bool ExportStates(int first, int count, void *states, bool device);
    int32_t ImportStates(int first, int count, const void *states, bool device);
    // The session batch scattered a core state of another rate than fs() into a stream itself (bulk session import): what
    // ImportState notes when it brings one in.
    void NoteStreamOfOtherRate() { mixed_rates_ = true; }
    // The block trace (include/aecm_batch.h: WebRtcAecmBatch_SetBlockTrace).  While a buffer is attached every block a device-pointer
    // launch processes also writes one 32-byte record: block k of the stream at position s of the launch (ProcessBlocksRange: s from
    // `first`) at trace_dev + 32 * (s * stream_stride + k * block_stride).  trace_dev == nullptr detaches.  The caller owns the buffer
    // and its size, as for the output.  The host-pointer forms and ProcessRecordings refuse to run while one is attached.
    // 0, or kErrBadParameter (nothing changed): a pointer that is not 4-byte aligned, a stride <= 0.
    int32_t SetBlockTrace(void *trace_dev, int64_t stream_stride, int64_t block_stride);
    bool block_trace_attached() const { return switches_.trace; }
    void set_variant(int v) { switches_.variant = v; }
    // blocks = 0: every launch in the one-stream-per-wave form.  min_streams < 0: launches of more streams than the chip
    // holds waves take the queue form (the default); otherwise launches of more than min_streams streams do (tests).
    void set_queue_chunk(int blocks, int min_streams) {
        policy_.queue_chunk_blocks = blocks < 0 ? 0 : blocks > kMaxQueueChunk ? kMaxQueueChunk : blocks;
        policy_.queue_chunk_explicit = true;
        policy_.queue_min_streams = min_streams;
    }
    static constexpr int kMaxQueueChunk = 1 << 20;
    int DescribeLaunch(int num_blocks, bool has_clean, int *chunk_blocks) const;
    // n <= 0: never.  A threshold set through the ABI is taken as it is: launches of any length from n streams
    void set_pipelined_min_streams(int n) { policy_.pipelined_min_streams = n > 0 ? n : 0x7fffffff; policy_.pipelined_min_blocks = 1; }
    const LaunchPolicy &launch_policy() const { return policy_; }
    bool set_launch_policy(const LaunchPolicy &p);       // false (nothing changed): not a valid policy, or one for another CU count than the device's
    int variant() const { return switches_.variant; }
    const StatePtrs &state_ptrs() const { return st_; }      // for kernels launched by the session batch on stream()

private:
    BatchEngine() = default;
    bool PatchScalars(const int32_t *fields, const int32_t *values, int n, int first, int count);
    bool FlushTimers() { return HarvestTimers(true); }

    int device_ = 0;
    LaunchPolicy policy_;                // DefaultLaunchPolicy of device_'s CU count until the caller sets another
    // The chunk-queue form's control words (grown on first use) and the error word a wave raises when it gives up waiting.
    uint32_t *queue_ctl_ = nullptr, *queue_err_ = nullptr;
    size_t queue_ctl_bytes_ = 0;
    bool queue_unchecked_ = false;       // a queue launch has been enqueued since the error word was last read
    bool launch_failed_ = false;         // a wave of a queue launch gave up: sticky until Init (CheckQueueError)
    // Runs the plan on these state pointers (already offset to the launch's first stream) and this io; decides nothing.
    bool LaunchBlocks(const StatePtrs &st, const IoView &io, const LaunchPlan &plan);
    bool TimedLaunch(const IoView &io, int first, const LaunchPlan &plan);
    LaunchSwitches switches_;
    TraceView trace_{nullptr, 0, 0};     // what SetBlockTrace attached (switches_.trace says whether)
    // The plan's way to the device: a pinned staging buffer (grown on first use) and the event behind its last upload -- the
    // buffer is rewritten only when that copy has run, so ragged launches queue back to back like the others.
    uint32_t *plan_host_ = nullptr;
    size_t plan_host_words_ = 0;
    hipEvent_t plan_uploaded_ = nullptr;
    bool plan_upload_pending_ = false;
    bool EnsurePlanStaging(size_t words);
    bool UploadPlanWords(const std::vector<uint32_t> &plan_words, uint32_t *dst_dev);
    bool CheckQueueError();
    bool Drain();
    bool EnsureLaunchErrorWord();
    bool EnsureLaunchControl(size_t need);
    int trace_streams_ = 0;              // diagnostics builds (-DAECM_PIPE_TRACE) only
    int num_streams_ = 0;
    bool initialized_ = false;
    int fs_ = 0;
    hipStream_t stream_ = nullptr;
    StatePtrs st_{nullptr, nullptr, nullptr, nullptr};
    uint32_t *consts_dev_ = nullptr;     // kernel constants blob (aecm_state.h)
    uint32_t *image_vec_dev_ = nullptr;
    int32_t *image_scal_dev_ = nullptr;
    uint32_t *other_vec_dev_ = nullptr;   // the initial image of the rate that is not fs_ (InitStreamsAtRate)
    int32_t *other_scal_dev_ = nullptr;
    uint8_t *select_dev_ = nullptr;       // [num_streams_] InitStreamsOfOtherRate's selection
    // Launch timing: a small ring of HIP event pairs recorded around every block-kernel launch on stream_.
    // ProcessBlocks only harvests pairs that have already completed (hipEventQuery) and waits for the oldest
    // one only when the ring is full, so launches queue back to back; the getters harvest everything.
    static constexpr int kTimerSlots = 16;
    hipEvent_t ev_start_[kTimerSlots] = {}, ev_stop_[kTimerSlots] = {};
    int timer_head_ = 0, timer_pending_ = 0;     // oldest pending slot, number of pending slots
    bool HarvestTimers(bool wait_all);
    float last_ms_ = 0.f;
    double total_ms_ = 0.0;
    int64_t launches_ = 0;
    // staging for ProcessBlocksHost and ProcessBlocksRaggedHost: far | near | [clean] | out (aecm_host_rows.h: StagedIo)
    int16_t *stage_dev_ = nullptr;
    size_t stage_elems_ = 0;
    static constexpr int kHostChunkStreams = 8192;
    bool ProcessBlocksHostPipelined(const IoView &io_host, int num_blocks);
    // Small host calls (the single-session ABI: one to three blocks of one stream): the kernel reads its inputs from and
    // writes its output to a pinned host buffer mapped into the device's address space, so a call is two small host
    // copies, one launch and one synchronisation -- no staging copies, no timing events.
    static constexpr size_t kMappedBytes = 64 * 1024;
    int16_t *mapped_host_ = nullptr, *mapped_dev_ = nullptr;
    bool ProcessBlocksHostMapped(const IoView &io_host, int num_blocks);
    // scratch of ProcessRecordings (grow-only; the streams of a batch are processed in chunks that fit it)
    static constexpr size_t kRecordingScratchBytes = size_t(1) << 30;
    int32_t *rec_maps_ = nullptr;
    size_t rec_maps_elems_ = 0;
    int16_t *rec_scratch_ = nullptr;
    size_t rec_scratch_elems_ = 0;
    bool EnsureRecordingScratch(size_t map_elems, size_t sample_elems);
    bool mixed_rates_ = false;            // ImportState brought in a stream of the other sampling rate
    // staging of the host forms of ExportStates / ImportStates (grow-only, at most kStateStageStreams blobs) + the validation verdict
    static constexpr int kStateStageStreams = 8192;
    uint8_t *state_stage_ = nullptr;
    size_t state_stage_bytes_ = 0;
    uint32_t *state_verdict_ = nullptr;
    bool EnsureStateStage(int streams);
    hipStream_t download_stream_ = nullptr;    // ProcessBlocksHost: downloads overlap the next chunk's uploads
};

}  // namespace aecm
#endif  // AECM_AMD_ENGINE_H_
