// Launchers of the gfx950 kernels (aecm_block_kernels.hip, aecm_kernels.hip).  Host-callable, HIP runtime types only.
#ifndef AECM_AMD_KERNELS_H_
#define AECM_AMD_KERNELS_H_

#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "aecm_flow_plan.h"
#include "aecm_session_trace.h"
#include "aecm_state.h"

namespace aecm {

#ifndef AECM_WAVES_PER_WORKGROUP
#define AECM_WAVES_PER_WORKGROUP 4
#endif
constexpr int kWavesPerWorkgroup = AECM_WAVES_PER_WORKGROUP;    // 256 threads: 4 streams share one copy of the LDS tables

enum KernelVariant : int {
    kVariantSafe = 0,   // ds_bpermute shuffles only
    kVariantFast = 1    // DPP / permlane-swap cross-lane primitives (default)
};

// Process n_blocks consecutive blocks of streams [0, n_streams) -- one wavefront per stream.
// blocks_per_stream (device, may be null): stream s processes blocks_per_stream[s] <= n_blocks blocks
// instead (batches whose streams have different amounts of audio pending).
// phase_priority (fast variant): the kernel variants for launches of more streams than RotationStreamLimit(CU count of the device the
// launch runs on); launches of at most that many are fully resident from the start and take the variants built for that occupancy.
hipError_t LaunchProcessBlocks(const StatePtrs &st, const IoView &io, int n_streams, int n_blocks, int variant,
                               bool phase_priority, hipStream_t stream, const int32_t *blocks_per_stream = nullptr);
int RotationStreamLimit(int compute_units);

// The chunk-queue form of the same launch (aecm_block_kernels.hip): items of chunk_blocks blocks claimed in order by a
// grid that just fills the chip.  ctl: QueueControlBytes(n_streams) of device memory owned by the engine (cleared by the
// launch); *err (device, never cleared by a launch) becomes non-zero if a wave gave up waiting for its predecessor.
size_t QueueControlBytes(int n_streams);
bool QueueLaunchApplies(int n_streams, int n_blocks, int variant, int chunk_blocks, int min_streams);
hipError_t LaunchProcessBlocksQueued(const StatePtrs &st, const IoView &io, int n_streams, int n_blocks, int chunk_blocks,
                                     int resident_waves, uint32_t *ctl, uint32_t *err, hipStream_t stream);
int ResidentWaves(int compute_units);
// Workgroups of a queue launch (equal-length and ragged) under a policy of resident_waves: never 0.
int QueueGridWorkgroups(int n_streams, int resident_waves);
// The ragged queue (aecm_process_ragged_queue_kernel): stream s runs len[s] blocks.  Behind the equal-length form's control words
// (RaggedPlanOffsetWords(n_streams) words into ctl) lies the plan the host uploads before the launch, on the same stream: len[S],
// order[S] (streams by length, longest first), first_item[n_chunks + 1] (aecm_engine.h: RaggedPlan).  n_items = first_item[n_chunks].
size_t RaggedPlanOffsetWords(int n_streams);
size_t RaggedQueueControlBytes(int n_streams, int n_chunks);
hipError_t LaunchProcessBlocksRaggedQueued(const StatePtrs &st, const IoView &io, int n_streams, int live_streams, uint32_t n_items, int chunk_blocks,
                                           int resident_waves, uint32_t *ctl, uint32_t *err, hipStream_t stream);

// The same three launches with a block trace attached (aecm_trace_kernels.hip: aecm_trace_process_kernel, aecm_trace_queue_kernel,
// aecm_trace_ragged_queue_kernel): block k of the stream at position s of the launch also writes its 32-byte record to
// tv.records + kTraceWords * (s * tv.stream_stride + k * tv.block_stride) (aecm_state.h: TraceView; tv.records must not be null).
// The arguments besides tv, the control buffers and the results are those of the launches above.  There is no traced pipelined launch.
hipError_t LaunchTraceBlocks(const StatePtrs &st, const IoView &io, const TraceView &tv, int n_streams, int n_blocks, int variant, bool phase_priority,
                             hipStream_t stream, const int32_t *blocks_per_stream = nullptr);
hipError_t LaunchTraceBlocksQueued(const StatePtrs &st, const IoView &io, const TraceView &tv, int n_streams, int n_blocks, int chunk_blocks,
                                   int resident_waves, uint32_t *ctl, uint32_t *err, hipStream_t stream);
hipError_t LaunchTraceBlocksRaggedQueued(const StatePtrs &st, const IoView &io, const TraceView &tv, int n_streams, int live_streams, uint32_t n_items,
                                         int chunk_blocks, int resident_waves, uint32_t *ctl, uint32_t *err, hipStream_t stream);

// The pipelined form of a launch the chip holds at once (aecm_block_kernels.hip): a workgroup serves four streams with one
// "back" wave per stream and, in waves of their own, the state-independent forward transforms one block ahead (front waves)
// and -- in some shapes -- the inverse transforms one block behind (tail waves).  Fast variant, every stream the same number of
// blocks; a launch with a clean input (io.near_clean) takes aecm_process_pipelined_clean_kernel, in the shapes PipelinedCleanShapeFor gives.
struct PipeShape {
    int tail_waves;      // 0 or 2 per workgroup
    int front_waves;     // 2 (two streams each) or 4 (one each; with tail waves only)
    bool raw;            // the front waves hand over the transforms' outputs, the back waves form the spectra
    bool balance;        // progress feedback on the front waves' issue priority (needs `progress`)
    int delay_waves;     // 0, 4 or (with gain waves) 2 per workgroup: the delay estimator in waves of its own, one block ahead of the back waves (with tail waves, not raw)
    int gain_waves;      // 0 or 4 per workgroup: the gain half of the back waves' work in waves of its own, one block behind the channel half (with delay waves)
    int wgs_per_round;   // the device's CUs: workgroups i, i + wgs_per_round, ... are taken to share a CU (the dispatcher deals them out in turn) and start their slots on different SIMDs
    int rot;             // slot rotations: front | gain << 2 | delay << 4 | per workgroup of a CU << 6 | tail << 8 (the kernel's slot_of)
    int prio;            // the roles' issue priorities: front | tail << 2 | delay << 4 | gain << 6 (the channel / middle / back waves': by phase, 1..3)
    int workgroups;      // of the launch: ceil(n_streams / 4) .. n_streams; the streams are dealt out evenly (the first n_streams % workgroups serve one more)
};
// What a caller may wish for the shape instead of leaving it to the launch's size (experiments, tests: AecmLaunchPolicy in
// include/aecm_batch.h carries the same fields); < 0 = by size.  A wish is taken where the shape exists and fits.
struct PipeWishes {
    int tail_waves = -1, front_waves = -1, raw = -1, delay_waves = -1, gain_waves = -1;
    int spread = 1;          // != 0: every CU gets the shape's full count of workgroups, of fewer than four streams each where the launch is short of streams
    int wgs_per_cu = 0;      // > 0: workgroups of the shape a CU takes (0: what the shape is built for)
    int rot = -1;            // >= 0: PipeShape::rot
    int prio = -1;           // >= 0: PipeShape::prio
};
// The shape a launch of this size takes on a device of compute_units CUs.
PipeShape PipelinedShapeFor(int n_streams, int n_blocks, int compute_units, const PipeWishes &wishes = PipeWishes());
// The same for a launch with a clean near-end input: by the same sizes, on the shapes the clean kernel is carried in (formed spectra,
// no balance: 6, 8, 12 and 16 waves); a wish for another shape lands on the nearest of them.  The stream limits are those of the
// shapes without a clean input (aecm_block_kernels.hip asserts that the larger hand-over slots leave the workgroups per CU alone).
PipeShape PipelinedCleanShapeFor(int n_streams, int n_blocks, int compute_units, const PipeWishes &wishes = PipeWishes());
int PipelinedStreamLimit(int compute_units, int tail_waves, int front_waves = 2, int delay_waves = 0, int gain_waves = 0, int wgs_per_cu = 0);
// Waves of a workgroup of this shape, and how many such workgroups a CU holds at once (by the wave slots the kernel is built for and the LDS it declares).
int PipelinedWorkgroupWaves(const PipeShape &shape);
int PipelinedWorkgroupsPerCu(const PipeShape &shape);
// progress: PipelinedControlBytes(shape.workgroups) of device memory owned by the engine (cleared by the launch): 16 bits per
// workgroup, by which the workgroups of a balanced launch keep in step.
size_t PipelinedControlBytes(int n_workgroups);
size_t PipelinedTraceOffsetBytes(int n_workgroups);     // diagnostics builds (-DAECM_PIPE_TRACE): where the per-wave records follow the progress words
hipError_t LaunchProcessBlocksPipelined(const StatePtrs &st, const IoView &io, int n_streams, int n_blocks, const PipeShape &shape, uint32_t *progress,
                                        hipStream_t stream);
// The same form for streams of different lengths (aecm_process_pipelined_ragged_kernel: the unbalanced shapes): plan_dev =
// RaggedPipePlanWords(n_workgroups, n_streams) words uploaded ahead of the launch on the same stream -- slot_stream[n_workgroups][4]
// (the stream of each of a workgroup's four slots, -1 = empty), then len[n_streams] (aecm_engine.h: RaggedPipePlan).  A slot whose
// stream has ended keeps the workgroup's barriers and does nothing else; a stream of length 0 has no slot.  With a clean input
// (io.near_clean): aecm_process_pipelined_ragged_clean_kernel, in the shapes PipelinedCleanShapeFor gives; any other shape is
// hipErrorInvalidValue.
size_t RaggedPipePlanWords(int n_workgroups, int n_streams);
hipError_t LaunchProcessBlocksPipelinedRagged(const StatePtrs &st, const IoView &io, int n_streams, const PipeShape &shape, int n_workgroups,
                                              const uint32_t *plan_dev, hipStream_t stream);

// Replicate one stream image (vec: kNumVec*64 words, scal: 64 words, both on the device) into
// streams [first, first + count) and clear their far-spectrum history.
hipError_t LaunchBroadcastImage(const StatePtrs &st, const uint32_t *image_vec, const int32_t *image_scal,
                                int first, int count, hipStream_t stream);

// The same image into the streams s of [0, count) with select_dev[s] != 0 (device array), one launch.
hipError_t LaunchBroadcastImageSelect(const StatePtrs &st, const uint32_t *image_vec, const int32_t *image_scal, const uint8_t *select_dev, int count,
                                      hipStream_t stream);

// Overwrite a few scalar fields (field ids from ScalField) of streams [first, first + count).  The fields travel as a
// kernel argument: no staging copy, nothing for the host to wait for.
constexpr int kMaxPatchFields = 16;
struct ScalarPatch {
    int32_t n;
    int32_t field[kMaxPatchFields], value[kMaxPatchFields];
};
hipError_t LaunchPatchScalars(const StatePtrs &st, const ScalarPatch &patch, int first, int count, hipStream_t stream);

// Bulk state snapshots of streams [first, first + count): blobs_dev = count blobs of kStateBlobBytes (aecm_state_check.h:
// 32-byte header + lane vectors + scalars + far-spectrum history), anything the device can address.  Validate: result_dev[0]
// (preset to 0xffffffff) becomes the index of the first blob the kernels may not run on, result_dev[1] (preset to 0) gets bit 0
// when a blob of another sampling rate than fs_batch is among them; Scatter writes the blobs into the streams unchecked.
hipError_t LaunchGatherStates(const StatePtrs &st, int first, int count, void *blobs_dev, hipStream_t stream);
hipError_t LaunchValidateStates(const void *blobs_dev, int count, int fs_batch, uint32_t *result_dev, hipStream_t stream);
hipError_t LaunchScatterStates(const StatePtrs &st, int first, int count, const void *blobs_dev, hipStream_t stream);

// Session-schedule gather / scatter (aecm_session_flow.h: RecordingSchedule), all streams at once.
//   dst[s][j] = map[j] >= 0 ? src[s*src_stride + map[j]] : 0            j in [0, n)
hipError_t LaunchGatherByMap(const int16_t *src, int64_t src_stride, const int32_t *map_dev, int64_t n, int16_t *dst,
                             int64_t dst_stride, int n_streams, hipStream_t stream);
//   out[s][j] = v >= 0 ? blocks[s][v] : (v == -1 ? 0 : near[s][-(v+2)])  with v = map[j]
//   sample_limit_dev (may be null; S entries): out[s][j] = 0 for j >= sample_limit_dev[s] (the stream's recording ended there)
hipError_t LaunchAssembleOutput(const int16_t *blocks, int64_t blocks_stride, const int16_t *near, int64_t near_stride,
                                const int32_t *map_dev, int64_t n, int16_t *out, int64_t out_stride, int n_streams,
                                hipStream_t stream, const int32_t *sample_limit_dev = nullptr);

// Streaming sessions (aecm_sessions.cpp): per-session sample rings of `ring_len` (power of two) int16 in HBM, indexed by
// wrapping stream positions.
struct TickIo {
    const int16_t *far_in, *near_in, *clean_in;   // [S][io_stride]; clean_in may be null
    int16_t *out;                                 // [S][io_stride]
    int64_t io_stride;
    int32_t n;                                    // samples of this tick (80 or 160)
    int16_t *far_ring, *near_ring, *clean_ring, *out_ring;   // [S][ring_len]
    int64_t ring_len, near_pos;
};

// The device-resident session machinery: the wrapper itself (jitter buffer, start-up gating, delay compensation,
// 80 -> 64 re-blocking, output stuffing) as position arithmetic on per-session state in HBM (aecm_flow_plan.h), so every
// session has its own msInSndCardBuf / call pattern / age and the host does nothing per session.  A tick is two launches:
//   aecm_flow_plan_kernel   one LANE per session: FlowTick on the session's state (field-major, coalesced) -> its plan
//   aecm_tick_flow_kernel   one WAVEFRONT per session: plan into scalar registers, append the tick's samples to the rings,
//                           frame the far end, run the blocks, assemble the output
// Per session in HBM besides TickIo's rings: kFlowFieldsUsed int32 of wrapper state, kFlowPlanWords of plan, a ring of
// kFlowFarFrameRing samples holding the framed far stream, and the two 80-sample replay rows of far-end underruns
// (farendOld, echo_control_mobile.cc:57).
struct TickFlowIo {
    int32_t *state;                    // [kFlowFieldsUsed][S]
    int32_t *plans;                    // [S][kFlowPlanWords]
    int16_t *far_frames;               // [S][kFlowFarFrameRing]
    int16_t *far_old;                  // [S][2 * 80]
    const int16_t *ms_per_session;     // [S] or null: everybody gets `ms`
    const uint8_t *flags_per_session;  // [S] or null: everybody gets `flags` (kFlowNoFarend | kFlowSplitCalls; kFlowIdle per session, sparse launch only)
    int32_t ms, flags, fs;
};
hipError_t LaunchTickFlow(const StatePtrs &st, const TickIo &io, const TickFlowIo &fio, int n_streams, hipStream_t stream);
// A tick in which sessions sit out (fio.flags_per_session carries kFlowIdle for them), or the first ticks after such a one
// (sessions may still lag behind the object's near position: aecm_flow_plan.h, F_NEAR_LAG):
//   aecm_flow_plan_sparse_kernel   one lane per session over ALL sessions: an idle lane counts its lag, a live one brings its
//                                  session back in step and plans; with `live` set it also writes the live sessions' ids,
//                                  ascending, to that list (block_base: FlowLiveBlockBases of the tick's flags)
//   aecm_tick_flow_sparse_kernel   wavefront w serves session live[w]: ceil(live_count / 4) workgroups; none for live_count 0
// live == nullptr: nobody idles in this tick -- the tick launch is the dense aecm_tick_flow_kernel over everybody.
struct TickSparseIo {
    int16_t *near_ring, *clean_ring;   // [S][ring_len]; clean_ring may be null
    int64_t ring_len;
    uint32_t *live;                    // [S] device list the planning kernel fills, or null
    const uint32_t *block_base;        // [ceil(S / kFlowPlanBlock)] live sessions before each planning workgroup (with live)
    int32_t deferred_lag;              // added to every session's lag first: the ticks nobody made (no launch told the sessions)
};
// mixed_plan: the planning launch is aecm_flow_plan_mixed_kernel instead -- the same, with every session at its OWN rate (the
// core state's S_MULT, not fio.fs) and kFlowHalfCall in the flags: one call pair of 80 samples in a 160-sample tick, after which
// the session lags 80 samples (aecm_flow_plan.h: FlowTickMixed).  The tick launch is the same either way.
hipError_t LaunchTickFlowSparse(const StatePtrs &st, const TickIo &io, const TickFlowIo &fio, const TickSparseIo &sp, int n_streams, int live_count,
                                hipStream_t stream, bool mixed_plan = false);
// A tick of `calls` (1 .. kFlowMaxTickCalls) call pairs of io.n samples per session (aecm_tick_calls_kernels.hip): call c uses
// samples [c n, (c + 1) n) of every row (io.io_stride >= calls * io.n).  Two launches whatever `calls` is:
//   aecm_flow_plan_calls_kernel   everything the sparse planning kernel does, then FlowTickCalls: fio.plans is
//                                 [S][calls][kFlowPlanWords] here
//   aecm_tick_calls_kernel        wavefront w serves session live[w]; the core state is loaded once, stays in registers across
//                                 the calls and is stored once
// Always by the live list (sp.live and sp.block_base must be set; everybody live: block_base[b] = b * kFlowPlanBlock).  Every
// session at fio.fs: the caller refuses objects that hold a session of another rate.
hipError_t LaunchTickCalls(const StatePtrs &st, const TickIo &io, const TickFlowIo &fio, const TickSparseIo &sp, int n_streams, int live_count,
                           int calls, hipStream_t stream);
// The planning launch alone (aecm_tick_calls_plan_kernels.hip; LaunchTickCalls calls it).
hipError_t LaunchPlanCalls(const TickIo &io, const TickFlowIo &fio, const TickSparseIo &sp, int n_streams, int calls, hipStream_t stream);
// A packet tick (aecm_tick_packets_kernels.hip; WebRtcAecmSessions_TickPackets): `calls` call pairs per session, every session at
// its own rate (st.scal: S_MULT) and its own call size n_s -- 80 for a session flagged kFlowHalfCall in a tick of io.n == 160, else
// io.n -- on PACKED rows: call c uses samples [c n_s, (c + 1) n_s) of the session's rows (io.io_stride >= calls * io.n).
//   aecm_flow_plan_packets_kernel   what aecm_flow_plan_calls_kernel does, with FlowTickPackets at the lane's rate: fio.plans is
//                                   [S][calls][kFlowPlanWords], every plan carrying its call size in n_frames
//   aecm_tick_packets_kernel        aecm_tick_calls_kernel with the call size and the row step taken from the session's plans
// Always by the live list, as LaunchTickCalls.
hipError_t LaunchTickPackets(const StatePtrs &st, const TickIo &io, const TickFlowIo &fio, const TickSparseIo &sp, int n_streams, int live_count,
                             int calls, hipStream_t stream);
// The planning launch alone (aecm_tick_packets_plan_kernels.hip; LaunchTickPackets calls it).
hipError_t LaunchPlanPackets(const StatePtrs &st, const TickIo &io, const TickFlowIo &fio, const TickSparseIo &sp, int n_streams, int calls,
                             hipStream_t stream);
// A split tick (aecm_tick_split_kernels.hip; AECM_SESSION_NO_CLEAN): the tick carries a clean plane (io.clean_in) and per-session flags,
// clean_count > 0 of the calling sessions take their clean row, plain_count > 0 carry kFlowNoClean and take none.  Always by the live
// lists: sp.live holds FlowSplitListEntries(n_streams) entries -- the ids of the first kind, ascending, at [0, clean_count), those of
// the second at [plain_start, plain_start + plain_count), plain_start = FlowPlainListStart(clean_count) -- sp.block_base and
// split.plain_base the sessions of either kind before each planning workgroup (aecm_flow_clean.h: FlowScanFlagsClean).
//   aecm_flow_plan_split_kernel<mixed_plan>   what aecm_flow_plan_sparse_kernel / aecm_flow_plan_mixed_kernel do, filling both lists
//   aecm_tick_split_kernel                    workgroups [0, plain_start / 4) run the tick body with a clean input on the first list,
//                                             the others the body without on the second
// two_launches: the tick launch as one launch per list instead, by the sparse tick kernel's text (the caller's choice by the size of
// the tick: SessionBatch::SplitTickTwoLaunches).
struct TickSplitIo {
    const uint32_t *plain_base;        // [ceil(S / kFlowPlanBlock)]
    int32_t clean_count, plain_count;
    uint32_t plain_start;
};
hipError_t LaunchTickSplit(const StatePtrs &st, const TickIo &io, const TickFlowIo &fio, const TickSparseIo &sp, const TickSplitIo &split, int n_streams,
                           bool mixed_plan, bool two_launches, hipStream_t stream);
// The planning launch alone (aecm_tick_split_plan_kernels.hip; LaunchTickSplit calls it).
hipError_t LaunchPlanSplit(const StatePtrs &st, const TickIo &io, const TickFlowIo &fio, const TickSparseIo &sp, const TickSplitIo &split, int n_streams,
                           bool mixed_plan, hipStream_t stream);
// A split tick of `calls` call pairs per session (aecm_tick_split_calls_kernels.hip; WebRtcAecmSessions_SetSplitCallTicks): the lists,
// the counts and the clean plane of LaunchTickSplit, the rows and fio.plans ([S][calls][kFlowPlanWords]) of LaunchTickCalls /
// LaunchTickPackets.  Three launches whatever `calls` is:
//   aecm_flow_plan_split_calls_kernel / aecm_flow_plan_split_packets_kernel   the K-call / packet planning lane, filling both lists
//   aecm_tick_split_calls_kernel<true> / aecm_tick_split_packets_kernel<true>     the loop-form tick body with a clean input over the
//                                                                                 first list, ceil(clean_count / 4) workgroups
//   aecm_tick_split_calls_kernel<false> / aecm_tick_split_packets_kernel<false>   the body without over the second list
// Calls: every session at fio.fs and calls of io.n samples; Packets: every session at its own rate and call size, rows packed.
hipError_t LaunchTickSplitCalls(const StatePtrs &st, const TickIo &io, const TickFlowIo &fio, const TickSparseIo &sp, const TickSplitIo &split, int n_streams,
                                int calls, hipStream_t stream);
hipError_t LaunchTickSplitPackets(const StatePtrs &st, const TickIo &io, const TickFlowIo &fio, const TickSparseIo &sp, const TickSplitIo &split, int n_streams,
                                  int calls, hipStream_t stream);
// The planning launches alone (aecm_tick_split_calls_plan_kernels.hip; the two above call them).
hipError_t LaunchPlanSplitCalls(const TickIo &io, const TickFlowIo &fio, const TickSparseIo &sp, const TickSplitIo &split, int n_streams, int calls,
                                hipStream_t stream);
hipError_t LaunchPlanSplitPackets(const StatePtrs &st, const TickIo &io, const TickFlowIo &fio, const TickSparseIo &sp, const TickSplitIo &split,
                                  int n_streams, int calls, hipStream_t stream);
// The planning launch of LaunchTickFlow (sp == nullptr) / LaunchTickFlowSparse alone (aecm_kernels.hip; both call it).
hipError_t LaunchPlanFlow(const StatePtrs &st, const TickIo &io, const TickFlowIo &fio, const TickSparseIo *sp, int n_streams, bool mixed_plan,
                          hipStream_t stream);
// The three tick launches of one call pair per session with a session trace attached (aecm_tick_trace_kernels.hip;
// include/aecm_batch.h: AecmSessionTrace): the planning launches are the ones above, unchanged; the tick launch is the traced twin of
// the untraced one, and every session it serves also writes its 64-byte record to
// tv.records + kSessionTraceWords * (s * tv.session_stride + tv.tick_slot_offset) (aecm_session_trace.h: SessionTraceView; tv.records
// must not be null).  The other arguments and the results are those of the launches above.  (The traced K-call / packet ticks are the
// call trace's, below.)
hipError_t LaunchTickFlowTraced(const StatePtrs &st, const TickIo &io, const TickFlowIo &fio, const SessionTraceView &tv, int n_streams, hipStream_t stream);
hipError_t LaunchTickFlowSparseTraced(const StatePtrs &st, const TickIo &io, const TickFlowIo &fio, const TickSparseIo &sp, const SessionTraceView &tv,
                                      int n_streams, int live_count, hipStream_t stream, bool mixed_plan = false);
hipError_t LaunchTickSplitTraced(const StatePtrs &st, const TickIo &io, const TickFlowIo &fio, const TickSparseIo &sp, const TickSplitIo &split,
                                 const SessionTraceView &tv, int n_streams, bool mixed_plan, bool two_launches, hipStream_t stream);
// The K-call and the packet tick with a call trace attached (aecm_call_trace_plan_kernels.hip, aecm_call_trace_kernels.hip;
// include/aecm_batch.h: WebRtcAecmSessions_SetCallTrace): LaunchTickCalls / LaunchTickPackets by twins of both of their kernels, and
// every session that calls also gets one record per call (aecm_session_trace.h: CallTraceView has the placement; cv.records must
// not be null) --
//   aecm_plan_calls_traced_kernel / aecm_plan_packets_traced_kernel             the planning lane stores words 0..7 of call c's
//                                   record as it plans call c, from its own registers
//   aecm_calls_traced_tick_kernel / aecm_packets_traced_tick_kernel             lanes 0..7 store words 8..15 behind call c's blocks
// The other arguments and the results are those of the untraced launches.
hipError_t LaunchTickCallsTraced(const StatePtrs &st, const TickIo &io, const TickFlowIo &fio, const TickSparseIo &sp, const CallTraceView &cv, int n_streams,
                                 int live_count, int calls, hipStream_t stream);
hipError_t LaunchTickPacketsTraced(const StatePtrs &st, const TickIo &io, const TickFlowIo &fio, const TickSparseIo &sp, const CallTraceView &cv, int n_streams,
                                   int live_count, int calls, hipStream_t stream);
// The planning launches alone (aecm_call_trace_plan_kernels.hip; the two above call them).
hipError_t LaunchPlanCallsTraced(const TickIo &io, const TickFlowIo &fio, const TickSparseIo &sp, const CallTraceView &cv, int n_streams, int calls,
                                 hipStream_t stream);
hipError_t LaunchPlanPacketsTraced(const StatePtrs &st, const TickIo &io, const TickFlowIo &fio, const TickSparseIo &sp, const CallTraceView &cv, int n_streams,
                                   int calls, hipStream_t stream);
int TickWorkgroupWaves();        // sessions per workgroup of the tick kernel
int TickWorkgroupsPerCu();       // workgroups of it a CU holds at once
// Far-end bursts: WebRtcAecm_BufferFarend calls WITHOUT a Process (reference echo_control_mobile.cc:215-234), one wavefront
// per session.  Session s makes clamp(calls_per_session[s] - call_base, 0, max_calls) calls of io.n samples (max_calls each
// when calls_per_session is null) on io.far_in[s][c * io.n .. + io.n): delay compensation when past the start-up phase, then
// what fits into the jitter buffer goes to the far ring.  Of io only far_in / io_stride / n / far_ring / ring_len are used; every
// session at its own rate (st.scal: S_MULT), not fio.fs.
hipError_t LaunchBufferFarend(const StatePtrs &st, const TickIo &io, const TickFlowIo &fio, const uint8_t *calls_per_session, int call_base, int max_calls,
                              int n_streams, hipStream_t stream);
// WebRtcAecm_Init of the wrapper side of sessions [first, first + count): wrapper state as after Init (aecm_flow_plan.h:
// FlowFieldStartsAtOne), far / output rings, framed-far ring and replay rows reading as never written (zero).  Only the
// ring pointers, ring_len and the state / far_frames / far_old pointers of io / fio are used.
hipError_t LaunchResetSessions(const TickIo &io, const TickFlowIo &fio, int n_streams, int first, int count, hipStream_t stream);

// Diagnostics: `count` independent 128-point transforms of the block kernel's fft128, one wavefront
// each, on natural-order data (data[k] = re[128] then im[128] of transform k, in place).  variant:
// 0 forward of real input, 1 forward complex, 2 inverse; scales[k] = the inverse's accumulated scale.
// Outputs nobody consumes in the block path are returned as 0 (forward: im of bins >= 64; inverse: im).
hipError_t LaunchFft128(int16_t *data_dev, int32_t *scales_dev, int variant, int fast, int count, const uint32_t *consts_dev,
                        hipStream_t stream);

// Audit build only (-DAECM_CHECKED): how often a "provably fits" precondition of the block DSP was violated on
// the device since the last reset -- [0] mul24 operands, [1] as_i16 arguments (aecm_ops.h).  Synchronises the
// device.  hipErrorNotSupported in the shipped build, whose kernels carry no checks.
hipError_t ReadCheckCounters(uint64_t counters[2], bool reset);
// The share of aecm_block_kernels.hip (device symbols are per translation unit); ReadCheckCounters adds it in.  Does not synchronise.
hipError_t ReadBlockKernelCheckCounters(uint64_t counters[2], bool reset);
// The share of aecm_trace_kernels.hip (the traced block kernels); ReadCheckCounters adds it in as well.  Does not synchronise.
hipError_t ReadTraceKernelCheckCounters(uint64_t counters[2], bool reset);
// The share of aecm_tick_trace_kernels.hip (the traced tick kernels); ReadCheckCounters adds it in as well.  Does not synchronise.
hipError_t ReadTickTraceCheckCounters(uint64_t counters[2], bool reset);
// The share of aecm_call_trace_kernels.hip (the traced K-call and packet tick kernels); ReadCheckCounters adds it in as well.  Does not synchronise.
hipError_t ReadCallTraceCheckCounters(uint64_t counters[2], bool reset);
// The share of aecm_tick_calls_kernels.hip, for callers that audit K-call ticks (ReadCheckCounters does not add it in).  Does not synchronise.
hipError_t ReadTickCallsCheckCounters(uint64_t counters[2], bool reset);
// The share of aecm_tick_packets_kernels.hip, likewise.
hipError_t ReadTickPacketsCheckCounters(uint64_t counters[2], bool reset);
// The share of aecm_tick_split_kernels.hip, likewise.
hipError_t ReadTickSplitCheckCounters(uint64_t counters[2], bool reset);
// The share of aecm_tick_split_calls_kernels.hip; WebRtcAecmBatch_GetCheckCounters adds it in.  Does not synchronise.
hipError_t ReadTickSplitCallsCheckCounters(uint64_t counters[2], bool reset);

// Device self test of the wave primitives; counters[0..7] are failure counts (all must be 0):
//  0 shfl_xor, 1 exchange, 2 reduce_max/min/add, 3 shift_up1, 4 bpermute/readlane/writelane, 5 ballot,
//  6 isqrt31 (exhaustive over [0, 2^31) when exhaustive != 0, else 2^24 samples), 7 table upload.
hipError_t LaunchSelfTest(uint64_t *counters_dev, int exhaustive, const uint32_t *consts_dev, hipStream_t stream);

// Diagnostics, the ops probe (aecm_ops_probe_kernels.hip): entry `op` of aecm_ops_table.inc -- one primitive of aecm_ops.h or
// plain-integer helper of aecm_wave.h -- on n operand tuples (a_dev, b_dev, c_dev: n words each; those above the op's arity may
// be null).  form 0: thread i evaluates tuple i, out_dev[n]; form 1: wave w evaluates tuple w with wave-uniform operands,
// out_dev[2 n] = the results, then per tuple 0 or kOpsProbeNonUniform (a lane disagreed with lane 0).
// hipErrorInvalidValue, and no launch, for an op or form there is none of, n <= 0 or n > kOpsProbeMaxTuples.
constexpr int kOpsProbeMaxTuples = 1 << 20;
constexpr int kOpsProbeNonUniform = 0x5E471E1;
hipError_t LaunchOpsProbe(int op, int form, const int *a_dev, const int *b_dev, const int *c_dev, int *out_dev, int n, hipStream_t stream);
int OpsProbeCount();
const char *OpsProbeName(int op);      // null outside [0, OpsProbeCount())
int OpsProbeArity(int op);             // 1..3; 0 outside the table
// The share of aecm_ops_probe_kernels.hip in the audit counters; WebRtcAecmBatch_GetCheckCounters adds it in.  Does not synchronise.
hipError_t ReadOpsProbeCheckCounters(uint64_t counters[2], bool reset);

}  // namespace aecm
#endif  // AECM_AMD_KERNELS_H_
