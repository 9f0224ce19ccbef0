/*
 * Batch extension of the AECM C ABI: S independent AECM block streams resident on one MI355X,
 * one wavefront per stream.  Not present in the reference; it is the data-parallel form of the
 * reference's block-level core interface (aecm/aecm_core.h:149-239):
 *
 *   WebRtcAecmBatch_Create/Free      <->  WebRtcAecm_CreateCore / FreeCore   (aecm_core.h:149,198)
 *   WebRtcAecmBatch_Init             <->  WebRtcAecm_InitCore                (aecm_core.h:166)
 *                                         + default set_config (echo_control_mobile.cc:183-188)
 *   WebRtcAecmBatch_set_config       <->  core part of WebRtcAecm_set_config (echo_control_mobile.cc:410-479)
 *   WebRtcAecmBatch_Control          <->  WebRtcAecm_Control                 (aecm_core.h:200)
 *   WebRtcAecmBatch_ProcessBlocks    <->  T x WebRtcAecm_ProcessBlock per stream (aecm_core.h:235)
 *   WebRtcAecmBatch_InitEchoPath / GetEchoPath <-> WebRtcAecm_InitEchoPathCore (aecm_core.h:187) /
 *                                         WebRtcAecm_GetEchoPath (echo_control_mobile.h:191)
 *
 * Return codes follow echo_control_mobile.h: 0 ok, -1 NULL handle, 12002 not initialised,
 * 12003 NULL data pointer, 12004 bad parameter, 12000 device (HIP) failure.
 *
 * Audio layout: sample i of block b of stream s is at base[s*stream_stride + b*block_stride + i]
 * (strides in int16 elements).  Stream-major "files" are (stream_stride, block_stride) = (T*64, 64);
 * a tick-major server layout [T][S][64] is (64, S*64).  Each wavefront reads/writes whole 128-byte
 * lines either way.
 */
#ifndef AECM_MI355X_BATCH_H_
#define AECM_MI355X_BATCH_H_

#include <stddef.h>
#include <stdint.h>

#include "echo_control_mobile.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct AecmBatch AecmBatch;

enum { AECM_BATCH_DIGEST_WORDS = 24 };
enum { AECM_KERNEL_SAFE = 0, AECM_KERNEL_FAST = 1 };

/* Allocates device state for num_streams streams on HIP device device_id.  NULL on failure. */
AecmBatch *WebRtcAecmBatch_Create(int32_t num_streams, int32_t device_id);
void WebRtcAecmBatch_Free(AecmBatch *b);

int32_t WebRtcAecmBatch_num_streams(const AecmBatch *b);

/* (Re)initialises every stream for sampFreq in {8000, 16000}, default config cng=1, echoMode=3. */
int32_t WebRtcAecmBatch_Init(AecmBatch *b, int32_t sampFreq);
/* Applies config to streams [first, first+count); count < 0 means "to the end". */
int32_t WebRtcAecmBatch_set_config(AecmBatch *b, AecmConfig config, int32_t first, int32_t count);
/* WebRtcAecm_Control (aecm_core.cc:477-482) for streams [first, first+count).  Deviation from the reference, on purpose:
 * the reference stores both arguments unchecked (narrowed to int16_t) and later uses fixedDelay as an offset into the
 * 100-slot far history (aecm_core.cc:157-172).  Here values the core could not hold or index with are refused with
 * AECM_BAD_PARAMETER_ERROR instead of being narrowed silently: fixed_delay must lie in [-32768, 100) (negative = "use
 * the delay estimator", as in the reference), nlp_flag in [-32768, 32767]. */
int32_t WebRtcAecmBatch_Control(AecmBatch *b, int32_t fixed_delay, int32_t nlp_flag, int32_t first, int32_t count);

/* Runs num_blocks consecutive 64-sample blocks of every stream.  All four pointers are DEVICE
 * pointers (near_clean may be NULL).  Asynchronous on the engine's HIP stream. */
int32_t WebRtcAecmBatch_ProcessBlocks(AecmBatch *b, const int16_t *far_dev, const int16_t *near_dev,
                                      const int16_t *near_clean_dev, int16_t *out_dev, int64_t stream_stride,
                                      int64_t block_stride, int32_t num_blocks);
/* Same with HOST pointers: copies in, runs, copies out, synchronises. */
int32_t WebRtcAecmBatch_ProcessBlocksHost(AecmBatch *b, const int16_t *far_host, const int16_t *near_host,
                                          const int16_t *near_clean_host, int16_t *out_host, int64_t stream_stride,
                                          int64_t block_stride, int32_t num_blocks);
/* Whole recordings as sessions (batched form of the reference CLI's loop, main.cc:105-143): every
 * stream is treated as a freshly initialised WebRtcAecm_* session that receives num_calls pairs of
 * WebRtcAecm_BufferFarend(far, samples_per_call) + WebRtcAecm_Process(near, near_clean, out,
 * samples_per_call, msInSndCardBuf) (near_clean may be NULL, reference echo_control_mobile.h:135-140).  The session wrapper and frame adapter of the reference
 * (echo_control_mobile.cc:236-408, aecm_core.cc:501-572) only move samples, so they are run once on
 * the host in the index domain and applied to all streams as a device-side gather / scatter around
 * WebRtcAecmBatch_ProcessBlocks.  Call after WebRtcAecmBatch_Init (+ set_config) on fresh streams.
 * far/near/near_clean/out: [S][stream_stride] with stream_stride >= num_calls * samples_per_call; samples beyond
 * that are not touched.  Returns 0 or AECM_BAD_PARAMETER_WARNING exactly as each session would.
 * Synchronous. */
int32_t WebRtcAecmBatch_ProcessRecordings(AecmBatch *b, const int16_t *far_dev, const int16_t *near_dev,
                                          const int16_t *near_clean_dev, int16_t *out_dev, int64_t stream_stride,
                                          int32_t samples_per_call, int32_t num_calls, int16_t msInSndCardBuf);
int32_t WebRtcAecmBatch_ProcessRecordingsHost(AecmBatch *b, const int16_t *far_host, const int16_t *near_host,
                                              const int16_t *near_clean_host, int16_t *out_host, int64_t stream_stride,
                                              int32_t samples_per_call, int32_t num_calls, int16_t msInSndCardBuf);
/* Ragged batches: a corpus of recordings never has one length.
 * As WebRtcAecmBatch_ProcessBlocks, but stream s runs its first blocks_per_stream_host[s] blocks only (host array, S entries
 * in [0, num_blocks], read before the call returns; AECM_BAD_PARAMETER_ERROR and nothing changed otherwise).  Its state
 * afterwards is the state after exactly that many WebRtcAecm_ProcessBlock calls; its out blocks beyond that are not written,
 * a stream of length 0 is not touched at all.  The device's work is proportional to the SUM of the lengths: large launches are
 * cut into (chunk, stream) items over the streams still live in each chunk (the chunk queue, below).  Every length equal to
 * num_blocks is exactly WebRtcAecmBatch_ProcessBlocks.  Asynchronous like it.  The Host form is a convenience for tests and small
 * batches: it stages S x num_blocks dense rows through pageable copies (a short stream's unused blocks as zeros), runs, copies only
 * the blocks that were written back into out_host and synchronises; a corpus is fed through device pointers or a registered host buffer. */
int32_t WebRtcAecmBatch_ProcessBlocksRagged(AecmBatch *b, const int16_t *far_dev, const int16_t *near_dev, const int16_t *near_clean_dev,
                                            int16_t *out_dev, int64_t stream_stride, int64_t block_stride, int32_t num_blocks,
                                            const int32_t *blocks_per_stream_host);
int32_t WebRtcAecmBatch_ProcessBlocksRaggedHost(AecmBatch *b, const int16_t *far_host, const int16_t *near_host, const int16_t *near_clean_host,
                                                int16_t *out_host, int64_t stream_stride, int64_t block_stride, int32_t num_blocks,
                                                const int32_t *blocks_per_stream_host);
/* As WebRtcAecmBatch_ProcessRecordings(Host): session s makes calls_per_stream_host[s] <= num_calls call pairs (host array, S entries
 * in [0, num_calls]).  codes_host (S entries, may be NULL): what each session's calls returned (the first non-zero code; 0 for a
 * session without calls); the function returns 0 or the first non-zero of them.  out rows are 0 from calls * samples_per_call to
 * num_calls * samples_per_call; a session's state afterwards is the state after its own last call.  A session one of whose calls
 * returns an error (not the AECM_BAD_PARAMETER_WARNING of an out-of-range msInSndCardBuf) is not run: its row is all zeros, its state
 * untouched, its code reported; the other sessions run. */
int32_t WebRtcAecmBatch_ProcessRecordingsRagged(AecmBatch *b, const int16_t *far_dev, const int16_t *near_dev, const int16_t *near_clean_dev,
                                                int16_t *out_dev, int64_t stream_stride, int32_t samples_per_call, int32_t num_calls,
                                                const int32_t *calls_per_stream_host, int16_t msInSndCardBuf, int32_t *codes_host);
int32_t WebRtcAecmBatch_ProcessRecordingsRaggedHost(AecmBatch *b, const int16_t *far_host, const int16_t *near_host, const int16_t *near_clean_host,
                                                    int16_t *out_host, int64_t stream_stride, int32_t samples_per_call, int32_t num_calls,
                                                    const int32_t *calls_per_stream_host, int16_t msInSndCardBuf, int32_t *codes_host);
int32_t WebRtcAecmBatch_Synchronize(AecmBatch *b);

/* Duration of the most recent timed ProcessBlocks kernel, from HIP events recorded around the launch on
 * the engine's own stream (waits for it to finish).
 * Timed: every launch made by WebRtcAecmBatch_ProcessBlocks and by the staged form of ProcessBlocksHost /
 * ProcessRecordings*.  NOT timed (latency paths that would pay for the event pair): host calls of at most 64 KiB of
 * audio, which run the kernel directly on a pinned mapped buffer (the whole single-session WebRtcAecm_* ABI; switch
 * off with AECM_HOST_MAPPED=0), and the session ticks (WebRtcAecmSessions_Tick*).  For those, GetTimers / GetLastLaunchMs
 * keep reporting the last timed launch. */
int32_t WebRtcAecmBatch_GetLastLaunchMs(AecmBatch *b, float *ms);
/* Sum of the timed kernel durations (see above) since the last call to WebRtcAecmBatch_ResetTimers and their count. */
int32_t WebRtcAecmBatch_GetTimers(AecmBatch *b, double *total_ms, int64_t *launches);
int32_t WebRtcAecmBatch_ResetTimers(AecmBatch *b);

/* Per-stream stored echo channel (65 x int16 = 130 bytes), as echo_control_mobile.h:172,191. */
int32_t WebRtcAecmBatch_InitEchoPath(AecmBatch *b, int32_t stream, const void *echo_path, size_t size_bytes);
int32_t WebRtcAecmBatch_GetEchoPath(AecmBatch *b, int32_t stream, void *echo_path, size_t size_bytes);

/* Full snapshot of one stream's device state (checkpoint / migration between batches or GPUs): a 32-byte
 * header (magic, layout version, sampling rate, layout sizes) + lane-vector words, scalars and far-spectrum
 * history, WebRtcAecmBatch_state_size_bytes() bytes.  A stream restored with ImportState continues bit-exactly
 * where the exported one stopped.  ImportState refuses (AECM_BAD_PARAMETER_ERROR) a blob whose header is not
 * this build's layout or whose index-like fields are out of range.  Importing a stream of the other sampling
 * rate is allowed (the rate is part of the state) but disables WebRtcAecmBatch_ProcessRecordings
 * (AECM_UNSUPPORTED_FUNCTION_ERROR) until the next WebRtcAecmBatch_Init. */
size_t WebRtcAecmBatch_state_size_bytes(void);
int32_t WebRtcAecmBatch_ExportState(AecmBatch *b, int32_t stream, void *state, size_t size_bytes);
int32_t WebRtcAecmBatch_ImportState(AecmBatch *b, int32_t stream, const void *state, size_t size_bytes);

/* The same for streams [first, first + count) at once: `states` = count snapshots of WebRtcAecmBatch_state_size_bytes()
 * each, back to back (size_bytes = count x that).  One gather (scatter) launch on the device and one copy per 8 192 streams
 * instead of three blocking copies per stream.  The *Device forms take anything the device can address: device memory
 * (e.g. the staging buffer of a peer-to-peer migration), or the alias of a caller-owned host buffer registered with
 * WebRtcAecmBatch_RegisterHostBuffer -- the kernels then write (read) the snapshots in place over the link.
 * ImportStates is all or nothing: every snapshot is validated exactly like ImportState validates one (on the device for
 * the *Device form) before any stream is touched; AECM_BAD_PARAMETER_ERROR if one of them may not be run on. */
int32_t WebRtcAecmBatch_ExportStates(AecmBatch *b, int32_t first, int32_t count, void *states_host, size_t size_bytes);
int32_t WebRtcAecmBatch_ImportStates(AecmBatch *b, int32_t first, int32_t count, const void *states_host, size_t size_bytes);
/* (The *Device forms: states_dev must be 4-byte aligned -- AECM_BAD_PARAMETER_ERROR otherwise -- and, for ImportStatesDevice, must not
 * change while the call runs: the blobs are validated by one launch and written into the streams by a second one.) */
int32_t WebRtcAecmBatch_ExportStatesDevice(AecmBatch *b, int32_t first, int32_t count, void *states_dev, size_t size_bytes);
int32_t WebRtcAecmBatch_ImportStatesDevice(AecmBatch *b, int32_t first, int32_t count, const void *states_dev, size_t size_bytes);

/* 24-word digest of one stream's complete state (canonical order: oracle/aecm_oracle.c). */
int32_t WebRtcAecmBatch_GetDigest(AecmBatch *b, int32_t stream, uint32_t digest[AECM_BATCH_DIGEST_WORDS]);

/* ---- Block trace: what every block decided ------------------------------------------------------------
 * Opt-in.  While a trace buffer is attached to a batch, every block that a device-pointer block launch processes
 * (WebRtcAecmBatch_ProcessBlocks, WebRtcAecmBatch_ProcessBlocksRagged; with and without near_clean_dev) also writes one 32-byte
 * record: the estimated echo delay, the far-end activity, the suppression gain ... of that stream directly after that block -- every
 * field the value WebRtcAecmBatch_ExportState / GetDigest would show there, i.e. the named member of the reference's state after its
 * WebRtcAecm_ProcessBlock for that block.  Little endian; the digest word each field is read from in brackets.
 * Audio, state and digests are identical with and without a trace; with none attached nothing changes at all. */
typedef struct AecmBlockTrace {
    uint32_t tot_count;             /*  0  AecmCore::totCount                        [0]        */
    int16_t delay;                  /*  4  BinaryDelayEstimator::last_delay; -2: none yet  [13] */
    int16_t startup_state;          /*  6  startupState                              [2, low]   */
    int16_t vad;                    /*  8  currentVADValue                           [7, low]   */
    int16_t vad_update_count;       /* 10  vadUpdateCount                            [7, high]  */
    int16_t far_log_energy;         /* 12  farLogEnergy                              [4, low]   */
    int16_t far_energy_min;         /* 14  farEnergyMin                              [4, high]  */
    int16_t far_energy_max;         /* 16  farEnergyMax                              [5, low]   */
    int16_t far_energy_vad;         /* 18  farEnergyVAD                              [6, low]   */
    int16_t sup_gain;               /* 20  supGain                                   [12, low]  */
    int16_t near_q;                 /* 22  dfaNoisyQDomain                           [3, low]   */
    int32_t delay_min_probability;  /* 24  BinaryDelayEstimator::minimum_probability [14]       */
    int32_t delay_last_probability; /* 28  BinaryDelayEstimator::last_delay_probability [15]    */
} AecmBlockTrace;
size_t WebRtcAecmBatch_block_trace_size_bytes(void);      /* 32 */
/* Attaches trace_dev (device memory; NULL detaches).  Strides are in records: block k of a launch, for the stream at position s of
 * that launch, is written at trace_dev + 32 * (s * stream_stride + k * block_stride).  k counts from 0 in every launch -- the
 * convention of the audio's strides, so a stream-major buffer [S][T] is (T, 1) and a tick-major one [T][S] is (1, S).  A ragged stream
 * of length L writes exactly its records 0 .. L - 1, one of length 0 none; everything else in the buffer is untouched.  The caller owns
 * the buffer and its size, as for out_dev.
 * Returns 0, or AECM_BAD_PARAMETER_ERROR with nothing changed for a NULL batch, a pointer that is not 4-byte aligned, or a stride <= 0.
 * While a trace is attached:
 *  - the host-pointer forms -- WebRtcAecmBatch_ProcessBlocksHost, WebRtcAecmBatch_ProcessBlocksRaggedHost -- and the whole
 *    WebRtcAecmBatch_ProcessRecordings* family (whose call-to-block map is not block-aligned) return
 *    AECM_UNSUPPORTED_FUNCTION_ERROR with nothing run and nothing changed;
 *  - a launch never takes the pipelined form (the traced values live in four different role waves there): a size that would be
 *    pipelined -- by default 2 .. 4 096 streams -- runs one wavefront per stream; the chunk queue and the one-wave forms are chosen
 *    as always.  Results do not depend on the launch form.  WebRtcAecmBatch_DescribeLaunch answers for the traced launch. */
int32_t WebRtcAecmBatch_SetBlockTrace(AecmBatch *b, void *trace_dev, int64_t stream_stride, int64_t block_stride);

/* ---- Streaming batch of sessions --------------------------------------------------------------------
 * S independent WebRtcAecm_* sessions that share one call pattern (a media server's 10 ms clock):
 * every WebRtcAecmSessions_Tick is, for each stream s,
 *     WebRtcAecm_BufferFarend(inst_s, far[s], nrOfSamples);
 *     WebRtcAecm_Process(inst_s, near[s], near_clean ? near_clean[s] : NULL, out[s], nrOfSamples, msInSndCardBuf);
 * (reference echo_control_mobile.h:87,135) with identical results and return code.  Audio is held in
 * per-stream rings in HBM; the reference's jitter buffer / start-up gating / delay compensation /
 * 80->64 re-blocking run on the device, per session, as position arithmetic on per-session state
 * (csrc/aecm_flow_plan.h), so sessions need not have anything in common but the tick.
 * far/near/near_clean/out: [S][stream_stride] int16, device pointers (Tick) or host pointers (TickHost);
 * near_clean may be NULL, but a batch must either always or never pass it (the clean ring is only kept
 * up to date by ticks that carry it). */
typedef struct AecmSessions AecmSessions;
AecmSessions *WebRtcAecmSessions_Create(int32_t num_streams, int32_t device_id);
void WebRtcAecmSessions_Free(AecmSessions *s);
int32_t WebRtcAecmSessions_Init(AecmSessions *s, int32_t sampFreq);
int32_t WebRtcAecmSessions_set_config(AecmSessions *s, AecmConfig config);
int32_t WebRtcAecmSessions_Tick(AecmSessions *s, const int16_t *far_dev, const int16_t *near_dev,
                                const int16_t *near_clean_dev, int16_t *out_dev, int64_t stream_stride, size_t nrOfSamples,
                                int16_t msInSndCardBuf);
int32_t WebRtcAecmSessions_TickHost(AecmSessions *s, const int16_t *far_host, const int16_t *near_host,
                                    const int16_t *near_clean_host, int16_t *out_host, int64_t stream_stride,
                                    size_t nrOfSamples, int16_t msInSndCardBuf);

/* The same with one msInSndCardBuf per session (host array, S entries): session s runs
 *     WebRtcAecm_Process(inst_s, ..., msInSndCardBuf_host[s]).
 * codes_host (S entries, may be NULL) receives each session's return code; the function returns 0 or the
 * first non-zero code.  Any number of distinct msInSndCardBuf histories per object; Tick and TickPerSession may
 * be mixed. */
int32_t WebRtcAecmSessions_TickPerSession(AecmSessions *s, const int16_t *far_dev, const int16_t *near_dev,
                                          const int16_t *near_clean_dev, int16_t *out_dev, int64_t stream_stride,
                                          size_t nrOfSamples, const int16_t *msInSndCardBuf_host, int32_t *codes_host);
int32_t WebRtcAecmSessions_TickPerSessionHost(AecmSessions *s, const int16_t *far_host, const int16_t *near_host,
                                              const int16_t *near_clean_host, int16_t *out_host, int64_t stream_stride,
                                              size_t nrOfSamples, const int16_t *msInSndCardBuf_host, int32_t *codes_host);
/* The same with per-session call flags (host array, S entries): AECM_SESSION_NO_FAREND = this session gets NO
 * WebRtcAecm_BufferFarend call in this tick (far-end underrun; its WebRtcAecm_Process then replays the previous
 * far frame, reference echo_control_mobile.cc:369-380) -- its far row is ignored. */
enum {
    AECM_SESSION_NO_FAREND = 1,
    /* 160-sample ticks only: this session makes TWO WebRtcAecm_BufferFarend + WebRtcAecm_Process call pairs of 80 samples
     * in this tick (first half, then second half of its rows) instead of one pair of 160 samples -- sessions with
     * different call sizes in one object (the reference treats the two cadences differently,
     * echo_control_mobile.cc:282-283, 384-385).  codes_host then receives the first non-zero code of the two calls. */
    AECM_SESSION_SPLIT_CALLS = 2,
    /* This session makes NEITHER call in this tick: its reference instance receives no WebRtcAecm_BufferFarend and no
     * WebRtcAecm_Process in the interval (the call has ended, the slot was never used, the near-end packet is late, the call
     * is on hold).  Nothing of its state changes, what it has pending stays pending, and when it calls again it continues bit
     * for bit -- however long the stretch.  The other bits of its flag byte are ignored; its far, near, near_clean,
     * msInSndCardBuf_host and out entries are not read; codes_host[s] is 0 and takes no part in the "first non-zero code".
     * The device-pointer forms (TickFlags, TickAsync) never write an idle session's out row; TickFlagsHost, which stages
     * whole planes, copies every session's input rows to the device (the kernels read the live ones only; no rows at all in a
     * tick nobody makes) and delivers an idle session's out row as zeros.  The tick's device work is by the
     * sessions that call: a planning launch over all sessions, and a tick launch of ceil(live / 4) workgroups
     * (WebRtcAecmSessions_DescribeTickLive).  A tick in which every session is idle launches nothing and returns 0 (the
     * arguments are checked as always, the object's position advances, done_hip_event is recorded behind wait_hip_event).
     * far may be NULL when every session is idle or carries AECM_SESSION_NO_FAREND.
     * A tick whose flags name nobody idle gives what the tick without a flags array gives, and in an object whose sessions
     * are all in step -- nobody has sat out a tick since the last tick everybody made -- it is that tick: the same launches,
     * the same kernels.  The first tick everybody makes after idle ticks still takes the planning launch that brings sessions
     * back in step (then the dense tick kernel); from the next one on the object is as if nobody had ever idled. */
    AECM_SESSION_IDLE = 4
};
enum {
    /* 160-sample ticks only: this session makes ONE WebRtcAecm_BufferFarend + WebRtcAecm_Process call pair of 80 samples in this
     * tick, on the first half of its rows (10 ms of an 8 kHz call next to 10 ms of 16 kHz calls).  The second half of its far /
     * near / near_clean rows never influences anything; out[s][80..160) is not written by the device-pointer forms and comes back
     * as zeros from TickFlagsHost.  With a tick of 80 samples, or together with AECM_SESSION_SPLIT_CALLS:
     * AECM_BAD_PARAMETER_ERROR, nothing changed.  Ignored in an idle session's byte like every other bit.
     * A tick in which a session makes a half call, and every tick of an object that holds a session of another rate than its
     * own (below: WebRtcAecmSessions_InitRates), takes the planning launch that knows per-session rates and call sizes; the tick
     * launch is the one it would be anyway.  An object whose sessions all run at its own rate and make no half calls takes
     * exactly the launches it takes without this flag. */
    AECM_SESSION_HALF_CALL = 8
};
enum {
    /* A clean near-end input PER SESSION -- one object per clock, not per kind of call: behind one 10 ms clock some calls sit behind a
     * noise suppressor and some do not.  On a tick that passes near_clean, this session's WebRtcAecm_Process is called with
     * nearendClean = NULL: its near_clean row is not read (it may hold anything), its clean ring is neither written nor read, and
     * the output of its start-up phase is the copy of its noisy near end (echo_control_mobile.cc:285-291).  Every other session of
     * the tick gets its near_clean row, as without the flag.  Outputs, codes, echo paths and the complete session state are bit for
     * bit those of one reference instance per session, each called with or without the clean pointer as flagged.
     * Accepted by TickFlags, TickFlagsHost and TickAsync, and by TickCalls* / TickPackets* with calls == 1, which are those ticks;
     * it combines with every other flag, with per-session msInSndCardBuf and with sessions of the other rate.
     *   - A session is of ONE kind for its life between two initialisations: "always" or "never".  (A reference instance whose clean
     *     pointer comes and goes hands out stale contents of its clean frame buffer; that is not reproduced, and not attempted.)  The
     *     object keeps per session what its Process calls carried so far -- WebRtcAecmSessions_GetSessionCleanMode -- reset by Init,
     *     InitRates, InitSession, InitSessionRate and ImportSession*: an imported session starts at "no call yet", the caller
     *     continues it as it was exported.
     *   - A tick in which some calling session carries the flag is accepted only if every calling session either has made no Process
     *     call since its last initialisation or gets what all its calls got.  Otherwise: AECM_BAD_PARAMETER_ERROR, nothing changed --
     *     not the sessions, not the object's position.  The check follows the other argument checks, in their order.
     *   - Once an object has accepted such a tick since its last Init, every later Tick* and WebRtcAecmSessions_Process* is checked
     *     the same way (a tick without flags, or without the flag, gives every calling session the clean input it passes, or none):
     *     an unflagged tick cannot silently hand a "never" session a clean input.  An object that never uses the flag is never
     *     refused for this reason and behaves as it always has.
     *   - Idle sessions: ignored in an idle session's byte like every other bit; an idle session is exempt from the check.
     *   - near_clean == NULL: the flag is ignored, the tick is the tick without it.
     *   - No calling session carries the flag: exactly the tick without it, the same launches, the same kernels.
     *   - Every calling session carries it: the launches of the tick without a clean input; near_clean is not touched.
     *   - Otherwise the tick always goes by the live lists (as with idle sessions): one planning launch that writes the list of the
     *     sessions with a clean input and, from the next multiple of four entries on, the list of those without; then, up to four
     *     times the sessions the device holds at once (28 672 on an MI355X), one tick launch whose first ceil(with / 4) workgroups
     *     serve the first list and the others the second, and for larger ticks one tick launch per list
     *     (WebRtcAecmSessions_SplitCleanTwoLaunches).
     *   - TickFlagsHost stages the whole near_clean plane as always; the flagged sessions' rows are never read by a kernel.
     *   - calls > 1 (TickCalls*, TickPackets*) with a calling session that carries the flag and near_clean != NULL:
     *     AECM_UNSUPPORTED_FUNCTION_ERROR, nothing changed -- unless the object's switch WebRtcAecmSessions_SetSplitCallTicks is on
     *     (below; off in a new object).  With it, the tick is the loop written at TickCalls / TickPackets with the flagged sessions' K
     *     Process calls getting nearendClean = NULL: none of the K pieces of a flagged session's near_clean row is read, everything
     *     said above holds for all K calls, and the history rule is applied once per tick (a tick gives a session the same kind for
     *     all of its calls).  While a call trace is attached (WebRtcAecmSessions_SetCallTrace), K-call ticks of mixed kinds are
     *     not supported yet: AECM_UNSUPPORTED_FUNCTION_ERROR whatever the switch says.
     *   - Snapshots: layout, version and the export code are unchanged.  The clean tail of a "never" session's snapshot is whatever
     *     its never-read ring row holds; it influences nothing. */
    AECM_SESSION_NO_CLEAN = 16
};
int32_t WebRtcAecmSessions_TickFlags(AecmSessions *s, const int16_t *far_dev, const int16_t *near_dev,
                                     const int16_t *near_clean_dev, int16_t *out_dev, int64_t stream_stride, size_t nrOfSamples,
                                     const int16_t *msInSndCardBuf_host, const uint8_t *flags_host, int32_t *codes_host);
int32_t WebRtcAecmSessions_TickFlagsHost(AecmSessions *s, const int16_t *far_host, const int16_t *near_host,
                                         const int16_t *near_clean_host, int16_t *out_host, int64_t stream_stride,
                                         size_t nrOfSamples, const int16_t *msInSndCardBuf_host, const uint8_t *flags_host,
                                         int32_t *codes_host);

/* The asynchronous form: the tick's two launches are enqueued on the object's own HIP stream and the call returns
 * without waiting for them, so a caller that keeps its audio on the device can issue tick t + 1 (and its own producer /
 * consumer kernels) while tick t runs.  Device pointers only (or device aliases of registered host buffers, below).
 *   msInSndCardBuf_host == NULL : every session gets msInSndCardBuf; else S entries, read before the call returns
 *   flags_host                  : NULL or S entries (needs msInSndCardBuf_host), read before the call returns
 *   codes_host                  : NULL or S entries, written before the call returns (the codes do not depend on the device)
 *   wait_hip_event (hipEvent_t) : NULL, or an event the tick's kernels wait for (the caller's producer of far / near)
 *   done_hip_event (hipEvent_t) : NULL, or an event recorded behind the tick (the caller's consumer of out waits for it)
 * The far / near / out buffers must stay untouched until the tick has run (done_hip_event or WebRtcAecmSessions_Synchronize).
 * Every other WebRtcAecmSessions_* call is ordered behind the ticks enqueued so far; the synchronous Tick forms
 * wait for everything. */
int32_t WebRtcAecmSessions_TickAsync(AecmSessions *s, const int16_t *far_dev, const int16_t *near_dev, const int16_t *near_clean_dev,
                                     int16_t *out_dev, int64_t stream_stride, size_t nrOfSamples, int16_t msInSndCardBuf,
                                     const int16_t *msInSndCardBuf_host, const uint8_t *flags_host, int32_t *codes_host,
                                     void *wait_hip_event, void *done_hip_event);
/* Several call pairs per tick: the 20 ms packet of Opus or G.711 (and the 40 and 60 ms ones) on 10 ms calls.  A tick of
 * `calls` = K call pairs of nrOfSamples = n samples is, for every session s that calls, exactly
 *     for (c = 0; c < K; ++c) {
 *         WebRtcAecm_BufferFarend(inst_s, far[s] + c * n, n);                                   (unless AECM_SESSION_NO_FAREND)
 *         WebRtcAecm_Process(inst_s, near[s] + c * n, clean ? clean[s] + c * n : NULL, out[s] + c * n, n, ms_s);
 *     }
 * -- bit for bit K ordinary ticks on the same rows (outputs, codes, echo path, the complete session state), and interchangeable
 * with them at any point of a session's life; NOT WebRtcAecmSessions_BufferFarend(calls) followed by Process, which is far, far,
 * near.  K ordinary ticks cost K planning launches, K tick launches and K round trips of the core state; this is one planning
 * launch and one tick launch that keeps a session's core state in registers across its K call pairs.
 *   rows                        : [S][stream_stride] with stream_stride >= calls * nrOfSamples; call c uses samples [c n, (c + 1) n)
 *   calls                       : 1 .. AECM_SESSION_MAX_TICK_CALLS.  calls == 1 is TickAsync / TickFlags with the same arguments:
 *                                 the same launches, the same kernels
 *   msInSndCardBuf(_host)       : as in TickAsync -- one value per session, used for all K calls
 *   codes_host[s]               : the first non-zero code of the session's calls (0 for an idle session); the function returns 0 or
 *                                 the first non-zero code
 *   AECM_SESSION_IDLE           : the session makes none of the K pairs and falls calls * n samples behind the object; its out row
 *                                 is not written by the device forms and comes back as zeros from the Host form; everything said
 *                                 of idle sessions above stays true
 *   AECM_SESSION_NO_FAREND      : none of the session's K pairs has a WebRtcAecm_BufferFarend
 *   AECM_SESSION_SPLIT_CALLS, AECM_SESSION_HALF_CALL on a session that calls, with calls > 1: AECM_BAD_PARAMETER_ERROR
 * With calls > 1, an object that holds a session of another rate than its own (WebRtcAecmSessions_InitRates and friends) is
 * refused with AECM_UNSUPPORTED_FUNCTION_ERROR: such a session gets its 10 ms through half calls, and K half calls per row is a
 * layout of its own: WebRtcAecmSessions_TickPackets, below.  So is the safe kernel variant, as for every tick.  The arguments are checked in the
 * reference's order (NULL, uninitialised, sizes -- calls out of range and a short stride are AECM_BAD_PARAMETER_ERROR --, then a
 * poisoned object); a refused call changes nothing, neither the sessions nor the object's position.  K-call ticks, ordinary
 * ticks, bursts, Process, InitSession*, set_config_session, Export / ImportSession(s) and ticks of another K mix freely.
 * TickCalls waits for the tick, TickCallsHost stages host audio like TickFlagsHost (its staging grows to calls * n samples per
 * row, once), TickCallsAsync is TickAsync's form. */
enum { AECM_SESSION_MAX_TICK_CALLS = 6 };      /* 60 ms of 10 ms calls */
int32_t WebRtcAecmSessions_TickCalls(AecmSessions *s, const int16_t *far_dev, const int16_t *near_dev, const int16_t *near_clean_dev,
                                     int16_t *out_dev, int64_t stream_stride, size_t nrOfSamples, int32_t calls, int16_t msInSndCardBuf,
                                     const int16_t *msInSndCardBuf_host, const uint8_t *flags_host, int32_t *codes_host);
int32_t WebRtcAecmSessions_TickCallsHost(AecmSessions *s, const int16_t *far_host, const int16_t *near_host, const int16_t *near_clean_host,
                                         int16_t *out_host, int64_t stream_stride, size_t nrOfSamples, int32_t calls, int16_t msInSndCardBuf,
                                         const int16_t *msInSndCardBuf_host, const uint8_t *flags_host, int32_t *codes_host);
int32_t WebRtcAecmSessions_TickCallsAsync(AecmSessions *s, const int16_t *far_dev, const int16_t *near_dev, const int16_t *near_clean_dev,
                                          int16_t *out_dev, int64_t stream_stride, size_t nrOfSamples, int32_t calls, int16_t msInSndCardBuf,
                                          const int16_t *msInSndCardBuf_host, const uint8_t *flags_host, int32_t *codes_host,
                                          void *wait_hip_event, void *done_hip_event);
/* Packet ticks: K-call ticks for objects that hold both rates and for half calls.  One tick is one PACKET of `calls` = K 10 ms calls
 * per session; every session runs at its own rate and its own call size, and its samples are PACKED.  For every session s that
 * calls, with n_s = 80 if its flag byte carries AECM_SESSION_HALF_CALL (needs nrOfSamples == 160), else n_s = nrOfSamples:
 *     for (c = 0; c < K; ++c) {
 *         WebRtcAecm_BufferFarend(inst_s, far[s] + c * n_s, n_s);                               (unless AECM_SESSION_NO_FAREND)
 *         WebRtcAecm_Process(inst_s, near[s] + c * n_s, clean ? clean[s] + c * n_s : NULL, out[s] + c * n_s, n_s, ms_s);
 *     }
 * inst_s being a reference instance initialised at the session's own rate -- outputs, codes, echo paths and ExportSession(s)
 * snapshots are bit for bit those calls.  A decoded 20 ms G.711 packet is 160 contiguous samples at the start of its row, not two
 * 80-sample halves 160 apart: the server that carries G.711 and wideband calls on one 20 ms packet clock keeps the mixed object
 * (slots recycled for either rate, calls migrating to either rate) AND pays one planning launch, one tick launch and one round
 * trip of the core state per packet.
 *   rows                        : [S][stream_stride] with stream_stride >= calls * nrOfSamples for every row; the device forms
 *                                 neither read nor write a half-call session's samples [K * 80, K * 160), the Host form returns
 *                                 them as zeros
 *   calls == 1                  : TickFlags / TickAsync with the same arguments: the same launches, the same kernels
 *   calls > 1, no calling session flagged HALF_CALL, no session of another rate: TickCalls, by its launches and kernels
 *   otherwise                   : for a half-call session bit for bit K ordinary ticks flagged HALF_CALL on re-laid rows (ordinary
 *                                 tick c gets row[c * 80 .. c * 80 + 80) in the first half of a 160-sample row); the session ends
 *                                 K * 80 samples behind the object, as after those K ticks
 *   accepted                    : objects holding both rates, in either direction (a 16 kHz object with 8 kHz sessions on half calls
 *                                 or on full 160-sample calls, an 8 kHz object ticking 80 samples with 16 kHz sessions);
 *                                 AECM_SESSION_IDLE (the session falls calls * nrOfSamples behind; everything said of idle sessions
 *                                 stays true), AECM_SESSION_NO_FAREND, per-session msInSndCardBuf, a clean near-end input
 *   refused, changing nothing   : calls outside 1 .. AECM_SESSION_MAX_TICK_CALLS, a short stride, HALF_CALL with nrOfSamples == 80,
 *                                 SPLIT_CALLS on a calling session with calls > 1: AECM_BAD_PARAMETER_ERROR; the safe kernel
 *                                 variant: AECM_UNSUPPORTED_FUNCTION_ERROR.  The arguments are checked in the reference's order, as
 *                                 TickCalls does.
 * Measured on an MI355X against K back-to-back ticks flagged HALF_CALL of a twin object (profiles/r20_tick_packets.txt), K = 2 / 3 / 6:
 * 65 536 sessions, half of them 8 kHz on half calls 0.89 / 0.82 / 0.75 of the K ticks, all of them 0.74 / 0.68 / 0.56; 4 096 sessions
 * 0.72 / 0.62 / 0.50 and 0.64 / 0.53 / 0.39; a uniform object without half calls 0.93 / 0.87 / 0.82 and 0.80 / 0.69 / 0.60 (TickCalls itself).
 * Packet ticks mix freely with ordinary ticks, TickCalls, bursts, Process, InitSession*, set_config_session and
 * Export / ImportSession(s), at any point of a session's life.  TickPackets waits for the tick, TickPacketsHost stages host audio
 * as TickCallsHost does, TickPacketsAsync is TickAsync's form. */
int32_t WebRtcAecmSessions_TickPackets(AecmSessions *s, const int16_t *far_dev, const int16_t *near_dev, const int16_t *near_clean_dev,
                                       int16_t *out_dev, int64_t stream_stride, size_t nrOfSamples, int32_t calls, int16_t msInSndCardBuf,
                                       const int16_t *msInSndCardBuf_host, const uint8_t *flags_host, int32_t *codes_host);
int32_t WebRtcAecmSessions_TickPacketsHost(AecmSessions *s, const int16_t *far_host, const int16_t *near_host, const int16_t *near_clean_host,
                                           int16_t *out_host, int64_t stream_stride, size_t nrOfSamples, int32_t calls, int16_t msInSndCardBuf,
                                           const int16_t *msInSndCardBuf_host, const uint8_t *flags_host, int32_t *codes_host);
int32_t WebRtcAecmSessions_TickPacketsAsync(AecmSessions *s, const int16_t *far_dev, const int16_t *near_dev, const int16_t *near_clean_dev,
                                            int16_t *out_dev, int64_t stream_stride, size_t nrOfSamples, int32_t calls, int16_t msInSndCardBuf,
                                            const int16_t *msInSndCardBuf_host, const uint8_t *flags_host, int32_t *codes_host,
                                            void *wait_hip_event, void *done_hip_event);
/* Far-end bursts.  The reference lets a caller make ANY number of WebRtcAecm_BufferFarend calls between two
 * WebRtcAecm_Process calls (echo_control_mobile.h:87,135) -- what a jittery network produces: no far frame for a tick or
 * two, then several at once.  Each call runs the delay compensation once the session is past its start-up phase and then
 * appends to the 4 000-sample jitter buffer, which drops what does not fit (echo_control_mobile.cc:215-234, 575-594;
 * ring_buffer.c:142-170).  WebRtcAecmSessions_BufferFarend makes, for every session s,
 *     for (c = 0; c < (calls_host ? calls_host[s] : calls); ++c) WebRtcAecm_BufferFarend(inst_s, far[s] + c * nrOfSamples, nrOfSamples);
 * far: [S][stream_stride] int16 with stream_stride >= calls * nrOfSamples; calls in [0, 255]; calls_host: NULL or S entries
 * <= calls, read before the call returns.  Returns what the reference's call returns (0; AECM_NULL_POINTER_ERROR,
 * AECM_UNINITIALIZED_ERROR, AECM_BAD_PARAMETER_ERROR for the arguments, in its order).
 * WebRtcAecmSessions_Process is the other half: every session's WebRtcAecm_Process WITHOUT a WebRtcAecm_BufferFarend (a tick
 * in which every session carries AECM_SESSION_NO_FAREND); msInSndCardBuf_host / codes_host as in TickPerSession, both may be
 * NULL.  With the two, k = 0, 1, 2, ... far calls per near call and session are expressed as: BufferFarend with
 * calls_host[s] = k_s, then Process.  The Tick* forms remain the one-launch shape of the common k = 1 (TickFlags: k in
 * {0, 1} per session); in TickFlags / TickAsync far may be NULL when every session carries AECM_SESSION_NO_FAREND.
 * "The far end arrived, the near end is late" is the same pair with AECM_SESSION_IDLE: BufferFarend with calls_host[s] = 1 for those
 * sessions (0 for the others), AECM_SESSION_IDLE for them in the tick, and their WebRtcAecm_Process when the near end is there
 * (a later tick with AECM_SESSION_NO_FAREND, or Process).
 * BufferFarend (device pointers) and BufferFarendAsync are enqueued on the object's stream like ticks; BufferFarend and
 * BufferFarendHost wait for it, BufferFarendAsync does not (events as in TickAsync; the far rows must stay untouched
 * until the launch has run). */
int32_t WebRtcAecmSessions_BufferFarend(AecmSessions *s, const int16_t *far_dev, int64_t stream_stride, size_t nrOfSamples, int32_t calls,
                                        const uint8_t *calls_host);
int32_t WebRtcAecmSessions_BufferFarendHost(AecmSessions *s, const int16_t *far_host, int64_t stream_stride, size_t nrOfSamples, int32_t calls,
                                            const uint8_t *calls_host);
int32_t WebRtcAecmSessions_BufferFarendAsync(AecmSessions *s, const int16_t *far_dev, int64_t stream_stride, size_t nrOfSamples, int32_t calls,
                                             const uint8_t *calls_host, void *wait_hip_event, void *done_hip_event);
int32_t WebRtcAecmSessions_Process(AecmSessions *s, const int16_t *near_dev, const int16_t *near_clean_dev, int16_t *out_dev, int64_t stream_stride,
                                   size_t nrOfSamples, int16_t msInSndCardBuf, const int16_t *msInSndCardBuf_host, int32_t *codes_host);
int32_t WebRtcAecmSessions_ProcessHost(AecmSessions *s, const int16_t *near_host, const int16_t *near_clean_host, int16_t *out_host,
                                       int64_t stream_stride, size_t nrOfSamples, int16_t msInSndCardBuf, const int16_t *msInSndCardBuf_host,
                                       int32_t *codes_host);
int32_t WebRtcAecmSessions_Synchronize(AecmSessions *s);
/* AECM_KERNEL_FAST (default) / AECM_KERNEL_SAFE for the object's block engine.  The tick kernel is built on the fast
 * primitives only: with the safe variant selected, ticks return AECM_UNSUPPORTED_FUNCTION_ERROR (and change nothing).
 * Far-end bursts (WebRtcAecmSessions_BufferFarend*) are accepted under either variant and make the reference's
 * WebRtcAecm_BufferFarend calls as always. */
int32_t WebRtcAecmSessions_SetKernelVariant(AecmSessions *s, int32_t variant);
/* Diagnostics (tools/bench_sessions.py --occupancy): on != 0 sends every tick through the live list and the sparse tick kernel,
 * idle sessions or not, so that the cost of the indirection itself can be measured.  Results do not change. */
int32_t WebRtcAecmSessions_ForceSparseTicks(AecmSessions *s, int32_t on);
/* What the WebRtcAecm_Process calls of `session` carried since its last initialisation (AECM_SESSION_NO_CLEAN):
 * *mode = 0 no Process call yet, 1 every one carried a clean input, 2 none did, 3 both (only in an object that never used the flag).
 * Needs no device. */
int32_t WebRtcAecmSessions_GetSessionCleanMode(AecmSessions *s, int32_t session, int32_t *mode);
/* Diagnostics (tools/bench_split_clean.py): the tick launch of a tick with sessions of both kinds.  on < 0 (the default of a new
 * object): one fused launch up to four times the sessions the device holds at once, one launch per list beyond; on == 0: always the
 * fused launch; on > 0: always one launch per list.  Results do not change. */
int32_t WebRtcAecmSessions_SplitCleanTwoLaunches(AecmSessions *s, int32_t on);
/* K-call and packet ticks with a clean input PER SESSION: one packet clock, some legs behind a noise suppressor and some not.
 * Off (the default of a new object): nothing differs from an object without this call -- TickCalls* / TickPackets* with calls > 1,
 * near_clean != NULL and a calling session that carries AECM_SESSION_NO_CLEAN return AECM_UNSUPPORTED_FUNCTION_ERROR.
 * On (on != 0): those ticks (sync, Host and Async forms) are accepted.  For every session that calls the result is the loop written
 * at TickCalls / TickPackets, a flagged session's K WebRtcAecm_Process calls getting nearendClean = NULL and every other session's
 * clean[s] + c * n_s: bit for bit K ordinary ticks with the same flags on the same (packet ticks: re-laid) rows -- outputs, codes,
 * echo paths and ExportSession(s) snapshots -- and interchangeable with them at any point of a session's life.
 *   - The history rule of AECM_SESSION_NO_CLEAN applies unchanged: a tick that would change a calling session's kind is
 *     AECM_BAD_PARAMETER_ERROR, nothing changed.
 *   - No calling session flagged: exactly the K-call / packet tick with a clean input, by its launches.  Every calling session
 *     flagged: the K-call / packet tick without a clean plane; near_clean is not touched and no clean ring is made.
 *   - Otherwise: one planning launch that plans the K calls of every session and writes both live lists, then one tick launch per
 *     list, each keeping its sessions' core state in registers across the K call pairs (WebRtcAecmSessions_SplitCleanTwoLaunches
 *     does not apply: there is no fused form).  Measured on an MI355X against K back-to-back ordinary ticks with the same flags of
 *     a twin object (profiles/r33_split_calls.txt), K = 2 / 3 / 6, half the sessions flagged: 65 536 sessions 0.89 / 0.84 / 0.79 of
 *     the K ticks, 4 096 sessions 0.95 / 0.86 / 0.75; a quarter or three quarters flagged 0.91 .. 0.77 and 0.99 .. 0.77 (the least
 *     for K = 2 in small objects, where the ramp-down and ramp-up between the two tick launches is most of the packet).
 *   - Everything else TickCalls* / TickPackets* refuse stays refused, in the same order: SPLIT_CALLS, HALF_CALL in TickCalls, two
 *     rates in TickCalls, the safe kernel variant, an attached session trace.
 *   - While a call trace is attached (WebRtcAecmSessions_SetCallTrace) such a tick stays AECM_UNSUPPORTED_FUNCTION_ERROR, on or off.
 * A switch of the object like SplitCleanTwoLaunches and ForceSparseTicks: it keeps its value across Init / InitRates, and it is
 * host state read when a tick is planned, so it is ordered behind the ticks already enqueued; no synchronisation is needed.
 * Returns 0; -1 for a NULL object. */
int32_t WebRtcAecmSessions_SetSplitCallTicks(AecmSessions *s, int32_t on);

/* ---- Session trace: where every call stands, per tick, without stopping the clock ------------------------------
 * Opt-in, per object.  While a trace buffer is attached, every session that calls in a tick of ONE call pair per session also writes
 * one 64-byte record: has its canceller left start-up, which delay does the wrapper steer by, how full is its far-end jitter buffer,
 * and -- in `core` -- what the block trace shows of the core state after the tick's last block (echo delay estimate, far-end activity,
 * suppression gain ...).  Every wrapper field is the value WebRtcAecmSessions_ExportSession would show directly after that tick, taken
 * from the wrapper words of the snapshot (the named member of the reference's AecMobile, echo_control_mobile.cc:42-79; the 16-bit
 * fields are the low halves of their words); `core` is AecmBlockTrace of the core blob of that same snapshot.  Little endian.
 * Audio, codes, state and snapshots are identical with and without a trace; with none attached every launch is the launch it is
 * without this feature, with the same kernels. */
typedef struct AecmSessionTrace {      /* 64 bytes */
    uint32_t tick;                     /*  0  number of this tick, counted from 0 at attachment                            */
    int16_t  blocks;                   /*  4  blocks the core ran for this session in this tick: the advance of the snapshot's
                                        *     block position over the tick, divided by 64 (0 in the start-up phase)         */
    int16_t  samp_khz;                 /*  6  8 or 16: the session's own rate                                              */
    int16_t  ms_in_snd_card_buf;       /*  8  msInSndCardBuf (after the reference's + 10)                                  */
    int16_t  known_delay;              /* 10  knownDelay                                                                   */
    int16_t  filt_delay;               /* 12  filtDelay                                                                    */
    int16_t  buf_size_start;           /* 14  bufSizeStart                                                                 */
    int16_t  ec_startup;               /* 16  ECstartup: 1 while the session is in its start-up phase                      */
    int16_t  check_buff_size;          /* 18  checkBuffSize                                                                */
    int16_t  delay_change;             /* 20  delayChange                                                                  */
    int16_t  last_delay_diff;          /* 22  lastDelayDiff                                                                */
    int32_t  far_buffered;             /* 24  samples in the far-end jitter buffer, 0 .. 4000                              */
    int32_t  time_for_delay_change;    /* 28  timeForDelayChange                                                           */
    AecmBlockTrace core;               /* 32  the core state after the tick's last block, exactly AecmBlockTrace           */
} AecmSessionTrace;
size_t WebRtcAecmSessions_session_trace_size_bytes(void);      /* 64 */
/* Attaches trace_dev (device memory, or a registered host alias: WebRtcAecmBatch_RegisterHostBuffer; NULL detaches).  Strides are in
 * records: tick number j since attachment writes session s's record at
 *     trace_dev + 64 * (s * session_stride + (j % ring_ticks) * tick_stride).
 * ring_ticks == 1 keeps "the latest record per session", a larger ring keeps history: a session-major buffer [S][R] is (R, 1, R), a
 * tick-major one [R][S] is (1, S, R).  The caller owns the buffer and its size, as for out_dev.  Attaching (again) starts the count at 0.
 *  - A session that runs no block in a tick (start-up phase) still gets its record, with the core state it holds.
 *  - A session that carries AECM_SESSION_IDLE gets no record: its slot keeps its bytes, and the `tick` field of what it holds tells a
 *    consumer how old that is.  A tick in which nobody calls writes nothing and still counts.
 *  - Traced: every tick of ONE call pair per session -- Tick, TickPerSession, TickFlags, TickAsync, their Host forms, Process /
 *    ProcessHost, and TickCalls* / TickPackets* with calls == 1 -- with every flag (AECM_SESSION_SPLIT_CALLS: one record for the tick,
 *    taken after the second call), with per-session msInSndCardBuf, with sessions of both rates, with and without a clean input.
 *    WebRtcAecmSessions_BufferFarend* writes no record.
 *  - While a trace is attached, TickCalls* / TickPackets* with calls > 1 return AECM_UNSUPPORTED_FUNCTION_ERROR and change nothing:
 *    not the sessions, not the position, not the tick count.  (Those ticks keep the core state in registers across their calls; a
 *    record per call from that loop is the call trace's, below: WebRtcAecmSessions_SetCallTrace.)
 *  - A refused tick of any kind does not advance the count.
 *  - With TickAsync the records are visible where out is: behind done_hip_event or WebRtcAecmSessions_Synchronize.
 *  - SetSessionTrace is ordered behind the ticks already enqueued: they write where they were told to when they were enqueued.
 * Returns 0, or AECM_BAD_PARAMETER_ERROR with nothing changed (an attached trace stays attached) for a NULL object, a pointer that is
 * not 4-byte aligned, a stride <= 0 or ring_ticks <= 0. */
int32_t WebRtcAecmSessions_SetSessionTrace(AecmSessions *s, void *trace_dev, int64_t session_stride, int64_t tick_stride, int32_t ring_ticks);
/* *ticks = the ticks accepted since the trace was attached (0 while none is attached).  Needs no device. */
int32_t WebRtcAecmSessions_GetSessionTraceTicks(AecmSessions *s, int64_t *ticks);

/* ---- Call trace: one AecmSessionTrace record per session and CALL PAIR, K-call and packet ticks too ------------------------------
 * The session trace above refuses the ticks a packet server runs on (TickCalls* / TickPackets* with calls > 1).  The call trace is a
 * second, separate opt-in with the same record and a switch of its own: while it is attached the object counts CALL SLOTS -- an
 * accepted tick with argument calls = K advances the count by K, an ordinary tick or Process by 1 -- and every session that calls
 * writes one 64-byte AecmSessionTrace record per call slot.  The struct is unchanged; its `tick` field holds the slot number j + c for
 * call c of a tick that started at count j, and the record lies at
 *     trace_dev + 64 * (s * session_stride + ((j + c) % ring_calls) * call_stride).
 * The contract: the buffer after a K-call or packet tick is byte for byte the buffer that K ordinary ticks under SetSessionTrace
 * leave with the same geometry on the same rows (for a half-call session of a packet tick: K AECM_SESSION_HALF_CALL ticks on re-laid
 * rows, as TickPackets defines its equivalence).  So every wrapper field is what ExportSession would show directly after that call
 * pair, `blocks` is the blocks the core ran in that call, and `core` is AecmBlockTrace of the core state after that call's last
 * block -- or of the state the session holds, for a call that ran none.
 *  - ring_calls == 1 keeps the latest call's record.  With ring_calls < K the buffer is what writing the K records in order gives.
 *  - A session that carries AECM_SESSION_IDLE gets no records: its slots keep their bytes, and the count still advances by K.  A tick
 *    nobody makes writes nothing and still counts.
 *  - Traced: TickCalls*, TickPackets* (Device, Host and Async forms) with any calls they accept, and everything the session trace
 *    traces -- AECM_SESSION_NO_FAREND, per-session msInSndCardBuf, both rates, with and without a clean input.  With calls == 1 a
 *    tick is the session trace's tick with the slot number as its number (AECM_SESSION_SPLIT_CALLS / AECM_SESSION_HALF_CALL: one
 *    record for the slot).  WebRtcAecmSessions_BufferFarend* writes no record and does not count.
 *  - Everything TickCalls* / TickPackets* refuse without a trace is refused with one (a calling AECM_SESSION_NO_CLEAN session with
 *    calls > 1 and a clean plane -- AECM_UNSUPPORTED_FUNCTION_ERROR also where WebRtcAecmSessions_SetSplitCallTicks is on: such
 *    ticks are not call-traced; the safe kernel variant; ...), and a refused tick changes nothing: not the sessions, not the
 *    position, not the count.
 *  - Records are visible where out is; SetCallTrace is ordered behind the ticks already enqueued, without a synchronisation.
 *  - At most one of the two traces is attached: SetCallTrace while a session trace is attached, and SetSessionTrace while a call
 *    trace is, return AECM_BAD_PARAMETER_ERROR and leave the attached one attached.  NULL detaches only its own kind.
 *    GetSessionTraceTicks keeps answering for the session trace only (0 while a call trace is attached).
 * An object that never calls SetCallTrace launches the kernels and gives the refusals it always did.
 * Returns 0, or AECM_BAD_PARAMETER_ERROR with nothing changed for a NULL object, a pointer that is not 4-byte aligned, a
 * stride <= 0, ring_calls <= 0, or a session trace that is attached.  Attaching (again) starts the count at 0. */
int32_t WebRtcAecmSessions_SetCallTrace(AecmSessions *s, void *trace_dev, int64_t session_stride, int64_t call_stride, int32_t ring_calls);
/* *calls = the call slots counted since the call trace was attached (0 while none is attached).  Needs no device. */
int32_t WebRtcAecmSessions_GetCallTraceCalls(AecmSessions *s, int64_t *calls);

/* Zero-copy host audio.  A caller-owned host buffer is pinned and mapped into the device's address space once
 * (hipHostRegister); *device_alias is then a device pointer that every *_dev argument of this header accepts
 * (WebRtcAecmBatch_ProcessBlocks, WebRtcAecmSessions_Tick / TickAsync ...): the kernels read the samples and write the
 * output in place over the link -- no staging copies, no pageable-memory transfers (the *Host forms stage through
 * pageable copies: 1.44 ms per tick of 65 536 sessions against the numbers in INTEGRATION.md for this form). */
int32_t WebRtcAecmBatch_RegisterHostBuffer(int32_t device_id, void *host, size_t size_bytes, void **device_alias);
int32_t WebRtcAecmBatch_UnregisterHostBuffer(int32_t device_id, void *host);

/* Per-session control while the other sessions keep running (a media server recycling one slot when a call
 * ends).  `session` in [0, S); same return codes as the single-session functions they mirror:
 *   InitSession           <-> WebRtcAecm_Init(inst_s, same sampFreq)   (echo_control_mobile.h:70): fresh core state,
 *                             fresh jitter buffer / start-up phase, default config (cng on, echoMode 3)
 *   set_config_session    <-> WebRtcAecm_set_config(inst_s, config)   (:156)
 *   InitEchoPath / GetEchoPath <-> WebRtcAecm_InitEchoPath / GetEchoPath (:172, :191), 130 bytes
 * InitSession and set_config_session are kernel launches ordered before the next tick on the object's stream (no
 * synchronisation with the host); InitEchoPath / GetEchoPath synchronise. */
int32_t WebRtcAecmSessions_InitSession(AecmSessions *s, int32_t session);
int32_t WebRtcAecmSessions_set_config_session(AecmSessions *s, int32_t session, AecmConfig config);
int32_t WebRtcAecmSessions_InitEchoPath(AecmSessions *s, int32_t session, const void *echo_path, size_t size_bytes);
int32_t WebRtcAecmSessions_GetEchoPath(AecmSessions *s, int32_t session, void *echo_path, size_t size_bytes);

/* Snapshot of ONE live session (checkpoint; migration of a call into another AecmSessions object, on another GPU):
 * everything the reference keeps per instance -- AecMobile's wrapper members and its far-end jitter buffer
 * (echo_control_mobile.cc:42-79), the core's frame buffers and the core state (aecm_core.h:41-141) -- in a form that does
 * not depend on the object it was taken from.  A session imported into any slot of any object of the same sampling rate
 * continues bit-exactly where the exported one stopped, whatever the two objects' ages; the exporting object is not
 * changed.  ImportSession refuses (AECM_BAD_PARAMETER_ERROR, nothing changed) a snapshot of another layout or rate, one
 * whose wrapper state could not have been reached (buffer fills, pending samples, flags), and a core state ImportState
 * would refuse.  Both calls wait for the ticks enqueued so far. */
size_t WebRtcAecmSessions_session_size_bytes(void);
int32_t WebRtcAecmSessions_ExportSession(AecmSessions *s, int32_t session, void *snapshot, size_t size_bytes);
int32_t WebRtcAecmSessions_ImportSession(AecmSessions *s, int32_t session, const void *snapshot, size_t size_bytes);

/* The same for a LIST of sessions at once -- draining a GPU for maintenance, rebalancing calls between GPUs, checkpointing an
 * object: one gather (scatter) launch on the device for the whole list instead of about ten blocking copies and a host pass
 * per session.  sessions_host: count distinct session indices in [0, S), any order; NULL means 0 .. count-1.  snapshots: count
 * snapshots of WebRtcAecmSessions_session_size_bytes() each, back to back, in list order (size_bytes = count x that).
 *   Every snapshot is byte for byte what ExportSession of that session would have written at that moment; the exporting
 * object is not changed.  All four calls are ordered behind the ticks and bursts already enqueued on the object's stream and
 * return when their work is done.
 *   The host forms stage through a grow-only device buffer of at most 256 snapshots (8.4 MiB): one copy per 256 sessions, the
 * copy of each chunk ordered before the next gather.  The *Device forms take anything the device can address -- device memory
 * (the staging buffer of a peer-to-peer migration) or the alias of a host buffer registered with
 * WebRtcAecmBatch_RegisterHostBuffer -- 4-byte aligned; a 16-byte-aligned buffer moves 16 bytes per lane.  For
 * ImportSessionsDevice the buffer must not change while the call runs.
 *   ImportSessions is all or nothing: every snapshot is validated by ImportSession's rules (any_rate != 0:
 * ImportSessionAnyRate's) before any slot is touched -- on the host for the host form, by a validation launch and one read-back
 * for the *Device form; a refused list changes nothing.  After a successful import the object is exactly what `count` single
 * imports would have left (session rates, the clean near-end ring).
 *   count == 0: 0, nothing happens.  AECM_BAD_PARAMETER_ERROR (nothing changed): count < 0, another size_bytes, an index out of
 * range, a duplicate in the list (export and import alike), a device pointer that is not 4-byte aligned, a snapshot
 * ImportSession would refuse.  AECM_NULL_POINTER_ERROR: snapshots NULL with count > 0.  An uninitialised or poisoned object:
 * as ExportSession. */
int32_t WebRtcAecmSessions_ExportSessions(AecmSessions *s, const int32_t *sessions_host, int32_t count, void *snapshots_host, size_t size_bytes);
int32_t WebRtcAecmSessions_ImportSessions(AecmSessions *s, const int32_t *sessions_host, int32_t count, const void *snapshots_host, size_t size_bytes, int32_t any_rate);
int32_t WebRtcAecmSessions_ExportSessionsDevice(AecmSessions *s, const int32_t *sessions_host, int32_t count, void *snapshots_dev, size_t size_bytes);
int32_t WebRtcAecmSessions_ImportSessionsDevice(AecmSessions *s, const int32_t *sessions_host, int32_t count, const void *snapshots_dev, size_t size_bytes, int32_t any_rate);

/* Sessions of both sampling rates in ONE object -- one object per clock, not per rate: narrowband (8 kHz, 10 ms = 80 samples)
 * and wideband (16 kHz, 10 ms = 160 samples) calls tick together, a 160-sample tick with AECM_SESSION_HALF_CALL for the
 * sessions whose 10 ms are 80 samples.  Every session runs at its own rate wherever the reference looks at an instance's rate
 * (echo_control_mobile.cc:142-191, 236-283, 384-387, 534-594; the core's wideband branch): in Tick*, BufferFarend* and
 * Process* alike.  The call size of BufferFarend* and Process* stays one value per call for the whole object.
 * ExportSession writes the session's own rate into the snapshot; ImportSession of an object whose own rate that is takes it
 * (a call moves between uniform and mixed objects in both directions).
 *
 * InitRates: as WebRtcAecmSessions_Init(s, sampFreq); then every session k with rates_host[k] != sampFreq (S entries, each 8000
 * or 16000; AECM_BAD_PARAMETER_ERROR and nothing changed otherwise) is a fresh WebRtcAecm_Init(inst_k, rates_host[k]).
 * sampFreq stays the object's own rate: what InitSession and ImportSession mean by "the same rate".
 * InitSessionRate: InitSession at a rate of the caller's choice, WebRtcAecm_Init(inst_s, sampFreq).  A launch on the object's
 * stream, ordered before the next tick like InitSession.
 * ImportSessionAnyRate: ImportSession that also takes a snapshot of the other rate (header and core state must agree on it);
 * the slot then runs at the snapshot's rate.  Everything ImportSession refuses for another reason is refused here too. */
int32_t WebRtcAecmSessions_InitRates(AecmSessions *s, int32_t sampFreq, const int32_t *rates_host);
int32_t WebRtcAecmSessions_InitSessionRate(AecmSessions *s, int32_t session, int32_t sampFreq);
int32_t WebRtcAecmSessions_GetSessionRate(AecmSessions *s, int32_t session, int32_t *sampFreq);
int32_t WebRtcAecmSessions_ImportSessionAnyRate(AecmSessions *s, int32_t session, const void *snapshot, size_t size_bytes);

/* AECM_KERNEL_FAST (default) or AECM_KERNEL_SAFE cross-lane primitives. */
int32_t WebRtcAecmBatch_SetKernelVariant(AecmBatch *b, int32_t variant);

/* How a ProcessBlocks launch is scheduled on the device; results do not depend on it.  A launch of more streams than
 * the pipelined form takes (4 096 on an MI355X) is cut into chunks of chunk_blocks blocks that resident wavefronts
 * claim in order from a queue, so that all streams advance together and the launch does not end at low occupancy
 * (default: 128 blocks; the default is quartered, to at least 8, while every stream's wavefront is resident at once -- a
 * chunk_blocks set through this call is taken as it is).  (Shorthand for the queue_* fields of AecmLaunchPolicy, below.)
 * chunk_blocks = 0: one wavefront keeps one stream for the whole launch, always.  min_streams < 0 (default): the
 * threshold above; >= 0: the queue form above that many streams (diagnostics / tests). */
int32_t WebRtcAecmBatch_SetLaunchChunking(AecmBatch *b, int32_t chunk_blocks, int32_t min_streams);
/* Launches the chip holds at once (<= 16 streams per compute unit = 4 096 streams on an MI355X; fast variant; with a clean
 * near-end input only after WebRtcAecmBatch_SetCleanPipelining) run pipelined: a workgroup serves up to four streams with the state-independent transforms of a block in
 * "front" wavefronts of their own, one block ahead of the rest.  Shape by streams per compute unit: up to 8 (2 048 streams)
 * sixteen wavefronts per workgroup, two workgroups per unit -- the delay estimator one block ahead, the gain half of the block and
 * the inverse transforms one block behind, each in wavefronts of their own; up to 12 (3 072) eight wavefronts (front and "tail"
 * wavefronts of two streams each), three workgroups per unit; above that six (no tail wavefronts), four per unit, the workgroups kept
 * in step through progress feedback on their front wavefronts' issue priority.  Every compute unit gets the shape's full count of
 * workgroups, of one to four streams each, so that unit loads differ by at most one stream.
 * min_streams: the smallest batch that takes this form (default 2; <= 0: never).  Results do not depend on it.
 * By default launches of one or two blocks keep one wavefront per stream (the pipeline's fill and drain steps cost more than
 * they save there); after this call launches of any length from min_streams streams are pipelined.  (Shorthand for
 * pipelined_min_streams / pipelined_min_blocks of AecmLaunchPolicy, below; its pipe_* fields override the shape.) */
int32_t WebRtcAecmBatch_SetLaunchPipelining(AecmBatch *b, int32_t min_streams);
/* Ragged launches (WebRtcAecmBatch_ProcessBlocksRagged, WebRtcAecmBatch_ProcessRecordingsRagged) that the chip holds at once, pipelined:
 * enable != 0 and such a launch takes the pipelined form above instead of one wavefront per stream when the fast variant is selected,
 * there is no clean near-end input (a ragged launch with one is pipelined by a switch of its own,
 * WebRtcAecmBatch_SetRaggedCleanPipelining, and by nothing else), the streams that have blocks to run (not the batch's size: 100 live
 * streams of 65 536 qualify) are
 * within [pipelined_min_streams, pipelined_max_streams] and the longest has at least pipelined_min_blocks blocks.  All lengths equal
 * stays the equal-length launch, and the chunk queue keeps what it takes today.  A workgroup still marches its (up to) four streams in
 * lock step -- every wavefront executes as many barriers as the workgroup's longest stream has blocks -- and a slot whose stream has
 * ended only keeps the barriers.  Which stream shares a workgroup and a compute unit with which is planned on the host, longest first
 * onto the unit with the fewest blocks (WebRtcAecmBatch_RaggedPipePlan).  The unbalanced shapes only: a launch whose size would
 * pick the balanced six-wavefront shape takes the plain one.  Per batch; OFF by default: the form is new, and although it measured
 * 1.3 to 2.9 times the one-wavefront-per-stream launch at 256 ... 4 096 streams (profiles/r10_ragged_pipelined.txt), which kernel
 * existing callers run is changed in a step of its own, not as a side effect of adding the form.
 * Results never depend on it.  AECM_BAD_PARAMETER_ERROR for a NULL batch. */
int32_t WebRtcAecmBatch_SetRaggedPipelining(AecmBatch *b, int32_t enable);
/* Equal-length launches WITH a clean near-end input (near_clean_dev: the output of a noise suppressor next to the noisy signal) that
 * the chip holds at once, pipelined: enable != 0 and such a launch takes the pipelined form under exactly the conditions of a launch
 * without a clean input -- fast variant, pipelined_min_streams <= streams <= pipelined_max_streams, at least pipelined_min_blocks
 * blocks -- instead of one wavefront per stream.  The front wavefronts then run three transforms per block and hand the clean
 * spectrum on; the shapes are those with formed spectra and without progress feedback: by workgroups of four streams per compute
 * unit, up to two sixteen wavefronts (shape bits 0x1a02), up to three eight (0x002), above that six (0x000); pipe_* wishes that
 * name another shape land on the nearest of these (the raw hand-over is dropped, four front wavefronts without delay and gain
 * wavefronts become two; pipe_delay_waves 4 with pipe_gain_waves 0 gives twelve wavefronts, 0x802) -- never a launch error.
 * DescribeLaunch reports these launches with the shape bits + 0x2000.  ProcessRecordings* with a clean input run their blocks
 * through the same launch rule.  Ragged launches with a clean input stay as they are (one wavefront per stream, or the chunk
 * queue), whatever this switch and WebRtcAecmBatch_SetRaggedPipelining say: their pipelined form has a switch of its own,
 * WebRtcAecmBatch_SetRaggedCleanPipelining; a ragged call whose lengths are all equal IS the equal-length launch.  out_dev may
 * alias near_clean_dev as for every other form (no input row is read after
 * an output row of the same launch has been written).  Per batch; OFF by default, for the reason given above: with it off every
 * launch takes exactly the form it took before the switch existed.  Static checks, and the sweep to run: profiles/r11_clean_pipelined.txt.
 * Results never depend on it.  AECM_BAD_PARAMETER_ERROR for a NULL batch. */
int32_t WebRtcAecmBatch_SetCleanPipelining(AecmBatch *b, int32_t enable);
/* Ragged launches WITH a clean near-end input that the chip holds at once, pipelined: enable != 0 and such a launch
 * (WebRtcAecmBatch_ProcessBlocksRagged, WebRtcAecmBatch_ProcessRecordingsRagged* with a clean input) takes the pipelined form instead of
 * one wavefront per stream when the fast variant is selected, the chunk queue does not take it, the streams that have blocks to run
 * are within [pipelined_min_streams, pipelined_max_streams] and the longest has at least pipelined_min_blocks blocks -- the rule of
 * WebRtcAecmBatch_SetRaggedPipelining, by the same host-made plan (WebRtcAecmBatch_RaggedPipePlan's placement), in the shapes of
 * WebRtcAecmBatch_SetCleanPipelining (0x1a02 / 0x002 / 0x000, 0x802 by wish; pipe_* wishes land on the nearest of these, never a
 * launch error), reported with the shape bits + 0x2000.  A switch of its own because the other two keep their meaning: with this one
 * off a ragged launch with a clean input takes exactly the form and kernel it took before this switch existed, whatever the other two say,
 * and this one changes no launch without a clean input and no equal-length launch (all lengths equal IS the equal-length launch, under
 * WebRtcAecmBatch_SetCleanPipelining's rule).  A stream that ends before its workgroup does leaves its state exactly as after its own
 * last block; blocks at and beyond a stream's length are neither read nor written, and out_dev may alias near_clean_dev.
 * Per batch; OFF by default, for the reason given above, although it measured 1.16 to 2.24 times the one-wavefront-per-stream launch at
 * 256 ... 4 096 streams (profiles/r15_ragged_clean_pipelined.txt, with the static checks).
 * Results never depend on it.  AECM_BAD_PARAMETER_ERROR for a NULL batch. */
int32_t WebRtcAecmBatch_SetRaggedCleanPipelining(AecmBatch *b, int32_t enable);
/* Which form a ProcessBlocks launch of num_blocks blocks over the whole batch takes, with (has_clean_input != 0) or
 * without a clean near-end input (for measurement tools that must name
 * the kernel they time): 0 = one wavefront per stream, kernel variants for launches the chip holds at once; 1 = one
 * wavefront per stream, issue priority by phase; 2 = the chunk queue (*chunk_blocks, if not NULL, receives the chunk);
 * 3 = pipelined (*chunk_blocks then receives the shape: the "tail" wavefronts per workgroup, 0 or 2, + 0x100 when the
 * launch balances its workgroups' progress, + 0x200 with four front wavefronts instead of two, + 0x400 when the back
 * wavefronts form the spectra, + 0x800 with delay wavefronts, + 0x1000 with gain wavefronts, + 0x2000 for the kernel that takes
 * a clean near-end input: WebRtcAecmBatch_SetCleanPipelining -- on a batch this call answers by the batch's own switch). */
#define AECM_LAUNCH_RESIDENT 0
#define AECM_LAUNCH_PER_STREAM 1
#define AECM_LAUNCH_CHUNK_QUEUE 2
#define AECM_LAUNCH_PIPELINED 3
int32_t WebRtcAecmBatch_DescribeLaunch(const AecmBatch *b, int32_t num_blocks, int32_t has_clean_input, int32_t *chunk_blocks);
/* The same answer for a batch of num_streams streams (fast variant, the default launch policy) on a device with
 * compute_units compute units -- no device and no batch needed (capacity planning; -1 for a non-positive argument). */
int32_t WebRtcAecmBatch_DescribeLaunchFor(int32_t num_streams, int32_t compute_units, int32_t num_blocks, int32_t has_clean_input,
                                          int32_t *chunk_blocks);

/* The launch policy: every threshold and wish that decides how a ProcessBlocks launch is scheduled, as ONE value.  The library derives
 * it from the device's compute units (WebRtcAecmBatch_DefaultLaunchPolicy does the same without a device) and from what its kernels are
 * built for; a caller may read it, change fields and set it back (per batch).  Results never depend on it.  The shipped library reads
 * no environment variable: experiments set a policy, or use a build with -DAECM_EXPERIMENTS (tools/ab_build.py) whose default policy
 * takes the AECM_* wishes of the environment.
 *   struct_size            sizeof(AecmLaunchPolicy) of the caller's header (the calls refuse another size)
 *   compute_units          of the device (Set refuses a policy made for another count)
 *   queue_chunk_blocks     chunk queue: blocks per item (128); 0 = never the queue: one wavefront keeps one stream for the whole launch
 *   queue_chunk_explicit   0: the default length, quartered (to at least 8) while every stream's wavefront is resident at once; 1: as given
 *   queue_min_streams      the queue above this many streams; -1: above pipelined_max_streams
 *   pipelined_min_streams  the smallest batch whose launches run pipelined (2); larger than the batch: never
 *   pipelined_min_blocks   the shortest launch that does (3: the pipeline's fill and drain steps cost more than they save below)
 *   pipelined_max_streams  the largest batch that does (16 per compute unit: what the chip holds of the widest shape)
 *   resident_waves         wavefronts of the one-wavefront-per-stream kernels the chip holds (28 per compute unit)
 *   rotation_stream_limit  launches of at most this many streams take the kernel variants built for full residency
 *   pipe_*                 wishes for the pipelined form's shape, -1 = by size (tests, experiments): tail wavefronts 0 / 2, front wavefronts
 *                          2 / 4, raw hand-over 0 / 1, delay wavefronts 0 / 2 / 4, gain wavefronts 0 / 4; pipe_spread 1 = every compute
 *                          unit gets the shape's full count of workgroups, of fewer than four streams each where the launch is short of
 *                          streams (0: workgroups of four); pipe_wgs_per_cu > 0 = workgroups of the shape a compute unit takes;
 *                          pipe_rot >= 0 = the slot rotations, pipe_prio >= 0 = the role wavefronts' issue priorities (csrc/aecm_kernels.h:
 *                          PipeShape::rot / prio) */
typedef struct AecmLaunchPolicy {
    int32_t struct_size;
    int32_t compute_units;
    int32_t queue_chunk_blocks, queue_chunk_explicit, queue_min_streams;
    int32_t pipelined_min_streams, pipelined_min_blocks, pipelined_max_streams;
    int32_t resident_waves, rotation_stream_limit;
    int32_t pipe_tail_waves, pipe_front_waves, pipe_raw, pipe_delay_waves, pipe_gain_waves, pipe_spread, pipe_wgs_per_cu, pipe_rot, pipe_prio;
} AecmLaunchPolicy;
int32_t WebRtcAecmBatch_DefaultLaunchPolicy(int32_t compute_units, AecmLaunchPolicy *policy);
int32_t WebRtcAecmBatch_GetLaunchPolicy(const AecmBatch *b, AecmLaunchPolicy *policy);
int32_t WebRtcAecmBatch_SetLaunchPolicy(AecmBatch *b, const AecmLaunchPolicy *policy);
/* What a launch looks like on the device, for capacity planning (no device needed): the form and its detail as DescribeLaunch gives
 * them, the grid, and how the grid quantises on the chip -- rounds_x1000 = 1000 x workgroups / (compute units x workgroups a compute
 * unit holds at once): 1000 = the chip exactly full once; 9140 = nine full rounds and a last one 14 % full (65 536 sessions' tick);
 * and how evenly a pipelined launch loads the compute units (cu_load_evenness_x1000: batches that are multiples of the unit count
 * lose nothing, one stream more loses up to 1 / (streams per unit + 1) of the frame rate).
 * policy == NULL: the default policy of compute_units.  WebRtcAecmSessions_DescribeTick: the same for one tick of num_sessions sessions. */
typedef struct AecmLaunchDescription {
    int32_t form, chunk_blocks, shape;
    int32_t workgroups, waves_per_workgroup, workgroups_per_cu, rounds_x1000;
    /* pipelined launches keep every stream on one compute unit for the whole launch, so the launch ends when the fullest unit does:
     * 1000 x (streams / compute units) / (streams on the fullest unit) -- 1000 when the batch is a multiple of the unit count,
     * 800 for 1 025 streams on 256 units (one unit carries five streams, the average four).  1000 for the other forms (the chunk queue
     * balances dynamically; one wavefront per stream runs in rounds: rounds_x1000). */
    int32_t cu_load_evenness_x1000;
} AecmLaunchDescription;
int32_t WebRtcAecmBatch_DescribeLaunchDetail(const AecmLaunchPolicy *policy, int32_t compute_units, int32_t num_streams, int32_t num_blocks,
                                             int32_t has_clean_input, AecmLaunchDescription *out);
/* WebRtcAecmBatch_DescribeLaunchDetail with the batch's opt-in for clean inputs (WebRtcAecmBatch_SetCleanPipelining) as an argument.
 * clean_pipelining = 0: exactly that call's answer.  Otherwise a launch with a clean input is pipelined under the conditions of one
 * without (form 3, shape bits + 0x2000); launches without a clean input are described as before.  (AecmLaunchPolicy is unchanged:
 * the switch is a property of the batch, not of the policy.) */
int32_t WebRtcAecmBatch_DescribeLaunchDetailEx(const AecmLaunchPolicy *policy, int32_t compute_units, int32_t num_streams, int32_t num_blocks,
                                               int32_t has_clean_input, int32_t clean_pipelining, AecmLaunchDescription *out);
/* The same for a launch of a batch with a block trace attached (WebRtcAecmBatch_SetBlockTrace), no device needed: never form 3 -- where
 * WebRtcAecmBatch_DescribeLaunchDetail says pipelined this says one wavefront per stream -- and that call's answer everywhere else. */
int32_t WebRtcAecmBatch_DescribeTracedLaunch(const AecmLaunchPolicy *policy, int32_t compute_units, int32_t num_streams, int32_t num_blocks,
                                             int32_t has_clean_input, AecmLaunchDescription *out);
/* The same for a ragged launch (WebRtcAecmBatch_ProcessBlocksRagged) of num_streams streams with these lengths, no device needed: form,
 * chunk and grid as above -- the chunk queue when more streams than the queue's threshold have blocks to run and the longest has at
 * least two chunks, else one wavefront per stream; never pipelined (this call describes a batch that has not opted in:
 * WebRtcAecmBatch_SetRaggedPipelining, WebRtcAecmBatch_DescribeRaggedLaunchEx); every length equal: exactly DescribeLaunchDetail of that length --
 * plus the queue's item count (*items = sum of ceil(length / chunk); 0 for the other forms), and the sum and the maximum of the
 * lengths in blocks: the useful work and the critical path.  items / sum_blocks / max_blocks may be NULL. */
int32_t WebRtcAecmBatch_DescribeRaggedLaunch(const AecmLaunchPolicy *policy, int32_t compute_units, int32_t num_streams,
                                             const int32_t *blocks_per_stream_host, int32_t has_clean_input, AecmLaunchDescription *out,
                                             int64_t *items, int64_t *sum_blocks, int32_t *max_blocks);
/* WebRtcAecmBatch_DescribeRaggedLaunch with the batch's opt-in (WebRtcAecmBatch_SetRaggedPipelining) as an argument.  ragged_pipelining
 * = 0: exactly that call's answer.  Otherwise a launch the rule of SetRaggedPipelining takes is described as form 3: shape as
 * DescribeLaunchDetail gives it (chunk_blocks 0), the workgroups of the plan (up to the last one that holds a stream), and
 * cu_load_evenness_x1000 = 1000 x (mean blocks per compute unit) / (blocks on the fullest unit) -- the launch ends when that unit
 * does.  The mean is over the units the launch's shape puts workgroups on, min(compute units, workgroups of the shape): a launch of
 * fewer workgroups than the device has units (100 live streams on 256 units) is not called uneven for the units it leaves idle. */
int32_t WebRtcAecmBatch_DescribeRaggedLaunchEx(const AecmLaunchPolicy *policy, int32_t compute_units, int32_t num_streams,
                                               const int32_t *blocks_per_stream_host, int32_t has_clean_input, int32_t ragged_pipelining,
                                               AecmLaunchDescription *out, int64_t *items, int64_t *sum_blocks, int32_t *max_blocks);
/* WebRtcAecmBatch_DescribeRaggedLaunchEx with the batch's opt-in for ragged launches with a clean input
 * (WebRtcAecmBatch_SetRaggedCleanPipelining) as one more argument.  ragged_clean_pipelining = 0: exactly that call's answer.  Otherwise
 * a launch with a clean input that the rule of SetRaggedCleanPipelining takes is described as form 3, shape bits + 0x2000, with the
 * plan's workgroups and cu_load_evenness_x1000 as above; launches without a clean input are described as before. */
int32_t WebRtcAecmBatch_DescribeRaggedLaunchEx2(const AecmLaunchPolicy *policy, int32_t compute_units, int32_t num_streams,
                                                const int32_t *blocks_per_stream_host, int32_t has_clean_input, int32_t ragged_pipelining,
                                                int32_t ragged_clean_pipelining, AecmLaunchDescription *out, int64_t *items, int64_t *sum_blocks,
                                                int32_t *max_blocks);
/* The same for the launch WebRtcAecmBatch_ProcessBlocksRagged would make on THIS batch (blocks_per_stream_host: its num_streams
 * entries): under its launch policy, its kernel variant (a batch on the safe variant is never pipelined) and its
 * WebRtcAecmBatch_SetRaggedPipelining and WebRtcAecmBatch_SetRaggedCleanPipelining switches -- what the engine itself decides by.
 * -1 for a NULL batch. */
int32_t WebRtcAecmBatch_DescribeRaggedLaunchOf(const AecmBatch *b, const int32_t *blocks_per_stream_host, int32_t has_clean_input,
                                               AecmLaunchDescription *out, int64_t *items, int64_t *sum_blocks, int32_t *max_blocks);
/* Diagnostics: the plan a ragged pipelined launch runs by, whether or not the launch rule would pick the form.  slot_stream[4 x
 * *workgroups] (capacity entries available; 4 x 4 x compute units always suffice under the default policy): the stream in each of
 * the four slots of each workgroup, -1 = empty.  Workgroups i, i + compute units, ... share a compute unit.  Streams of length 0
 * appear nowhere.  AECM_BAD_PARAMETER_ERROR: no stream has blocks, more of them have than pipelined_max_streams, a negative length,
 * or too small a capacity. */
int32_t WebRtcAecmBatch_RaggedPipePlan(const AecmLaunchPolicy *policy, int32_t compute_units, int32_t num_streams,
                                       const int32_t *blocks_per_stream_host, int32_t *slot_stream, int32_t capacity, int32_t *workgroups);
/* Diagnostics: the plan a ragged chunk-queue launch with chunks of chunk_blocks blocks runs by.  order[num_streams]: the streams by
 * length, longest first (equal lengths in stream order); *num_chunks = ceil(longest / chunk_blocks); first_item[*num_chunks + 1]
 * (first_item_capacity entries available): the items of chunk c are the numbers first_item[c] .. first_item[c + 1], item
 * first_item[c] + r being (chunk c, stream order[r]) -- the streams with more than c * chunk_blocks blocks. */
int32_t WebRtcAecmBatch_RaggedPlan(int32_t num_streams, const int32_t *blocks_per_stream_host, int32_t chunk_blocks, int32_t *order,
                                   int32_t *first_item, int32_t first_item_capacity, int32_t *num_chunks);
int32_t WebRtcAecmSessions_DescribeTick(int32_t num_sessions, int32_t compute_units, AecmLaunchDescription *out);
/* The same for a tick of an object of num_sessions sessions in which live_sessions call and the others carry AECM_SESSION_IDLE:
 * the tick launch's grid and rounds_x1000 are by the live count (0 workgroups when nobody calls); live_sessions == num_sessions
 * answers exactly as DescribeTick.  AECM_BAD_PARAMETER_ERROR for live_sessions outside [0, num_sessions]. */
int32_t WebRtcAecmSessions_DescribeTickLive(int32_t num_sessions, int32_t live_sessions, int32_t compute_units, AecmLaunchDescription *out);
/* The HIP device WebRtcAecm_Create (which has no device argument) puts its sessions on from now on; process-wide, default 0. */
int32_t WebRtcAecm_SetDefaultDevice(int32_t device_id);

/* Device self test of the wave primitives on device_id; failures[0..7] must all be 0 afterwards
 * (see webrtc_aecm_amd/csrc/aecm_kernels.h).  exhaustive != 0 checks floor-sqrt on all of [0, 2^31). */
int32_t WebRtcAecmBatch_SelfTest(int32_t device_id, int32_t exhaustive, uint64_t failures[8]);

/* Precondition audit (diagnostics).  The block kernel replaces some of the reference's arithmetic by cheaper
 * instructions where an operand range is provable (24-bit multiplies, int16 narrowings that are the identity).
 * libaecm_mi355x_checked.so is the same library built with -DAECM_CHECKED: its kernels verify every such claim at
 * run time and count violations -- counters[0] 24-bit multiply operands, counters[1] int16 narrowings -- while still
 * producing exact results.  The shipped library carries no checks and returns AECM_UNSUPPORTED_FUNCTION_ERROR. */
int32_t WebRtcAecmBatch_GetCheckCounters(int32_t device_id, uint64_t counters[2], int32_t reset);

/* Diagnostics: `count` independent 128-point transforms of the block kernel's own FFT code, on host
 * data in natural order (transform k: data[k*256 .. +128) = re, [.. +256) = im, in place).  variant 0 =
 * forward of real input (im ignored), 1 = forward complex, 2 = inverse (reference
 * WebRtcSpl_ComplexBitReverse + ComplexFFT / ComplexIFFT, aecm/complex_fft.c:181-491, mode 1);
 * scales[k] receives the inverse transform's return value.  Outputs the block path never consumes
 * come back as 0: forward -> im of bins >= 64, inverse -> im.  kernel_variant as in SetKernelVariant. */
int32_t WebRtcAecmBatch_DebugFft128(int32_t device_id, int16_t *data_host, int32_t *scales_host, int32_t variant,
                                    int32_t kernel_variant, int32_t count);

/* Diagnostics, the ops probe: one fixed-point primitive of the block DSP (an entry of webrtc_aecm_amd/csrc/aecm_ops_table.inc:
 * the functions of aecm_ops.h and the plain-integer helpers of aecm_wave.h), alone, on n operand tuples (a[i], b[i], c[i]) -- the
 * device definition of the function, as the kernels compile it, for comparison with its host definition.  All pointers are host
 * memory, n words each; b and c may be NULL where the op takes fewer operands.
 *   form 0  lane form: thread i evaluates tuple i, operands in vector registers.
 *   form 1  uniform form: wave i evaluates tuple i with wave-uniform operands (the compiler may keep it on the scalar unit);
 *           nonuniform[i] (may be NULL) is non-zero if a lane's result differed from lane 0's.  Lane form writes zeros there.
 * For the ops whose last operand is wave-uniform by contract (dot2_i16_uc, mad16_lo_uc, mad16_hi_uc) lane form takes c of the
 * first tuple of every aligned group of 64: give such groups one value.
 * The shipped library ASSUMES each primitive's precondition (24-bit operands of mul24, ...): tuples outside it have no defined
 * result there; the audit twin counts them (GetCheckCounters) and computes the exact result.
 * AECM_BAD_PARAMETER_ERROR, and nothing is launched, for an op outside [0, DebugOpsCount()), a form other than 0 / 1, n <= 0,
 * n > 2^20, or a NULL pointer the op's operand count needs.  DebugOpName: the entry's name, NULL outside the table. */
int32_t WebRtcAecmBatch_DebugOps(int32_t device_id, int32_t op, int32_t form, const int32_t *a, const int32_t *b, const int32_t *c,
                                 int32_t *out, int32_t *nonuniform, int32_t n);
int32_t WebRtcAecmBatch_DebugOpsCount(void);
const char *WebRtcAecmBatch_DebugOpName(int32_t op);

/* Name, CU count and clock of the device the library would use (diagnostics). */
int32_t WebRtcAecmBatch_DeviceInfo(int32_t device_id, char *name, size_t name_len, int32_t *compute_units,
                                   int32_t *clock_khz);
/* Its PCI bus id ("0000:05:00.0"; bus_id_len >= 13): which physical GPU a rank of a multi-GPU run really had. */
int32_t WebRtcAecmBatch_DevicePciBusId(int32_t device_id, char *bus_id, size_t bus_id_len);

#ifdef __cplusplus
}
#endif
#endif /* AECM_MI355X_BATCH_H_ */
