// extern "C" surface of libaecm_mi355x.so: the reference's session ABI (include/echo_control_mobile.h)
// and the batch extension (include/aecm_batch.h).  Plain pointers and sizes only.
#include <hip/hip_runtime_api.h>
#include <stddef.h>
#include <string.h>

#include <new>
#include <vector>

#include "../../include/aecm_batch.h"
#include "../../include/echo_control_mobile.h"
#include "aecm_engine.h"
#include "aecm_session.h"
#include "aecm_sessions.h"

using aecm::BatchEngine;
using aecm::Session;

struct AecmBatch {
    BatchEngine *engine;
};

struct AecmSessions {
    aecm::SessionBatch *batch;
};

extern "C" {

// ---- session ABI (reference aecm/echo_control_mobile.h:46-202) -----------------------------------

void *WebRtcAecm_Create(void) { return Session::Create(); }

void WebRtcAecm_Free(void *inst) { delete static_cast<Session *>(inst); }

int32_t WebRtcAecm_Init(void *inst, int32_t sampFreq) {
    if (inst == nullptr) return -1;
    return static_cast<Session *>(inst)->Init(sampFreq);
}

int32_t WebRtcAecm_GetBufferFarendError(void *inst, const int16_t *farend, size_t nrOfSamples) {
    if (inst == nullptr) return -1;
    return static_cast<Session *>(inst)->BufferFarendError(farend, nrOfSamples);
}

int32_t WebRtcAecm_BufferFarend(void *inst, const int16_t *farend, size_t nrOfSamples) {
    if (inst == nullptr) return -1;
    return static_cast<Session *>(inst)->BufferFarend(farend, nrOfSamples);
}

int32_t WebRtcAecm_Process(void *inst, const int16_t *nearendNoisy, const int16_t *nearendClean, int16_t *out,
                           size_t nrOfSamples, int16_t msInSndCardBuf) {
    if (inst == nullptr) return -1;
    return static_cast<Session *>(inst)->Process(nearendNoisy, nearendClean, out, nrOfSamples, msInSndCardBuf);
}

int32_t WebRtcAecm_set_config(void *inst, AecmConfig config) {
    if (inst == nullptr) return -1;
    return static_cast<Session *>(inst)->SetConfig(config.cngMode, config.echoMode);
}

int32_t WebRtcAecm_InitEchoPath(void *inst, const void *echo_path, size_t size_bytes) {
    if (inst == nullptr) return -1;
    return static_cast<Session *>(inst)->InitEchoPath(echo_path, size_bytes);
}

int32_t WebRtcAecm_GetEchoPath(void *inst, void *echo_path, size_t size_bytes) {
    if (inst == nullptr) return -1;
    return static_cast<Session *>(inst)->GetEchoPath(echo_path, size_bytes);
}

size_t WebRtcAecm_echo_path_size_bytes(void) { return aecm::kBins * sizeof(int16_t); }

// ---- batch extension -------------------------------------------------------------------------------

AecmBatch *WebRtcAecmBatch_Create(int32_t num_streams, int32_t device_id) {
    BatchEngine *e = BatchEngine::Create(num_streams, device_id);
    if (!e) return nullptr;
    AecmBatch *b = new (std::nothrow) AecmBatch{e};
    if (!b) delete e;
    return b;
}

void WebRtcAecmBatch_Free(AecmBatch *b) {
    if (!b) return;
    delete b->engine;
    delete b;
}

int32_t WebRtcAecmBatch_num_streams(const AecmBatch *b) { return b ? b->engine->num_streams() : -1; }

int32_t WebRtcAecmBatch_Init(AecmBatch *b, int32_t sampFreq) {
    if (!b) return -1;
    if (sampFreq != 8000 && sampFreq != 16000) return AECM_BAD_PARAMETER_ERROR;
    return b->engine->Init(sampFreq) ? 0 : AECM_UNSPECIFIED_ERROR;
}

static int32_t CheckRange(const AecmBatch *b, int32_t first, int32_t *count) {
    if (!b) return -1;
    if (!b->engine->initialized()) return AECM_UNINITIALIZED_ERROR;
    if (*count < 0) *count = b->engine->num_streams() - first;
    if (first < 0 || *count < 0 || first + *count > b->engine->num_streams()) return AECM_BAD_PARAMETER_ERROR;
    return 0;
}

int32_t WebRtcAecmBatch_set_config(AecmBatch *b, AecmConfig config, int32_t first, int32_t count) {
    if (int32_t rc = CheckRange(b, first, &count)) return rc;
    if (config.cngMode != AecmFalse && config.cngMode != AecmTrue) return AECM_BAD_PARAMETER_ERROR;
    if (config.echoMode < 0 || config.echoMode > 4) return AECM_BAD_PARAMETER_ERROR;
    return b->engine->SetConfig(config.cngMode, config.echoMode, first, count) ? 0 : AECM_UNSPECIFIED_ERROR;
}

int32_t WebRtcAecmBatch_Control(AecmBatch *b, int32_t fixed_delay, int32_t nlp_flag, int32_t first, int32_t count) {
    if (int32_t rc = CheckRange(b, first, &count)) return rc;
    // the reference uses fixedDelay unchecked as a far-history offset (aecm_core.cc:157-172, MAX_DELAY = 100 slots)
    // and narrows both arguments to int16_t: validated as the values the core will hold -- anything outside
    // [-32768, kHistory) is refused (a large negative int32 would otherwise wrap into range or beyond it)
    if (fixed_delay < -32768 || fixed_delay >= aecm::kHistory) return AECM_BAD_PARAMETER_ERROR;
    if (nlp_flag < -32768 || nlp_flag > 32767) return AECM_BAD_PARAMETER_ERROR;
    return b->engine->Control(fixed_delay, nlp_flag, first, count) ? 0 : AECM_UNSPECIFIED_ERROR;
}

static int32_t CheckIo(const AecmBatch *b, const void *far_p, const void *near_p, const void *out_p, int32_t num_blocks) {
    if (!b) return -1;
    if (!b->engine->initialized()) return AECM_UNINITIALIZED_ERROR;
    if (!far_p || !near_p || !out_p) return AECM_NULL_POINTER_ERROR;
    if (num_blocks < 0) return AECM_BAD_PARAMETER_ERROR;
    return 0;
}

int32_t WebRtcAecmBatch_ProcessBlocks(AecmBatch *b, const int16_t *far_dev, const int16_t *near_dev,
                                      const int16_t *near_clean_dev, int16_t *out_dev, int64_t stream_stride,
                                      int64_t block_stride, int32_t num_blocks) {
    if (int32_t rc = CheckIo(b, far_dev, near_dev, out_dev, num_blocks)) return rc;
    if (num_blocks == 0) return 0;
    aecm::IoView io{far_dev, near_dev, near_clean_dev, out_dev, stream_stride, block_stride};
    return b->engine->ProcessBlocks(io, num_blocks) ? 0 : AECM_UNSPECIFIED_ERROR;
}

int32_t WebRtcAecmBatch_ProcessBlocksHost(AecmBatch *b, const int16_t *far_host, const int16_t *near_host,
                                          const int16_t *near_clean_host, int16_t *out_host, int64_t stream_stride,
                                          int64_t block_stride, int32_t num_blocks) {
    if (int32_t rc = CheckIo(b, far_host, near_host, out_host, num_blocks)) return rc;
    if (b->engine->block_trace_attached()) return AECM_UNSUPPORTED_FUNCTION_ERROR;      // the block trace is for device-pointer launches
    if (num_blocks == 0) return 0;
    aecm::IoView io{far_host, near_host, near_clean_host, out_host, stream_stride, block_stride};
    return b->engine->ProcessBlocksHost(io, num_blocks) ? 0 : AECM_UNSPECIFIED_ERROR;
}

static int32_t ProcessRecordings(AecmBatch *b, const int16_t *far_p, const int16_t *near_p, const int16_t *clean_p,
                                 int16_t *out_p, int64_t stream_stride, int32_t samples_per_call, int32_t num_calls, int16_t ms,
                                 bool host) {
    if (int32_t rc = CheckIo(b, far_p, near_p, out_p, num_calls)) return rc;
    if (b->engine->block_trace_attached()) return AECM_UNSUPPORTED_FUNCTION_ERROR;      // (a recording's call-to-block map is not block-aligned)
    if (samples_per_call != 80 && samples_per_call != 160) return AECM_BAD_PARAMETER_ERROR;
    if (stream_stride < (int64_t)samples_per_call * num_calls) return AECM_BAD_PARAMETER_ERROR;
    if (num_calls == 0) return 0;
    int32_t rc = 0;
    if (!b->engine->ProcessRecordings(far_p, near_p, clean_p, out_p, stream_stride, samples_per_call, num_calls, ms, host, &rc))
        return AECM_UNSPECIFIED_ERROR;
    return rc;
}

int32_t WebRtcAecmBatch_ProcessRecordings(AecmBatch *b, const int16_t *far_dev, const int16_t *near_dev,
                                          const int16_t *near_clean_dev, int16_t *out_dev, int64_t stream_stride,
                                          int32_t samples_per_call, int32_t num_calls, int16_t msInSndCardBuf) {
    return ProcessRecordings(b, far_dev, near_dev, near_clean_dev, out_dev, stream_stride, samples_per_call, num_calls,
                             msInSndCardBuf, false);
}

int32_t WebRtcAecmBatch_ProcessRecordingsHost(AecmBatch *b, const int16_t *far_host, const int16_t *near_host,
                                              const int16_t *near_clean_host, int16_t *out_host, int64_t stream_stride,
                                              int32_t samples_per_call, int32_t num_calls, int16_t msInSndCardBuf) {
    return ProcessRecordings(b, far_host, near_host, near_clean_host, out_host, stream_stride, samples_per_call, num_calls,
                             msInSndCardBuf, true);
}

// ---- ragged batches: one length per stream ---------------------------------------------------------------
static int32_t CheckLengths(const AecmBatch *b, const int32_t *lens, int32_t limit) {
    if (!lens) return AECM_NULL_POINTER_ERROR;
    for (int32_t s = 0; s < b->engine->num_streams(); ++s)
        if (lens[s] < 0 || lens[s] > limit) return AECM_BAD_PARAMETER_ERROR;
    return 0;
}

int32_t WebRtcAecmBatch_ProcessBlocksRagged(AecmBatch *b, const int16_t *far_dev, const int16_t *near_dev, const int16_t *near_clean_dev,
                                            int16_t *out_dev, int64_t stream_stride, int64_t block_stride, int32_t num_blocks,
                                            const int32_t *blocks_per_stream_host) {
    if (int32_t rc = CheckIo(b, far_dev, near_dev, out_dev, num_blocks)) return rc;
    if (int32_t rc = CheckLengths(b, blocks_per_stream_host, num_blocks)) return rc;
    if (num_blocks == 0) return 0;
    aecm::IoView io{far_dev, near_dev, near_clean_dev, out_dev, stream_stride, block_stride};
    return b->engine->ProcessBlocksRagged(io, num_blocks, blocks_per_stream_host);
}

int32_t WebRtcAecmBatch_ProcessBlocksRaggedHost(AecmBatch *b, const int16_t *far_host, const int16_t *near_host, const int16_t *near_clean_host,
                                                int16_t *out_host, int64_t stream_stride, int64_t block_stride, int32_t num_blocks,
                                                const int32_t *blocks_per_stream_host) {
    if (int32_t rc = CheckIo(b, far_host, near_host, out_host, num_blocks)) return rc;
    if (b->engine->block_trace_attached()) return AECM_UNSUPPORTED_FUNCTION_ERROR;
    if (int32_t rc = CheckLengths(b, blocks_per_stream_host, num_blocks)) return rc;
    if (num_blocks == 0) return 0;
    aecm::IoView io{far_host, near_host, near_clean_host, out_host, stream_stride, block_stride};
    return b->engine->ProcessBlocksRaggedHost(io, num_blocks, blocks_per_stream_host);
}

static int32_t ProcessRecordingsRagged(AecmBatch *b, const int16_t *far_p, const int16_t *near_p, const int16_t *clean_p, int16_t *out_p,
                                       int64_t stream_stride, int32_t samples_per_call, int32_t num_calls, const int32_t *calls, int16_t ms,
                                       int32_t *codes, bool host) {
    if (int32_t rc = CheckIo(b, far_p, near_p, out_p, num_calls)) return rc;
    if (b->engine->block_trace_attached()) return AECM_UNSUPPORTED_FUNCTION_ERROR;      // (a recording's call-to-block map is not block-aligned)
    if (samples_per_call != 80 && samples_per_call != 160) return AECM_BAD_PARAMETER_ERROR;
    if (stream_stride < (int64_t)samples_per_call * num_calls) return AECM_BAD_PARAMETER_ERROR;
    if (int32_t rc = CheckLengths(b, calls, num_calls)) return rc;
    if (num_calls == 0) {
        for (int32_t s = 0; codes && s < b->engine->num_streams(); ++s) codes[s] = 0;
        return 0;
    }
    int32_t rc = 0;
    if (!b->engine->ProcessRecordingsRagged(far_p, near_p, clean_p, out_p, stream_stride, samples_per_call, num_calls, calls, ms, host, &rc, codes))
        return AECM_UNSPECIFIED_ERROR;
    return rc;
}

int32_t WebRtcAecmBatch_ProcessRecordingsRagged(AecmBatch *b, const int16_t *far_dev, const int16_t *near_dev, const int16_t *near_clean_dev,
                                                int16_t *out_dev, int64_t stream_stride, int32_t samples_per_call, int32_t num_calls,
                                                const int32_t *calls_per_stream_host, int16_t msInSndCardBuf, int32_t *codes_host) {
    return ProcessRecordingsRagged(b, far_dev, near_dev, near_clean_dev, out_dev, stream_stride, samples_per_call, num_calls,
                                   calls_per_stream_host, msInSndCardBuf, codes_host, false);
}

int32_t WebRtcAecmBatch_ProcessRecordingsRaggedHost(AecmBatch *b, const int16_t *far_host, const int16_t *near_host, const int16_t *near_clean_host,
                                                    int16_t *out_host, int64_t stream_stride, int32_t samples_per_call, int32_t num_calls,
                                                    const int32_t *calls_per_stream_host, int16_t msInSndCardBuf, int32_t *codes_host) {
    return ProcessRecordingsRagged(b, far_host, near_host, near_clean_host, out_host, stream_stride, samples_per_call, num_calls,
                                   calls_per_stream_host, msInSndCardBuf, codes_host, true);
}

int32_t WebRtcAecmBatch_Synchronize(AecmBatch *b) {
    if (!b) return -1;
    return b->engine->Synchronize() ? 0 : AECM_UNSPECIFIED_ERROR;
}

int32_t WebRtcAecmBatch_GetLastLaunchMs(AecmBatch *b, float *ms) {
    if (!b) return -1;
    if (!ms) return AECM_NULL_POINTER_ERROR;
    return b->engine->LastLaunchMs(ms) ? 0 : AECM_UNSPECIFIED_ERROR;
}

int32_t WebRtcAecmBatch_GetTimers(AecmBatch *b, double *total_ms, int64_t *launches) {
    if (!b) return -1;
    if (!total_ms || !launches) return AECM_NULL_POINTER_ERROR;
    return b->engine->Timers(total_ms, launches) ? 0 : AECM_UNSPECIFIED_ERROR;
}

int32_t WebRtcAecmBatch_ResetTimers(AecmBatch *b) {
    if (!b) return -1;
    b->engine->ResetTimers();
    return 0;
}

int32_t WebRtcAecmBatch_InitEchoPath(AecmBatch *b, int32_t stream, const void *echo_path, size_t size_bytes) {
    if (!b) return -1;
    if (!echo_path) return AECM_NULL_POINTER_ERROR;
    if (size_bytes != aecm::kBins * sizeof(int16_t)) return AECM_BAD_PARAMETER_ERROR;
    if (!b->engine->initialized()) return AECM_UNINITIALIZED_ERROR;
    if (stream < 0 || stream >= b->engine->num_streams()) return AECM_BAD_PARAMETER_ERROR;
    int16_t tmp[aecm::kBins];
    memcpy(tmp, echo_path, sizeof tmp);
    return b->engine->SetEchoPath(stream, tmp) ? 0 : AECM_UNSPECIFIED_ERROR;
}

int32_t WebRtcAecmBatch_GetEchoPath(AecmBatch *b, int32_t stream, void *echo_path, size_t size_bytes) {
    if (!b) return -1;
    if (!echo_path) return AECM_NULL_POINTER_ERROR;
    if (size_bytes != aecm::kBins * sizeof(int16_t)) return AECM_BAD_PARAMETER_ERROR;
    if (!b->engine->initialized()) return AECM_UNINITIALIZED_ERROR;
    if (stream < 0 || stream >= b->engine->num_streams()) return AECM_BAD_PARAMETER_ERROR;
    int16_t tmp[aecm::kBins];
    if (!b->engine->GetEchoPath(stream, tmp)) return AECM_UNSPECIFIED_ERROR;
    memcpy(echo_path, tmp, sizeof tmp);
    return 0;
}

size_t WebRtcAecmBatch_state_size_bytes(void) { return BatchEngine::kStateBytes; }

static int32_t CheckState(const AecmBatch *b, int32_t stream, const void *state, size_t size_bytes) {
    if (!b) return -1;
    if (!state) return AECM_NULL_POINTER_ERROR;
    if (size_bytes != BatchEngine::kStateBytes) return AECM_BAD_PARAMETER_ERROR;
    if (!b->engine->initialized()) return AECM_UNINITIALIZED_ERROR;
    if (stream < 0 || stream >= b->engine->num_streams()) return AECM_BAD_PARAMETER_ERROR;
    return 0;
}

int32_t WebRtcAecmBatch_ExportState(AecmBatch *b, int32_t stream, void *state, size_t size_bytes) {
    if (int32_t rc = CheckState(b, stream, state, size_bytes)) return rc;
    return b->engine->ExportState(stream, state) ? 0 : AECM_UNSPECIFIED_ERROR;
}

int32_t WebRtcAecmBatch_ImportState(AecmBatch *b, int32_t stream, const void *state, size_t size_bytes) {
    if (int32_t rc = CheckState(b, stream, state, size_bytes)) return rc;
    return b->engine->ImportState(stream, state);
}

static int32_t CheckStates(const AecmBatch *b, int32_t first, int32_t count, const void *states, size_t size_bytes) {
    if (!b) return -1;
    if (!states) return AECM_NULL_POINTER_ERROR;
    if (!b->engine->initialized()) return AECM_UNINITIALIZED_ERROR;
    if (first < 0 || count < 0 || count > b->engine->num_streams() - first) return AECM_BAD_PARAMETER_ERROR;
    if (size_bytes != (size_t)count * BatchEngine::kStateBytes) return AECM_BAD_PARAMETER_ERROR;
    return 0;
}

int32_t WebRtcAecmBatch_ExportStates(AecmBatch *b, int32_t first, int32_t count, void *states_host, size_t size_bytes) {
    if (int32_t rc = CheckStates(b, first, count, states_host, size_bytes)) return rc;
    return b->engine->ExportStates(first, count, states_host, false) ? 0 : AECM_UNSPECIFIED_ERROR;
}

int32_t WebRtcAecmBatch_ImportStates(AecmBatch *b, int32_t first, int32_t count, const void *states_host, size_t size_bytes) {
    if (int32_t rc = CheckStates(b, first, count, states_host, size_bytes)) return rc;
    return b->engine->ImportStates(first, count, states_host, false);
}

int32_t WebRtcAecmBatch_ExportStatesDevice(AecmBatch *b, int32_t first, int32_t count, void *states_dev, size_t size_bytes) {
    if (int32_t rc = CheckStates(b, first, count, states_dev, size_bytes)) return rc;
    if (reinterpret_cast<uintptr_t>(states_dev) & 3) return AECM_BAD_PARAMETER_ERROR;        // the kernels move 32-bit words
    return b->engine->ExportStates(first, count, states_dev, true) ? 0 : AECM_UNSPECIFIED_ERROR;
}

int32_t WebRtcAecmBatch_ImportStatesDevice(AecmBatch *b, int32_t first, int32_t count, const void *states_dev, size_t size_bytes) {
    if (int32_t rc = CheckStates(b, first, count, states_dev, size_bytes)) return rc;
    return b->engine->ImportStates(first, count, states_dev, true);
}

int32_t WebRtcAecmBatch_GetDigest(AecmBatch *b, int32_t stream, uint32_t digest[AECM_BATCH_DIGEST_WORDS]) {
    if (!b) return -1;
    if (!digest) return AECM_NULL_POINTER_ERROR;
    if (!b->engine->initialized()) return AECM_UNINITIALIZED_ERROR;
    if (stream < 0 || stream >= b->engine->num_streams()) return AECM_BAD_PARAMETER_ERROR;
    return b->engine->Digest(stream, digest) ? 0 : AECM_UNSPECIFIED_ERROR;
}

static_assert(sizeof(AecmBlockTrace) == aecm::kTraceWords * sizeof(uint32_t), "the block trace record is eight words");
size_t WebRtcAecmBatch_block_trace_size_bytes(void) { return sizeof(AecmBlockTrace); }

int32_t WebRtcAecmBatch_SetBlockTrace(AecmBatch *b, void *trace_dev, int64_t stream_stride, int64_t block_stride) {
    if (!b) return AECM_BAD_PARAMETER_ERROR;
    return b->engine->SetBlockTrace(trace_dev, stream_stride, block_stride);
}

int32_t WebRtcAecmBatch_SetKernelVariant(AecmBatch *b, int32_t variant) {
    if (!b) return -1;
    if (variant != AECM_KERNEL_SAFE && variant != AECM_KERNEL_FAST) return AECM_BAD_PARAMETER_ERROR;
    b->engine->set_variant(variant);
    return 0;
}

int32_t WebRtcAecmBatch_SetLaunchChunking(AecmBatch *b, int32_t chunk_blocks, int32_t min_streams) {
    if (!b) return -1;
    if (chunk_blocks < 0 || chunk_blocks > (1 << 20)) return AECM_BAD_PARAMETER_ERROR;
    b->engine->set_queue_chunk(chunk_blocks, min_streams);
    return 0;
}

int32_t WebRtcAecmBatch_SetLaunchPipelining(AecmBatch *b, int32_t min_streams) {
    if (!b) return -1;
    b->engine->set_pipelined_min_streams(min_streams);
    return 0;
}

int32_t WebRtcAecmBatch_SetRaggedPipelining(AecmBatch *b, int32_t enable) {
    if (!b) return AECM_BAD_PARAMETER_ERROR;
    b->engine->set_ragged_pipelining(enable != 0);
    return 0;
}

int32_t WebRtcAecmBatch_SetCleanPipelining(AecmBatch *b, int32_t enable) {
    if (!b) return AECM_BAD_PARAMETER_ERROR;
    b->engine->set_clean_pipelining(enable != 0);
    return 0;
}

int32_t WebRtcAecmBatch_SetRaggedCleanPipelining(AecmBatch *b, int32_t enable) {
    if (!b) return AECM_BAD_PARAMETER_ERROR;
    b->engine->set_ragged_clean_pipelining(enable != 0);
    return 0;
}

int32_t WebRtcAecmBatch_DescribeLaunch(const AecmBatch *b, int32_t num_blocks, int32_t has_clean_input, int32_t *chunk_blocks) {
    if (!b) return -1;
    return b->engine->DescribeLaunch(num_blocks, has_clean_input != 0, chunk_blocks);
}

int32_t WebRtcAecmBatch_DescribeLaunchFor(int32_t num_streams, int32_t compute_units, int32_t num_blocks, int32_t has_clean_input,
                                          int32_t *chunk_blocks) {
    if (num_streams <= 0 || compute_units <= 0 || num_blocks <= 0) return -1;
    const aecm::LaunchPolicy p = aecm::DefaultLaunchPolicy(compute_units);
    const aecm::LaunchDescription d = aecm::DescribePlan(p, aecm::PlanLaunch(p, aecm::LaunchSwitches(), num_streams, num_blocks, has_clean_input != 0));
    if (chunk_blocks) *chunk_blocks = d.detail();
    return d.form;
}

// ---- the launch policy as one value (aecm_engine.h: LaunchPolicy) --------------------------------------
static void PolicyToAbi(const aecm::LaunchPolicy &p, AecmLaunchPolicy *o) {
    *o = AecmLaunchPolicy{(int32_t)sizeof(AecmLaunchPolicy), p.compute_units, p.queue_chunk_blocks, p.queue_chunk_explicit ? 1 : 0, p.queue_min_streams,
                          p.pipelined_min_streams, p.pipelined_min_blocks, p.pipelined_max_streams, p.resident_waves, p.rotation_stream_limit,
                          p.pipe.tail_waves, p.pipe.front_waves, p.pipe.raw, p.pipe.delay_waves, p.pipe.gain_waves, p.pipe.spread, p.pipe.wgs_per_cu, p.pipe.rot, p.pipe.prio};
}
static aecm::LaunchPolicy PolicyFromAbi(const AecmLaunchPolicy &a) {
    aecm::LaunchPolicy p;
    p.compute_units = a.compute_units;
    p.queue_chunk_blocks = a.queue_chunk_blocks;
    p.queue_chunk_explicit = a.queue_chunk_explicit != 0;
    p.queue_min_streams = a.queue_min_streams;
    p.pipelined_min_streams = a.pipelined_min_streams > 0 ? a.pipelined_min_streams : 0x7fffffff;
    p.pipelined_min_blocks = a.pipelined_min_blocks;
    p.pipelined_max_streams = a.pipelined_max_streams;
    p.resident_waves = a.resident_waves;
    p.rotation_stream_limit = a.rotation_stream_limit;
    p.pipe.tail_waves = a.pipe_tail_waves;
    p.pipe.front_waves = a.pipe_front_waves;
    p.pipe.raw = a.pipe_raw;
    p.pipe.delay_waves = a.pipe_delay_waves;
    p.pipe.gain_waves = a.pipe_gain_waves;
    p.pipe.spread = a.pipe_spread;
    p.pipe.wgs_per_cu = a.pipe_wgs_per_cu;
    p.pipe.rot = a.pipe_rot;
    p.pipe.prio = a.pipe_prio;
    return p;
}

int32_t WebRtcAecmBatch_DefaultLaunchPolicy(int32_t compute_units, AecmLaunchPolicy *policy) {
    if (!policy) return AECM_NULL_POINTER_ERROR;
    if (compute_units <= 0) return AECM_BAD_PARAMETER_ERROR;
    PolicyToAbi(aecm::DefaultLaunchPolicy(compute_units), policy);
    return 0;
}

int32_t WebRtcAecmBatch_GetLaunchPolicy(const AecmBatch *b, AecmLaunchPolicy *policy) {
    if (!b) return -1;
    if (!policy) return AECM_NULL_POINTER_ERROR;
    PolicyToAbi(b->engine->launch_policy(), policy);
    return 0;
}

int32_t WebRtcAecmBatch_SetLaunchPolicy(AecmBatch *b, const AecmLaunchPolicy *policy) {
    if (!b) return -1;
    if (!policy) return AECM_NULL_POINTER_ERROR;
    if (policy->struct_size != (int32_t)sizeof(AecmLaunchPolicy)) return AECM_BAD_PARAMETER_ERROR;
    return b->engine->set_launch_policy(PolicyFromAbi(*policy)) ? 0 : AECM_BAD_PARAMETER_ERROR;
}

static void DescriptionToAbi(const aecm::LaunchDescription &d, AecmLaunchDescription *o) {
    *o = AecmLaunchDescription{d.form, d.chunk_blocks, d.shape, d.workgroups, d.waves_per_workgroup, d.workgroups_per_cu, d.rounds_x1000, d.cu_load_evenness_x1000};
}

int32_t WebRtcAecmBatch_DescribeLaunchDetail(const AecmLaunchPolicy *policy, int32_t compute_units, int32_t num_streams, int32_t num_blocks,
                                             int32_t has_clean_input, AecmLaunchDescription *out) {
    return WebRtcAecmBatch_DescribeLaunchDetailEx(policy, compute_units, num_streams, num_blocks, has_clean_input, 0, out);
}

// The policy a planning call runs by: the caller's if it is a valid one, else the default one of compute_units; 0 or the error code.
static int32_t ResolvePolicy(const AecmLaunchPolicy *policy, int32_t compute_units, aecm::LaunchPolicy *p) {
    if (policy) {
        if (policy->struct_size != (int32_t)sizeof(AecmLaunchPolicy)) return AECM_BAD_PARAMETER_ERROR;
        *p = PolicyFromAbi(*policy);
        if (!aecm::LaunchPolicyValid(*p) || p->compute_units <= 0) return AECM_BAD_PARAMETER_ERROR;
    } else {
        if (compute_units <= 0) return AECM_BAD_PARAMETER_ERROR;
        *p = aecm::DefaultLaunchPolicy(compute_units);
    }
    return 0;
}

// The longest of the lengths; 0 or AECM_BAD_PARAMETER_ERROR (a negative length).
static int32_t LongestLength(const int32_t *lens, int32_t num_streams, int32_t *longest) {
    *longest = 0;
    for (int32_t s = 0; s < num_streams; ++s) {
        if (lens[s] < 0) return AECM_BAD_PARAMETER_ERROR;
        if (lens[s] > *longest) *longest = lens[s];
    }
    return 0;
}

// What the ragged describing calls return: the description and (each may be null) the plan's sums.
static int32_t RaggedDescriptionToAbi(const aecm::LaunchDescription &d, const aecm::LaunchPlan &plan, AecmLaunchDescription *out, int64_t *items,
                                      int64_t *sum_blocks, int32_t *max_blocks) {
    if (d.form < 0) return AECM_BAD_PARAMETER_ERROR;
    DescriptionToAbi(d, out);
    if (items) *items = d.form == 2 ? plan.ragged.items : 0;
    if (sum_blocks) *sum_blocks = plan.ragged.sum_blocks;
    if (max_blocks) *max_blocks = plan.ragged.max_blocks;
    return 0;
}

int32_t WebRtcAecmBatch_DescribeLaunchDetailEx(const AecmLaunchPolicy *policy, int32_t compute_units, int32_t num_streams, int32_t num_blocks,
                                               int32_t has_clean_input, int32_t clean_pipelining, AecmLaunchDescription *out) {
    if (!out) return AECM_NULL_POINTER_ERROR;
    if (num_streams <= 0 || num_blocks <= 0) return AECM_BAD_PARAMETER_ERROR;
    aecm::LaunchPolicy p;
    if (const int32_t rc = ResolvePolicy(policy, compute_units, &p)) return rc;
    const aecm::LaunchSwitches sw{aecm::kVariantFast, false, clean_pipelining != 0};
    DescriptionToAbi(aecm::DescribePlan(p, aecm::PlanLaunch(p, sw, num_streams, num_blocks, has_clean_input != 0)), out);
    return 0;
}

int32_t WebRtcAecmBatch_DescribeTracedLaunch(const AecmLaunchPolicy *policy, int32_t compute_units, int32_t num_streams, int32_t num_blocks,
                                             int32_t has_clean_input, AecmLaunchDescription *out) {
    if (!out) return AECM_NULL_POINTER_ERROR;
    if (num_streams <= 0 || num_blocks <= 0) return AECM_BAD_PARAMETER_ERROR;
    aecm::LaunchPolicy p;
    if (const int32_t rc = ResolvePolicy(policy, compute_units, &p)) return rc;
    aecm::LaunchSwitches sw;
    sw.trace = true;
    DescriptionToAbi(aecm::DescribePlan(p, aecm::PlanLaunch(p, sw, num_streams, num_blocks, has_clean_input != 0)), out);
    return 0;
}

int32_t WebRtcAecmBatch_DescribeRaggedLaunchEx2(const AecmLaunchPolicy *policy, int32_t compute_units, int32_t num_streams,
                                                const int32_t *blocks_per_stream_host, int32_t has_clean_input, int32_t ragged_pipelining,
                                                int32_t ragged_clean_pipelining, AecmLaunchDescription *out, int64_t *items, int64_t *sum_blocks,
                                                int32_t *max_blocks) {
    if (!out || !blocks_per_stream_host) return AECM_NULL_POINTER_ERROR;
    if (num_streams <= 0) return AECM_BAD_PARAMETER_ERROR;
    aecm::LaunchPolicy p;
    int32_t longest = 0;
    if (const int32_t rc = ResolvePolicy(policy, compute_units, &p)) return rc;
    if (const int32_t rc = LongestLength(blocks_per_stream_host, num_streams, &longest)) return rc;
    const aecm::LaunchSwitches sw{aecm::kVariantFast, ragged_pipelining != 0, false, ragged_clean_pipelining != 0};
    const aecm::LaunchPlan plan = aecm::PlanRaggedLaunch(p, sw, num_streams, longest, blocks_per_stream_host, has_clean_input != 0);
    return RaggedDescriptionToAbi(aecm::DescribePlan(p, plan), plan, out, items, sum_blocks, max_blocks);
}

int32_t WebRtcAecmBatch_DescribeRaggedLaunchEx(const AecmLaunchPolicy *policy, int32_t compute_units, int32_t num_streams,
                                               const int32_t *blocks_per_stream_host, int32_t has_clean_input, int32_t ragged_pipelining,
                                               AecmLaunchDescription *out, int64_t *items, int64_t *sum_blocks, int32_t *max_blocks) {
    return WebRtcAecmBatch_DescribeRaggedLaunchEx2(policy, compute_units, num_streams, blocks_per_stream_host, has_clean_input, ragged_pipelining, 0, out,
                                                   items, sum_blocks, max_blocks);
}

int32_t WebRtcAecmBatch_DescribeRaggedLaunch(const AecmLaunchPolicy *policy, int32_t compute_units, int32_t num_streams,
                                             const int32_t *blocks_per_stream_host, int32_t has_clean_input, AecmLaunchDescription *out,
                                             int64_t *items, int64_t *sum_blocks, int32_t *max_blocks) {
    return WebRtcAecmBatch_DescribeRaggedLaunchEx(policy, compute_units, num_streams, blocks_per_stream_host, has_clean_input, 0, out, items,
                                                  sum_blocks, max_blocks);
}

int32_t WebRtcAecmBatch_DescribeRaggedLaunchOf(const AecmBatch *b, const int32_t *blocks_per_stream_host, int32_t has_clean_input,
                                               AecmLaunchDescription *out, int64_t *items, int64_t *sum_blocks, int32_t *max_blocks) {
    if (!b) return -1;
    if (!out || !blocks_per_stream_host) return AECM_NULL_POINTER_ERROR;
    int32_t longest = 0;
    if (const int32_t rc = LongestLength(blocks_per_stream_host, b->engine->num_streams(), &longest)) return rc;
    aecm::LaunchPlan plan;
    const aecm::LaunchDescription d = b->engine->DescribeRaggedLaunch(longest, blocks_per_stream_host, has_clean_input != 0, &plan);
    return RaggedDescriptionToAbi(d, plan, out, items, sum_blocks, max_blocks);
}

int32_t WebRtcAecmBatch_RaggedPipePlan(const AecmLaunchPolicy *policy, int32_t compute_units, int32_t num_streams,
                                       const int32_t *blocks_per_stream_host, int32_t *slot_stream, int32_t capacity, int32_t *workgroups) {
    if (!blocks_per_stream_host || !slot_stream || !workgroups) return AECM_NULL_POINTER_ERROR;
    if (num_streams <= 0) return AECM_BAD_PARAMETER_ERROR;
    aecm::LaunchPolicy p;
    int32_t longest = 0;
    if (const int32_t rc = ResolvePolicy(policy, compute_units, &p)) return rc;
    if (const int32_t rc = LongestLength(blocks_per_stream_host, num_streams, &longest)) return rc;
    int32_t live = 0;
    for (int32_t s = 0; s < num_streams; ++s) live += blocks_per_stream_host[s] > 0;
    if (live == 0 || live > p.pipelined_max_streams) return AECM_BAD_PARAMETER_ERROR;
    aecm::RaggedPipePlan plan;
    if (!aecm::BuildRaggedPipePlan(blocks_per_stream_host, num_streams, aecm::RaggedPipeShapeFor(live, longest, p.compute_units, p.pipe),
                                   p.compute_units, &plan))
        return AECM_BAD_PARAMETER_ERROR;
    if (capacity < 4 * plan.workgroups) return AECM_BAD_PARAMETER_ERROR;
    *workgroups = plan.workgroups;
    for (int32_t i = 0; i < 4 * plan.workgroups; ++i) slot_stream[i] = plan.slot_stream()[i];
    return 0;
}

int32_t WebRtcAecmBatch_RaggedPlan(int32_t num_streams, const int32_t *blocks_per_stream_host, int32_t chunk_blocks, int32_t *order,
                                   int32_t *first_item, int32_t first_item_capacity, int32_t *num_chunks) {
    if (!blocks_per_stream_host || !order || !first_item || !num_chunks) return AECM_NULL_POINTER_ERROR;
    if (num_streams <= 0 || chunk_blocks <= 0) return AECM_BAD_PARAMETER_ERROR;
    int32_t longest = 0;
    if (const int32_t rc = LongestLength(blocks_per_stream_host, num_streams, &longest)) return rc;
    aecm::RaggedPlan plan;
    if (!aecm::BuildRaggedPlan(blocks_per_stream_host, num_streams, longest, chunk_blocks, &plan)) return AECM_BAD_PARAMETER_ERROR;
    if (plan.items >= (int64_t(1) << 31) || first_item_capacity < plan.n_chunks + 1) return AECM_BAD_PARAMETER_ERROR;
    *num_chunks = plan.n_chunks;
    for (int32_t s = 0; s < num_streams; ++s) order[s] = (int32_t)plan.order()[s];
    for (int32_t c = 0; c <= plan.n_chunks; ++c) first_item[c] = (int32_t)plan.first_item()[c];
    return 0;
}

int32_t WebRtcAecmSessions_DescribeTick(int32_t num_sessions, int32_t compute_units, AecmLaunchDescription *out) {
    if (!out) return AECM_NULL_POINTER_ERROR;
    if (num_sessions <= 0 || compute_units <= 0) return AECM_BAD_PARAMETER_ERROR;
    DescriptionToAbi(aecm::DescribeTickLaunch(num_sessions, compute_units), out);
    return 0;
}

int32_t WebRtcAecmSessions_DescribeTickLive(int32_t num_sessions, int32_t live_sessions, int32_t compute_units, AecmLaunchDescription *out) {
    if (!out) return AECM_NULL_POINTER_ERROR;
    if (num_sessions <= 0 || compute_units <= 0 || live_sessions < 0 || live_sessions > num_sessions) return AECM_BAD_PARAMETER_ERROR;
    DescriptionToAbi(aecm::DescribeTickLaunchLive(num_sessions, live_sessions, compute_units), out);
    return 0;
}

int32_t WebRtcAecm_SetDefaultDevice(int32_t device_id) {
    if (device_id < 0) return AECM_BAD_PARAMETER_ERROR;
    Session::SetDefaultDevice(device_id);
    return 0;
}

// ---- streaming batch of sessions ---------------------------------------------------------------------

AecmSessions *WebRtcAecmSessions_Create(int32_t num_streams, int32_t device_id) {
    aecm::SessionBatch *sb = aecm::SessionBatch::Create(num_streams, device_id);
    if (!sb) return nullptr;
    return new AecmSessions{sb};
}

void WebRtcAecmSessions_Free(AecmSessions *s) {
    if (!s) return;
    delete s->batch;
    delete s;
}

int32_t WebRtcAecmSessions_Init(AecmSessions *s, int32_t sampFreq) { return s ? s->batch->Init(sampFreq) : -1; }

int32_t WebRtcAecmSessions_set_config(AecmSessions *s, AecmConfig config) {
    return s ? s->batch->SetConfig(config.cngMode, config.echoMode) : -1;
}

int32_t WebRtcAecmSessions_InitSession(AecmSessions *s, int32_t session) { return s ? s->batch->InitSession(session) : -1; }

size_t WebRtcAecmSessions_session_size_bytes(void) { return aecm::SessionBatch::kSessionBytes; }

int32_t WebRtcAecmSessions_ExportSession(AecmSessions *s, int32_t session, void *snapshot, size_t size_bytes) {
    if (!s) return -1;
    if (!snapshot) return AECM_NULL_POINTER_ERROR;
    if (size_bytes != aecm::SessionBatch::kSessionBytes) return AECM_BAD_PARAMETER_ERROR;
    return s->batch->ExportSession(session, snapshot);
}

int32_t WebRtcAecmSessions_ImportSession(AecmSessions *s, int32_t session, const void *snapshot, size_t size_bytes) {
    if (!s) return -1;
    if (!snapshot) return AECM_NULL_POINTER_ERROR;
    if (size_bytes != aecm::SessionBatch::kSessionBytes) return AECM_BAD_PARAMETER_ERROR;
    return s->batch->ImportSession(session, snapshot);
}

int32_t WebRtcAecmSessions_ImportSessionAnyRate(AecmSessions *s, int32_t session, const void *snapshot, size_t size_bytes) {
    if (!s) return -1;
    if (!snapshot) return AECM_NULL_POINTER_ERROR;
    if (size_bytes != aecm::SessionBatch::kSessionBytes) return AECM_BAD_PARAMETER_ERROR;
    return s->batch->ImportSession(session, snapshot, true);
}

static int32_t CheckSessionsBulk(const AecmSessions *s, int32_t count, const void *snapshots, size_t size_bytes) {
    if (!s) return -1;
    if (count < 0) return AECM_BAD_PARAMETER_ERROR;
    if (count == 0) return 0;
    if (!snapshots) return AECM_NULL_POINTER_ERROR;
    if (size_bytes != (size_t)count * aecm::SessionBatch::kSessionBytes) return AECM_BAD_PARAMETER_ERROR;
    return 0;
}

int32_t WebRtcAecmSessions_ExportSessions(AecmSessions *s, const int32_t *sessions_host, int32_t count, void *snapshots_host, size_t size_bytes) {
    if (int32_t rc = CheckSessionsBulk(s, count, snapshots_host, size_bytes)) return rc;
    return s->batch->ExportSessions(sessions_host, count, snapshots_host, false);
}

int32_t WebRtcAecmSessions_ImportSessions(AecmSessions *s, const int32_t *sessions_host, int32_t count, const void *snapshots_host, size_t size_bytes,
                                          int32_t any_rate) {
    if (int32_t rc = CheckSessionsBulk(s, count, snapshots_host, size_bytes)) return rc;
    return s->batch->ImportSessions(sessions_host, count, snapshots_host, false, any_rate != 0);
}

int32_t WebRtcAecmSessions_ExportSessionsDevice(AecmSessions *s, const int32_t *sessions_host, int32_t count, void *snapshots_dev, size_t size_bytes) {
    if (int32_t rc = CheckSessionsBulk(s, count, snapshots_dev, size_bytes)) return rc;
    return s->batch->ExportSessions(sessions_host, count, snapshots_dev, true);
}

int32_t WebRtcAecmSessions_ImportSessionsDevice(AecmSessions *s, const int32_t *sessions_host, int32_t count, const void *snapshots_dev, size_t size_bytes,
                                                int32_t any_rate) {
    if (int32_t rc = CheckSessionsBulk(s, count, snapshots_dev, size_bytes)) return rc;
    return s->batch->ImportSessions(sessions_host, count, snapshots_dev, true, any_rate != 0);
}

int32_t WebRtcAecmSessions_InitRates(AecmSessions *s, int32_t sampFreq, const int32_t *rates_host) { return s ? s->batch->InitRates(sampFreq, rates_host) : -1; }

int32_t WebRtcAecmSessions_InitSessionRate(AecmSessions *s, int32_t session, int32_t sampFreq) {
    return s ? s->batch->InitSessionRate(session, sampFreq) : -1;
}

int32_t WebRtcAecmSessions_GetSessionRate(AecmSessions *s, int32_t session, int32_t *sampFreq) {
    return s ? s->batch->GetSessionRate(session, sampFreq) : -1;
}

int32_t WebRtcAecmSessions_set_config_session(AecmSessions *s, int32_t session, AecmConfig config) {
    return s ? s->batch->SetConfigSession(session, config.cngMode, config.echoMode) : -1;
}

int32_t WebRtcAecmSessions_InitEchoPath(AecmSessions *s, int32_t session, const void *echo_path, size_t size_bytes) {
    return s ? s->batch->InitEchoPathSession(session, echo_path, size_bytes) : -1;
}

int32_t WebRtcAecmSessions_GetEchoPath(AecmSessions *s, int32_t session, void *echo_path, size_t size_bytes) {
    return s ? s->batch->GetEchoPathSession(session, echo_path, size_bytes) : -1;
}

// nrOfSamples stays a size_t all the way down: 2^32 + 80 must be refused like the reference does, not narrowed to 80.
int32_t WebRtcAecmSessions_Tick(AecmSessions *s, const int16_t *far_dev, const int16_t *near_dev,
                                const int16_t *near_clean_dev, int16_t *out_dev, int64_t stream_stride, size_t nrOfSamples,
                                int16_t msInSndCardBuf) {
    if (!s) return -1;
    return s->batch->Tick(far_dev, near_dev, near_clean_dev, out_dev, stream_stride, nrOfSamples, msInSndCardBuf, nullptr,
                          nullptr, nullptr, false);
}

int32_t WebRtcAecmSessions_TickHost(AecmSessions *s, const int16_t *far_host, const int16_t *near_host,
                                    const int16_t *near_clean_host, int16_t *out_host, int64_t stream_stride,
                                    size_t nrOfSamples, int16_t msInSndCardBuf) {
    if (!s) return -1;
    return s->batch->Tick(far_host, near_host, near_clean_host, out_host, stream_stride, nrOfSamples, msInSndCardBuf,
                          nullptr, nullptr, nullptr, true);
}

int32_t WebRtcAecmSessions_TickPerSession(AecmSessions *s, const int16_t *far_dev, const int16_t *near_dev,
                                          const int16_t *near_clean_dev, int16_t *out_dev, int64_t stream_stride,
                                          size_t nrOfSamples, const int16_t *msInSndCardBuf_host, int32_t *codes_host) {
    if (!s) return -1;
    if (!msInSndCardBuf_host) return AECM_NULL_POINTER_ERROR;
    return s->batch->Tick(far_dev, near_dev, near_clean_dev, out_dev, stream_stride, nrOfSamples, 0, msInSndCardBuf_host,
                          nullptr, codes_host, false);
}

int32_t WebRtcAecmSessions_TickPerSessionHost(AecmSessions *s, const int16_t *far_host, const int16_t *near_host,
                                              const int16_t *near_clean_host, int16_t *out_host, int64_t stream_stride,
                                              size_t nrOfSamples, const int16_t *msInSndCardBuf_host, int32_t *codes_host) {
    if (!s) return -1;
    if (!msInSndCardBuf_host) return AECM_NULL_POINTER_ERROR;
    return s->batch->Tick(far_host, near_host, near_clean_host, out_host, stream_stride, nrOfSamples, 0,
                          msInSndCardBuf_host, nullptr, codes_host, true);
}

int32_t WebRtcAecmSessions_TickFlags(AecmSessions *s, const int16_t *far_dev, const int16_t *near_dev,
                                     const int16_t *near_clean_dev, int16_t *out_dev, int64_t stream_stride, size_t nrOfSamples,
                                     const int16_t *msInSndCardBuf_host, const uint8_t *flags_host, int32_t *codes_host) {
    if (!s) return -1;
    if (!msInSndCardBuf_host || !flags_host) return AECM_NULL_POINTER_ERROR;
    return s->batch->Tick(far_dev, near_dev, near_clean_dev, out_dev, stream_stride, nrOfSamples, 0, msInSndCardBuf_host,
                          flags_host, codes_host, false);
}

int32_t WebRtcAecmSessions_TickFlagsHost(AecmSessions *s, const int16_t *far_host, const int16_t *near_host,
                                         const int16_t *near_clean_host, int16_t *out_host, int64_t stream_stride,
                                         size_t nrOfSamples, const int16_t *msInSndCardBuf_host, const uint8_t *flags_host,
                                         int32_t *codes_host) {
    if (!s) return -1;
    if (!msInSndCardBuf_host || !flags_host) return AECM_NULL_POINTER_ERROR;
    return s->batch->Tick(far_host, near_host, near_clean_host, out_host, stream_stride, nrOfSamples, 0,
                          msInSndCardBuf_host, flags_host, codes_host, true);
}

int32_t WebRtcAecmSessions_TickAsync(AecmSessions *s, const int16_t *far_dev, const int16_t *near_dev, const int16_t *near_clean_dev,
                                     int16_t *out_dev, int64_t stream_stride, size_t nrOfSamples, int16_t msInSndCardBuf,
                                     const int16_t *msInSndCardBuf_host, const uint8_t *flags_host, int32_t *codes_host,
                                     void *wait_hip_event, void *done_hip_event) {
    if (!s) return -1;
    if (flags_host && !msInSndCardBuf_host) return AECM_NULL_POINTER_ERROR;
    return s->batch->TickAsync(far_dev, near_dev, near_clean_dev, out_dev, stream_stride, nrOfSamples, msInSndCardBuf,
                               msInSndCardBuf_host, flags_host, codes_host, wait_hip_event, done_hip_event);
}

// K call pairs per session and tick (20 .. 60 ms packets on 10 ms calls): SessionBatch::Enqueue with `calls`.
static_assert(AECM_SESSION_MAX_TICK_CALLS == aecm::kFlowMaxTickCalls, "AECM_SESSION_MAX_TICK_CALLS");
int32_t WebRtcAecmSessions_TickCalls(AecmSessions *s, const int16_t *far_dev, const int16_t *near_dev, const int16_t *near_clean_dev,
                                     int16_t *out_dev, int64_t stream_stride, size_t nrOfSamples, int32_t calls, int16_t msInSndCardBuf,
                                     const int16_t *msInSndCardBuf_host, const uint8_t *flags_host, int32_t *codes_host) {
    if (!s) return -1;
    if (flags_host && !msInSndCardBuf_host) return AECM_NULL_POINTER_ERROR;
    return s->batch->Tick(far_dev, near_dev, near_clean_dev, out_dev, stream_stride, nrOfSamples, msInSndCardBuf, msInSndCardBuf_host,
                          flags_host, codes_host, false, 0, calls);
}

int32_t WebRtcAecmSessions_TickCallsHost(AecmSessions *s, const int16_t *far_host, const int16_t *near_host, const int16_t *near_clean_host,
                                         int16_t *out_host, int64_t stream_stride, size_t nrOfSamples, int32_t calls, int16_t msInSndCardBuf,
                                         const int16_t *msInSndCardBuf_host, const uint8_t *flags_host, int32_t *codes_host) {
    if (!s) return -1;
    if (flags_host && !msInSndCardBuf_host) return AECM_NULL_POINTER_ERROR;
    return s->batch->Tick(far_host, near_host, near_clean_host, out_host, stream_stride, nrOfSamples, msInSndCardBuf, msInSndCardBuf_host,
                          flags_host, codes_host, true, 0, calls);
}

int32_t WebRtcAecmSessions_TickCallsAsync(AecmSessions *s, const int16_t *far_dev, const int16_t *near_dev, const int16_t *near_clean_dev,
                                          int16_t *out_dev, int64_t stream_stride, size_t nrOfSamples, int32_t calls, int16_t msInSndCardBuf,
                                          const int16_t *msInSndCardBuf_host, const uint8_t *flags_host, int32_t *codes_host,
                                          void *wait_hip_event, void *done_hip_event) {
    if (!s) return -1;
    if (flags_host && !msInSndCardBuf_host) return AECM_NULL_POINTER_ERROR;
    return s->batch->TickAsync(far_dev, near_dev, near_clean_dev, out_dev, stream_stride, nrOfSamples, msInSndCardBuf, msInSndCardBuf_host,
                               flags_host, codes_host, wait_hip_event, done_hip_event, 0, calls);
}

// One packet of K 10 ms calls per session and tick, every session at its own rate and call size, on packed rows: SessionBatch::Enqueue
// with `calls` and `packets`.
int32_t WebRtcAecmSessions_TickPackets(AecmSessions *s, const int16_t *far_dev, const int16_t *near_dev, const int16_t *near_clean_dev,
                                       int16_t *out_dev, int64_t stream_stride, size_t nrOfSamples, int32_t calls, int16_t msInSndCardBuf,
                                       const int16_t *msInSndCardBuf_host, const uint8_t *flags_host, int32_t *codes_host) {
    if (!s) return -1;
    if (flags_host && !msInSndCardBuf_host) return AECM_NULL_POINTER_ERROR;
    return s->batch->Tick(far_dev, near_dev, near_clean_dev, out_dev, stream_stride, nrOfSamples, msInSndCardBuf, msInSndCardBuf_host,
                          flags_host, codes_host, false, 0, calls, true);
}

int32_t WebRtcAecmSessions_TickPacketsHost(AecmSessions *s, const int16_t *far_host, const int16_t *near_host, const int16_t *near_clean_host,
                                           int16_t *out_host, int64_t stream_stride, size_t nrOfSamples, int32_t calls, int16_t msInSndCardBuf,
                                           const int16_t *msInSndCardBuf_host, const uint8_t *flags_host, int32_t *codes_host) {
    if (!s) return -1;
    if (flags_host && !msInSndCardBuf_host) return AECM_NULL_POINTER_ERROR;
    return s->batch->Tick(far_host, near_host, near_clean_host, out_host, stream_stride, nrOfSamples, msInSndCardBuf, msInSndCardBuf_host,
                          flags_host, codes_host, true, 0, calls, true);
}

int32_t WebRtcAecmSessions_TickPacketsAsync(AecmSessions *s, const int16_t *far_dev, const int16_t *near_dev, const int16_t *near_clean_dev,
                                            int16_t *out_dev, int64_t stream_stride, size_t nrOfSamples, int32_t calls, int16_t msInSndCardBuf,
                                            const int16_t *msInSndCardBuf_host, const uint8_t *flags_host, int32_t *codes_host,
                                            void *wait_hip_event, void *done_hip_event) {
    if (!s) return -1;
    if (flags_host && !msInSndCardBuf_host) return AECM_NULL_POINTER_ERROR;
    return s->batch->TickAsync(far_dev, near_dev, near_clean_dev, out_dev, stream_stride, nrOfSamples, msInSndCardBuf, msInSndCardBuf_host,
                               flags_host, codes_host, wait_hip_event, done_hip_event, 0, calls, true);
}

int32_t WebRtcAecmSessions_BufferFarend(AecmSessions *s, const int16_t *far_dev, int64_t stream_stride, size_t nrOfSamples, int32_t calls,
                                        const uint8_t *calls_host) {
    return s ? s->batch->BufferFarend(far_dev, stream_stride, nrOfSamples, calls, calls_host, false, true, nullptr, nullptr) : -1;
}

int32_t WebRtcAecmSessions_BufferFarendHost(AecmSessions *s, const int16_t *far_host, int64_t stream_stride, size_t nrOfSamples, int32_t calls,
                                            const uint8_t *calls_host) {
    return s ? s->batch->BufferFarend(far_host, stream_stride, nrOfSamples, calls, calls_host, true, true, nullptr, nullptr) : -1;
}

int32_t WebRtcAecmSessions_BufferFarendAsync(AecmSessions *s, const int16_t *far_dev, int64_t stream_stride, size_t nrOfSamples, int32_t calls,
                                             const uint8_t *calls_host, void *wait_hip_event, void *done_hip_event) {
    return s ? s->batch->BufferFarend(far_dev, stream_stride, nrOfSamples, calls, calls_host, false, false, wait_hip_event, done_hip_event) : -1;
}

int32_t WebRtcAecmSessions_Process(AecmSessions *s, const int16_t *near_dev, const int16_t *near_clean_dev, int16_t *out_dev, int64_t stream_stride,
                                   size_t nrOfSamples, int16_t msInSndCardBuf, const int16_t *msInSndCardBuf_host, int32_t *codes_host) {
    if (!s) return -1;
    return s->batch->Tick(nullptr, near_dev, near_clean_dev, out_dev, stream_stride, nrOfSamples, msInSndCardBuf, msInSndCardBuf_host, nullptr,
                          codes_host, false, AECM_SESSION_NO_FAREND);
}

int32_t WebRtcAecmSessions_ProcessHost(AecmSessions *s, const int16_t *near_host, const int16_t *near_clean_host, int16_t *out_host,
                                       int64_t stream_stride, size_t nrOfSamples, int16_t msInSndCardBuf, const int16_t *msInSndCardBuf_host,
                                       int32_t *codes_host) {
    if (!s) return -1;
    return s->batch->Tick(nullptr, near_host, near_clean_host, out_host, stream_stride, nrOfSamples, msInSndCardBuf, msInSndCardBuf_host, nullptr,
                          codes_host, true, AECM_SESSION_NO_FAREND);
}

int32_t WebRtcAecmSessions_Synchronize(AecmSessions *s) { return s ? s->batch->Synchronize() : -1; }

int32_t WebRtcAecmSessions_ForceSparseTicks(AecmSessions *s, int32_t on) {
    if (!s) return -1;
    s->batch->ForceSparseTicks(on != 0);
    return 0;
}

static_assert(AECM_SESSION_NO_CLEAN == aecm::kFlowNoClean, "AECM_SESSION_NO_CLEAN");
int32_t WebRtcAecmSessions_GetSessionCleanMode(AecmSessions *s, int32_t session, int32_t *mode) {
    return s ? s->batch->GetSessionCleanMode(session, mode) : -1;
}

int32_t WebRtcAecmSessions_SplitCleanTwoLaunches(AecmSessions *s, int32_t on) {
    if (!s) return -1;
    s->batch->SplitCleanTwoLaunches(on);
    return 0;
}

int32_t WebRtcAecmSessions_SetSplitCallTicks(AecmSessions *s, int32_t on) {
    if (!s) return -1;
    s->batch->SetSplitCallTicks(on != 0);
    return 0;
}

// The session trace: the record is aecm_session_trace.h's eight words and the block trace's eight.
static_assert(sizeof(AecmSessionTrace) == aecm::kSessionTraceWords * sizeof(uint32_t) && offsetof(AecmSessionTrace, core) == aecm::kSessionTraceHeaderWords * sizeof(uint32_t) &&
                  offsetof(AecmSessionTrace, far_buffered) == 24 && offsetof(AecmSessionTrace, time_for_delay_change) == 28,
              "the session trace record is sixteen words, the wrapper half first");
size_t WebRtcAecmSessions_session_trace_size_bytes(void) { return sizeof(AecmSessionTrace); }

int32_t WebRtcAecmSessions_SetSessionTrace(AecmSessions *s, void *trace_dev, int64_t session_stride, int64_t tick_stride, int32_t ring_ticks) {
    if (!s) return AECM_BAD_PARAMETER_ERROR;
    return s->batch->SetSessionTrace(trace_dev, session_stride, tick_stride, ring_ticks);
}

int32_t WebRtcAecmSessions_GetSessionTraceTicks(AecmSessions *s, int64_t *ticks) {
    if (!s) return AECM_BAD_PARAMETER_ERROR;
    if (!ticks) return AECM_NULL_POINTER_ERROR;
    *ticks = s->batch->session_trace_ticks();
    return 0;
}

// The call trace: the same record per call slot.
int32_t WebRtcAecmSessions_SetCallTrace(AecmSessions *s, void *trace_dev, int64_t session_stride, int64_t call_stride, int32_t ring_calls) {
    if (!s) return AECM_BAD_PARAMETER_ERROR;
    return s->batch->SetCallTrace(trace_dev, session_stride, call_stride, ring_calls);
}

int32_t WebRtcAecmSessions_GetCallTraceCalls(AecmSessions *s, int64_t *calls) {
    if (!s) return AECM_BAD_PARAMETER_ERROR;
    if (!calls) return AECM_NULL_POINTER_ERROR;
    *calls = s->batch->call_trace_calls();
    return 0;
}

int32_t WebRtcAecmSessions_SetKernelVariant(AecmSessions *s, int32_t variant) {
    if (!s) return -1;
    if (variant != AECM_KERNEL_SAFE && variant != AECM_KERNEL_FAST) return AECM_BAD_PARAMETER_ERROR;
    s->batch->engine()->set_variant(variant);
    return 0;
}

// Caller-owned host audio, pinned and mapped once: the alias returned is a device pointer every *_dev argument accepts.
int32_t WebRtcAecmBatch_RegisterHostBuffer(int32_t device_id, void *host, size_t size_bytes, void **device_alias) {
    if (!host || !device_alias) return AECM_NULL_POINTER_ERROR;
    if (size_bytes == 0) return AECM_BAD_PARAMETER_ERROR;
    if (hipSetDevice(device_id) != hipSuccess) return AECM_BAD_PARAMETER_ERROR;
    const hipError_t e = hipHostRegister(host, size_bytes, hipHostRegisterMapped | hipHostRegisterPortable);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return e == hipErrorHostMemoryAlreadyRegistered ? AECM_BAD_PARAMETER_ERROR : AECM_UNSPECIFIED_ERROR;
    }
    void *dev = nullptr;
    if (hipHostGetDevicePointer(&dev, host, 0) != hipSuccess || !dev) {
        (void)hipHostUnregister(host);
        return AECM_UNSPECIFIED_ERROR;
    }
    *device_alias = dev;
    return 0;
}

int32_t WebRtcAecmBatch_UnregisterHostBuffer(int32_t device_id, void *host) {
    if (!host) return AECM_NULL_POINTER_ERROR;
    if (hipSetDevice(device_id) != hipSuccess) return AECM_BAD_PARAMETER_ERROR;
    if (hipDeviceSynchronize() != hipSuccess) return AECM_UNSPECIFIED_ERROR;      // nothing may still be reading or writing it
    if (hipHostUnregister(host) != hipSuccess) {
        (void)hipGetLastError();                       // not a registered buffer: the caller's mistake, not a sticky device error
        return AECM_BAD_PARAMETER_ERROR;
    }
    return 0;
}

int32_t WebRtcAecmBatch_SelfTest(int32_t device_id, int32_t exhaustive, uint64_t failures[8]) {
    if (!failures) return AECM_NULL_POINTER_ERROR;
    if (hipSetDevice(device_id) != hipSuccess) return AECM_UNSPECIFIED_ERROR;
    uint64_t *dev = nullptr;
    uint32_t *consts = nullptr;
    std::vector<uint32_t> blob;
    aecm::BuildKernelConstants(&blob);
    if (hipMalloc((void **)&dev, 8 * sizeof(uint64_t)) != hipSuccess) return AECM_UNSPECIFIED_ERROR;
    if (hipMalloc((void **)&consts, blob.size() * 4) != hipSuccess) { (void)hipFree(dev); return AECM_UNSPECIFIED_ERROR; }
    int32_t rc = AECM_UNSPECIFIED_ERROR;
    if (hipMemcpy(consts, blob.data(), blob.size() * 4, hipMemcpyHostToDevice) == hipSuccess &&
        hipMemset(dev, 0, 8 * sizeof(uint64_t)) == hipSuccess && aecm::LaunchSelfTest(dev, exhaustive, consts, nullptr) == hipSuccess &&
        hipDeviceSynchronize() == hipSuccess &&
        hipMemcpy(failures, dev, 8 * sizeof(uint64_t), hipMemcpyDeviceToHost) == hipSuccess)
        rc = 0;
    (void)hipFree(dev);
    (void)hipFree(consts);
    return rc;
}

int32_t WebRtcAecmBatch_GetCheckCounters(int32_t device_id, uint64_t counters[2], int32_t reset) {
    if (!counters) return AECM_NULL_POINTER_ERROR;
    if (hipSetDevice(device_id) != hipSuccess) return AECM_UNSPECIFIED_ERROR;
    hipError_t e = aecm::ReadCheckCounters(counters, reset != 0);
    if (e == hipErrorNotSupported) return AECM_UNSUPPORTED_FUNCTION_ERROR;
    if (e != hipSuccess) return AECM_UNSPECIFIED_ERROR;
    uint64_t probe[2] = {0, 0};                            // the ops probe's unit keeps a pair of its own (DebugOps)
    e = aecm::ReadOpsProbeCheckCounters(probe, reset != 0);
    if (e != hipSuccess) return AECM_UNSPECIFIED_ERROR;
    counters[0] += probe[0];
    counters[1] += probe[1];
    uint64_t split_calls[2] = {0, 0};                      // so do the split K-call / packet tick kernels (SetSplitCallTicks)
    e = aecm::ReadTickSplitCallsCheckCounters(split_calls, reset != 0);
    if (e != hipSuccess) return AECM_UNSPECIFIED_ERROR;
    counters[0] += split_calls[0];
    counters[1] += split_calls[1];
    return 0;
}

int32_t WebRtcAecmBatch_DebugFft128(int32_t device_id, int16_t *data_host, int32_t *scales_host, int32_t variant,
                                    int32_t kernel_variant, int32_t count) {
    if (!data_host || !scales_host) return AECM_NULL_POINTER_ERROR;
    if (variant < 0 || variant > 2 || count < 0) return AECM_BAD_PARAMETER_ERROR;
    if (count == 0) return 0;
    if (hipSetDevice(device_id) != hipSuccess) return AECM_UNSPECIFIED_ERROR;
    std::vector<uint32_t> blob;
    aecm::BuildKernelConstants(&blob);
    int16_t *data = nullptr;
    int32_t *scales = nullptr;
    uint32_t *consts = nullptr;
    const size_t bytes = (size_t)count * 256 * sizeof(int16_t);
    int32_t rc = AECM_UNSPECIFIED_ERROR;
    if (hipMalloc((void **)&data, bytes) == hipSuccess && hipMalloc((void **)&scales, (size_t)count * 4) == hipSuccess &&
        hipMalloc((void **)&consts, blob.size() * 4) == hipSuccess &&
        hipMemcpy(consts, blob.data(), blob.size() * 4, hipMemcpyHostToDevice) == hipSuccess &&
        hipMemcpy(data, data_host, bytes, hipMemcpyHostToDevice) == hipSuccess &&
        aecm::LaunchFft128(data, scales, variant, kernel_variant != 0, count, consts, nullptr) == hipSuccess &&
        hipDeviceSynchronize() == hipSuccess && hipMemcpy(data_host, data, bytes, hipMemcpyDeviceToHost) == hipSuccess &&
        hipMemcpy(scales_host, scales, (size_t)count * 4, hipMemcpyDeviceToHost) == hipSuccess)
        rc = 0;
    (void)hipFree(data);
    (void)hipFree(scales);
    (void)hipFree(consts);
    return rc;
}

int32_t WebRtcAecmBatch_DebugOpsCount(void) { return aecm::OpsProbeCount(); }

const char *WebRtcAecmBatch_DebugOpName(int32_t op) { return aecm::OpsProbeName(op); }

int32_t WebRtcAecmBatch_DebugOps(int32_t device_id, int32_t op, int32_t form, const int32_t *a, const int32_t *b, const int32_t *c,
                                 int32_t *out, int32_t *nonuniform, int32_t n) {
    // everything is refused before a device is touched
    const int arity = aecm::OpsProbeArity(op);
    if (arity == 0 || (form != 0 && form != 1) || n <= 0 || n > aecm::kOpsProbeMaxTuples) return AECM_BAD_PARAMETER_ERROR;
    if (!a || (arity >= 2 && !b) || (arity >= 3 && !c) || !out) return AECM_BAD_PARAMETER_ERROR;
    if (hipSetDevice(device_id) != hipSuccess) return AECM_UNSPECIFIED_ERROR;
    const int32_t *host[3] = {a, arity >= 2 ? b : nullptr, arity >= 3 ? c : nullptr};
    int32_t *dev[3] = {nullptr, nullptr, nullptr}, *out_dev = nullptr;
    const size_t bytes = (size_t)n * sizeof(int32_t), out_bytes = form == 0 ? bytes : 2 * bytes;
    bool ok = hipMalloc((void **)&out_dev, out_bytes) == hipSuccess && hipMemset(out_dev, 0, out_bytes) == hipSuccess;
    for (int k = 0; ok && k < 3; ++k) {
        if (!host[k]) continue;
        ok = hipMalloc((void **)&dev[k], bytes) == hipSuccess && hipMemcpy(dev[k], host[k], bytes, hipMemcpyHostToDevice) == hipSuccess;
    }
    int32_t rc = AECM_UNSPECIFIED_ERROR;
    if (ok && aecm::LaunchOpsProbe(op, form, dev[0], dev[1], dev[2], out_dev, n, nullptr) == hipSuccess && hipDeviceSynchronize() == hipSuccess &&
        hipMemcpy(out, out_dev, bytes, hipMemcpyDeviceToHost) == hipSuccess) {
        rc = 0;
        if (nonuniform) {
            if (form == 0) memset(nonuniform, 0, bytes);
            else if (hipMemcpy(nonuniform, out_dev + n, bytes, hipMemcpyDeviceToHost) != hipSuccess) rc = AECM_UNSPECIFIED_ERROR;
        }
    }
    for (int k = 0; k < 3; ++k)
        if (dev[k]) (void)hipFree(dev[k]);
    if (out_dev) (void)hipFree(out_dev);
    return rc;
}

int32_t WebRtcAecmBatch_DeviceInfo(int32_t device_id, char *name, size_t name_len, int32_t *compute_units,
                                   int32_t *clock_khz) {
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device_id) != hipSuccess) return AECM_UNSPECIFIED_ERROR;
    if (name && name_len) {
        strncpy(name, prop.gcnArchName, name_len - 1);
        name[name_len - 1] = 0;
    }
    if (compute_units) *compute_units = prop.multiProcessorCount;
    if (clock_khz) *clock_khz = prop.clockRate;
    return 0;
}

int32_t WebRtcAecmBatch_DevicePciBusId(int32_t device_id, char *bus_id, size_t bus_id_len) {
    if (!bus_id) return AECM_NULL_POINTER_ERROR;
    if (bus_id_len < 13) return AECM_BAD_PARAMETER_ERROR;                     // "0000:00:00.0" + NUL
    return hipDeviceGetPCIBusId(bus_id, (int)bus_id_len, device_id) == hipSuccess ? 0 : AECM_UNSPECIFIED_ERROR;
}

}  // extern "C"
