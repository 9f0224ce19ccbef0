// The traced twins of the block kernels (aecm_block_kernels.hip): the same launch forms with a block trace attached
// (include/aecm_batch.h: AecmBlockTrace, WebRtcAecmBatch_SetBlockTrace).  Besides its 128 bytes of output every block writes one
// 32-byte record of what it decided -- the delay estimate, the far-end activity, the suppression gain ... as GetDigest would show
// them directly after that block:
//   aecm_trace_process_kernel        one wavefront per stream (aecm_process_kernel's twin)
//   aecm_trace_queue_kernel          the chunk queue (aecm_process_queue_kernel's)
//   aecm_trace_ragged_queue_kernel   the ragged chunk queue (aecm_process_ragged_queue_kernel's)
// There is no traced pipelined form: there the traced values live in four different role waves; PlanLaunch gives a launch that
// would be pipelined one wavefront per stream while a trace is attached (results never depend on the form).
//
// A unit of its own rather than a template parameter of the block kernels: their instruction streams, and the records under
// profiles/ keyed on them, stay exactly what they are, and a launch without a trace runs what it always ran.  The kernels here
// are those kernels' text with BlockEngine::run_stream_traced in run_stream_io's place, on the SAME engine instantiations (the
// lean block loop where there is no clean input), compiled with the same flags (build.py: SOURCE_FLAGS): a trace observes the
// arithmetic that ships.  The queue's claim / wait / publish steps are the shared ones (aecm_block_queue.h).
//
// The record (BlockEngine::block_trace_row, aecm_wave.h): the wave-uniform values are packed into eight words on the scalar side,
// put into lanes 0..7 of one vector register with eight v_writelane, and stored by those lanes as one 32-byte row -- a plain
// vector store like the audio rows', never part of the sc1 state hand-over between the chunks of a stream: nobody reads a record
// inside a launch, and QueuePublish's s_waitcnt vmcnt(0) covers them like every other store of the chunk.
#define AECM_TABLE_ATTR __device__
#define AECM_CHECK_UNIT trace      // (aecm_kernel_common.h: the unit's pair of audit counters)
#include "aecm_kernel_common.h"
#include "aecm_block_queue.h"

namespace aecm {

// This unit's share of the audit counters (see ReadCheckCounters in aecm_kernels.hip).
AECM_DEFINE_CHECK_COUNTERS(ReadTraceKernelCheckCounters)

template <bool kFast, bool kHasClean, bool kPhasePrio = true>
__global__ __launch_bounds__(64 * kWavesPerWorkgroup)
__attribute__((amdgpu_waves_per_eu(kPhasePrio ? AECM_WAVES_PER_EU : AECM_ROTATION_WAVES_PER_EU, AECM_MAX_WAVES_PER_EU)))
void aecm_trace_process_kernel(StatePtrs st, IoView io, TraceView tv, int n_streams, int n_blocks, const int32_t *blocks_per_stream) {
    FillLdsTables<64 * kWavesPerWorkgroup>(st.consts);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t stream = (int64_t)blockIdx.x * kWavesPerWorkgroup + wave;
    if (stream >= n_streams) return;
    if (blocks_per_stream) {
        n_blocks = __builtin_amdgcn_readfirstlane(blocks_per_stream[stream]);
        if (n_blocks <= 0) return;
    }
    using E = BlockEngine<Gfx950Wave<kFast, kPhasePrio>, kHasClean>;
    typename E::TracedIo tio = E::traced_io(io, tv, stream, 0);
    E::run_stream_traced(st, tio, stream, n_blocks);
}

// The chunk queue: item i = (chunk i / S, stream i % S); the records of a chunk's blocks are those of the launch's blocks
// chunk x chunk_blocks + blk (traced_io offsets the audio and the records by the chunk's first block alike).
template <bool kHasClean>
__global__ __launch_bounds__(64 * kWavesPerWorkgroup)
__attribute__((amdgpu_waves_per_eu(AECM_WAVES_PER_EU, AECM_MAX_WAVES_PER_EU)))
void aecm_trace_queue_kernel(StatePtrs st, IoView io, TraceView tv, int n_streams, int n_blocks, int chunk_blocks, int n_chunks, uint32_t *ctl,
                             uint32_t *err) {
    FillLdsTables<64 * kWavesPerWorkgroup>(st.consts);
    using E = BlockEngine<Gfx950Wave<true, true, false, true, !kHasClean>, kHasClean>;       // aecm_process_queue_kernel's
    const uint32_t n_items = (uint32_t)n_streams * (uint32_t)n_chunks;
    uint32_t *done = ctl + kQueueCtlWords;
    for (;;) {
        const uint32_t item = QueueClaim(ctl);
        if (item >= n_items) break;
        if (__builtin_amdgcn_readfirstlane((int)__hip_atomic_load(err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) != 0) break;
        const uint32_t chunk = item / (uint32_t)n_streams;
        const uint32_t stream = item - chunk * (uint32_t)n_streams;
        if (!QueueWait(done, stream, chunk, chunk_blocks, err)) return;
        const int first = (int)chunk * chunk_blocks;
        const int nb = n_blocks - first < chunk_blocks ? n_blocks - first : chunk_blocks;
        typename E::TracedIo tio = E::traced_io(io, tv, (int64_t)stream, first);
        E::run_stream_traced(st, tio, (int64_t)stream, nb);
        QueuePublish(done, stream, chunk);
    }
}

// The ragged chunk queue: the plan behind done[] as aecm_process_ragged_queue_kernel reads it -- len[S], order[S],
// first_item[n_chunks + 1].  A stream of length L writes the records 0 .. L - 1, a stream of length 0 has no item and writes none.
template <bool kHasClean>
__global__ __launch_bounds__(64 * kWavesPerWorkgroup)
__attribute__((amdgpu_waves_per_eu(AECM_WAVES_PER_EU, AECM_MAX_WAVES_PER_EU)))
void aecm_trace_ragged_queue_kernel(StatePtrs st, IoView io, TraceView tv, int n_streams, uint32_t n_items, int chunk_blocks, uint32_t *ctl,
                                    uint32_t *err) {
    FillLdsTables<64 * kWavesPerWorkgroup>(st.consts);
    using E = BlockEngine<Gfx950Wave<true, true, false, true, !kHasClean>, kHasClean>;
    uint32_t *done = ctl + kQueueCtlWords;
    const uint32_t *len = done + n_streams, *order = len + n_streams, *first_item = order + n_streams;      // written by the host before the launch
    uint32_t chunk = 0, chunk_first = 0;                                      // the cursor: first_item[chunk] <= every later claim of this wave
    uint32_t chunk_end = (uint32_t)__builtin_amdgcn_readfirstlane((int)first_item[1]);
    for (;;) {
        const uint32_t item = QueueClaim(ctl);
        if (item >= n_items) break;
        if (__builtin_amdgcn_readfirstlane((int)__hip_atomic_load(err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) != 0) break;
        while (item >= chunk_end) {                                           // item < n_items = first_item[n_chunks]: stops at a chunk < n_chunks
            ++chunk;
            chunk_first = chunk_end;
            chunk_end = (uint32_t)__builtin_amdgcn_readfirstlane((int)first_item[chunk + 1]);
        }
        const uint32_t stream = (uint32_t)__builtin_amdgcn_readfirstlane((int)order[item - chunk_first]);
        if (stream >= (uint32_t)n_streams) {                                  // not a plan BuildRaggedPlan made: touch nothing
            __hip_atomic_store(err, 0x80000000u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            return;
        }
        if (!QueueWait(done, stream, chunk, chunk_blocks, err)) return;
        const int first = (int)chunk * chunk_blocks;
        const int left = __builtin_amdgcn_readfirstlane((int)len[stream]) - first;
        const int nb = left < chunk_blocks ? left : chunk_blocks;
        if (nb > 0) {
            typename E::TracedIo tio = E::traced_io(io, tv, (int64_t)stream, first);
            E::run_stream_traced(st, tio, (int64_t)stream, nb);
        }
        QueuePublish(done, stream, chunk);
    }
}

// ---- launchers: the untraced ones' (aecm_block_kernels.hip) with the trace view as one more kernel argument ----------------
hipError_t LaunchTraceBlocks(const StatePtrs &st, const IoView &io, const TraceView &tv, int n_streams, int n_blocks, int variant, bool phase_priority,
                             hipStream_t stream, const int32_t *blocks_per_stream) {
    if (n_streams <= 0 || n_blocks <= 0) return hipSuccess;
    if (!tv.records) return hipErrorInvalidValue;
    const dim3 grid((n_streams + kWavesPerWorkgroup - 1) / kWavesPerWorkgroup);
    const dim3 block(64 * kWavesPerWorkgroup);
    const size_t lds = sizeof(LdsTables);
    const bool clean = io.near_clean != nullptr;
    const bool phase = phase_priority;
#define AECM_LAUNCH(F, C, P) hipLaunchKernelGGL((aecm_trace_process_kernel<F, C, P>), grid, block, lds, stream, st, io, tv, n_streams, n_blocks, blocks_per_stream)
    if (variant == kVariantFast) {
        if (clean) { if (phase) AECM_LAUNCH(true, true, true); else AECM_LAUNCH(true, true, false); }
        else { if (phase) AECM_LAUNCH(true, false, true); else AECM_LAUNCH(true, false, false); }
    } else {
        if (clean) AECM_LAUNCH(false, true, false);
        else AECM_LAUNCH(false, false, false);
    }
#undef AECM_LAUNCH
    return hipGetLastError();
}

hipError_t LaunchTraceBlocksQueued(const StatePtrs &st, const IoView &io, const TraceView &tv, int n_streams, int n_blocks, int chunk_blocks,
                                   int resident_waves, uint32_t *ctl, uint32_t *err, hipStream_t stream) {
    if (!tv.records || n_streams <= 0 || n_blocks <= 0 || chunk_blocks <= 0) return hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(ctl, 0, QueueControlBytes(n_streams), stream);
    if (e != hipSuccess) return e;
    const int n_chunks = (n_blocks + chunk_blocks - 1) / chunk_blocks;
    const dim3 grid(QueueGridWorkgroups(n_streams, resident_waves));
    const dim3 block(64 * kWavesPerWorkgroup);
    const size_t lds = sizeof(LdsTables);
    if (io.near_clean != nullptr)
        hipLaunchKernelGGL((aecm_trace_queue_kernel<true>), grid, block, lds, stream, st, io, tv, n_streams, n_blocks, chunk_blocks, n_chunks, ctl, err);
    else
        hipLaunchKernelGGL((aecm_trace_queue_kernel<false>), grid, block, lds, stream, st, io, tv, n_streams, n_blocks, chunk_blocks, n_chunks, ctl, err);
    return hipGetLastError();
}

hipError_t LaunchTraceBlocksRaggedQueued(const StatePtrs &st, const IoView &io, const TraceView &tv, int n_streams, int live_streams, uint32_t n_items,
                                         int chunk_blocks, int resident_waves, uint32_t *ctl, uint32_t *err, hipStream_t stream) {
    if (!tv.records || n_streams <= 0 || live_streams <= 0 || n_items == 0 || chunk_blocks <= 0) return hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(ctl, 0, QueueControlBytes(n_streams), stream);
    if (e != hipSuccess) return e;
    const dim3 grid(QueueGridWorkgroups(live_streams, resident_waves));
    const dim3 block(64 * kWavesPerWorkgroup);
    const size_t lds = sizeof(LdsTables);
    if (io.near_clean != nullptr)
        hipLaunchKernelGGL((aecm_trace_ragged_queue_kernel<true>), grid, block, lds, stream, st, io, tv, n_streams, n_items, chunk_blocks, ctl, err);
    else
        hipLaunchKernelGGL((aecm_trace_ragged_queue_kernel<false>), grid, block, lds, stream, st, io, tv, n_streams, n_items, chunk_blocks, ctl, err);
    return hipGetLastError();
}

}  // namespace aecm
