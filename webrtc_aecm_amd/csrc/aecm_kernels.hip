// gfx950 kernels of the MI355X AECM engine other than the block kernels (aecm_block_kernels.hip): state maintenance,
// the session schedule's gather / scatter, the streaming-session tick kernels, the device self-test.
#define AECM_TABLE_ATTR __device__
#include <initializer_list>

#include "aecm_kernel_common.h"
#include "aecm_state_check.h"

namespace aecm {

AECM_DEFINE_CHECK_COUNTERS(ReadThisUnitCheckCounters)      // (used below only)
// Audit counters of the -DAECM_CHECKED build (aecm_ops.h): this unit's pair, the block kernels', the traced block kernels', the
// traced tick kernels' and the traced K-call / packet tick kernels', behind everything the device still has to do;
// hipErrorNotSupported in the shipped build.
hipError_t ReadCheckCounters(uint64_t counters[2], bool reset) {
#if defined(AECM_CHECKED)
    hipError_t e = hipDeviceSynchronize();
    if (e != hipSuccess) return e;
    uint64_t sum[2] = {0, 0};
    for (const auto read : {ReadThisUnitCheckCounters, ReadBlockKernelCheckCounters, ReadTraceKernelCheckCounters, ReadTickTraceCheckCounters,
                            ReadCallTraceCheckCounters}) {
        uint64_t share[2] = {0, 0};
        e = read(share, reset);
        if (e != hipSuccess) return e;
        sum[0] += share[0];
        sum[1] += share[1];
    }
    counters[0] = sum[0];
    counters[1] = sum[1];
    return hipSuccess;
#else
    (void)counters;
    (void)reset;
    return hipErrorNotSupported;
#endif
}

// ---- state maintenance ---------------------------------------------------------------------------

// One stream image (vec, scal) into stream s, far-spectrum history cleared: the work of one workgroup.
__device__ __forceinline__ void WriteStreamImage(const StatePtrs &st, int64_t s, const uint32_t *image_vec, const int32_t *image_scal) {
    uint32_t *vec = st.vec + s * (int64_t)kVecWordsPerStream;
    for (int i = threadIdx.x; i < (int)kVecWordsPerStream; i += blockDim.x) vec[i] = image_vec[i];
    int32_t *scal = st.scal + s * (int64_t)kNumScal;
    for (int i = threadIdx.x; i < kNumScal; i += blockDim.x) scal[i] = image_scal[i];
    uint32_t *hist = reinterpret_cast<uint32_t *>(st.hist + s * (int64_t)kHistWordsPerStream);
    for (int i = threadIdx.x; i < (int)kHistWordsPerStream / 2; i += blockDim.x) hist[i] = 0u;
}

__global__ void aecm_broadcast_image_kernel(StatePtrs st, const uint32_t *image_vec, const int32_t *image_scal,
                                            int first, int count) {
    if (blockIdx.x >= (unsigned)count) return;
    WriteStreamImage(st, (int64_t)first + blockIdx.x, image_vec, image_scal);
}

// The same for the streams select[s] != 0 among [0, count): WebRtcAecm_Init at another rate than the object's for some of
// its sessions, in one launch over all of them (WebRtcAecmSessions_InitRates).
__global__ void aecm_broadcast_image_select_kernel(StatePtrs st, const uint32_t *image_vec, const int32_t *image_scal, const uint8_t *select, int count) {
    if (blockIdx.x >= (unsigned)count || !select[blockIdx.x]) return;
    WriteStreamImage(st, (int64_t)blockIdx.x, image_vec, image_scal);
}

hipError_t LaunchBroadcastImageSelect(const StatePtrs &st, const uint32_t *image_vec, const int32_t *image_scal, const uint8_t *select_dev, int count,
                                      hipStream_t stream) {
    if (count <= 0) return hipSuccess;
    hipLaunchKernelGGL(aecm_broadcast_image_select_kernel, dim3(count), dim3(256), 0, stream, st, image_vec, image_scal, select_dev, count);
    return hipGetLastError();
}

hipError_t LaunchBroadcastImage(const StatePtrs &st, const uint32_t *image_vec, const int32_t *image_scal, int first,
                                int count, hipStream_t stream) {
    if (count <= 0) return hipSuccess;
    hipLaunchKernelGGL(aecm_broadcast_image_kernel, dim3(count), dim3(256), 0, stream, st, image_vec, image_scal, first,
                       count);
    return hipGetLastError();
}

__global__ void aecm_patch_scalars_kernel(StatePtrs st, ScalarPatch patch, int first, int count) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)count * patch.n) return;
    const int64_t s = first + i / patch.n;
    const int f = (int)(i % patch.n);
    st.scal[s * (int64_t)kNumScal + patch.field[f]] = patch.value[f];
}

hipError_t LaunchPatchScalars(const StatePtrs &st, const ScalarPatch &patch, int first, int count, hipStream_t stream) {
    if (count <= 0 || patch.n <= 0) return hipSuccess;
    const int64_t total = (int64_t)count * patch.n;
    hipLaunchKernelGGL(aecm_patch_scalars_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, st, patch, first, count);
    return hipGetLastError();
}

// ---- bulk state snapshots (aecm_state_check.h: header + vec + scal + hist per stream) ---------------------------------
// One workgroup per stream; a blob is kStateBlobBytes / 4 words: 8 header words, then the three regions as they lie in HBM.
constexpr int kBlobHeaderWords = (int)(kStateHeaderBytes / 4), kBlobVecWords = (int)kVecWordsPerStream, kBlobScalWords = kNumScal,
              kBlobHistWords = (int)(kHistWordsPerStream / 2), kBlobWords = (int)(kStateBlobBytes / 4);
static_assert(kBlobHeaderWords + kBlobVecWords + kBlobScalWords + kBlobHistWords == kBlobWords, "blob layout");

__global__ __launch_bounds__(256) void aecm_gather_states_kernel(StatePtrs st, int first, uint32_t *blobs) {
    const int64_t s = (int64_t)first + blockIdx.x;
    uint32_t *blob = blobs + (int64_t)blockIdx.x * kBlobWords;
    const uint32_t *vec = st.vec + s * (int64_t)kVecWordsPerStream;
    const uint32_t *scal = reinterpret_cast<const uint32_t *>(st.scal + s * (int64_t)kNumScal);
    const uint32_t *hist = reinterpret_cast<const uint32_t *>(st.hist + s * (int64_t)kHistWordsPerStream);
    if (threadIdx.x < kBlobHeaderWords) {
        const uint32_t header[kBlobHeaderWords] = {kSnapshotMagic, kStateLayoutVersion, scal[S_MULT] * 8000u, (uint32_t)kNumVec, (uint32_t)kNumScal,
                                                   (uint32_t)kHistory, (uint32_t)kLanes, 0u};
        blob[threadIdx.x] = header[threadIdx.x];
    }
    for (int i = threadIdx.x; i < kBlobVecWords; i += 256) blob[kBlobHeaderWords + i] = vec[i];
    if (threadIdx.x < kBlobScalWords) blob[kBlobHeaderWords + kBlobVecWords + threadIdx.x] = scal[threadIdx.x];
    for (int i = threadIdx.x; i < kBlobHistWords; i += 256) blob[kBlobHeaderWords + kBlobVecWords + kBlobScalWords + i] = hist[i];
}

// result[0] = index of the first blob that may not be run on (atomicMin; the caller presets 0xffffffff), result[1] |= 1 when a
// blob of another sampling rate than fs_batch is among them.  64 threads per blob: thread t checks scalar field t and lane t,
// thread 0 the rule over the four supGainErrParam words as well.
__global__ __launch_bounds__(64) void aecm_validate_states_kernel(const uint32_t *blobs, int fs_batch, uint32_t *result) {
    const uint32_t *blob = blobs + (int64_t)blockIdx.x * kBlobWords;
    SnapshotHeader h;
    h.magic = blob[0]; h.version = blob[1]; h.fs = blob[2]; h.num_vec = blob[3]; h.num_scal = blob[4]; h.history = blob[5]; h.lanes = blob[6]; h.reserved = blob[7];
    const int t = threadIdx.x;
    const uint32_t *vec = blob + kBlobHeaderWords, *scal = vec + kBlobVecWords;
    int defect = SnapshotHeaderOk(h) ? 0 : 1;
    if (!defect) defect = ScalarFieldDefect(t, (int32_t)scal[t], (int)h.fs);
    if (!defect && t == 0) defect = SupGainErrParamsDefect((int32_t)scal[S_SG_A], (int32_t)scal[S_SG_D], (int32_t)scal[S_SG_DAB], (int32_t)scal[S_SG_DBD]);
    if (!defect) defect = LaneWordsDefect(t, vec[V_NEARFILT * kLanes + t], vec[V_NOISE * kLanes + t], vec[V_MEAN * kLanes + t], vec[V_M01 * kLanes + t]);
    if (__ballot(defect != 0) != 0 && t == 0) atomicMin(result, blockIdx.x);
    if (t == 0 && !defect && (int)h.fs != fs_batch) atomicOr(result + 1, 1u);
}

__global__ __launch_bounds__(256) void aecm_scatter_states_kernel(StatePtrs st, int first, const uint32_t *blobs) {
    const int64_t s = (int64_t)first + blockIdx.x;
    const uint32_t *blob = blobs + (int64_t)blockIdx.x * kBlobWords + kBlobHeaderWords;
    uint32_t *vec = st.vec + s * (int64_t)kVecWordsPerStream;
    uint32_t *scal = reinterpret_cast<uint32_t *>(st.scal + s * (int64_t)kNumScal);
    uint32_t *hist = reinterpret_cast<uint32_t *>(st.hist + s * (int64_t)kHistWordsPerStream);
    for (int i = threadIdx.x; i < kBlobVecWords; i += 256) vec[i] = blob[i];
    if (threadIdx.x < kBlobScalWords) scal[threadIdx.x] = blob[kBlobVecWords + threadIdx.x];
    for (int i = threadIdx.x; i < kBlobHistWords; i += 256) hist[i] = blob[kBlobVecWords + kBlobScalWords + i];
}

hipError_t LaunchGatherStates(const StatePtrs &st, int first, int count, void *blobs_dev, hipStream_t stream) {
    if (count <= 0) return hipSuccess;
    hipLaunchKernelGGL(aecm_gather_states_kernel, dim3(count), dim3(256), 0, stream, st, first, static_cast<uint32_t *>(blobs_dev));
    return hipGetLastError();
}
hipError_t LaunchValidateStates(const void *blobs_dev, int count, int fs_batch, uint32_t *result_dev, hipStream_t stream) {
    if (count <= 0) return hipSuccess;
    hipLaunchKernelGGL(aecm_validate_states_kernel, dim3(count), dim3(64), 0, stream, static_cast<const uint32_t *>(blobs_dev), fs_batch, result_dev);
    return hipGetLastError();
}
hipError_t LaunchScatterStates(const StatePtrs &st, int first, int count, const void *blobs_dev, hipStream_t stream) {
    if (count <= 0) return hipSuccess;
    hipLaunchKernelGGL(aecm_scatter_states_kernel, dim3(count), dim3(256), 0, stream, st, first, static_cast<const uint32_t *>(blobs_dev));
    return hipGetLastError();
}

// ---- session-schedule gather / scatter ---------------------------------------------------------------

// One workgroup per (stream, 256-sample tile); the stream index is folded into blockIdx.x (no 65 535 grid.y limit).
__global__ void aecm_gather_by_map_kernel(const int16_t *src, int64_t src_stride, const int32_t *map, int64_t n,
                                          int16_t *dst, int64_t dst_stride, unsigned tiles) {
    const int64_t s = blockIdx.x / tiles;
    const int64_t j = (int64_t)(blockIdx.x % tiles) * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const int32_t m = map[j];
    dst[s * dst_stride + j] = m >= 0 ? src[s * src_stride + m] : (int16_t)0;
}

// The host side cuts batches so that n_streams * tiles fits a 31-bit grid (aecm_engine.cpp).
hipError_t LaunchGatherByMap(const int16_t *src, int64_t src_stride, const int32_t *map_dev, int64_t n, int16_t *dst,
                             int64_t dst_stride, int n_streams, hipStream_t stream) {
    if (n <= 0 || n_streams <= 0) return hipSuccess;
    const int64_t tiles = (n + 255) / 256;
    if (tiles * n_streams > 0x7fffffffll) return hipErrorInvalidValue;
    hipLaunchKernelGGL(aecm_gather_by_map_kernel, dim3((unsigned)(tiles * n_streams)), dim3(256), 0, stream, src,
                       src_stride, map_dev, n, dst, dst_stride, (unsigned)tiles);
    return hipGetLastError();
}

__global__ void aecm_assemble_output_kernel(const int16_t *blocks, int64_t blocks_stride, const int16_t *near,
                                            int64_t near_stride, const int32_t *map, int64_t n, int16_t *out,
                                            int64_t out_stride, unsigned tiles, const int32_t *sample_limit) {
    const int64_t s = blockIdx.x / tiles;
    const int64_t j = (int64_t)(blockIdx.x % tiles) * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const int32_t v = map[j];
    int16_t r = 0;
    if (sample_limit && j >= sample_limit[s]) r = 0;       // behind this stream's last call (ragged recordings): nothing was processed
    else if (v >= 0) r = blocks[s * blocks_stride + v];
    else if (v <= -2) r = near[s * near_stride + (-(int64_t)v - 2)];
    out[s * out_stride + j] = r;
}

hipError_t LaunchAssembleOutput(const int16_t *blocks, int64_t blocks_stride, const int16_t *near, int64_t near_stride,
                                const int32_t *map_dev, int64_t n, int16_t *out, int64_t out_stride, int n_streams,
                                hipStream_t stream, const int32_t *sample_limit_dev) {
    if (n <= 0 || n_streams <= 0) return hipSuccess;
    const int64_t tiles = (n + 255) / 256;
    if (tiles * n_streams > 0x7fffffffll) return hipErrorInvalidValue;
    hipLaunchKernelGGL(aecm_assemble_output_kernel, dim3((unsigned)(tiles * n_streams)), dim3(256), 0, stream,
                       blocks, blocks_stride, near, near_stride, map_dev, n, out, out_stride, (unsigned)tiles, sample_limit_dev);
    return hipGetLastError();
}

// ---- device-resident session machinery (aecm_flow_plan.h) ---------------------------------------------
#include "aecm_tick_unit.h"      // TickBlockIo, the build's choices for the tick kernels, AECM_TICK_LIVE_SESSION

// One lane per session: the tick's session machinery for 64 sessions per wavefront.
__global__ __launch_bounds__(256)
void aecm_flow_plan_kernel(TickFlowIo fio, int n, unsigned near_pos, int n_streams) {
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= n_streams) return;
    FlowRegs r;
    for (int k = 0; k < kFlowTickFields; ++k) r.v[k] = fio.state[(size_t)k * n_streams + s];
    const int ms = fio.ms_per_session ? (int)fio.ms_per_session[s] : fio.ms;
    const int flags = fio.flags_per_session ? (int)fio.flags_per_session[s] : fio.flags;
    FlowPlan p;
    FlowTick(r, fio.fs, n, ms, flags, near_pos, p);
    for (int k = 0; k < kFlowTickFields; ++k) fio.state[(size_t)k * n_streams + s] = r.v[k];
    int32_t w[kFlowPlanWords];
    FlowPackPlan(p, w);
    int4 *dst = reinterpret_cast<int4 *>(fio.plans + (size_t)s * kFlowPlanWords);
    for (int q = 0; q < kFlowPlanWords / 4; ++q) dst[q] = make_int4(w[4 * q], w[4 * q + 1], w[4 * q + 2], w[4 * q + 3]);
}

// The same for a tick in which sessions may sit out (kFlowIdle) or may have done so before: idle lanes count their session's lag,
// returning ones are brought back in step, and with a live list to fill (sp.live) a calling lane writes its session's id to its
// slot of it.  The text is shared with the other planning kernels (aecm_flow_plan_list.inc, aecm_flow_plan_lane.inc).
static_assert(kFlowPlanBlock == 256, "the planning kernels run 256 lanes per workgroup");
__global__ __launch_bounds__(256)
void aecm_flow_plan_sparse_kernel(TickFlowIo fio, TickSparseIo sp, int n, unsigned near_pos, int n_streams) {
    __shared__ uint32_t wave_counts[kFlowPlanBlock / 64];
#define AECM_FLOW_PLAN_LIST_GUARD if (sp.live)
#include "aecm_flow_plan_list.inc"
#define AECM_FLOW_PLAN_IDLE_SAMPLES n
#define AECM_FLOW_PLAN_TICK(p) FlowTick(r, fio.fs, n, ms, flags, near_pos, p)
#include "aecm_flow_plan_lane.inc"
}

// The planning launch of a tick of an object of mixed rates / call sizes (aecm_flow_plan.h: FlowRouteTickMixed): the object holds
// sessions of both rates, or a session makes a half call (kFlowHalfCall) in this tick.  Everything the sparse planning kernel
// above does, except that the lane takes its session's rate from the core state (scal = StatePtrs::scal, S_MULT: what the block
// engine itself goes by) instead of the object's, and plans with FlowTickMixed: a half call is one call pair of 80 samples that
// leaves the session 80 samples behind.
__device__ __forceinline__ void FlowPlanMixedBody(const TickFlowIo &fio, const TickSparseIo &sp, const int32_t *scal, int n, unsigned near_pos,
                                                   int n_streams, uint32_t *wave_counts) {
#define AECM_FLOW_PLAN_LIST_GUARD if (sp.live)
#include "aecm_flow_plan_list.inc"
#define AECM_FLOW_PLAN_IDLE_SAMPLES n
#define AECM_FLOW_PLAN_TICK(p) FlowTickMixed(r, scal[(size_t)s * kNumScal + S_MULT] == 2 ? 16000 : 8000, n, ms, flags, near_pos, p)
#include "aecm_flow_plan_lane.inc"
}
__global__ __launch_bounds__(256)
void aecm_flow_plan_mixed_kernel(TickFlowIo fio, TickSparseIo sp, const int32_t *__restrict__ scal, int n, unsigned near_pos, int n_streams) {
    __shared__ uint32_t wave_counts[kFlowPlanBlock / 64];
    FlowPlanMixedBody(fio, sp, scal, n, near_pos, n_streams, wave_counts);
}

// (aecm_tick_unit.h: four sessions per workgroup, 7 waves per SIMD, and the measurements behind both.)
template <bool kHasClean>
__global__ __launch_bounds__(64 * kTickFlowWaves) __attribute__((amdgpu_waves_per_eu(AECM_TICK_FLOW_WAVES_PER_EU, 8)))
void aecm_tick_flow_kernel(StatePtrs st, TickIo io, TickFlowIo fio, int n_streams) {
    const int64_t s = (int64_t)blockIdx.x * kTickFlowWaves + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int lane = threadIdx.x & 63;
#include "aecm_tick_flow_body.inc"
}
// The tick of the sessions that call, in an object where others sit the tick out (AECM_SESSION_IDLE): wavefront w of the grid
// serves session live[w], w < live_count (the list aecm_flow_plan_sparse_kernel wrote; AECM_TICK_LIVE_SESSION, aecm_tick_unit.h,
// ahead of the early state loads).
template <bool kHasClean>
__global__ __launch_bounds__(64 * kTickFlowWaves) __attribute__((amdgpu_waves_per_eu(AECM_TICK_FLOW_WAVES_PER_EU, 8)))
void aecm_tick_flow_sparse_kernel(StatePtrs st, TickIo io, TickFlowIo fio, int n_streams, const uint32_t *__restrict__ live, int live_count) {
    const int64_t wave_id = (int64_t)blockIdx.x * kTickFlowWaves + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    AECM_TICK_LIVE_SESSION(live, live_count, wave_id)
    const int lane = threadIdx.x & 63;
#include "aecm_tick_flow_body.inc"
}

int TickWorkgroupWaves() { return kTickFlowWaves; }
int TickWorkgroupsPerCu() {       // by the wave slots the kernel is built for, and by the LDS its tables take
    const int by_waves = 4 * AECM_TICK_FLOW_WAVES_PER_EU / kTickFlowWaves, by_lds = (int)((160 * 1024) / sizeof(LdsTables));
    return by_waves < by_lds ? by_waves : by_lds;
}

// The planning launch of a tick of one call pair alone (the launchers below call it, and their traced twins in
// aecm_tick_trace_kernels.hip): sp == nullptr: the dense planning kernel; else the sparse one or, with mixed_plan, the mixed one.
hipError_t LaunchPlanFlow(const StatePtrs &st, const TickIo &io, const TickFlowIo &fio, const TickSparseIo *sp, int n_streams, bool mixed_plan,
                          hipStream_t stream) {
    if (n_streams <= 0) return hipSuccess;
    const dim3 grid((n_streams + 255) / 256), block(256);
    if (!sp) hipLaunchKernelGGL(aecm_flow_plan_kernel, grid, block, 0, stream, fio, io.n, (unsigned)io.near_pos, n_streams);
    else if (mixed_plan) hipLaunchKernelGGL(aecm_flow_plan_mixed_kernel, grid, block, 0, stream, fio, *sp, st.scal, io.n, (unsigned)io.near_pos, n_streams);
    else hipLaunchKernelGGL(aecm_flow_plan_sparse_kernel, grid, block, 0, stream, fio, *sp, io.n, (unsigned)io.near_pos, n_streams);
    return hipGetLastError();
}

hipError_t LaunchTickFlow(const StatePtrs &st, const TickIo &io, const TickFlowIo &fio, int n_streams, hipStream_t stream) {
    if (n_streams <= 0) return hipSuccess;
    (void)LaunchPlanFlow(st, io, fio, nullptr, n_streams, false, stream);
    const dim3 grid((n_streams + kTickFlowWaves - 1) / kTickFlowWaves), block(64 * kTickFlowWaves);
    const size_t lds = sizeof(LdsTables);
    if (io.clean_in) hipLaunchKernelGGL((aecm_tick_flow_kernel<true>), grid, block, lds, stream, st, io, fio, n_streams);
    else hipLaunchKernelGGL((aecm_tick_flow_kernel<false>), grid, block, lds, stream, st, io, fio, n_streams);
    return hipGetLastError();
}

hipError_t LaunchTickFlowSparse(const StatePtrs &st, const TickIo &io, const TickFlowIo &fio, const TickSparseIo &sp, int n_streams, int live_count,
                                hipStream_t stream, bool mixed_plan) {
    if (n_streams <= 0) return hipSuccess;
    if (live_count < 0 || live_count > n_streams || (sp.live && !sp.block_base)) return hipErrorInvalidValue;
    // the planning launch runs over ALL sessions (the idle ones count their lag); the tick launch over the live ones only
    (void)LaunchPlanFlow(st, io, fio, &sp, n_streams, mixed_plan, stream);
    const dim3 block(64 * kTickFlowWaves);
    const size_t lds = sizeof(LdsTables);
    if (!sp.live) {                        // nobody idles in this tick (some had, before): everybody is live, the dense tick kernel
        const dim3 grid((n_streams + kTickFlowWaves - 1) / kTickFlowWaves);
        if (io.clean_in) hipLaunchKernelGGL((aecm_tick_flow_kernel<true>), grid, block, lds, stream, st, io, fio, n_streams);
        else hipLaunchKernelGGL((aecm_tick_flow_kernel<false>), grid, block, lds, stream, st, io, fio, n_streams);
    } else if (live_count > 0) {
        const dim3 grid((live_count + kTickFlowWaves - 1) / kTickFlowWaves);
        if (io.clean_in) hipLaunchKernelGGL((aecm_tick_flow_sparse_kernel<true>), grid, block, lds, stream, st, io, fio, n_streams, sp.live, live_count);
        else hipLaunchKernelGGL((aecm_tick_flow_sparse_kernel<false>), grid, block, lds, stream, st, io, fio, n_streams, sp.live, live_count);
    }
    return hipGetLastError();
}

// WebRtcAecm_BufferFarend calls without a Process (far-end bursts), one wavefront per session: the few wrapper fields a
// burst touches (aecm_flow_plan.h: FlowBurstReads) into scalar registers, replay frames the burst could lap in the far
// ring to their rows first, then call by call FlowFarendCall and the accepted samples into the far ring.  Session s makes
// clamp(calls_per_session[s] - call_base, 0, max_calls) calls (everybody max_calls without the array) on the samples
// far_in[s][c * n .. + n), c = 0, 1, ...
__global__ __launch_bounds__(256)
void aecm_buffer_farend_kernel(TickIo io, TickFlowIo fio, const int32_t *__restrict__ scal, const uint8_t *calls_per_session, int call_base, int max_calls,
                               int n_streams) {
    const int64_t s = (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (s >= n_streams) return;
    const int lane = threadIdx.x & 63;
    int calls = max_calls;
    if (calls_per_session) calls = FlowMin(FlowMax((int)calls_per_session[s] - call_base, 0), max_calls);
    calls = __builtin_amdgcn_readfirstlane(calls);
    if (calls <= 0) return;
    FlowRegs r;
    FlowBurstReads([&](int f) { r.v[f] = __builtin_amdgcn_readfirstlane(fio.state[(size_t)f * n_streams + s]); });
    // the session's own rate: the core state's (what the block engine goes by)
    const int mask = (int)io.ring_len - 1, n = io.n, mult = __builtin_amdgcn_readfirstlane(scal[s * kNumScal + S_MULT]) == 2 ? 2 : 1;
    int16_t *fr = io.far_ring + s * io.ring_len, *old = fio.far_old + s * (2 * kFlowFrame);
    const int16_t *fin = io.far_in + s * io.io_stride;
    FlowBurst b;
    FlowBurstBegin(r, n, calls, b);
    if (b.spill[0] | b.spill[1]) {
        for (int i = 0; i < 2; ++i) {
            if (!b.spill[i]) continue;
            int16_t *row = old + i * kFlowFrame;
            const int16_t a0 = fr[(b.spill_pos[i] + lane) & mask], a1 = fr[(b.spill_pos[i] + 64 + (lane & 15)) & mask];
            row[lane] = a0;
            if (lane < kFlowFrame - 64) row[64 + lane] = a1;
        }
        // the rows have their samples (the stores above needed the loaded values) before the burst may overwrite them in the ring
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    }
    for (int c = 0; c < calls; ++c) {
        const unsigned pos = (unsigned)r.v[F_FAR_WP];
        const int accepted = FlowFarendCall(r, mult, n);
        for (int j = lane; j < accepted; j += 64) fr[(pos + (unsigned)j) & mask] = fin[c * n + j];
    }
    if (lane == 0) FlowBurstWrites([&](int f) { fio.state[(size_t)f * n_streams + s] = r.v[f]; });
}

hipError_t LaunchBufferFarend(const StatePtrs &st, const TickIo &io, const TickFlowIo &fio, const uint8_t *calls_per_session, int call_base, int max_calls,
                              int n_streams, hipStream_t stream) {
    if (n_streams <= 0 || max_calls <= 0) return hipSuccess;
    hipLaunchKernelGGL(aecm_buffer_farend_kernel, dim3((n_streams + 3) / 4), dim3(256), 0, stream, io, fio, st.scal, calls_per_session, call_base, max_calls,
                       n_streams);
    return hipGetLastError();
}

__global__ __launch_bounds__(256)
void aecm_reset_sessions_kernel(TickIo io, TickFlowIo fio, int n_streams, int first) {
    const int64_t s = (int64_t)first + blockIdx.x;
    auto zero = [&](int16_t *row, int64_t n_samples) {                       // rows are 4-byte aligned and even-sized
        uint32_t *w = reinterpret_cast<uint32_t *>(row);
        for (int64_t i = threadIdx.x; i < n_samples / 2; i += 256) w[i] = 0u;
    };
    zero(io.far_ring + s * io.ring_len, io.ring_len);
    zero(io.out_ring + s * io.ring_len, io.ring_len);
    zero(fio.far_frames + s * kFlowFarFrameRing, kFlowFarFrameRing);
    zero(fio.far_old + s * (2 * kFlowFrame), 2 * kFlowFrame);
    if (threadIdx.x < kFlowFieldsUsed) fio.state[(size_t)threadIdx.x * n_streams + s] = FlowFieldStartsAtOne((int)threadIdx.x) ? 1 : 0;
}

hipError_t LaunchResetSessions(const TickIo &io, const TickFlowIo &fio, int n_streams, int first, int count, hipStream_t stream) {
    if (count <= 0) return hipSuccess;
    hipLaunchKernelGGL(aecm_reset_sessions_kernel, dim3(count), dim3(256), 0, stream, io, fio, n_streams, first);
    return hipGetLastError();
}

// ---- self test of the wave primitives ------------------------------------------------------------

__device__ __forceinline__ unsigned Mix(unsigned x) {
    x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
    return x;
}

template <int Q>
__device__ __forceinline__ void TestExchange(int va, int vb, uint64_t *fails) {
    int a0 = va, b0 = vb, a1 = va, b1 = vb;
    Gfx950Wave<false>::exchange<Q>(a0, b0);
    Gfx950Wave<true>::exchange<Q>(a1, b1);
    // definition: lanes with bit Q clear keep a, b <- partner's a; lanes with bit Q set keep b, a <- partner's b
    const int lane = threadIdx.x & 63;
    const int pa = __shfl(va, lane ^ (1 << Q)), pb = __shfl(vb, lane ^ (1 << Q));
    const int ea = ((lane >> Q) & 1) ? pb : va, eb = ((lane >> Q) & 1) ? vb : pa;
    if (a0 != ea || b0 != eb) atomicAdd((unsigned long long *)&fails[1], 1ull);
    if (a1 != ea || b1 != eb) atomicAdd((unsigned long long *)&fails[1], 1ull);
}

// exchange_all (the N-transform form, DPP-select assembly for the quad stages) against N applications of the definition
template <int Q, int N>
__device__ __forceinline__ void TestExchangeAll(int va, int vb, uint64_t *fails) {
    const int lane = threadIdx.x & 63;
    int aa[N], bb[N], ea[N], eb[N];
    for (int n = 0; n < N; ++n) {
        aa[n] = (int)Mix((unsigned)va + 0x9e37u * n);
        bb[n] = (int)Mix((unsigned)vb ^ (0x85ebu * (n + 1)));
        const int pa = __shfl(aa[n], lane ^ (1 << Q)), pb = __shfl(bb[n], lane ^ (1 << Q));
        ea[n] = ((lane >> Q) & 1) ? pb : aa[n];
        eb[n] = ((lane >> Q) & 1) ? bb[n] : pa;
    }
    Gfx950Wave<true>::exchange_all<Q, N>(aa, bb);
    for (int n = 0; n < N; ++n)
        if (aa[n] != ea[n] || bb[n] != eb[n]) atomicAdd((unsigned long long *)&fails[1], 1ull);
}

__global__ __launch_bounds__(256) void aecm_selftest_kernel(uint64_t *fails, int exhaustive, const uint32_t *consts) {
    FillLdsTables<256>(consts);
    using S = Gfx950Wave<false>;
    using F = Gfx950Wave<true>;
    const int lane = threadIdx.x & 63;
    const unsigned gid = blockIdx.x * blockDim.x + threadIdx.x;
    auto bump = [&](int k) { atomicAdd((unsigned long long *)&fails[k], 1ull); };

    if (blockIdx.x < 64) {
        for (int round = 0; round < 16; ++round) {
            const int v = (int)Mix(gid * 977u + round * 131071u + 1u);
            const int w = (int)Mix(gid * 31u + round * 8191u + 7u);
            // 0: xor shuffles against __shfl with an explicit source lane
            if (F::shfl_xor<1>(v) != __shfl(v, lane ^ 1)) bump(0);
            if (F::shfl_xor<2>(v) != __shfl(v, lane ^ 2)) bump(0);
            if (F::shfl_xor<4>(v) != __shfl(v, lane ^ 4)) bump(0);
            if (F::shfl_xor<8>(v) != __shfl(v, lane ^ 8)) bump(0);
            if (F::shfl_xor<16>(v) != __shfl(v, lane ^ 16)) bump(0);
            if (F::shfl_xor<32>(v) != __shfl(v, lane ^ 32)) bump(0);
            // 1: FFT operand exchange on every lane bit
            TestExchange<0>(v, w, fails); TestExchange<1>(v, w, fails); TestExchange<2>(v, w, fails);
            TestExchange<3>(v, w, fails); TestExchange<4>(v, w, fails); TestExchange<5>(v, w, fails);
            TestExchangeAll<0, 1>(v, w, fails); TestExchangeAll<0, 2>(v, w, fails); TestExchangeAll<0, 3>(v, w, fails);
            TestExchangeAll<1, 1>(v, w, fails); TestExchangeAll<1, 2>(v, w, fails); TestExchangeAll<1, 3>(v, w, fails);
            TestExchangeAll<2, 2>(v, w, fails); TestExchangeAll<5, 3>(v, w, fails);
            // 2: reductions against a serial readlane loop
            int mx = (int)0x80000000, mn = 0x7fffffff, sm = 0;
            for (int i = 0; i < 64; ++i) {
                const int x = __shfl(v, i);
                mx = x > mx ? x : mx; mn = x < mn ? x : mn; sm = add(sm, x);
            }
            if (F::reduce_max(v) != mx || S::reduce_max(v) != mx) bump(2);
            if (F::reduce_min(v) != mn || S::reduce_min(v) != mn) bump(2);
            if (F::reduce_add(v) != sm || S::reduce_add(v) != sm) bump(2);
            {   // merged reductions
                int a0, a1, a2, a3, mn2, mx2;
                int sw = 0, mxw = (int)0x80000000, mnv = 0x7fffffff, mxq = (int)0x80000000;
                const int q = (int)(Mix((unsigned)w) >> 1);            // >= 0 (reduce_min_max negates)
                const int z = (int)Mix((unsigned)v ^ 0x51ed27u), u4 = (int)Mix((unsigned)w + 77u);
                int sz = 0, su = 0;
                for (int i = 0; i < 64; ++i) {
                    const int xw = __shfl(w, i), xz = __shfl(z, i), xu = __shfl(u4, i), xq = __shfl(q, i), xv = __shfl(v, i);
                    sw = add(sw, xw); sz = add(sz, xz); su = add(su, xu);
                    mxw = xw > mxw ? xw : mxw; mnv = xv < mnv ? xv : mnv; mxq = xq > mxq ? xq : mxq;
                }
                F::reduce_max2(v, w, a0, a1);
                if (a0 != mx || a1 != mxw) bump(2);
                S::reduce_max2(v, w, a0, a1);
                if (a0 != mx || a1 != mxw) bump(2);
                F::reduce_min_max(v, q, mn2, mx2);
                if (mn2 != mnv || mx2 != mxq) bump(2);
                S::reduce_min_max(v, q, mn2, mx2);
                if (mn2 != mnv || mx2 != mxq) bump(2);
                F::reduce_add4(v, w, z, u4, a0, a1, a2, a3);
                if (a0 != sm || a1 != sw || a2 != sz || a3 != su) bump(2);
                S::reduce_add4(v, w, z, u4, a0, a1, a2, a3);
                if (a0 != sm || a1 != sw || a2 != sz || a3 != su) bump(2);
            }
            // 3: whole-wave shift by one lane with fill
            const int up = __shfl(v, lane == 0 ? 0 : lane - 1);
            const int expect_up = lane == 0 ? 12345 + round : up;
            if (F::shift_up1(v, 12345 + round) != expect_up || S::shift_up1(v, 12345 + round) != expect_up) bump(3);
            // 4: bpermute / readlane / writelane
            const int src = (int)(Mix(gid + round) & 63u);
            if (F::bpermute(v, src) != __shfl(v, src)) bump(4);
            const int sel_lane = (round * 7 + (int)blockIdx.x) & 63;
            if (F::readlane(v, sel_lane) != __shfl(v, sel_lane)) bump(4);
            const int wl = F::writelane(v, 424242, sel_lane);
            if (wl != (lane == sel_lane ? 424242 : v)) bump(4);
            // 4 (cont.): packed-int16 primitives against their portable definitions
            {
                const int x = v, y = w, c = (int)Mix(gid ^ 0x9e3779b9u);
                const int ed = add(add(mul(sext16(x), sext16(y)), mul(sar(x, 16), sar(y, 16))), c);
                if (dot2_i16(x, y, c) != ed) bump(4);
                if (pack_hi16(x, y) != (int)(((unsigned)x >> 16) | ((unsigned)y & 0xffff0000u))) bump(4);
                int lo = sext16(x), hi = sar(x, 16);
                lo = lo < 0 ? (lo == -32768 ? 32767 : -lo) : lo;
                hi = hi < 0 ? (hi == -32768 ? 32767 : -hi) : hi;
                if (pk_abs_sat_i16(x) != ((lo & 0xffff) | (int)((unsigned)hi << 16))) bump(4);
                if (pk_abs_sat_i16((int)0x80008000) != 0x7fff7fff) bump(4);
                // v_mad_i32_i16 with and without op_sel, vector and scalar addend
                const int uc = (int)Mix((unsigned)round * 2654435761u + blockIdx.x);   // wave-uniform
                if (mad16_lo(x, y, c) != add(mul(sext16(x), sext16(y)), c)) bump(4);
                if (mad16_hi(x, y, c) != add(mul(sar(x, 16), sext16(y)), c)) bump(4);
                if (mad16_lo_uc(x, y, uc) != add(mul(sext16(x), sext16(y)), uc)) bump(4);
                if (mad16_hi_uc(x, y, uc) != add(mul(sar(x, 16), sext16(y)), uc)) bump(4);
                if (mad16_lo((int)0x80008000, -32768, 1) != 0x40000001 || mad16_hi((int)0x7fff0000, -32768, -32770) != (int)0xbffffffe) bump(4);
                {   // per-half saturating add (v_pk_add_i16 clamp): random words and words that saturate either way
                    const int xs[3] = {x, (int)0x7fff8000, (int)0x80017ffe}, ys[3] = {y, (int)0x0001ffff, (int)0xfffe0003};
                    for (int k = 0; k < 3; ++k) {
                        int lo = sext16(xs[k]) + sext16(ys[k]), hi = sar(xs[k], 16) + sar(ys[k], 16);
                        lo = lo > 32767 ? 32767 : lo < -32768 ? -32768 : lo;
                        hi = hi > 32767 ? 32767 : hi < -32768 ? -32768 : hi;
                        if (pk_add_sat_i16(xs[k], ys[k]) != ((lo & 0xffff) | (int)((unsigned)hi << 16))) bump(4);
                    }
                }
                const int ml = imax(sext16(x), sext16(y)), mh = imax(sar(x, 16), sar(y, 16));
                if (pk_max_i16(x, y) != ((ml & 0xffff) | (int)((unsigned)mh << 16))) bump(4);
                // per half "non-zero" (v_pk_min_u16 with an inline constant, as assembly); random words and words with an empty half
                const int xz[4] = {x, x & 0xffff, (int)((unsigned)x & 0xffff0000u), 0};
                for (int k = 0; k < 4; ++k)
                    if (pk_nonzero_u16(xz[k]) != ((((unsigned)xz[k] & 0xffffu) != 0 ? 1 : 0) | (((unsigned)xz[k] >> 16) != 0 ? 0x10000 : 0))) bump(4);
            }
            // 5: ballot bit order
            const bool p = (v >> 3) & 1;
            const uint64_t bal = F::ballot(p);
            if (((bal >> lane) & 1ull) != (p ? 1ull : 0ull)) bump(5);
            if (__builtin_popcountll(bal) != F::reduce_add(p ? 1 : 0)) bump(5);
        }
        // 7: LDS tables
        if (threadIdx.x < 64) {
            {   // last stage: lane t uses entry bitrev6(t); stage 0: entry 0 for every lane
                int wre, wim, brev = 0;
                for (int b = 0; b < 6; ++b) brev |= ((lane >> b) & 1) << (5 - b);
                F::template twiddles<6, false>(wre, wim);
                if (sext16(wre) != kAecmTwiddleCosQ15[brev] || sar(wre, 16) != kAecmTwiddleSinQ15[brev]) bump(7);
                if (sext16(wim) != -kAecmTwiddleSinQ15[brev] || sar(wim, 16) != kAecmTwiddleCosQ15[brev]) bump(7);
                F::template twiddles<6, true>(wre, wim);
                if (sext16(wre) != kAecmTwiddleCosQ15[brev] || sar(wre, 16) != -kAecmTwiddleSinQ15[brev]) bump(7);
                F::template twiddles<0, true>(wre, wim);
                if (wre != 32767 || wim != (int)(32767u << 16)) bump(7);
            }
            if (F::hann(lane + 1) != kAecmSqrtHanningQ14[lane + 1]) bump(7);
            for (int i = lane; i < 360; i += 64)
                if (F::cos360(i) != kAecmCosQ13[i] || F::sin360(i) != kAecmSinQ13[i]) bump(7);
        }
    }
    // 6: floor(sqrt) -- exhaustive over [0, 2^31) in grid-stride, or a 2^24-point sample
    const uint64_t total = exhaustive ? (1ull << 31) : (1ull << 24);
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = gid; i < total; i += stride) {
        const unsigned x = exhaustive ? (unsigned)i : (Mix((unsigned)i) & 0x7fffffffu);
        const uint64_t r = (unsigned)F::isqrt31((int)x);
        if (r * r > x || (r + 1) * (r + 1) <= x) bump(6);
    }
    // 6 (cont.): floor(n / d) of the Wiener gain for EVERY divisor 1..65535: dividends around multiples of d (where an
    // off-by-one would show), the extremes, and random ones -- 64 (quick) or 1 024 (exhaustive) dividends per divisor and thread slot
    {
        const int per = exhaustive ? 1024 : 64;
        for (uint64_t i = gid; i < 65535ull * (unsigned)per; i += stride) {
            const unsigned d = 1u + (unsigned)(i % 65535ull), j = (unsigned)(i / 65535ull);
            const unsigned h = Mix((unsigned)i * 2654435761u + 12345u);
            unsigned n;
            switch (j & 7u) {
                case 0: n = h; break;
                case 1: n = (h / d) * d; break;                       // an exact multiple
                case 2: n = (h / d) * d - 1u; break;                  // one below a multiple (wraps to 2^32 - 1 for h < d)
                case 3: n = (h / d) * d + d - 1u; break;
                case 4: n = 0xffffffffu - (h & 0xffffu); break;       // the top of the range
                case 5: n = h & 0xffffu; break;                       // small dividends
                case 6: n = (0xffffffffu / d) * d - (j >> 3 & 1u); break;
                default: n = h >> (h & 31u); break;
            }
            if ((unsigned)F::divu_u32_u16((int)n, (int)d) != n / d) bump(6);
        }
    }
    // edge values
    if (gid == 0) {
        const unsigned edges[7] = {0u, 1u, 0x7fffffffu, 0x7ffea810u /*46340^2*/, 0x7ffea80fu, 0x40000000u, 0x80000000u};
        for (int k = 0; k < 7; ++k) {
            const uint64_t r = (unsigned)F::isqrt31((int)edges[k]);
            if (r * r > edges[k] || (r + 1) * (r + 1) <= edges[k]) bump(6);
        }
    }
}

template <bool kFast>
__global__ __launch_bounds__(256) void aecm_fft128_kernel(int16_t *data, int32_t *scales, int variant, int count,
                                                          const uint32_t *consts) {
    FillLdsTables<256>(consts);
    using E = BlockEngine<Gfx950Wave<kFast>, false>;
    const int lane = threadIdx.x & 63;
    const int k = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (k >= count) return;
    int16_t *re = data + (size_t)k * 256, *im = re + 128;
    int a = (re[lane] & 0xffff) | (int)((unsigned)(variant == 0 ? 0 : im[lane]) << 16);
    int b = (re[lane + 64] & 0xffff) | (int)((unsigned)(variant == 0 ? 0 : im[lane + 64]) << 16);
    int scale = 0;
    const int kp = Gfx950Wave<kFast>::opaque_const(32770);
    if (variant == 0) scale = E::template fft128<false, true>(a, b, kp);
    else if (variant == 1) scale = E::template fft128<false, false>(a, b, kp);
    else {
        scale = E::template fft128<true, false>(a, b, kp);
        a >>= 16;                                   // the inverse transform hands its real parts on in the upper halves
        b >>= 16;
    }
    int r = 0;
    for (int i = 0; i < 6; ++i) r |= ((lane >> i) & 1) << (5 - i);
    re[r] = (int16_t)a;
    re[r + 64] = (int16_t)b;
    im[r] = variant == 2 ? (int16_t)0 : (int16_t)(a >> 16);
    im[r + 64] = 0;
    if (lane == 0) scales[k] = scale;
}
hipError_t LaunchFft128(int16_t *data_dev, int32_t *scales_dev, int variant, int fast, int count, const uint32_t *consts_dev,
                        hipStream_t stream) {
    if (count <= 0) return hipSuccess;
    const dim3 grid((count + 3) / 4), block(256);
    if (fast) hipLaunchKernelGGL(aecm_fft128_kernel<true>, grid, block, sizeof(LdsTables), stream, data_dev, scales_dev, variant, count, consts_dev);
    else hipLaunchKernelGGL(aecm_fft128_kernel<false>, grid, block, sizeof(LdsTables), stream, data_dev, scales_dev, variant, count, consts_dev);
    return hipGetLastError();
}

hipError_t LaunchSelfTest(uint64_t *counters_dev, int exhaustive, const uint32_t *consts_dev, hipStream_t stream) {
    hipLaunchKernelGGL(aecm_selftest_kernel, dim3(exhaustive ? 4096 : 256), dim3(256), sizeof(LdsTables), stream,
                       counters_dev, exhaustive, consts_dev);
    return hipGetLastError();
}

}  // namespace aecm
