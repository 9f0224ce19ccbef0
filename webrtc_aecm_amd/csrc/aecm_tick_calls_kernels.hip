// The K-call tick of the streaming sessions (WebRtcAecmSessions_TickCalls): K = 2 .. 6 [BufferFarend] + Process call pairs
// of n samples per session in ONE planning launch and ONE tick launch -- the 20 / 40 / 60 ms packet interval of a media
// server on 10 ms calls.  K ordinary ticks load and store a session's core state K times; here it is loaded once, stays in
// registers across the K call pairs, and is stored once.
//   aecm_flow_plan_calls_kernel   one LANE per session: what aecm_flow_plan_sparse_kernel does (idle lanes, resync, the live
//                                 list), then FlowTickCalls -> K packed plans per session (aecm_tick_calls_plan_kernels.hip)
//   aecm_tick_calls_kernel        one WAVEFRONT per live session: for c = 0 .. K - 1 the five steps of a tick (append, spill,
//                                 far framing, blocks, output frames) with plan c and the rows offset by c * n
// A unit of its own: the tick kernels of aecm_kernels.hip stay, instruction for instruction, what they were.  Compiled with
// that unit's flags (build.py: SOURCE_FLAGS).
#define AECM_TABLE_ATTR __device__
#if defined(AECM_CHECKED)
#define g_aecm_check_fail g_aecm_check_fail_tick_calls      // device symbols are per translation unit (no relocatable device code)
#endif
#include "aecm_kernel_common.h"

namespace aecm {

#if defined(AECM_CHECKED)
__device__ unsigned long long g_aecm_check_fail_tick_calls[2];
#endif
// This unit's share of the audit counters of the -DAECM_CHECKED build (aecm_ops.h); hipErrorNotSupported in the shipped build.
hipError_t ReadTickCallsCheckCounters(uint64_t counters[2], bool reset) {
#if defined(AECM_CHECKED)
    unsigned long long host[2] = {0, 0};
    hipError_t e = hipMemcpyFromSymbol(host, HIP_SYMBOL(g_aecm_check_fail_tick_calls), sizeof host);
    if (e != hipSuccess) return e;
    counters[0] = host[0];
    counters[1] = host[1];
    if (reset) {
        const unsigned long long zero[2] = {0, 0};
        e = hipMemcpyToSymbol(HIP_SYMBOL(g_aecm_check_fail_tick_calls), zero, sizeof zero);
    }
    return e;
#else
    (void)counters;
    (void)reset;
    return hipErrorNotSupported;
#endif
}

// Where the blocks of ONE call fetch and deliver (the tick kernel's TickFlowBlockIo, for this unit).
template <bool kHasClean, class Append>
struct TickCallsBlockIo {
    using E = BlockEngine<Gfx950Wave<true, true, true>, kHasClean>;
    using Regs = typename E::Regs;
    const int16_t *far_src;          // the far ring itself (direct calls) or the framed far stream
    const int16_t *nr, *cr;          // near / clean rings of this session
    int16_t *out_row;                // output stream ring
    int far_mask, mask;
    unsigned far_pos, near_pos, out_pos;      // positions of the call's first block in far_src / the near rings / the output ring
    const Append &append;            // the call's samples -> rings
    __device__ __forceinline__ int far(const Regs &r, int b) const { return far_src[(far_pos + b * kBlock + r.lane) & far_mask]; }
    __device__ __forceinline__ int near(const Regs &r, int b) const { return nr[(near_pos + b * kBlock + r.lane) & mask]; }
    __device__ __forceinline__ int clean(const Regs &r, int b) const { return cr[(near_pos + b * kBlock + r.lane) & mask]; }
    __device__ __forceinline__ void out(const Regs &r, int b, int v) const { out_row[(out_pos + b * kBlock + r.brev) & mask] = (int16_t)v; }
    // The call's samples go into the rings here, then this wave's fetches must see this wave's stores -- those of this call
    // and those of the calls before it (far samples appended in call c are read from the ring by call c + 1).
    __device__ __forceinline__ void ready() const {
        append();
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    }
};

// Built like the tick kernel: four sessions per workgroup, 7 waves per SIMD (aecm_kernels.hip gives the measurements).
#ifndef AECM_TICK_CALLS_WAVES_PER_EU
#if defined(AECM_CHECKED)
#define AECM_TICK_CALLS_WAVES_PER_EU 4
#else
#define AECM_TICK_CALLS_WAVES_PER_EU 7
#endif
#endif
constexpr int kTickCallsWaves = 4;

// Wavefront w of the grid serves session live[w], w < live_count (ascending ids; the id wave-uniform and in a scalar register
// before anything is addressed by it).  The state loads are issued once, ahead of the table fill -- and ahead of every fence
// and every wide store of the kernel, so that the scalar half of the state arrives through scalar loads; the state stores
// happen once, behind the last call (not at all for a session whose K calls ran no block: still in its start-up phase).
template <bool kHasClean>
__global__ __launch_bounds__(64 * kTickCallsWaves) __attribute__((amdgpu_waves_per_eu(AECM_TICK_CALLS_WAVES_PER_EU, 8)))
void aecm_tick_calls_kernel(StatePtrs st, TickIo io, TickFlowIo fio, int n_streams, const uint32_t *__restrict__ live, int live_count, int calls) {
    const int64_t wave_id = (int64_t)blockIdx.x * kTickCallsWaves + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t id = (uint32_t)__builtin_amdgcn_readfirstlane((int)live[wave_id < live_count ? wave_id : 0]);
    const int64_t s = wave_id < live_count && id < (uint32_t)n_streams ? (int64_t)id : (int64_t)n_streams;
    const int lane_id = threadIdx.x & 63;
    using E = BlockEngine<Gfx950Wave<true, true, true>, kHasClean>;
    typename E::Regs r;
    const int64_t sl = s < n_streams ? s : 0;
    uint32_t *vec = st.vec + sl * (int64_t)kVecWordsPerStream;
    int32_t *scal = st.scal + sl * (int64_t)kNumScal;
    E::init_lane_constants(r, st.consts);
    E::load_state(r, vec, scal);
    FillLdsTables<64 * kTickCallsWaves>(st.consts);
    if (s >= n_streams) return;
    const int mask = (int)io.ring_len - 1;
    const int n = io.n;
    int16_t *fr = io.far_ring + s * io.ring_len, *nr = io.near_ring + s * io.ring_len;
    int16_t *cr = kHasClean ? io.clean_ring + s * io.ring_len : nullptr;
    int16_t *orow = io.out_ring + s * io.ring_len;
    int16_t *ff = fio.far_frames + s * kFlowFarFrameRing, *old = fio.far_old + s * (2 * kFlowFrame);
    // Four samples (8 bytes) per lane where everything is 8-byte aligned, as in the tick kernel; c * n samples are 160 c or
    // 320 c bytes, so the rows of every call are aligned when those of the first are.
    typedef short Quad __attribute__((ext_vector_type(4)));
    const bool rows_aligned = ((reinterpret_cast<uintptr_t>(io.far_in) | reinterpret_cast<uintptr_t>(io.near_in) |
                                reinterpret_cast<uintptr_t>(io.out) | (kHasClean ? reinterpret_cast<uintptr_t>(io.clean_in) : 0) |
                                (uintptr_t)(io.io_stride * 2)) & 7) == 0;
    const int32_t *plans = fio.plans + s * calls * kFlowPlanWords;
    bool ran = false;
    for (int c = 0; c < calls; ++c) {
        // The lane id of this call's sample movement, opaque and tied to c: otherwise every per-lane 64-bit ring and row address
        // of the loop body is hoisted out of the loop, stays live across the blocks and goes to scratch.
        int lane = lane_id;
        asm("" : "+v"(lane) : "s"(c));
        // 1. call c's plan into scalar registers (split into 16 independent scalars: aecm_tick_flow_body.inc)
        int32_t w[kFlowPlanWords];
        for (int k = 0; k < kFlowPlanWords; ++k) w[k] = __builtin_amdgcn_readfirstlane(plans[c * kFlowPlanWords + k]);
        for (int k = 0; k < kFlowPlanWords; ++k) asm("" : "+s"(w[k]));
        FlowPlan p;
        FlowUnpackPlan(w, p);
        // call c's rows and its place in the near rings
        const int16_t *fin = io.far_in + s * io.io_stride + c * n, *nin = io.near_in + s * io.io_stride + c * n;
        const int16_t *cin = kHasClean ? io.clean_in + s * io.io_stride + c * n : nullptr;
        int16_t *out = io.out + s * io.io_stride + c * n;
        const unsigned npos = (unsigned)io.near_pos + (unsigned)(c * n);
        // 2. the call's samples into the rings (one call: one far piece, far[0])
        const bool far_aligned = ((p.far[0].pos | p.far[0].count) & 3) == 0;
        const auto append = [&]() {
            if (rows_aligned && far_aligned) {
                if (lane < n / 4) {
                    const int j = 4 * lane;
                    if (j < p.far[0].count) *reinterpret_cast<Quad *>(fr + ((p.far[0].pos + (unsigned)j) & mask)) = *reinterpret_cast<const Quad *>(fin + j);
                    *reinterpret_cast<Quad *>(nr + ((npos + j) & mask)) = *reinterpret_cast<const Quad *>(nin + j);
                    if (kHasClean) *reinterpret_cast<Quad *>(cr + ((npos + j) & mask)) = *reinterpret_cast<const Quad *>(cin + j);
                }
            } else {
                for (int j = lane; j < n; j += 64) {
                    if (j < p.far[0].count) fr[(p.far[0].pos + (unsigned)j) & mask] = fin[j];
                    nr[(npos + j) & mask] = nin[j];
                    if (kHasClean) cr[(npos + j) & mask] = cin[j];
                }
            }
        };
        // 3. a replay frame about to be lapped in the far ring -> its row (read by the NEXT call at the earliest: behind the
        //    fence that ends this call), then the far end of the call's blocks
        if (p.spill[0] | p.spill[1]) {
            for (int i = 0; i < 2; ++i) {
                if (!p.spill[i]) continue;
                int16_t *row = old + i * kFlowFrame;
                const int16_t a0 = fr[(p.spill_pos[i] + lane) & mask], a1 = fr[(p.spill_pos[i] + 64 + (lane & 15)) & mask];
                row[lane] = a0;
                if (lane < kFlowFrame - 64) row[64 + lane] = a1;
            }
        }
        if (!p.direct && (p.frame[0].active | p.frame[1].active)) {
            // far stream position q, from the ring -- or, if it was appended in THIS call, from call c's input row (what the
            // calls before appended is in the ring, behind their fences)
            auto far_stream = [&](unsigned q) -> int16_t {
                const int r0 = (int)(q - p.far[0].pos);
                const bool in0 = r0 >= 0 && r0 < p.far[0].count;
                const int16_t ring = fr[q & mask], fresh = fin[in0 ? r0 : 0];
                return in0 ? fresh : ring;
            };
            // every load before any store: what direct calls left pending in the far ring, then the call's frames
            int16_t left = 0, v0[2] = {0, 0}, v1[2] = {0, 0};            // frame f: samples lane and 64 + lane (lanes 0..15)
            if (lane < p.left_count) left = fr[(p.blk_pos0 + p.left_delta + lane) & mask];
            for (int f = 0; f < 2; ++f) {
                const FlowFrame &q = p.frame[f];
                if (!q.active) continue;
                const int16_t *row = old + q.old_idx * kFlowFrame;
                v0[f] = q.far_from_stream ? far_stream(q.far_pos + lane) : row[lane];
                if (lane < kFlowFrame - 64) v1[f] = q.far_from_stream ? far_stream(q.far_pos + 64 + lane) : row[64 + lane];
            }
            if (lane < p.left_count) ff[(p.blk_pos0 + lane) & (kFlowFarFrameRing - 1)] = left;
            for (int f = 0; f < 2; ++f) {
                const FlowFrame &q = p.frame[f];
                if (!q.active) continue;
                ff[(q.frm_pos + lane) & (kFlowFarFrameRing - 1)] = v0[f];
                if (lane < kFlowFrame - 64) ff[(q.frm_pos + 64 + lane) & (kFlowFarFrameRing - 1)] = v1[f];
            }
        }
        // 4. the blocks, on the registers the calls before left (the fence between the stores above and the blocks' fetches:
        //    TickCallsBlockIo::ready)
        const int nb = p.n_blocks;
        if (nb > 0) {
            using Io = TickCallsBlockIo<kHasClean, decltype(append)>;
            Io bio{p.direct ? fr : ff, nr, cr, orow, p.direct ? mask : kFlowFarFrameRing - 1, mask,
                   p.direct ? p.blk_pos0 + p.far_delta : p.blk_pos0, p.near_base + p.blk_pos0, p.blk_pos0, append};
            E::run_blocks_loaded(r, st, bio, s, nb);
            ran = true;
        } else {
            append();                    // a call of the start-up phase: no blocks, but the rings take its samples
        }
        // the block outputs before the output frames read them; the call's appended samples, framed samples and replay
        // rows before call c + 1 reads them
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
        // 5. the output frames of call c, before call c + 1's blocks write further
        const int16_t *pass = kHasClean ? cin : nin;
        if (rows_aligned && ((p.frame[0].out_pos | p.frame[1].out_pos) & 3) == 0) {
            const int f = lane >= kFlowFrame / 4 ? 1 : 0, j = 4 * (lane - f * (kFlowFrame / 4));
            if (lane < p.n_frames * (kFlowFrame / 4)) {
                const Quad from_ring = *reinterpret_cast<const Quad *>(orow + ((p.frame[f].out_pos + j) & mask));
                const Quad from_input = *reinterpret_cast<const Quad *>(pass + f * kFlowFrame + j);
                *reinterpret_cast<Quad *>(out + f * kFlowFrame + j) = p.frame[f].active ? from_ring : from_input;
            }
        } else {
            for (int f = 0; f < 2; ++f) {
                if (f >= p.n_frames) continue;
                for (int j = lane; j < kFlowFrame; j += 64)
                    out[f * kFlowFrame + j] = p.frame[f].active ? orow[(p.frame[f].out_pos + j) & mask] : pass[f * kFlowFrame + j];
            }
        }
    }
    if (ran) E::store_state(r, vec, scal);
}

hipError_t LaunchTickCalls(const StatePtrs &st, const TickIo &io, const TickFlowIo &fio, const TickSparseIo &sp, int n_streams, int live_count,
                           int calls, hipStream_t stream) {
    if (n_streams <= 0) return hipSuccess;
    if (live_count < 0 || live_count > n_streams || !sp.live || !sp.block_base || calls < 1 || calls > kFlowMaxTickCalls) return hipErrorInvalidValue;
    // the planning launch runs over ALL sessions (the idle ones count their lag); the tick launch over the live ones only
    if (const hipError_t e = LaunchPlanCalls(io, fio, sp, n_streams, calls, stream)) return e;
    if (live_count > 0) {
        const dim3 grid((live_count + kTickCallsWaves - 1) / kTickCallsWaves), block(64 * kTickCallsWaves);
        const size_t lds = sizeof(LdsTables);
        if (io.clean_in) hipLaunchKernelGGL((aecm_tick_calls_kernel<true>), grid, block, lds, stream, st, io, fio, n_streams, sp.live, live_count, calls);
        else hipLaunchKernelGGL((aecm_tick_calls_kernel<false>), grid, block, lds, stream, st, io, fio, n_streams, sp.live, live_count, calls);
    }
    return hipGetLastError();
}

}  // namespace aecm
