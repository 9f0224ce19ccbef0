// The body of the loop-form tick kernels -- aecm_tick_calls_kernel (aecm_tick_calls_kernels.hip) and aecm_tick_packets_kernel
// (aecm_tick_packets_kernels.hip) -- as TEXT, included between the braces of each (the way of aecm_tick_flow_body.inc, and for its
// reason: the K-call kernels stay, token for token and so instruction for instruction, what they were;
// tests/golden/tick_calls_fingerprints.json).  In scope: st, io, fio, n_streams, live, live_count, calls, kHasClean, and
// what aecm_tick_unit.h defines (TickBlockIo, kTickCallsWaves, AECM_TICK_LIVE_SESSION).  The two kernels
// differ in ONE thing, where a call's sample count n -- which is also the step from one call's rows to the next -- comes from:
//   AECM_TICK_CALLS_SIZE_OF_LAUNCH   `const int n = io.n;` for the K-call tick (every session makes calls of the launch's n), else empty
//   AECM_TICK_CALLS_SIZE_OF_PLAN     `const int n = p.n_frames * kFlowFrame;` for the packet tick (the SESSION's call size, wave-uniform,
//                                    the same in all of its K plans: rows packed, near positions contiguous), else empty
// One optional hook, nothing where the includer defines none (every kernel without it keeps its tokens):
//   AECM_TICK_CALLS_AFTER_BLOCKS     a statement behind step 4 of every call, with c, p and r -- the core state behind call c's last
//                                    block, or as loaded for a call that ran none -- in scope: the call trace's tick kernels
//                                    (aecm_call_trace_kernels.hip) store the core half of call c's record here
#if !defined(AECM_TICK_CALLS_AFTER_BLOCKS)
#define AECM_TICK_CALLS_AFTER_BLOCKS
#endif
    const int64_t wave_id = (int64_t)blockIdx.x * kTickCallsWaves + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    AECM_TICK_LIVE_SESSION(live, live_count, wave_id)
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
    AECM_TICK_CALLS_SIZE_OF_LAUNCH
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
        AECM_TICK_CALLS_SIZE_OF_PLAN
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
        //    TickBlockIo::ready, aecm_tick_unit.h)
        const int nb = p.n_blocks;
        if (nb > 0) {
            using Io = TickBlockIo<kHasClean, decltype(append)>;
            Io bio{p.direct ? fr : ff, nr, cr, orow, p.direct ? mask : kFlowFarFrameRing - 1, mask,
                   p.direct ? p.blk_pos0 + p.far_delta : p.blk_pos0, p.near_base + p.blk_pos0, p.blk_pos0, append};
            E::run_blocks_loaded(r, st, bio, s, nb);
            ran = true;
        } else {
            append();                    // a call of the start-up phase: no blocks, but the rings take its samples
        }
        AECM_TICK_CALLS_AFTER_BLOCKS
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
#undef AECM_TICK_CALLS_AFTER_BLOCKS
