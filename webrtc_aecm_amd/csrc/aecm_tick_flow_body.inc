// The body of the tick kernels (aecm_kernels.hip: aecm_tick_flow_kernel, aecm_tick_flow_sparse_kernel; aecm_tick_split_kernels.hip:
// aecm_tick_split_kernel, aecm_tick_split_list_kernel), included into each behind aecm_tick_unit.h and after it has named its session: s (int64_t, wave-uniform, in a scalar register; >= n_streams: the wavefront serves nobody
// and leaves behind the table fill's barrier) and lane.  One text for both, so the two cannot drift apart -- and a text
// rather than a function, so that the dense kernel stays, instruction for instruction, the kernel it was before there was
// a sparse one.  The other forms were tried:
//   - the body as a __forceinline__ function template <kHasClean, kSparse> called from both kernels CHANGED the dense code
//     (3 654 -> 3 671 instructions without a clean input: the by-reference captures of `append` are resolved differently);
//   - one kernel template <kHasClean, kSparse> with `if constexpr` on the lines that differ and the live list as a last
//     argument that is an empty struct in the dense instantiations kept the dense instruction streams, but not the dense
//     kernels' names: tests/test_capi.py finds the dense tick kernel by its one-parameter mangled name and wants that name to
//     match one kernel only, so the dense kernel keeps its name and signature and the sparse one is a kernel of its own.
// What the including kernel provides: kHasClean, st, io, fio, n_streams, s, lane.
    // 1. the session's plan for this tick into scalar registers; requested before the table fill so that the fill hides
    //    the latency
    int32_t w[kFlowPlanWords];
    {
        const int32_t *pw = fio.plans + (s < n_streams ? s : 0) * kFlowPlanWords;
        for (int k = 0; k < kFlowPlanWords; ++k) w[k] = pw[k];
    }
#if AECM_TICK_EARLY_STATE_LOAD
    // the session's state loads are issued here, ahead of the table fill and its barrier: their latency runs next to the fill's
    using EarlyE = BlockEngine<Gfx950Wave<true, true, true>, kHasClean>;
    typename EarlyE::Regs early_r;
    {
        const int64_t sl = s < n_streams ? s : 0;
        EarlyE::init_lane_constants(early_r, st.consts);
        EarlyE::load_state(early_r, st.vec + sl * (int64_t)kVecWordsPerStream, st.scal + sl * (int64_t)kNumScal);
    }
#endif
    FillLdsTables<64 * kTickFlowWaves>(st.consts);
    if (s >= n_streams) return;
    // The 16 words arrive as one s_load_dwordx16 register tuple; left like that, the register allocator spills and reloads
    // the WHOLE tuple (16 v_writelane / v_readlane) around every use in another basic block.  Passing each word through an
    // empty asm makes them 16 independent scalars that are spilled one by one, and only where needed.
#if AECM_TICK_SPLIT_PLAN_WORDS
    for (int k = 0; k < kFlowPlanWords; ++k) asm("" : "+s"(w[k]));      // not volatile: a volatile asm counts as a memory clobber and turns the engine's scalar state loads into vector loads
#endif
    FlowPlan p;
    FlowUnpackPlan(w, p);
    const int mask = (int)io.ring_len - 1;
    const int n = io.n;
    const int16_t *fin = io.far_in + s * io.io_stride, *nin = io.near_in + s * io.io_stride;
    const int16_t *cin = kHasClean ? io.clean_in + s * io.io_stride : nullptr;
    int16_t *fr = io.far_ring + s * io.ring_len, *nr = io.near_ring + s * io.ring_len;
    int16_t *cr = kHasClean ? io.clean_ring + s * io.ring_len : nullptr;
    int16_t *orow = io.out_ring + s * io.ring_len;
    int16_t *ff = fio.far_frames + s * kFlowFarFrameRing, *old = fio.far_old + s * (2 * kFlowFrame);
    int16_t *out = io.out + s * io.io_stride;
    // 2. the tick's samples into the rings: what the jitter buffer accepted of the far end, all of the near end.  Four
    //    samples (8 bytes) per lane where everything is 8-byte aligned -- the caller's rows, and ring positions that are
    //    multiples of 4 (near positions always are: ticks are 80 or 160 samples; far positions unless a saturated jitter
    //    buffer accepted an odd count; rings are a multiple of 4 long, so a group never straddles the wrap) -- else one
    //    sample per lane.
    typedef short Quad __attribute__((ext_vector_type(4)));
    const bool rows_aligned = ((reinterpret_cast<uintptr_t>(io.far_in) | reinterpret_cast<uintptr_t>(io.near_in) |
                                reinterpret_cast<uintptr_t>(io.out) | (kHasClean ? reinterpret_cast<uintptr_t>(io.clean_in) : 0) |
                                (uintptr_t)(io.io_stride * 2)) & 7) == 0;
    const bool far_aligned = ((p.far[0].pos | p.far[0].count | p.far[1].pos | p.far[1].count) & 3) == 0;
    const auto append = [&]() {
        if (rows_aligned && far_aligned) {
            if (lane < n / 4) {
                const int j = 4 * lane;
                for (int c = 0; c < 2; ++c)
                    if (j >= p.far[c].src && j < p.far[c].src + p.far[c].count)
                        *reinterpret_cast<Quad *>(fr + ((p.far[c].pos + (unsigned)(j - p.far[c].src)) & mask)) = *reinterpret_cast<const Quad *>(fin + j);
                *reinterpret_cast<Quad *>(nr + (((unsigned)io.near_pos + j) & mask)) = *reinterpret_cast<const Quad *>(nin + j);
                if (kHasClean) *reinterpret_cast<Quad *>(cr + (((unsigned)io.near_pos + j) & mask)) = *reinterpret_cast<const Quad *>(cin + j);
            }
        } else {
            for (int j = lane; j < n; j += 64) {
                for (int c = 0; c < 2; ++c)
                    if (j >= p.far[c].src && j < p.far[c].src + p.far[c].count) fr[(p.far[c].pos + (unsigned)(j - p.far[c].src)) & mask] = fin[j];
                nr[((unsigned)io.near_pos + j) & mask] = nin[j];
                if (kHasClean) cr[((unsigned)io.near_pos + j) & mask] = cin[j];
            }
        }
    };
    // 3. the far end of the tick's blocks.  Usually (p.direct) it is one run of the far stream and the blocks fetch it from
    //    the far ring itself.  Otherwise (an underrun replay, a jump of the jitter buffer's read pointer, the first tick
    //    after start-up) the frames are laid out in the framed-far ring first.
    //    No fences here: a conditional fence before the engine's state loads makes the compiler fetch the scalar half of
    //    the state with vector loads.  None is needed either: the row a spill fills is not read before the next tick, and
    //    far samples that arrived in this very tick are taken from the input row instead of the ring.
    if (p.spill[0] | p.spill[1]) {           // rare: a replay frame is about to be lapped in the far ring -> its row
        for (int i = 0; i < 2; ++i) {
            if (!p.spill[i]) continue;
            int16_t *row = old + i * kFlowFrame;
            const int16_t a0 = fr[(p.spill_pos[i] + lane) & mask], a1 = fr[(p.spill_pos[i] + 64 + (lane & 15)) & mask];
            row[lane] = a0;
            if (lane < kFlowFrame - 64) row[64 + lane] = a1;
        }
    }
    if (!p.direct && (p.frame[0].active | p.frame[1].active)) {
        // far stream position q, from the ring -- or, if it was appended in this tick (a nearly empty jitter buffer), from
        // the piece of the input row it came from
        auto far_stream = [&](unsigned q) -> int16_t {
            const int r0 = (int)(q - p.far[0].pos), r1 = (int)(q - p.far[1].pos);
            const bool in0 = r0 >= 0 && r0 < p.far[0].count, in1 = r1 >= 0 && r1 < p.far[1].count;
            const int16_t ring = fr[q & mask], fresh = fin[in0 ? r0 : in1 ? p.far[1].src + r1 : 0];
            return (in0 || in1) ? fresh : ring;
        };
        // every load before any store: what direct ticks left pending in the far ring, then the tick's frames
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
    // 4. the blocks (the fence between the stores above and the blocks' fetches is TickBlockIo::ready, aecm_tick_unit.h)
    const int nb = p.n_blocks;
    if (nb > 0) {
        using Io = TickBlockIo<kHasClean, decltype(append)>;
        Io bio{p.direct ? fr : ff, nr, cr, orow, p.direct ? mask : kFlowFarFrameRing - 1, mask,
               p.direct ? p.blk_pos0 + p.far_delta : p.blk_pos0, p.near_base + p.blk_pos0, p.blk_pos0, append};
#if AECM_TICK_EARLY_STATE_LOAD
        Io::E::run_stream_loaded(early_r, st, bio, s, nb);
#else
        Io::E::run_stream_io(st, bio, s, nb);
#endif
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    } else {
        append();                    // a session still in its start-up phase: no blocks, but its rings take the samples
    }
    // 5. the output frames: block outputs (this tick's or, when stuffing, older ones) or the start-up copy of the
    //    (clean) near end (echo_control_mobile.cc:285-291)
    //    Output positions are multiples of 16 (blocks of 64, frames of 80, stuffing by 16): both frames as groups of four
    //    samples, 20 lanes each, when the caller's rows are aligned.
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
