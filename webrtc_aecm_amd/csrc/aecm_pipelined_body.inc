// The text of the pipelined kernels' body (aecm_block_kernels.hip includes it into aecm_process_pipelined_kernel,
// aecm_process_pipelined_ragged_kernel, aecm_process_pipelined_clean_kernel and aecm_process_pipelined_ragged_clean_kernel, behind
// `constexpr bool kRagged, kClean`; not a header: no guard, no declarations of its own).
// In scope: the template arguments kTail, kBalance, kRaw, kFront, kDelay, kGain and the kernel arguments st, io, streams_base,
// streams_rem, n_blocks, progress, n_workgroups, wgs_per_round, rot, prio.
    constexpr int kFrontBehind = kBalance ? kPipeFrontPrioBehind : AECM_PIPE_FRONT_PRIO;
    constexpr int kBoost = kBalance ? kPipeFrontSecondBoostBalanced : kPipeFrontSecondBoost;
#if defined(AECM_PIPE_TRACE)     // diagnostics build: per wave, when it started / ended (100 MHz wall clock) and how long it sat at barriers (shader clocks)
    const uint64_t trace_t0 = wall_clock64(), trace_c0 = clock64();
    uint64_t trace_wait = 0;
#define AECM_PIPE_BARRIER() do { const uint64_t c_ = clock64(); __syncthreads(); trace_wait += clock64() - c_; } while (0)
#else
#define AECM_PIPE_BARRIER() __syncthreads()
#endif
    static_assert(kTail == 0 || kTail == 2, "tail waves: two, of two streams each");
    static_assert(kDelay == 0 || (kPipeStreams % kDelay == 0 && !kRaw), "delay waves: in the shapes with formed spectra");
    static_assert(kGain == 0 || (kGain == kPipeStreams && kDelay != 0), "gain waves: one per stream, with delay waves");
    static_assert(!kRagged || !kBalance, "ragged launches: the unbalanced shapes (the balance's slowest-workgroup rule assumes equal work)");
    static_assert(!kClean || (!kRaw && !kBalance), "clean launches: formed spectra, no balance");
    constexpr int kWaves = PipeWaves(kTail, kFront, kDelay, kGain), kPipeFrontWaves = kFront, kPipeStreamsPerFront = kPipeStreams / kFront;
    constexpr int kLagD = kDelay ? 1 : 0, kLagG = kGain ? 1 : 0;           // steps the delay / gain waves put between the front waves and the rest
    constexpr int kSlots = 2 + kLagD + kLagG;
    PipeShared<kTail, kRaw, kDelay, kGain, kClean> &sh = *reinterpret_cast<PipeShared<kTail, kRaw, kDelay, kGain, kClean> *>(&g_lds[1]);        // behind the tables
    if (kBalance && threadIdx.x == 0) { sh.ahead = 0; sh.level = kFrontBehind; }
    FillLdsTables<64 * kWaves>(st.consts);                              // ends in a barrier
    using W = Gfx950Wave<true, true>;
    using E = BlockEngine<W, kClean>;
    using EF = BlockEngine<Gfx950Wave<true, false>, kClean>;              // the front and tail waves keep one priority (no per-phase s_setprio)
    // Clean launches (kClean): the front waves run the clean input's transform with the other two and hand the three spectra over as
    // BlockEngine::CleanHandOver (PipeCleanSlot); everything behind the delay waves works with the clean spectrum `cf` where the other
    // launches pass the near-end one twice.  c_old, the clean input's last block, shares V_OUTBUF's word with the overlap buffer: the
    // front wave loads its half at the start, and leaves the launch's last clean block in sh.c_last in its last (otherwise empty)
    // step -- before a barrier every wave executes -- for the wave that stores that word.  No input row is read again at the end:
    // out may alias an input.  Ragged and clean together: c_prev, like x_old and d_old, only advances while blk < the slot's own
    // length, so what a stream that ended before its workgroup did leaves in sh.c_last is the clean block at ITS last block; the
    // barriers per wave are those of the ragged form (n_blocks = the workgroup's longest slot in every role).
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    // This workgroup's streams (PipeSplit, below): streams_base of them, one more in the first streams_rem workgroups -- the
    // dispatcher deals workgroups out to the CUs in turn, so the CUs' loads differ by at most one stream.  A workgroup with fewer
    // than kPipeStreams streams keeps them in the slots that spread them over the waves that serve two slots each (front, tail,
    // delay waves): 1 -> slot 0; 2 -> slots 0, 2; 3 -> slots 0, 1, 2.  The waves of an empty slot only keep the barriers.
    const int wg = (int)blockIdx.x;
    // (equal-length launches only: a ragged launch's streams_base is its stream count, and its slots come from the plan)
    const int64_t first = kRagged ? 0 : (int64_t)wg * streams_base + (wg < streams_rem ? wg : streams_rem);
    const int live_mask = kRagged ? 0 : (0xf7510 >> (4 * (streams_base + (wg < streams_rem ? 1 : 0)))) & 0xf;
    // Ragged (kRagged): the streams of this workgroup's slots and their lengths come from a plan the host made (BuildRaggedPipePlan,
    // aecm_engine.cpp), which `progress` then points to: slot_stream[n_workgroups][kPipeStreams] (-1 = empty slot), then len[streams_base]
    // (streams_base = the streams of the launch).  Read only, with plain loads; nothing travels between workgroups.  Lock step needs
    // the same number of BARRIERS in every wave of a workgroup, not the same number of blocks per slot: every role's block loop runs
    // n_blocks = the longest of the workgroup's four lengths (an empty slot: 0) trips, and in trip blk a role works for its slot
    // only while blk < the slot's own length -- the role's lag behind the front waves is in the barriers before its loop, so
    // "blk < len" is "this slot's stream still has the block this role works on in this step" for every role.  A slot past its length
    // writes no hand-over slot and no output and loads no input row; its state waits in registers for the common end of the launch.
    const int32_t *const plan_slots = reinterpret_cast<const int32_t *>(progress) + (int64_t)wg * kPipeStreams;
    const int32_t *const plan_len = reinterpret_cast<const int32_t *>(progress) + (int64_t)n_workgroups * kPipeStreams;
    const auto plan_stream = [&](int k) -> int {                  // -1: empty (or not a stream of this launch: touch nothing)
        const int s = __builtin_amdgcn_readfirstlane(plan_slots[k]);
        return (unsigned)s < (unsigned)streams_base ? s : -1;
    };
    const auto slot_len = [&](int k) -> int {                     // wave-uniform; 0 for an empty slot
        if constexpr (kRagged) {
            const int s = plan_stream(k);
            const int l = s >= 0 ? __builtin_amdgcn_readfirstlane(plan_len[s]) : 0;
            return l > 0 ? l : 0;
        } else {
            return n_blocks;
        }
    };
    if constexpr (kRagged) {
        int longest = 0;
#pragma unroll
        for (int k = 0; k < kPipeStreams; ++k) { const int l = slot_len(k); longest = l > longest ? l : longest; }
        n_blocks = longest;
    }
    const auto slot_live = [&](int k) -> bool {
        if constexpr (kRagged) return slot_len(k) > 0;
        else return ((live_mask >> k) & 1) != 0;
    };
    const auto slot_stream = [&](int k) -> int64_t {
        if constexpr (kRagged) { const int s = plan_stream(k); return s >= 0 ? s : 0; }
        else return first + __builtin_popcount((unsigned)(live_mask & ((1 << k) - 1)));
    };
    // Which wave serves which slot.  The hardware deals a workgroup's waves out to the CU's four SIMDs in turn, so with the natural
    // numbering (wave = role's first wave + slot) every one-stream-per-wave role of a slot would sit on the same SIMD: a workgroup
    // with an empty slot leaves one SIMD idle and two workgroups with the same live slots crowd the same SIMDs -- a SIMD's vector
    // port carries the instruction stream of one stream's waves at 0.9 M frames/s and no more (measured: one five-stream CU among
    // four-stream CUs ran its streams at 0.43 instead of 0.60 M frames/s and held the whole launch up).  So the roles are
    // staggered (the front wave of slot k sits one SIMD further than its back wave, the gain wave two) and the workgroups that
    // share a CU -- workgroup i and i + wgs_per_round, ... -- each start one SIMD further.  Any bijection is correct.
    const int wg_rot = wgs_per_round > 0 ? (wg / wgs_per_round) * ((rot >> 6) & 3) : 0;
    const int rot_front = rot & 3, rot_gain = (rot >> 2) & 3, rot_delay = (rot >> 4) & 3, rot_tail = (rot >> 8) & 3;
    int k0 = 0;                                                                              // the first slot of a wave that serves several
    const auto ks = [&](int k) -> int { return (k0 + k) & (kPipeStreams - 1); };
    const auto slot_of = [&](int j, int role_rot) -> int { return (j + role_rot + wg_rot) & (kPipeStreams - 1); };
    static_assert((kPipeStreams & (kPipeStreams - 1)) == 0, "slot rotation");
    if (wave < kPipeStreams) {
        // ---- back (middle) wave: one stream, everything of a block after the forward transforms (and before the inverse one, with tail waves) ----
        typename E::Regs r;
        E::init_lane_constants(r, st.consts);
        const int slot = slot_of(wave, 0);
        const int64_t stream = slot_stream(slot);
        const bool live = slot_live(slot);
        const int len = slot_len(slot);
        uint32_t *vec = st.vec + stream * (int64_t)kVecWordsPerStream;
        int32_t *scal = st.scal + stream * (int64_t)kNumScal;
        uint16_t *hist = st.hist + stream * (int64_t)kHistWordsPerStream;
        typename E::StridedIo sio{io, stream * io.stream_stride};
        if (live) E::load_state(r, vec, scal);
        W::begin_stream();
        AECM_PIPE_BARRIER();                                              // step 0: the spectra of block 0 are in slots[0]
        if (kDelay != 0) AECM_PIPE_BARRIER();                             // step 1: the delay waves' first
        int slot_idx = 0;                                                 // blk mod kSlots
        for (int blk = 0; blk < n_blocks; ++blk) {                        // step blk + 1 (+ 1 with delay waves)
            if (live && (!kRagged || blk < len)) {
                const int lane = W::lane_id();
                typename E::Spectrum xf, df, cf;
                const typename E::Spectrum &clean = kClean ? cf : df;
                r.table_index = W::table_index_for_this_block();
                if constexpr (kClean) {
                    const PipeCleanSlot &slot_in = sh.slots[slot_idx][slot];
                    E::unpack_clean_hand_over({slot_in.clean_x[lane], slot_in.mags[lane], slot_in.clean_mag[lane], slot_in.scalars[lane]}, xf, df, cf);
                } else if constexpr (kRaw) {
                    const PipeRawSlot &slot_in = sh.slots[slot_idx][slot];
                    const int fa0 = slot_in.fa[0][lane], fb0 = slot_in.fb[0][lane], fa1 = slot_in.fa[1][lane], fb1 = slot_in.fb[1][lane];
                    const int q0 = __builtin_amdgcn_readfirstlane(slot_in.q[0]), q1 = __builtin_amdgcn_readfirstlane(slot_in.q[1]);
                    E::spectrum(r, fa0, fb0, q0, xf);
                    E::spectrum(r, fa1, fb1, q1, df);
                } else {
                    const PipeSlot &slot_in = sh.slots[slot_idx][slot];
                    // (restates E::unpack_hand_over: through the call the audit build's back waves are scheduled differently)
                    const int x = slot_in.near_x[lane], m = slot_in.mags[lane], sc = slot_in.scalars[lane];
                    xf.mag = zext16(m);
                    xf.mag64 = __builtin_amdgcn_readlane(sc, 0);
                    xf.q = __builtin_amdgcn_readlane(sc, 1);
                    xf.re = xf.im = 0;
                    xf.re64 = 0;
                    df.re = sext16(x);
                    df.im = sar(x, 16);
                    df.mag = lsr(m, 16);
                    df.re64 = __builtin_amdgcn_readlane(sc, 2);
                    df.mag64 = __builtin_amdgcn_readlane(sc, 3);
                    df.q = __builtin_amdgcn_readlane(sc, 4);
                }
                E::update_startup(r.u);
                int delay_given = 0, far_given = 0;
                if constexpr (kDelay != 0) {
                    delay_given = __builtin_amdgcn_readfirstlane(sh.delays[blk & 1][slot]);
                    far_given = sh.far_rows[blk & 1][slot][lane];
                }
                if constexpr (kTail != 0) {
                    if constexpr (kGain != 0) {
                        W::template phase_priority<3>();
                        E::track_q(r.u, df, clean);
                        const typename E::GainInput g = E::template channel_block<true>(r, hist, xf, df, delay_given, far_given);
                        PipeGainSlot &gs = sh.gains[blk & 1][slot];
                        gs.echo_est[lane] = g.echo_est;
                        if (lane == 0) { gs.echo_est64 = g.echo_est64; gs.far_q = g.far_q; gs.cur_vad = g.cur_vad; gs.near0 = g.near0; gs.stored0 = g.stored0; }
                    } else {
                        const typename E::TailInput t = E::template middle_block<kDelay != 0>(r, hist, xf, df, clean, delay_given, far_given);
                        PipeTailSlot &ts = sh.tails[blk & 1][slot];
                        ts.a[lane] = t.a;
                        ts.b[lane] = t.b;
                        if (lane == 0) ts.clean_q = t.clean_q;
                    }
                } else {
                    const typename E::TailInput t = E::template middle_block<kDelay != 0>(r, hist, xf, df, clean, delay_given, far_given);
                    const int out = E::tail_block(r, t.a, t.b, t.clean_q);        // (= back_block)
                    sio.out(r, blk, out);
                }
            }
            slot_idx = slot_idx + 1 == kSlots ? 0 : slot_idx + 1;
            AECM_PIPE_BARRIER();                                          // slots[blk & 1] are free again, block blk + 1 is in the others
        }
        if (kGain != 0) AECM_PIPE_BARRIER();                              // the gain waves' last step
        if (kTail != 0) AECM_PIPE_BARRIER();                              // the tail waves' last step
        if constexpr (kGain != 0) {
            AECM_PIPE_BARRIER();                                          // the gain wave's part of the state is in gain_state
            if (live) {
                const int lane = W::lane_id();
                const PipeGainState &g = sh.gain_state[slot];
                // (restates E::unpack_gain_state: through the call the sixteen-wave kernels are scheduled differently)
                const int nf = g.near_filt_ctrs[lane];
                r.b.echo_filt = g.echo_filt[lane];
                r.b.near_filt = sext16(nf); r.b.low_ctr = lsr(nf, 16) & 7; r.b.high_ctr = lsr(nf, 19) & 7;
                r.b.noise_est = g.noise_est[lane];
                Uniform &u = r.u;
                auto S = [&](int i) { return __builtin_amdgcn_readfirstlane(g.scal[i]); };
                u.seed = S(0); u.sup_gain = S(1); u.sup_gain_old = S(2); u.noise_ctr = S(3);
                r.b64.echo_filt = S(4); r.b64.near_filt = S(5); r.b64.noise_est = S(6); r.b64.low_ctr = S(7); r.b64.high_ctr = S(8);
            }
        }
        if constexpr (kClean && kTail == 0)
            if (live) r.c_old = sh.c_last[slot][W::lane_id()];            // (the front wave's last step lies before this wave's last barrier)
        if (live) E::template store_state<false, kTail == 0, kDelay == 0>(r, vec, scal);
    } else if (wave < kPipeStreams + kPipeFrontWaves) {
        // ---- front wave: two streams, the transforms of the block after the one their back waves are at ----
        typename EF::Regs r;
        EF::init_lane_constants(r, st.consts);
        int level = kBalance ? kFrontBehind : (prio & 3);                 // this group's base priority (without balance: the launch's, PipeShape::prio)
        SetPrioDynamic(level);
        k0 = slot_of((wave - kPipeStreams) * kPipeStreamsPerFront, rot_front);        // (a wave of two slots: k0 and the one after it, round the ring)
        int x_old[kPipeStreamsPerFront], d_old[kPipeStreamsPerFront], far_next[kPipeStreamsPerFront], near_next[kPipeStreamsPerFront];
        int c_prev[kPipeStreamsPerFront], clean_next[kPipeStreamsPerFront];      // (clean launches)
        bool live[kPipeStreamsPerFront];
        int len[kPipeStreamsPerFront];
        int64_t strm[kPipeStreamsPerFront];                               // (ragged: the plan is read once per wave)
        for (int k = 0; k < kPipeStreamsPerFront; ++k) {
            const int64_t stream = slot_stream(ks(k));
            live[k] = slot_live(ks(k));
            len[k] = slot_len(ks(k));
            strm[k] = stream;
            x_old[k] = d_old[k] = far_next[k] = near_next[k] = 0;
            if (live[k]) {
                EF::load_time_state(st.vec + stream * (int64_t)kVecWordsPerStream, r.lane, x_old[k], d_old[k]);
                typename EF::StridedIo sio{io, stream * io.stream_stride};
                far_next[k] = sio.far(r, 0);
                near_next[k] = sio.near(r, 0);
                if constexpr (kClean) {
                    int ovl_unused;
                    EF::load_tail_state(st.vec + stream * (int64_t)kVecWordsPerStream, r.lane, ovl_unused, c_prev[k]);
                    clean_next[k] = sio.clean(r, 0);
                }
            }
        }
        int slot_idx = 0;                                                 // blk mod kSlots
        for (int blk = 0; blk <= n_blocks; ++blk) {                      // step blk writes block blk (the last step: nothing)
            // Balance: the monitor's step at a group boundary (see above).  pv[] is only ever read under the condition it is
            // loaded under (no initialisation: a register written by a move while a load of an earlier trip may still be
            // pending in the compiler's eyes costs a wait for everything in flight at the top of every trip).
            const bool boundary = kBalance && (blk & kPipeGroupMask) == 0 && blk != 0;
            const bool monitor = boundary && wave == kPipeStreams;
            int pv[kPipeMonitorLoads];
            if (monitor) {
                // a workgroup's word is the 16-bit COMPLEMENT of its group count: the cleared buffer (and the unused half of an
                // odd last word) then reads as "as far ahead as can be", never as the slowest
                const int g = blk >> kPipeGroupLog2;
                __hip_atomic_store(reinterpret_cast<uint16_t *>(progress) + blockIdx.x, (uint16_t)(0xffff - (g < 0xffff ? g : 0xffff)),
                                   __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                const int lane = W::lane_id(), n_words = (n_workgroups + 1) >> 1;
#pragma unroll
                for (int i = 0; i < kPipeMonitorLoads; ++i) {
                    const int w = lane + 64 * i;
                    if (64 * i < n_words)
                        pv[i] = (int)__hip_atomic_load(progress + (w < n_words ? w : n_words - 1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
            }
            if (kBalance && kFrontBehind != AECM_PIPE_FRONT_PRIO && (blk & kPipeGroupMask) == 1 && blk > kPipeGroupMask) {
                level = __builtin_amdgcn_readfirstlane(sh.level);
                if (kBoost == 0) SetPrioDynamic(level);
            }
            if (blk < n_blocks) {
#pragma unroll
                for (int k = 0; k < kPipeStreamsPerFront; ++k) {
                    if (!live[k]) continue;
                    if (kRagged && blk >= len[k]) continue;
                    if (kBoost != 0) SetPrioDynamic(level + (k == 0 ? 0 : kBoost));      // folds to immediates without balance
                    const int far_cur = far_next[k], near_cur = near_next[k];
                    if (blk + 1 < (kRagged ? len[k] : n_blocks)) {                // never a row at or beyond the stream's length
                        typename EF::StridedIo sio{io, (kRagged ? strm[k] : slot_stream(ks(k))) * io.stream_stride};
                        far_next[k] = sio.far(r, blk + 1);
                        near_next[k] = sio.near(r, blk + 1);
                    }
                    int clean_cur = 0;
                    if constexpr (kClean) {
                        clean_cur = clean_next[k];
                        if (blk + 1 < (kRagged ? len[k] : n_blocks)) {            // (as the far and near rows above)
                            typename EF::StridedIo sio{io, (kRagged ? strm[k] : slot_stream(ks(k))) * io.stream_stride};
                            clean_next[k] = sio.clean(r, blk + 1);
                        }
                    }
                    r.table_index = Gfx950Wave<true, false>::table_index_for_this_block();
                    const int lane = W::lane_id();
                    if constexpr (kClean) {
                        typename EF::Spectrum xf, df, cf;
                        EF::front_block(r, x_old[k], far_cur, d_old[k], near_cur, c_prev[k], clean_cur, xf, df, cf);
                        const typename EF::CleanHandOver h = EF::pack_clean_hand_over(xf, df, cf);
                        PipeCleanSlot &slot = sh.slots[slot_idx][ks(k)];
                        slot.clean_x[lane] = h.clean_x;
                        slot.mags[lane] = h.mags;
                        slot.clean_mag[lane] = h.clean_mag;
                        slot.scalars[lane] = h.scalars;
                        c_prev[k] = clean_cur;
                    } else if constexpr (kRaw) {
                        int fa[2], fb[2], q[2];
                        EF::front_transforms(r, x_old[k], far_cur, d_old[k], near_cur, fa, fb, q);
                        PipeRawSlot &slot = sh.slots[slot_idx][ks(k)];
                        slot.fa[0][lane] = fa[0]; slot.fb[0][lane] = fb[0];
                        slot.fa[1][lane] = fa[1]; slot.fb[1][lane] = fb[1];
                        if (lane == 0) { slot.q[0] = q[0]; slot.q[1] = q[1]; }
                    } else {
                        typename EF::Spectrum xf, df, cf;
                        EF::front_block(r, x_old[k], far_cur, d_old[k], near_cur, 0, 0, xf, df, cf);
                        // (restates EF::pack_hand_over, store by store: through the call the stores come after all three words are
                        // formed, and the compiler then schedules the front waves' loop differently)
                        PipeSlot &slot = sh.slots[slot_idx][ks(k)];
                        slot.near_x[lane] = (df.re & 0xffff) | (int)((unsigned)df.im << 16);
                        slot.mags[lane] = xf.mag | (int)((unsigned)df.mag << 16);
                        int sc = 0;
                        sc = W::writelane(sc, xf.mag64, 0);
                        sc = W::writelane(sc, xf.q, 1);
                        sc = W::writelane(sc, df.re64, 2);
                        sc = W::writelane(sc, df.mag64, 3);
                        sc = W::writelane(sc, df.q, 4);
                        slot.scalars[lane] = sc;
                    }
                    x_old[k] = far_cur;
                    d_old[k] = near_cur;
                }
            }
            if constexpr (kClean) {
                if (blk == n_blocks) {                                    // the last step: the clean input's last block -> the wave that stores V_OUTBUF
#pragma unroll
                    for (int k = 0; k < kPipeStreamsPerFront; ++k)
                        if (live[k]) sh.c_last[ks(k)][W::lane_id()] = c_prev[k];
                }
            }
            if (monitor) {
                const int n_words = (n_workgroups + 1) >> 1;
                int m = pv[0];
#pragma unroll
                for (int i = 1; i < kPipeMonitorLoads; ++i)
                    if (64 * i < n_words) m = pk_max_u16(m, pv[i]);
                const int slowest = 0xffff - W::reduce_max(imax(zext16(m), lsr(m, 16)));      // group count of the slowest workgroup that has published
                const int lead = (blk >> kPipeGroupLog2) - slowest;
                sh.ahead = lead > AECM_PIPE_BALANCE_LEAD ? 1 : 0;
                sh.level = sh.ahead ? AECM_PIPE_FRONT_PRIO : kFrontBehind;
            }
            slot_idx = slot_idx + 1 == kSlots ? 0 : slot_idx + 1;
            AECM_PIPE_BARRIER();
        }
        if (kDelay != 0) AECM_PIPE_BARRIER();                             // the middle waves' last step
        if (kGain != 0) AECM_PIPE_BARRIER();                              // the gain waves' last step
        if (kTail != 0) AECM_PIPE_BARRIER();                              // the tail waves' last step
        if (kGain != 0) AECM_PIPE_BARRIER();                              // (state hand-over of the gain waves)
        for (int k = 0; k < kPipeStreamsPerFront; ++k)
            if (live[k]) EF::store_time_state(st.vec + (kRagged ? strm[k] : slot_stream(ks(k))) * (int64_t)kVecWordsPerStream, r.lane, x_old[k], d_old[k]);
    } else if (wave < kPipeStreams + kPipeFrontWaves + kTail) {
        // ---- tail wave: kPipeStreams / kTail streams, inverse transform + synthesis + output of the block BEFORE the one the middle waves are at ----
        constexpr int kPer = kPipeStreams / 2;
        typename EF::Regs r;
        EF::init_lane_constants(r, st.consts);
        SetPrioDynamic((prio >> 2) & 3);
        k0 = slot_of((wave - kPipeStreams - kPipeFrontWaves) * kPer, rot_tail);
        int ovl[kPer], c_old[kPer];
        bool live[kPer];
        int len[kPer];
        int64_t strm[kPer];
        for (int k = 0; k < kPer; ++k) {
            const int64_t stream = slot_stream(ks(k));
            live[k] = slot_live(ks(k));
            len[k] = slot_len(ks(k));
            strm[k] = stream;
            ovl[k] = c_old[k] = 0;
            if (live[k]) EF::load_tail_state(st.vec + stream * (int64_t)kVecWordsPerStream, r.lane, ovl[k], c_old[k]);
        }
        AECM_PIPE_BARRIER();                                              // steps 0 and 1 (and 2 with delay waves): nothing to do yet
        AECM_PIPE_BARRIER();
        if (kDelay != 0) AECM_PIPE_BARRIER();
        if (kGain != 0) AECM_PIPE_BARRIER();
        for (int blk = 0; blk < n_blocks; ++blk) {                        // step blk + 2 (+ 1 with delay waves, + 1 with gain waves)
#pragma unroll
            for (int k = 0; k < kPer; ++k) {
                if (!live[k]) continue;
                if (kRagged && blk >= len[k]) continue;                   // nothing behind len x 64 samples is written
                const PipeTailSlot &ts = sh.tails[blk & 1][ks(k)];
                const int lane = W::lane_id();
                const int a = ts.a[lane], b = ts.b[lane];
                const int clean_q = __builtin_amdgcn_readfirstlane(ts.clean_q);
                r.table_index = Gfx950Wave<true, false>::table_index_for_this_block();
                r.out_ovl = ovl[k];
                const int out = EF::tail_block(r, a, b, clean_q);
                ovl[k] = r.out_ovl;
                typename EF::StridedIo sio{io, (kRagged ? strm[k] : slot_stream(ks(k))) * io.stream_stride};
                sio.out(r, blk, out);
            }
            AECM_PIPE_BARRIER();
        }
        if (kGain != 0) AECM_PIPE_BARRIER();                              // (state hand-over of the gain waves)
        if constexpr (kClean)
            for (int k = 0; k < kPer; ++k)
                if (live[k]) c_old[k] = sh.c_last[ks(k)][W::lane_id()];
        for (int k = 0; k < kPer; ++k)
            if (live[k]) EF::store_tail_state(st.vec + (kRagged ? strm[k] : slot_stream(ks(k))) * (int64_t)kVecWordsPerStream, r.lane, ovl[k], c_old[k]);
    } else if constexpr (kDelay != 0) {
        if (wave < kPipeStreams + kPipeFrontWaves + kTail + kDelay) {
            // ---- delay wave: kPipeStreams / kDelay streams, the delay estimator of the block AFTER the one their channel waves are at ----
            constexpr int kPer = kPipeStreams / kDelay;
            typename EF::Regs r;
            EF::init_lane_constants(r, st.consts);
                SetPrioDynamic((prio >> 4) & 3);
            k0 = slot_of((wave - (kPipeStreams + kPipeFrontWaves + kTail)) * kPer, rot_delay);
            // the estimator's state per stream (BlockEngine::load_delay_state's fields), moved into r around each call
            int mean[kPer], bh0[kPer], bh1[kPer], m01[kPer], far_init[kPer], near_init[kPer], min_prob[kPer], last_prob[kPer], last_delay[kPer];
            int hist_pos[kPer], fixed_delay[kPer];                        // the channel wave's u.hist_pos, followed here
            bool live[kPer];
            int len[kPer];
            int64_t strm[kPer];
            auto swap_in = [&](int k) {
                r.mean = mean[k]; r.bh0 = bh0[k]; r.bh1 = bh1[k]; r.m01 = m01[k];
                r.u.far_init = far_init[k]; r.u.near_init = near_init[k]; r.u.min_prob = min_prob[k]; r.u.last_prob = last_prob[k];
                r.u.last_delay = last_delay[k]; r.u.fixed_delay = fixed_delay[k];
            };
            auto swap_out = [&](int k) {
                mean[k] = r.mean; bh0[k] = r.bh0; bh1[k] = r.bh1; m01[k] = r.m01;
                far_init[k] = r.u.far_init; near_init[k] = r.u.near_init; min_prob[k] = r.u.min_prob; last_prob[k] = r.u.last_prob;
                last_delay[k] = r.u.last_delay;
            };
#pragma unroll
            for (int k = 0; k < kPer; ++k) {
                const int64_t stream = slot_stream(ks(k));
                live[k] = slot_live(ks(k));
                len[k] = slot_len(ks(k));
                strm[k] = stream;
                hist_pos[k] = 0; fixed_delay[k] = -1;
                r.mean = r.bh0 = r.bh1 = r.m01 = 0;
                r.u.far_init = r.u.near_init = r.u.min_prob = r.u.last_prob = r.u.last_delay = 0;
                if (live[k]) {
                    const int32_t *scal = st.scal + stream * (int64_t)kNumScal;
                    EF::load_delay_state(r, st.vec + stream * (int64_t)kVecWordsPerStream, scal);
                    hist_pos[k] = __builtin_amdgcn_readfirstlane(scal[S_HISTPOS]);
                    fixed_delay[k] = __builtin_amdgcn_readfirstlane(scal[S_FIXED_DELAY]);
                }
                swap_out(k);
            }
            AECM_PIPE_BARRIER();                                          // step 0: nothing to do yet
            int slot_idx = 0, slot_before = kSlots - 1;
            for (int blk = 0; blk < n_blocks; ++blk) {                    // step blk + 1
                const int lane = W::lane_id();
                int far[kPer];
                bool fetch[kPer];
#pragma unroll
                for (int k = 0; k < kPer; ++k) {
                    fetch[k] = false;
                    if (!live[k]) continue;
                    if (kRagged && blk >= len[k]) continue;
                    const auto &slot = sh.slots[slot_idx][ks(k)];             // (PipeSlot or PipeCleanSlot: the same two rows)
                    const int m = slot.mags[lane], sc = slot.scalars[lane];
                    typename EF::Spectrum xf, df;
                    xf.mag = zext16(m);
                    xf.q = __builtin_amdgcn_readlane(sc, 1);
                    df.mag = lsr(m, 16);
                    df.q = __builtin_amdgcn_readlane(sc, 4);
                    r.table_index = Gfx950Wave<true, false>::table_index_for_this_block();
                    swap_in(k);
                    const int estimate = EF::delay_block(r, xf, df);
                    swap_out(k);
                    if (lane == 0) sh.delays[blk & 1][ks(k)] = estimate;
                    // AlignedFarend for the channel wave: the history row it would fetch next step.  The row of the block before this
                    // one is being written in this very step -- but that block's spectrum is still in its slot; older rows are in
                    // memory (written at least one barrier ago, or by an earlier launch); a delay of 0 is the block's own spectrum,
                    // which the channel wave has.
                    hist_pos[k] = hist_pos[k] + 1 >= kHistory ? 0 : hist_pos[k] + 1;
                    const int delay = EF::effective_delay(r.u, estimate);
                    fetch[k] = delay != 0;
                    if (delay != 0) {
                        const uint16_t *hist = st.hist + (kRagged ? strm[k] : slot_stream(ks(k))) * (int64_t)kHistWordsPerStream;
                        if (delay == 1 && blk > 0) far[k] = zext16(sh.slots[slot_before][ks(k)].mags[lane]);
                        else far[k] = Gfx950Wave<true, false>::load_u16(hist + EF::aligned_slot(hist_pos[k], delay) * kLanes, lane);
                    }
                }
#pragma unroll
                for (int k = 0; k < kPer; ++k)                            // (the stores after every stream's fetch is under way)
                    if (fetch[k]) sh.far_rows[blk & 1][ks(k)][lane] = far[k];
                slot_before = slot_idx;
                slot_idx = slot_idx + 1 == kSlots ? 0 : slot_idx + 1;
                AECM_PIPE_BARRIER();
            }
            AECM_PIPE_BARRIER();                                          // the channel waves' last step
            if (kGain != 0) AECM_PIPE_BARRIER();                          // the gain waves' last step
            if (kTail != 0) AECM_PIPE_BARRIER();                          // the tail waves' last step
            if (kGain != 0) AECM_PIPE_BARRIER();                          // (state hand-over of the gain waves)
#pragma unroll
            for (int k = 0; k < kPer; ++k) {
                if (!live[k]) continue;
                swap_in(k);
                const int64_t stream = kRagged ? strm[k] : slot_stream(ks(k));
                EF::store_delay_state(r, st.vec + stream * (int64_t)kVecWordsPerStream, st.scal + stream * (int64_t)kNumScal);
            }
        } else if constexpr (kGain != 0) {
            // ---- gain wave: one stream, gain_block of the block BEFORE the one its channel wave is at ----
            typename EF::Regs r;
            EF::init_lane_constants(r, st.consts);
                SetPrioDynamic((prio >> 6) & 3);
            const int k = slot_of(wave - (kPipeStreams + kPipeFrontWaves + kTail + kDelay), rot_gain);
            const int64_t stream = slot_stream(k);
            const bool live = slot_live(k);
            const int len = slot_len(k);
            if (live) EF::load_state(r, st.vec + stream * (int64_t)kVecWordsPerStream, st.scal + stream * (int64_t)kNumScal);
            AECM_PIPE_BARRIER();                                          // steps 0, 1, 2: nothing to do yet
            AECM_PIPE_BARRIER();
            AECM_PIPE_BARRIER();
            int slot_idx = 0;
            for (int blk = 0; blk < n_blocks; ++blk) {                    // step blk + 3
                if (live && (!kRagged || blk < len)) {
                    const int lane = W::lane_id();
                    typename EF::Spectrum df, cf;
                    const typename EF::Spectrum &clean = kClean ? cf : df;
                    if constexpr (kClean) {
                        const PipeCleanSlot &slot = sh.slots[slot_idx][k];
                        typename EF::Spectrum xf;
                        EF::unpack_clean_hand_over({slot.clean_x[lane], slot.mags[lane], slot.clean_mag[lane], slot.scalars[lane]}, xf, df, cf);
                    } else {
                        const PipeSlot &slot = sh.slots[slot_idx][k];
                        typename EF::Spectrum xf;                         // (of the far end this wave reads nothing)
                        EF::unpack_hand_over({slot.near_x[lane], slot.mags[lane], slot.scalars[lane]}, xf, df);
                    }
                    const PipeGainSlot &gs = sh.gains[blk & 1][k];
                    typename EF::GainInput g;
                    g.echo_est = gs.echo_est[lane];
                    g.echo_est64 = __builtin_amdgcn_readfirstlane(gs.echo_est64);
                    g.far_q = __builtin_amdgcn_readfirstlane(gs.far_q);
                    g.cur_vad = __builtin_amdgcn_readfirstlane(gs.cur_vad);
                    g.near0 = __builtin_amdgcn_readfirstlane(gs.near0);
                    g.stored0 = __builtin_amdgcn_readfirstlane(gs.stored0);
                    r.table_index = Gfx950Wave<true, false>::table_index_for_this_block();
                    EF::track_q(r.u, df, clean);
                    const typename EF::TailInput t = EF::gain_block(r, df, clean, g);
                    PipeTailSlot &ts = sh.tails[blk & 1][k];
                    ts.a[lane] = t.a;
                    ts.b[lane] = t.b;
                    if (lane == 0) ts.clean_q = t.clean_q;
                }
                slot_idx = slot_idx + 1 == kSlots ? 0 : slot_idx + 1;
                AECM_PIPE_BARRIER();
            }
            if (live) {                                                   // this wave's part of the state -> the channel wave (which stores the state)
                const int lane = W::lane_id();
                PipeGainState &g = sh.gain_state[k];                      // (restates EF::pack_gain_state, store by store, for the same reason as the front waves' pack)
                g.echo_filt[lane] = r.b.echo_filt;
                g.near_filt_ctrs[lane] = zext16(r.b.near_filt) | shl(r.b.low_ctr & 7, 16) | shl(r.b.high_ctr & 7, 19);
                g.noise_est[lane] = r.b.noise_est;
                if (lane == 0) {
                    const Uniform &u = r.u;
                    g.scal[0] = u.seed; g.scal[1] = u.sup_gain; g.scal[2] = u.sup_gain_old; g.scal[3] = u.noise_ctr;
                    g.scal[4] = r.b64.echo_filt; g.scal[5] = r.b64.near_filt; g.scal[6] = r.b64.noise_est; g.scal[7] = r.b64.low_ctr; g.scal[8] = r.b64.high_ctr;
                }
            }
            if (kTail != 0) AECM_PIPE_BARRIER();                          // the tail waves' last step
            AECM_PIPE_BARRIER();                                          // (state hand-over)
        }
    }
#if defined(AECM_PIPE_TRACE)
    if (!kRagged && (threadIdx.x & 63u) == 0) {      // (a ragged launch's `progress` is its plan, read only: no trace records)
        uint64_t *tr = reinterpret_cast<uint64_t *>(progress + 2 * ((n_workgroups + 3) / 4) * 2) + ((size_t)blockIdx.x * kPipeTraceWaves + wave) * 4;
        // where the wave ran: HW_ID (wave slot 3:0, SIMD 5:4, CU 11:8, SH 12, SE 15:13) above bit 40 of the wait count, XCC_ID above bit 40 of the total
        const uint64_t hw_id = __builtin_amdgcn_s_getreg((31 << 11) | 4), xcc_id = __builtin_amdgcn_s_getreg((31 << 11) | 20);
        tr[0] = trace_t0; tr[1] = wall_clock64(); tr[2] = (trace_wait & ((1ull << 40) - 1)) | ((hw_id & 0xffffff) << 40);
        tr[3] = ((clock64() - trace_c0) & ((1ull << 40) - 1)) | ((xcc_id & 0xf) << 40);
    }
#endif
