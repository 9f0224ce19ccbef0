// The block kernels of the MI355X AECM engine.  One block DSP (BlockEngine, aecm_wave.h) under three launch forms:
//   aecm_process_kernel            one wavefront per stream for the whole launch (described next)
//   aecm_process_queue_kernel      launches larger than the chip: (chunk, stream) items claimed in order by a resident grid
//   aecm_process_ragged_queue_kernel  the same queue for streams of different lengths: items by a host-made plan, longest streams first
//   aecm_process_pipelined_kernel  launches the chip holds at once: six waves per four streams, transforms one block ahead
//   aecm_process_pipelined_ragged_kernel  the same for streams of different lengths (opt-in): each slot of a workgroup its own length
//   aecm_process_pipelined_clean_kernel   the same for launches with a clean near-end input (opt-in): three transforms in the front waves
// (aecm_engine.cpp: PlanLaunch picks by the size of the launch; the forms give identical results.)
//
// The whole persistent state of a stream (~40 lane vectors + ~50 scalars) is loaded into registers once, n_blocks blocks
// are processed back to back (WebRtcAecm_ProcessBlock-equivalents, aecm_wave.h), and the state is written back once.  Per
// block a wave touches 3 x 128 B of audio I/O (prefetched one block ahead), writes one 128-byte far-spectrum row and reads
// at most one.  The constant tables (FFT twiddles, comfort-noise cos/sin, sqrt-Hanning) are staged in LDS by the prologue.
// No MFMA: nothing here is a dense contraction.
//
// Compiled with -mllvm -structurizecfg-skip-uniform-regions (build.py: SOURCE_FLAGS).  Every branch of the block loop is
// wave-uniform (scalar conditions); the structurizer otherwise rewrites each if / else into guarded single-entry regions
// joined by flow blocks -- extra scalar mask logic, extra branches and duplicated code that the nested data-dependent
// short paths of aecm_wave.h multiply: 3294 -> 2933 instructions in the kernel, 928 -> 983 M frames/s
// (profiles/r03_experiments.md section 7).  For the same reason this unit is compiled with SimplifyCFG's phi-to-select
// folding and the speculative-execution pass turned off (build.py: KEEP_BRANCHES_FLAGS): a uniform branch that skips a
// block costs nothing, its select form executes both sides on the vector port that bounds the kernel (983 -> 1 010 M,
// section 9).  A translation unit of its own so that it compiles next to the tick kernels' unit (aecm_kernels.hip) and its
// flags can differ from theirs.
#define AECM_TABLE_ATTR __device__
#define AECM_CHECK_UNIT blocks      // (aecm_kernel_common.h: the unit's pair of audit counters)
#include <type_traits>

#include "aecm_kernel_common.h"
#include "aecm_block_queue.h"

namespace aecm {

// This unit's share of the audit counters (see ReadCheckCounters in aecm_kernels.hip).
AECM_DEFINE_CHECK_COUNTERS(ReadBlockKernelCheckCounters)

// (The occupancy these kernels are built for -- AECM_WAVES_PER_EU, AECM_ROTATION_WAVES_PER_EU -- and the queue's claim / wait /
// publish steps live in aecm_block_queue.h, which the traced kernels' unit, aecm_trace_kernels.hip, includes too.)
template <bool kFast, bool kHasClean, bool kPhasePrio = true>
__global__ __launch_bounds__(64 * kWavesPerWorkgroup)
__attribute__((amdgpu_waves_per_eu(kPhasePrio ? AECM_WAVES_PER_EU : AECM_ROTATION_WAVES_PER_EU, AECM_MAX_WAVES_PER_EU)))
void aecm_process_kernel(StatePtrs st, IoView io, int n_streams, int n_blocks, const int32_t *blocks_per_stream) {
    FillLdsTables<64 * kWavesPerWorkgroup>(st.consts);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t stream = (int64_t)blockIdx.x * kWavesPerWorkgroup + wave;
    if (stream >= n_streams) return;
    if (blocks_per_stream) {
        n_blocks = __builtin_amdgcn_readfirstlane(blocks_per_stream[stream]);
        if (n_blocks <= 0) return;
    }
    BlockEngine<Gfx950Wave<kFast, kPhasePrio>, kHasClean>::run_stream(st, io, stream, n_blocks);
}

// ---- the chunk-queue form: one launch, (chunk, stream) items claimed in order by resident waves -------------------------
// A launch of S streams x T blocks in the form above gives every wave one stream for all T blocks.  Waves start when a slot
// frees up, so when the last stream has been handed out the resident waves are anywhere between their first and their last
// block, and the launch drains for most of a stream's duration at falling occupancy -- a SIMD below ~5 waves no longer
// fills its issue ports: measured 1.7-2.3 ms of an 83 ms launch at 65 536 streams, the same 2 ms of a 22 ms launch at 16 384
// (profiles/r04_experiments.md section 1).  Here the launch is cut into chunks of C blocks, item i = (chunk i / S, stream
// i % S), and a grid that just fills the chip claims items in order from one counter: all streams advance together, and
// what is left when the counter runs out is at most C blocks per wave -- the drain shrinks by T / C.
//
// A stream's chunk c + 1 is picked up by whichever wave comes next, on any CU of any XCD, so between chunks the state
// travels through memory at agent scope (Gfx950Wave<.., kCoherentState>: sc1 loads and stores, no fences -- a release
// fence at agent scope is a write-back of the XCD's whole L2).  Order: the claimer of item i - S holds it before item i is
// claimed (one counter), so a wave that finds done[stream] < chunk waits for a wave that is running -- no deadlock even
// when the grid is larger than the chip; with S >= the resident waves the wait practically never happens.  The wait is
// bounded anyway: a wave that gives up raises *err (never cleared by a launch; the engine reports it at the next
// synchronisation) and leaves.
// What the hand-over rests on.  This is the write-through publish form of the platform guide (cdna_hip_programming.md section 6,
// Guideline 16 / R1, and MI355X_MICROARCH.md "Workgroup dispatch, XCD placement & inter-workgroup visibility: valid forms"):
//   producer: every byte of the payload (state words, scalars, history rows) leaves the wave as an sc1 store -- a relaxed
//             agent-scope __hip_atomic_store of 4 / 2 bytes per lane, the kernel's natural store width, which the guide names as
//             the right form for such epilogues; sc1 stores are written through to memory and DROP the line from the XCD's L2 --
//             then `asm volatile("s_waitcnt vmcnt(0)")` in the publishing wave (inline asm: the compiler cannot drop or move
//             it), then ONE relaxed agent-scope flag store;
//   consumer: relaxed polls of the flag, then sc1 loads of the payload ("sc1 loads may replace the acquire only when the producer
//             stored sc1": they bypass the CU's L1 and are served where the eight XCDs agree).
// One wave produces and one wave consumes a stream's chunk, so "every writing wave drains" is that one s_waitcnt.  No
// buffer_wbl2 / buffer_inv anywhere: a release fence is a write-back of the XCD's whole L2 (the audio output rows of every
// resident wave), an acquire drops the CU's L1 under three other workgroups.  Measured cost of the fenced form
// (-DAECM_QUEUE_FENCES=1: release store / acquire poll on done[]; the same results): 65 536 streams 1 053 -> 1 030 M frames/s,
// 8 192 streams (32-block chunks) 983 -> 899 M.  The build switch stays for a platform whose sc1 semantics differ;
// tests/test_gpu_parity.py::test_chunk_queue_half_a_million_hand_overs and tools/soak_parity.py are the gate either way.
// (QueueClaim, QueueWait, QueuePublish: aecm_block_queue.h.)
template <bool kHasClean>
__global__ __launch_bounds__(64 * kWavesPerWorkgroup)
__attribute__((amdgpu_waves_per_eu(AECM_WAVES_PER_EU, AECM_MAX_WAVES_PER_EU)))
void aecm_process_queue_kernel(StatePtrs st, IoView io, int n_streams, int n_blocks, int chunk_blocks, int n_chunks, uint32_t *ctl,
                               uint32_t *err) {
    FillLdsTables<64 * kWavesPerWorkgroup>(st.consts);
    // without a clean input this is the headline kernel: it and its ragged twin below take the lean block loop (BlockEngine::kLeanItems)
    using E = BlockEngine<Gfx950Wave<true, true, false, true, !kHasClean>, kHasClean>;
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
        typename E::StridedIo sio{io, (int64_t)stream * io.stream_stride + (int64_t)first * io.block_stride};
        E::run_stream_io(st, sio, (int64_t)stream, nb);
        QueuePublish(done, stream, chunk);
    }
}

// ---- the ragged chunk queue: every stream its own number of blocks ---------------------------------------------------
// A corpus of recordings never has one length.  The work of this launch is the SUM of the streams' lengths, not S x the
// longest: the host sorts the streams by length, longest first (BuildRaggedPlan, aecm_engine.cpp), so that the streams
// live in chunk c -- those with more than c x chunk_blocks blocks -- are the ranks [0, live[c]) of that order, and the
// queue's items are, chunk-major, first_item[c] .. first_item[c] + live[c] (first_item = prefix sums of live).  Behind
// done[] the control buffer carries the plan (RaggedPlanOffsetWords): len[S], order[S], first_item[n_chunks + 1].
// A wave claims items from the one counter as above.  Its claims are monotone, so it finds an item's chunk with a cursor
// that only moves forward (amortised one load per item, no division), takes stream = order[item - first_item[chunk]] and
// runs min(chunk_blocks, len[stream] - chunk x chunk_blocks) >= 1 blocks.  Streams of length 0 have no item: nothing of
// theirs is read or written.
// The hand-over between chunks is the one described above, unchanged (sc1 payload, s_waitcnt, one relaxed flag store;
// relaxed polls, sc1 loads; AECM_QUEUE_FENCES), and so is the no-deadlock argument: the items are chunk-major and a stream
// live in chunk c is live in chunk c - 1, so item (c, s) has a larger number than item (c - 1, s) and is claimed after it
// (one counter).  A wave that finds done[s] < c therefore waits for a wave that HOLDS (c - 1, s): one that is running it,
// or is itself waiting for (c - 2, s) -- a chain that ends at a chunk 0, which waits for nobody.  Late chunks of a
// long-tailed batch have fewer live streams than the grid has waves: the surplus waves find the counter exhausted and
// leave, the tail runs as serially as a stream's chunks depend on each other.  The wait stays bounded and raises *err.
// (A kernel of its own with the equal-length kernel's item loop restated around the shared claim / wait / publish steps, not a
// template parameter of that kernel: the
// headline kernels' instruction streams stay exactly what they were.)
template <bool kHasClean>
__global__ __launch_bounds__(64 * kWavesPerWorkgroup)
__attribute__((amdgpu_waves_per_eu(AECM_WAVES_PER_EU, AECM_MAX_WAVES_PER_EU)))
void aecm_process_ragged_queue_kernel(StatePtrs st, IoView io, int n_streams, uint32_t n_items, int chunk_blocks, uint32_t *ctl, uint32_t *err) {
    FillLdsTables<64 * kWavesPerWorkgroup>(st.consts);
    // the same engine instantiation as aecm_process_queue_kernel's, as it always was (the compiler's inlining of the block loop
    // into either kernel depends on the two sharing it): without a clean input the ragged queue takes the lean block loop too
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
            typename E::StridedIo sio{io, (int64_t)stream * io.stream_stride + (int64_t)first * io.block_stride};
            E::run_stream_io(st, sio, (int64_t)stream, nb);
        }
        QueuePublish(done, stream, chunk);
    }
}

// ---- the pipelined form: launches the chip holds at once ------------------------------------------------------------
// With one wavefront per stream a launch of S <= 4 096 streams puts at most 4 waves on a SIMD, every one of them alternating
// between a stretch of dense vector work (the transforms) and a long scalar-heavy stretch (delay estimator, energies,
// channel bookkeeping, gains): 4 096 streams run at 75 % of the rate the issue ports sustain with 7 waves.  But a block's
// first third -- windows, forward transforms and magnitudes (BlockEngine::front_block, 36 % of its vector instructions) --
// depends on the input samples alone, not on the adaptive state.  Here a workgroup of SIX waves serves FOUR streams:
// waves 0..3 run back_block for one stream each, waves 4 and 5 run front_block for two streams each, one block ahead, and
// hand the spectra over through LDS (two buffers per stream, one barrier per block: while the back waves read the spectra
// of block b the front waves write those of block b + 1).  Per stream the sequential part of a block shrinks to the back
// part, and a SIMD holds 6 waves instead of 4 -- two of them nearly pure vector work that overlaps the others' scalar
// stretches by construction.  4 workgroups per CU (24 waves, 4 x 27 KB of LDS) = 4 096 streams on 256 CUs, all resident.
#ifndef AECM_PIPE_FRONT_PRIO
#define AECM_PIPE_FRONT_PRIO 0        // the front waves' issue priority (the back waves': by phase, 1..3).  Also in the sixteen-wave shape,
                                      // where the front waves are the longest link: 1 / 2 / 3 there cost 10-13 % (1 024 streams 613 -> 549 / 549 / 531)
#endif
constexpr int kPipeStreams = 4;
// Slot rotations: PipeShape::rot (the kernel's slot_of), chosen per shape in PipelinedShapeFor.  There is none per workgroup of a CU by
// default (rot bits 6-7): the hardware does that one itself -- traced (tools/pipe_trace.py, cu_mates), the second and third workgroup
// of a CU each start one SIMD further round the cycle 0, 2, 1, 3 than the one before; a software rotation on top brings the same
// slots back onto the same SIMDs (1 024 streams as 2 x 2 per CU: 620 -> 493 M frames/s).
// kFront front waves per workgroup: 2 (two streams each; the form for launches that fill the chip) or 4 (one stream each: ten-wave
// workgroups with two tail waves, two to a CU -- launches of up to 2 048 streams, where the chip has wave slots to spare and a
// front wave with two streams' transforms is the longest link of the chain).
// A third role (round 5): tail_block -- inverse transform, synthesis window, overlap-add, the output store: 19 % of a block's
// vector instructions and a long chain of LDS table reads and lane exchanges -- in kTail "tail" waves of their own, one block
// BEHIND the middle waves (which then run middle_block only): two waves of two streams, eight waves per workgroup, three
// workgroups per CU (launches of up to 3 072 streams).  The stream's sequential part
// shrinks once more (what a small launch is bound by) and a SIMD gets one more wave of dense vector work to fill its port with.
// A fourth role (round 5, small launches): delay_block -- both binary spectra, the bit histories, the 100 means; a chain of
// reductions and scalar decisions on state of its own, a sixth of the middle wave's instructions -- in kDelay "delay" waves, one
// stream each, one block AHEAD of the middle waves (between them and the front waves): the spectra then live for three steps
// (three slots per stream) and the delay reaches the middle wave through LDS.
// A fifth (smallest launches: at most one workgroup per CU): the back wave's remaining work in its two halves, channel_block
// (far history ... channel update: what the next block's echo estimate waits for) and gain_block (suppression gain ... comfort
// noise: fed by the channel half, otherwise state of its own), the second in kGain "gain" waves one block behind the first.
// Sixteen waves per four streams then: 4 channel, 4 front, 2 tail, 2 delay (two streams each), 4 gain -- the longest link of the
// chain is half of what it was.
constexpr int PipeWaves(int tail_waves, int front_waves = 2, int delay_waves = 0, int gain_waves = 0) {
    return kPipeStreams + front_waves + tail_waves + delay_waves + gain_waves;
}
struct PipeSlot {           // the spectra of one block of one stream on their way from the front to the back wave
    int near_x[kLanes];     // near-end spectrum, bins 0..63: re | im << 16 (im conjugated as the block path uses it)
    int mags[kLanes];       // far-end magnitude | near-end magnitude << 16 (both <= 46 340)
    int scalars[kLanes];    // lanes 0..4: far mag[64], far Q, near re[64], near mag[64], near Q
};
struct PipeRawSlot {        // the same hand-over BEFORE the spectra are formed (kRaw instantiations): the transforms' outputs
    int fa[2][kLanes], fb[2][kLanes];     // BlockEngine::front_transforms: far end [0], near end [1]
    int q[2], pad[2];
};
struct PipeCleanSlot {       // the hand-over of a launch with a clean near-end input: BlockEngine::CleanHandOver (aecm_wave.h), 256 B more
    int clean_x[kLanes];     // clean spectrum, bins 0..63: re | im << 16
    int mags[kLanes];        // far-end magnitude | near-end magnitude << 16 (PipeSlot's row)
    int clean_mag[kLanes];   // clean magnitude
    int scalars[kLanes];     // lanes 0, 1: far mag[64], Q; 3, 4: near mag[64], Q (PipeSlot's lanes); 5, 6, 7: clean re[64], mag[64], Q
};
struct PipeTailSlot {       // the residual spectrum of one block of one stream on its way from the middle to the tail wave
    int a[kLanes], b[kLanes];   // BlockEngine::TailInput
    int clean_q, pad[3];
};
struct PipeGainSlot {       // BlockEngine::GainInput on its way from the channel to the gain wave
    int echo_est[kLanes];
    int echo_est64, far_q, cur_vad, near0, stored0, pad[3];
};
struct PipeGainState {      // the gain wave's part of the stream state on its way to the channel wave, which stores the state (end of the launch)
    int echo_filt[kLanes], near_filt_ctrs[kLanes], noise_est[kLanes];      // (near_filt | low_ctr << 16 | high_ctr << 19: the V_NEARFILT layout)
    int scal[16];
};
// Clean launches: the clean input's samples of each stream's LAST block on their way from the front wave, which has them in
// registers, to the wave that stores V_OUTBUF (out_ovl | c_old << 16: the tail wave, or the back wave without tail waves) -- written
// in the front waves' last step, read behind the launch's last barrier.  (A base class: nothing is added to the other launches' LDS.)
template <bool kClean> struct PipeCleanLast {};
template <> struct PipeCleanLast<true> { int c_last[kPipeStreams][kLanes]; };
template <int kTail, bool kRaw = false, int kDelay = 0, int kGain = 0, bool kClean = false>
struct PipeShared : PipeCleanLast<kClean> {
    static_assert(!(kRaw && kClean), "clean launches: the formed-spectra hand-over");
    // [block modulo the ring: 2, + 1 with delay waves, + 1 with gain waves][stream of the workgroup]
    typename std::conditional<kRaw, PipeRawSlot, typename std::conditional<kClean, PipeCleanSlot, PipeSlot>::type>::type
        slots[2 + (kDelay ? 1 : 0) + (kGain ? 1 : 0)][kPipeStreams];
    PipeTailSlot tails[kTail ? 2 : 1][kTail ? kPipeStreams : 1];
    int delays[2][kPipeStreams];          // delay_block's result on its way from the delay to the middle wave ...
    int far_rows[kDelay ? 2 : 1][kDelay ? kPipeStreams : 1][kLanes];      // ... and the far-history row that goes with it (AlignedFarend)
    PipeGainSlot gains[kGain ? 2 : 1][kGain ? kPipeStreams : 1];
    PipeGainState gain_state[kGain ? kPipeStreams : 1];
    int ahead;                            // this workgroup leads the launch's slowest one by more than the allowed lead (balance, below)
    int level;                            // the front waves' base priority for the current group of blocks (balance)
};
#ifndef AECM_PIPE_TAIL_PRIO
#define AECM_PIPE_TAIL_PRIO 1         // the tail waves' issue priority
#endif
// Workgroups of the sixteen-wave shape a CU takes (experiments: two of them are 32 waves, eight per SIMD -- the kernel's 61 VGPRs allow it)
#ifndef AECM_PIPE_GAIN_WGS_PER_CU
#define AECM_PIPE_GAIN_WGS_PER_CU (PipeWorkgroupsPerCu<2, 4, 2, 4>())
#endif
// Which launches get delay and gain waves (the sixteen-wave shape) when the caller does not say, by the workgroups of four streams
// the launch makes and the CUs of the device: up to two sixteen-wave workgroups per CU (eight streams per CU).
// Round 5 gave this shape one workgroup per CU only (1 024 streams 492 -> 612 M frames/s with the gain waves, 256 streams 124 -> 155)
// because two of them measured 620 M at 2 048 streams against the ten-wave shape's 740: with 81 SGPRs the two never shared a CU
// (PipeWavesPerEu below), and with every one-stream role of a slot on the same SIMD a CU of five streams ran them at 0.43 instead of
// 0.60 M frames/s each.  Built for eight waves per SIMD and with the roles staggered over the SIMDs (the kernel's slot_of) the shape
// carries a CU's eight streams as well as the ten-wave shape and everything below better (profiles/r06_experiments.md):
// 1 280 streams 482 -> 650, 1 536: 571 -> 688, 1 792: 647 -> 702, 2 048: 738 / 734.
constexpr bool PipeDeepShapeByDefault(int n_wg, int cus) { return n_wg <= 2 * cus; }
#ifndef AECM_PIPE_GAIN_PRIO
#define AECM_PIPE_GAIN_PRIO 3         // the gain waves' issue priority (1 / 2 / 3: 1 024 streams 594 / 607 / 613 M frames/s)
#endif
#ifndef AECM_PIPE_DELAY_PRIO
#define AECM_PIPE_DELAY_PRIO 1        // the delay waves' issue priority
#endif

// Balance.  Every workgroup of a pipelined launch is resident from the start and has the same amount of work, but the SIMD's
// arbiter serves the highest priority first and then its OLDEST wave: the workgroups dispatched first pull ahead, finish
// early, and the launch ends at low occupancy (round 4: 4.71 of the 6 placed waves resident on average, vector port 76 %).
// Progress feedback: blocks are counted in groups of 2^AECM_PIPE_BALANCE_GROUP_LOG2.  At every group boundary the first
// front wave of a workgroup (the "monitor": front waves finish their step early and would otherwise just park at the
// barrier) publishes the workgroup's group count in its own word of progress[] (a write-through store, no atomic), reads
// everybody's words (n_workgroups / 64 loads of 64 lanes, issued at the top of its step and looked at at the end of it) and
// takes their minimum: a workgroup more than AECM_PIPE_BALANCE_LEAD groups ahead of the slowest one runs its FRONT waves at
// AECM_PIPE_FRONT_PRIO instead of kPipeFrontPrioBehind for the next group -- a workgroup advances at the pace of its front waves
// (the back waves run at higher priorities and park at the barrier until the spectra of the next block are there: measured 30 %
// of their time at 4 096 streams), so the front waves are the handle.  The level reaches them through LDS behind the barrier
// every wave executes anyway.  Stale words only make the verdict late.  AECM_PIPE_BALANCE 0: no launch takes the balanced form.
// (Tried and not built -- back-wave demotion, one level per group of lead, a sampled monitor, "behind the fastest" as the rule,
// seven-wave workgroups with one tail wave: profiles/r05_experiments.md, profiles/r09_experiments.md.)
#ifndef AECM_PIPE_BALANCE
#define AECM_PIPE_BALANCE 2
#endif
#ifndef AECM_PIPE_BALANCE_GROUP_LOG2
#define AECM_PIPE_BALANCE_GROUP_LOG2 4
#endif
#ifndef AECM_PIPE_BALANCE_LEAD
#define AECM_PIPE_BALANCE_LEAD 1
#endif
constexpr int kPipeFrontPrioBehind = 1;                 // the front waves' priority while their workgroup is NOT ahead (balanced launches)
// A front wave's priority rises by this while it works on its second stream (the rule of the back waves' phase table -- the
// priority rises with the progress through the step).  Not on top of the balance: 4 096 streams 862 M frames/s without, 844 with.
constexpr int kPipeFrontSecondBoost = 1, kPipeFrontSecondBoostBalanced = 0;
__device__ __forceinline__ void SetPrioDynamic(int p) {      // s_setprio takes an immediate
    if (p <= 0) __builtin_amdgcn_s_setprio(0);
    else if (p == 1) __builtin_amdgcn_s_setprio(1);
    else if (p == 2) __builtin_amdgcn_s_setprio(2);
    else __builtin_amdgcn_s_setprio(3);
}
constexpr int kPipeGroupLog2 = AECM_PIPE_BALANCE_GROUP_LOG2, kPipeGroupMask = (1 << kPipeGroupLog2) - 1;
constexpr int kPipeTraceWaves = 16;       // per-wave records per workgroup in the diagnostics build (the largest workgroup has 14)
constexpr int kPipeMonitorLoads = 10;     // x 64 lanes x 2 halves: launches of up to 1 280 workgroups are balanced, larger ones run as before

// (With delay waves everything behind the front waves is one step later: the delay waves work on block s - 1, the middle
// waves on block s - 2 out of slots[(s - 2) % 3], the tail waves on block s - 3; n_blocks + 3 barriers.)
// Synchronisation: ONE workgroup barrier per step.  In step s the front waves write the spectra of block s into slots[s & 1],
// the middle (back) waves work on block s - 1 out of slots[(s - 1) & 1] and, with tail waves, leave its residual spectrum in
// tails[(s - 1) & 1], which the tail waves turn into output samples in step s + 1.  Every wave of the workgroup executes
// n_blocks + 1 + (kTail ? 1 : 0) barriers whatever its role and whether or not its streams exist (a role's idle steps are the
// bare barriers in front of / behind its block loop).
// (Measured against rings with per-stream counters and no barrier -- pairs of waves that only wait for each other:
// slower, 4 096 streams 783 vs 818 M frames/s.  A wave parked at a barrier costs nothing; a wave polling a counter costs
// issue slots, and at the priority its last phase left it with it starves the wave it is waiting for.)
// kBalance: the progress feedback of the front waves' priority (above) is compiled in; launches that do not use it (fewer than
// four workgroups per CU) take the instantiation without it -- the same kernel with its monitor and its run-time priority
// levels switched off at run time measured 2 % slower there.
// kRaw: the front waves hand over the transforms' raw outputs and the back waves form the spectra (bin order, magnitudes: 40 of a
// stream's 198 front-part vector instructions) themselves.  For the balanced instantiation: with four workgroups per CU a
// workgroup advances at the pace of its front waves while its back waves sit at the barrier for a third of their time.
#ifndef AECM_PIPE_RAW_HANDOVER
#define AECM_PIPE_RAW_HANDOVER 1
#endif
// The occupancy a shape is built for.  Eight waves per SIMD need <= 64 VGPRs AND <= 80 SGPRs (MI355X_MICROARCH.md "Residency": with
// 82-96 SGPRs the hardware admits seven, whatever the compiler's occupancy line says): the sixteen-wave shape fits both without a
// spill, and two of its workgroups on a CU are exactly the 32 wave slots.  (Round 5 measured "two sixteen-wave workgroups per CU" as
// 620 M at 2 048 streams -- with 81 SGPRs they never were on a CU together; they took turns.)
#ifndef AECM_PIPE16_WAVES_PER_EU
#define AECM_PIPE16_WAVES_PER_EU 8
#endif
constexpr int PipeWavesPerEu(int gain_waves) {
#if defined(AECM_CHECKED)
    return AECM_WAVES_PER_EU;
#else
    return gain_waves != 0 ? AECM_PIPE16_WAVES_PER_EU : AECM_WAVES_PER_EU;
#endif
}
// The kernel's text is in aecm_pipelined_body.inc, included into two kernels: aecm_process_pipelined_kernel (kRagged = false: every
// stream n_blocks blocks; its name and six template arguments are what tools and tests find it by in the device assembly, and its
// instruction streams are the ones it had before the ragged form existed -- a body shared through an inlined function template
// with kRagged as its last parameter came out 2 to 29 instructions longer per instantiation) and
// aecm_process_pipelined_ragged_kernel (kRagged = true: every stream its own number of blocks, by a plan of the host's -- see
// "Ragged" at the body's first lines -- which `progress` points to; streams_base = the streams of the launch; the unbalanced shapes).
template <int kTail, bool kBalance, bool kRaw = false, int kFront = 2, int kDelay = 0, int kGain = 0>
__global__ __launch_bounds__(64 * PipeWaves(kTail, kFront, kDelay, kGain))
__attribute__((amdgpu_waves_per_eu(PipeWavesPerEu(kGain), AECM_MAX_WAVES_PER_EU)))
void aecm_process_pipelined_kernel(StatePtrs st, IoView io, int streams_base, int streams_rem, int n_blocks, uint32_t *progress, int n_workgroups,
                                    int wgs_per_round, int rot, int prio) {
    constexpr bool kRagged = false, kClean = false;
#include "aecm_pipelined_body.inc"
}
template <int kTail, bool kBalance, bool kRaw = false, int kFront = 2, int kDelay = 0, int kGain = 0>
__global__ __launch_bounds__(64 * PipeWaves(kTail, kFront, kDelay, kGain))
__attribute__((amdgpu_waves_per_eu(PipeWavesPerEu(kGain), AECM_MAX_WAVES_PER_EU)))
void aecm_process_pipelined_ragged_kernel(StatePtrs st, IoView io, int streams_base, int streams_rem, int n_blocks, uint32_t *progress, int n_workgroups,
                                           int wgs_per_round, int rot, int prio) {
    constexpr bool kRagged = true, kClean = false;
#include "aecm_pipelined_body.inc"
}
// The same body for launches with a clean near-end input (io.near_clean; opt-in per batch): the front waves run the third transform
// and hand the clean spectrum over in the near-end spectrum's place (PipeCleanSlot), the roles behind them run the three-signal
// block (BlockEngine<.., true>).  A kernel of its own, as the ragged one and for the same reason.  Formed spectra only, no balance:
// the shapes 6 / 8 / 12 / 16 waves (LaunchProcessBlocksPipelined's keys 20, 220, 4220, 42240).
template <int kTail, bool kBalance, bool kRaw = false, int kFront = 2, int kDelay = 0, int kGain = 0>
__global__ __launch_bounds__(64 * PipeWaves(kTail, kFront, kDelay, kGain))
__attribute__((amdgpu_waves_per_eu(PipeWavesPerEu(kGain), AECM_MAX_WAVES_PER_EU)))
void aecm_process_pipelined_clean_kernel(StatePtrs st, IoView io, int streams_base, int streams_rem, int n_blocks, uint32_t *progress, int n_workgroups,
                                          int wgs_per_round, int rot, int prio) {
    constexpr bool kRagged = false, kClean = true;
#include "aecm_pipelined_body.inc"
}
// Ragged launches with a clean input (opt-in per batch, a switch of its own): both of the above at once -- the plan's slots and
// lengths, the three-signal block.  The shapes that are both ragged and clean shapes: keys 20, 220, 4220, 42240.
template <int kTail, bool kBalance, bool kRaw = false, int kFront = 2, int kDelay = 0, int kGain = 0>
__global__ __launch_bounds__(64 * PipeWaves(kTail, kFront, kDelay, kGain))
__attribute__((amdgpu_waves_per_eu(PipeWavesPerEu(kGain), AECM_MAX_WAVES_PER_EU)))
void aecm_process_pipelined_ragged_clean_kernel(StatePtrs st, IoView io, int streams_base, int streams_rem, int n_blocks, uint32_t *progress, int n_workgroups,
                                                 int wgs_per_round, int rot, int prio) {
    constexpr bool kRagged = true, kClean = true;
#include "aecm_pipelined_body.inc"
}
#undef AECM_PIPE_BARRIER

// Streams a pipelined launch keeps resident at once: workgroups per CU by wave slots (4 SIMDs x 7) and by LDS (160 KB).
template <int kTail, int kFront = 2, int kDelay = 0, int kGain = 0, bool kClean = false>
constexpr int PipeWorkgroupsPerCu() {
    constexpr int by_waves = 4 * PipeWavesPerEu(kGain) / PipeWaves(kTail, kFront, kDelay, kGain);
    constexpr size_t shared = kClean ? sizeof(PipeShared<kTail, false, kDelay, kGain, true>)
                              : kDelay ? sizeof(PipeShared<kTail, false, kDelay, kGain>) : sizeof(PipeShared<kTail, true>);
    constexpr int by_lds = (int)((160 * 1024) / (sizeof(LdsTables) + shared));
    return by_waves < by_lds ? by_waves : by_lds;
}
// The clean shapes' larger hand-over slots (30 / 34 / 38 / 49 KB of LDS per workgroup with the tables) leave every carried shape the
// workgroups per CU that PipelinedStreamLimit -- and with it the launch rule's stream limit -- assumes for the shape without a clean input.
static_assert(PipeWorkgroupsPerCu<0, 2, 0, 0, true>() == PipeWorkgroupsPerCu<0>(), "clean six-wave shape: four workgroups per CU");
static_assert(PipeWorkgroupsPerCu<2, 2, 0, 0, true>() == PipeWorkgroupsPerCu<2>(), "clean eight-wave shape: three workgroups per CU");
static_assert(PipeWorkgroupsPerCu<2, 2, 4, 0, true>() == PipeWorkgroupsPerCu<2, 2, 4>(), "clean twelve-wave shape: two workgroups per CU");
static_assert(PipeWorkgroupsPerCu<2, 4, 2, 4, true>() == PipeWorkgroupsPerCu<2, 4, 2, 4>(), "clean sixteen-wave shape: two workgroups per CU");
// Streams a pipelined launch of this shape keeps resident at once: workgroups per CU by wave slots (4 SIMDs x 7) and by LDS (160 KB).
int PipelinedStreamLimit(int compute_units, int tail_waves, int front_waves, int delay_waves, int gain_waves, int wgs_per_cu) {
    const int per_cu = wgs_per_cu > 0 ? wgs_per_cu
                       : tail_waves == 0 ? PipeWorkgroupsPerCu<0>()
                       : gain_waves != 0 ? AECM_PIPE_GAIN_WGS_PER_CU
                       : delay_waves != 0 ? (front_waves == 4 ? PipeWorkgroupsPerCu<2, 4, 4>() : PipeWorkgroupsPerCu<2, 2, 4>())
                       : front_waves == 4 ? PipeWorkgroupsPerCu<2, 4>() : PipeWorkgroupsPerCu<2>();
    return (compute_units > 0 ? compute_units : 256) * per_cu * kPipeStreams;
}

// The shape of a pipelined launch by its size (measured: profiles/r05_experiments.md section 1.4; M frames/s, 2 048 blocks):
//   up to one workgroup per CU    (1 024 streams on 256 CUs)  two tail waves                                  372 -> 421
//   up to two per CU              (2 048)                     two tail waves, FOUR front waves, raw hand-over  600 -> 740
//   up to three per CU            (3 072)                     two tail waves, raw hand-over                    735 -> 795
//   more (four per CU: 4 096)                                 balance + raw hand-over (launches of >= 128 blocks)  816 -> 863
// tail_waves / front_waves / raw < 0: by this table; otherwise the caller's wish where the shape exists and fits (experiments).
PipeShape PipelinedShapeFor(int n_streams, int n_blocks, int compute_units, const PipeWishes &wishes) {
    const int tail_waves = wishes.tail_waves, front_waves = wishes.front_waves, raw = wishes.raw, delay_waves = wishes.delay_waves, gain_waves = wishes.gain_waves;
    const int spread = wishes.spread, wgs = wishes.wgs_per_cu;
    const int cus = compute_units > 0 ? compute_units : 256;
    const int n_wg = (n_streams + kPipeStreams - 1) / kPipeStreams;
    PipeShape sh{0, 2, false, false, 0, 0, cus, 0, 0, n_wg};
    const int want_tail = tail_waves < 0 ? 2 : tail_waves;
    if (want_tail >= 2 && n_streams <= PipelinedStreamLimit(cus, 2, 2, 0, 0, wgs)) sh.tail_waves = 2;
    const int want_front = front_waves < 0 ? (n_wg > cus ? 4 : 2) : front_waves;
    if (want_front >= 4 && sh.tail_waves == 2 && n_streams <= PipelinedStreamLimit(cus, 2, 4, 0, 0, wgs)) sh.front_waves = 4;
    sh.balance = sh.tail_waves == 0 && AECM_PIPE_BALANCE != 0 && n_blocks >= (8 << kPipeGroupLog2) && n_wg <= 128 * kPipeMonitorLoads && n_wg > 3 * cus;
    const bool want_raw = (raw < 0 ? (AECM_PIPE_RAW_HANDOVER != 0 && (sh.balance || (sh.tail_waves == 2 && n_wg > cus))) : raw != 0);
    // the raw form exists for: the balanced shape, and the two-tail shapes
    sh.raw = want_raw && (sh.balance || sh.tail_waves == 2);
    if (sh.balance && !want_raw) sh.balance = false;          // (no balanced instantiation without the raw hand-over)
    // delay waves: the two-tail shapes with formed spectra
    const int want_delay = delay_waves < 0 ? (PipeDeepShapeByDefault(n_wg, cus) ? kPipeStreams : 0) : delay_waves;
    // (Delay waves where the CU is short of issue slots rather than of independent work -- two delay waves next to four front waves
    // at two workgroups per CU, one for the workgroup's four streams at three and four per CU -- measured slower than the shapes
    // above: 2 048 streams 712 vs 740 M frames/s, 3 072 555 vs 796, 4 096 796 vs 859.  Not instantiated.)
    if (want_delay != 0 && sh.tail_waves == 2 && (raw < 0 || raw == 0) && n_streams <= PipelinedStreamLimit(cus, 2, 2, kPipeStreams, 0, wgs)) {
        sh.front_waves = 2;
        sh.delay_waves = kPipeStreams;
        sh.raw = false;
        // gain waves: the sixteen-wave shape (four front waves, two delay waves)
        const int want_gain = gain_waves < 0 ? (PipeDeepShapeByDefault(n_wg, cus) ? kPipeStreams : 0) : gain_waves;
        if (want_gain != 0 && (front_waves < 0 || front_waves == 4) && n_streams <= PipelinedStreamLimit(cus, 2, 4, 2, kPipeStreams, wgs)) {
            sh.gain_waves = kPipeStreams;
            sh.front_waves = 4;
            sh.delay_waves = 2;
        }
    }
    // Onto the set of kernels the library carries (LaunchProcessBlocksPipelined): four front waves exist with the raw hand-over (or with
    // delay and gain waves) only -- a wish for them without it gets the raw form rather than a launch error.
    if (sh.front_waves == 4 && sh.delay_waves == 0 && !sh.raw) sh.raw = true;
    // Even load (round 6).  The shape holds per_cu workgroups on a CU; with fewer workgroups of four streams than that on some CUs
    // the launch ends when the fullest CU does (1 536 streams = 384 workgroups: half the CUs carried two, the launch ran slower than
    // 1 024 streams).  Every CU gets its full count of workgroups instead, of three or four (two, one) streams each: the
    // dispatcher deals workgroups out to the CUs in turn, the first n_streams % workgroups of them serve one stream more
    // (the kernel's first lines), so the CUs' loads differ by at most one stream.
    if (spread != 0) {
        const int per_cu = PipelinedStreamLimit(cus, sh.tail_waves, sh.front_waves, sh.delay_waves, sh.gain_waves, wgs) / (cus * kPipeStreams);
        int full = per_cu * cus < n_streams ? per_cu * cus : n_streams;
        if (sh.balance && full > 128 * kPipeMonitorLoads) full = 128 * kPipeMonitorLoads;      // (what the monitor wave reads; n_wg fits: see balance above)
        if (full > sh.workgroups) sh.workgroups = full;
    }
    // The slot rotations (the kernel's slot_of; measured over all sixteen front x gain and front x tail combinations, M frames/s):
    //   sixteen waves, workgroups of one stream (two of them)   front + 1, gain + 2:  256 streams 186 -> 227, 512: 365 -> 441, 768: 507 -> 550
    //   sixteen waves, workgroups of two to four streams        front + 3, gain + 1:  1 024: 626 -> 673, 1 280: 537 -> 650, 1 536: 574 -> 688, 1 792: 641 -> 702
    //   eight waves (front and tail waves of two slots each)    front + 3, tail + 2:  2 304: 634 -> 679, 2 560: 706 -> 709, 2 816: 734 -> 753
    //   ten and six waves                                       none (nothing moved by more than the run-to-run spread)
    if (sh.gain_waves != 0) sh.rot = n_streams < 2 * sh.workgroups ? (1 | (2 << 2)) : (3 | (1 << 2));
    else if (sh.tail_waves == 2 && sh.front_waves == 2 && sh.delay_waves == 0) sh.rot = 3 | (2 << 8);
    else sh.rot = 0;
    if (wishes.rot >= 0) sh.rot = wishes.rot;
    // The roles' issue priorities (the channel / middle / back waves': by phase of the block, 1..3): front | tail << 2 | delay << 4 | gain << 6.
    // Swept like the rotations (profiles/r06_experiments.md section 1.5; M frames/s):
    //   sixteen waves, two to four streams per workgroup: the delay waves at 0 instead of 1    1 280 streams 648 -> 682, 1 536: 682 -> 684, 1 792: 700 -> 708, 2 048: 727 -> 721
    //     (workgroups of one stream keep 1: 512 streams 443 vs 432)
    //   eight waves, workgroups not all full: the tail waves at 0 instead of 1                 2 304 streams 676 -> 685, 2 560: 705 -> 732, 2 816: 751 -> 783 (3 072, all full: 787 at 1, 760 at 0)
    int tail_prio = AECM_PIPE_TAIL_PRIO, delay_prio = AECM_PIPE_DELAY_PRIO;
    if (sh.gain_waves != 0 && n_streams >= 2 * sh.workgroups) delay_prio = 0;
    if (sh.tail_waves == 2 && sh.front_waves == 2 && sh.delay_waves == 0 && n_streams < kPipeStreams * sh.workgroups) tail_prio = 0;
    sh.prio = AECM_PIPE_FRONT_PRIO | (tail_prio << 2) | (delay_prio << 4) | (AECM_PIPE_GAIN_PRIO << 6);
    if (wishes.prio >= 0) sh.prio = wishes.prio;
    return sh;
}

// The shape of a pipelined launch WITH a clean near-end input: the same rule by size on the set of shapes the clean kernel is carried
// in -- formed spectra, no balance: sixteen waves up to two workgroups of four per CU, eight waves up to three, six above (shape bits
// 0x1a02 / 0x002 / 0x000; twelve waves, 0x802, by wish) -- so a wish that names another shape lands on the nearest of these: the raw
// hand-over is dropped, four front waves without delay and gain waves become two.  Never a shape the launcher refuses.
PipeShape PipelinedCleanShapeFor(int n_streams, int n_blocks, int compute_units, const PipeWishes &wishes) {
    PipeWishes w = wishes;
    w.raw = 0;                                    // (also: no balance -- there is no balanced instantiation without the raw hand-over)
    PipeShape sh = PipelinedShapeFor(n_streams, n_blocks, compute_units, w);
    if (sh.front_waves == 4 && sh.gain_waves == 0) {
        w.front_waves = 2;
        sh = PipelinedShapeFor(n_streams, n_blocks, compute_units, w);
    }
    return sh;
}

int PipelinedWorkgroupWaves(const PipeShape &shape) { return PipeWaves(shape.tail_waves, shape.front_waves, shape.delay_waves, shape.gain_waves); }
int PipelinedWorkgroupsPerCu(const PipeShape &shape) {
    return PipelinedStreamLimit(1, shape.tail_waves, shape.front_waves, shape.delay_waves, shape.gain_waves) / kPipeStreams;
}

hipError_t LaunchProcessBlocksPipelined(const StatePtrs &st, const IoView &io, int n_streams, int n_blocks, const PipeShape &shape, uint32_t *progress,
                                        hipStream_t stream) {
    if (n_streams <= 0 || n_blocks <= 0) return hipSuccess;
    const int n_wg = shape.workgroups;
    if (n_wg <= 0 || (int64_t)n_wg * kPipeStreams < n_streams || n_wg > n_streams) return hipErrorInvalidValue;
    const dim3 grid(n_wg), block(64 * PipeWaves(shape.tail_waves, shape.front_waves, shape.delay_waves, shape.gain_waves));
    const int streams_base = n_streams / n_wg, streams_rem = n_streams % n_wg;
    if (shape.balance) {
        if (!progress || n_wg > 128 * kPipeMonitorLoads) return hipErrorInvalidValue;
        const hipError_t e = hipMemsetAsync(progress, 0, PipelinedControlBytes(n_wg), stream);
        if (e != hipSuccess) return e;
    }
#if !defined(AECM_PIPE_TRACE)
    if (!shape.balance) progress = nullptr;
#endif
#define AECM_LAUNCH_PIPE(T, B, R, F, D, G) hipLaunchKernelGGL((aecm_process_pipelined_kernel<T, B, R, F, D, G>), grid, block, sizeof(LdsTables) + sizeof(PipeShared<T, R, D, G>), \
                                                              stream, st, io, streams_base, streams_rem, n_blocks, progress, (int)grid.x, shape.wgs_per_round, shape.rot, shape.prio)
    // The instantiations the library carries (PipelinedShapeFor only ever asks for these).
    const int key = shape.gain_waves * 10000 + shape.delay_waves * 1000 + shape.tail_waves * 100 + shape.front_waves * 10 + (shape.raw ? 1 : 0);
#define AECM_LAUNCH_PIPE_CLEAN(T, F, D, G) hipLaunchKernelGGL((aecm_process_pipelined_clean_kernel<T, false, false, F, D, G>), grid, block,               \
                                                              sizeof(LdsTables) + sizeof(PipeShared<T, false, D, G, true>), stream, st, io, streams_base, \
                                                              streams_rem, n_blocks, nullptr, (int)grid.x, shape.wgs_per_round, shape.rot, shape.prio)
    if (io.near_clean != nullptr) {               // PipelinedCleanShapeFor only ever asks for these
        if (shape.balance) return hipErrorInvalidValue;
        if (key == 20) AECM_LAUNCH_PIPE_CLEAN(0, 2, 0, 0);
        else if (key == 220) AECM_LAUNCH_PIPE_CLEAN(2, 2, 0, 0);
        else if (key == 4220) AECM_LAUNCH_PIPE_CLEAN(2, 2, 4, 0);
        else if (key == 42240) AECM_LAUNCH_PIPE_CLEAN(2, 4, 2, 4);
        else return hipErrorInvalidValue;
    } else if (shape.balance) { if (key != 21) return hipErrorInvalidValue; AECM_LAUNCH_PIPE(0, true, true, 2, 0, 0); }
    else if (key == 20) AECM_LAUNCH_PIPE(0, false, false, 2, 0, 0);
    else if (key == 220) AECM_LAUNCH_PIPE(2, false, false, 2, 0, 0);
    else if (key == 221) AECM_LAUNCH_PIPE(2, false, true, 2, 0, 0);
    else if (key == 241) AECM_LAUNCH_PIPE(2, false, true, 4, 0, 0);
    else if (key == 4220) AECM_LAUNCH_PIPE(2, false, false, 2, 4, 0);
    else if (key == 42240) AECM_LAUNCH_PIPE(2, false, false, 4, 2, 4);
    else return hipErrorInvalidValue;
#undef AECM_LAUNCH_PIPE
#undef AECM_LAUNCH_PIPE_CLEAN
    return hipGetLastError();
}

// The ragged pipelined launch: plan_dev = RaggedPipePlanWords(n_workgroups, n_streams) words the caller has uploaded on `stream` --
// slot_stream[n_workgroups][4] (-1 = empty slot), then len[n_streams].  The unbalanced shapes only; a shape that asks for the
// balance is an error here (BuildRaggedPipePlan never makes one).  With a clean input (io.near_clean): the clean shapes only
// (PipelinedCleanShapeFor's), in aecm_process_pipelined_ragged_clean_kernel.
size_t RaggedPipePlanWords(int n_workgroups, int n_streams) { return (size_t)n_workgroups * kPipeStreams + (size_t)n_streams; }
hipError_t LaunchProcessBlocksPipelinedRagged(const StatePtrs &st, const IoView &io, int n_streams, const PipeShape &shape, int n_workgroups,
                                              const uint32_t *plan_dev, hipStream_t stream) {
    if (n_streams <= 0 || n_workgroups <= 0) return hipSuccess;
    if (!plan_dev || shape.balance || n_workgroups > shape.workgroups) return hipErrorInvalidValue;
    const dim3 grid(n_workgroups), block(64 * PipeWaves(shape.tail_waves, shape.front_waves, shape.delay_waves, shape.gain_waves));
    uint32_t *plan = const_cast<uint32_t *>(plan_dev);         // (the body's `progress` argument; a ragged instantiation only reads it)
#define AECM_LAUNCH_PIPE(T, R, F, D, G) hipLaunchKernelGGL((aecm_process_pipelined_ragged_kernel<T, false, R, F, D, G>), grid, block, sizeof(LdsTables) + sizeof(PipeShared<T, R, D, G>), \
                                                           stream, st, io, n_streams, 0, 0, plan, (int)grid.x, shape.wgs_per_round, shape.rot, shape.prio)
    const int key = shape.gain_waves * 10000 + shape.delay_waves * 1000 + shape.tail_waves * 100 + shape.front_waves * 10 + (shape.raw ? 1 : 0);
#define AECM_LAUNCH_PIPE_CLEAN(T, F, D, G) hipLaunchKernelGGL((aecm_process_pipelined_ragged_clean_kernel<T, false, false, F, D, G>), grid, block,       \
                                                              sizeof(LdsTables) + sizeof(PipeShared<T, false, D, G, true>), stream, st, io, n_streams, 0, \
                                                              0, plan, (int)grid.x, shape.wgs_per_round, shape.rot, shape.prio)
    if (io.near_clean != nullptr) {
        if (key == 20) AECM_LAUNCH_PIPE_CLEAN(0, 2, 0, 0);
        else if (key == 220) AECM_LAUNCH_PIPE_CLEAN(2, 2, 0, 0);
        else if (key == 4220) AECM_LAUNCH_PIPE_CLEAN(2, 2, 4, 0);
        else if (key == 42240) AECM_LAUNCH_PIPE_CLEAN(2, 4, 2, 4);
        else return hipErrorInvalidValue;
    } else if (key == 20) AECM_LAUNCH_PIPE(0, false, 2, 0, 0);
    else if (key == 220) AECM_LAUNCH_PIPE(2, false, 2, 0, 0);
    else if (key == 221) AECM_LAUNCH_PIPE(2, true, 2, 0, 0);
    else if (key == 241) AECM_LAUNCH_PIPE(2, true, 4, 0, 0);
    else if (key == 4220) AECM_LAUNCH_PIPE(2, false, 2, 4, 0);
    else if (key == 42240) AECM_LAUNCH_PIPE(2, false, 4, 2, 4);
    else return hipErrorInvalidValue;
#undef AECM_LAUNCH_PIPE
#undef AECM_LAUNCH_PIPE_CLEAN
    return hipGetLastError();
}

// The progress words of a pipelined launch: 16 bits per workgroup (cleared by the launch).
size_t PipelinedControlBytes(int n_workgroups) {
    const size_t n_wg = (size_t)n_workgroups;
#if defined(AECM_PIPE_TRACE)
    return 4 * ((n_wg + 3) / 4) * sizeof(uint32_t) + n_wg * kPipeTraceWaves * 4 * sizeof(uint64_t);      // progress halves (padded), then the trace records
#else
    return (n_wg + 2) / 2 * sizeof(uint32_t);
#endif
}
size_t PipelinedTraceOffsetBytes(int n_workgroups) {
    const size_t n_wg = (size_t)n_workgroups;
    return 4 * ((n_wg + 3) / 4) * sizeof(uint32_t);
}

size_t QueueControlBytes(int n_streams) { return ((size_t)kQueueCtlWords + (size_t)n_streams) * sizeof(uint32_t); }

// Whether a launch of this shape takes the chunk-queue kernel (chunk_blocks > 0: the engine's setting).
bool QueueLaunchApplies(int n_streams, int n_blocks, int variant, int chunk_blocks, int min_streams) {
    if (chunk_blocks <= 0 || variant != kVariantFast) return false;
    if (n_streams <= min_streams || n_blocks < 2 * chunk_blocks) return false;
    const int64_t items = (int64_t)n_streams * ((n_blocks + chunk_blocks - 1) / chunk_blocks);
    return items < (int64_t(1) << 31);
}

// The grid of a queue launch: what the chip keeps resident (the launch policy's resident_waves), no more than the streams need,
// never less than one workgroup (any grid drains the queue; a policy of fewer waves than a workgroup has gets one workgroup).
int QueueGridWorkgroups(int n_streams, int resident_waves) {
    const int resident_groups = resident_waves / kWavesPerWorkgroup;
    const int needed = (n_streams + kWavesPerWorkgroup - 1) / kWavesPerWorkgroup;
    const int groups = needed < resident_groups ? needed : resident_groups;
    return groups > 0 ? groups : 1;
}

hipError_t LaunchProcessBlocksQueued(const StatePtrs &st, const IoView &io, int n_streams, int n_blocks, int chunk_blocks,
                                     int resident_waves, uint32_t *ctl, uint32_t *err, hipStream_t stream) {
    hipError_t e = hipMemsetAsync(ctl, 0, QueueControlBytes(n_streams), stream);
    if (e != hipSuccess) return e;
    const int n_chunks = (n_blocks + chunk_blocks - 1) / chunk_blocks;
    const dim3 grid(QueueGridWorkgroups(n_streams, resident_waves));
    const dim3 block(64 * kWavesPerWorkgroup);
    const size_t lds = sizeof(LdsTables);
    if (io.near_clean != nullptr)
        hipLaunchKernelGGL((aecm_process_queue_kernel<true>), grid, block, lds, stream, st, io, n_streams, n_blocks, chunk_blocks, n_chunks, ctl, err);
    else
        hipLaunchKernelGGL((aecm_process_queue_kernel<false>), grid, block, lds, stream, st, io, n_streams, n_blocks, chunk_blocks, n_chunks, ctl, err);
    return hipGetLastError();
}

// The ragged form's control buffer: the equal-length form's words, then the plan -- len[S], order[S], first_item[n_chunks + 1].
size_t RaggedPlanOffsetWords(int n_streams) { return (size_t)kQueueCtlWords + (size_t)n_streams; }
size_t RaggedQueueControlBytes(int n_streams, int n_chunks) {
    return QueueControlBytes(n_streams) + (2 * (size_t)n_streams + (size_t)n_chunks + 1) * sizeof(uint32_t);
}

// ctl: RaggedQueueControlBytes of device memory whose plan part the caller has uploaded on `stream` (or will, ahead of this
// launch); live_streams = streams of non-zero length (the grid never needs more waves than that).
hipError_t LaunchProcessBlocksRaggedQueued(const StatePtrs &st, const IoView &io, int n_streams, int live_streams, uint32_t n_items, int chunk_blocks,
                                           int resident_waves, uint32_t *ctl, uint32_t *err, hipStream_t stream) {
    if (n_streams <= 0 || live_streams <= 0 || n_items == 0 || chunk_blocks <= 0) return hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(ctl, 0, QueueControlBytes(n_streams), stream);
    if (e != hipSuccess) return e;
    const dim3 grid(QueueGridWorkgroups(live_streams, resident_waves));
    const dim3 block(64 * kWavesPerWorkgroup);
    const size_t lds = sizeof(LdsTables);
    if (io.near_clean != nullptr)
        hipLaunchKernelGGL((aecm_process_ragged_queue_kernel<true>), grid, block, lds, stream, st, io, n_streams, n_items, chunk_blocks, ctl, err);
    else
        hipLaunchKernelGGL((aecm_process_ragged_queue_kernel<false>), grid, block, lds, stream, st, io, n_streams, n_items, chunk_blocks, ctl, err);
    return hipGetLastError();
}

int ResidentWaves(int compute_units) { return (compute_units > 0 ? compute_units : 256) * 4 * AECM_WAVES_PER_EU; }

int RotationStreamLimit(int compute_units) {
    return (compute_units > 0 ? compute_units : 256) * 4 * AECM_ROTATION_WAVES_PER_EU;
}

hipError_t LaunchProcessBlocks(const StatePtrs &st, const IoView &io, int n_streams, int n_blocks, int variant,
                               bool phase_priority, hipStream_t stream, const int32_t *blocks_per_stream) {
    if (n_streams <= 0 || n_blocks <= 0) return hipSuccess;
    const dim3 grid((n_streams + kWavesPerWorkgroup - 1) / kWavesPerWorkgroup);
    const dim3 block(64 * kWavesPerWorkgroup);
    const size_t lds = sizeof(LdsTables);
    const bool clean = io.near_clean != nullptr;
    // Issue priority by phase of the block when the launch is more waves than the chip holds at once (they then run in
    // rounds and spread over the phases by themselves), the per-block rotation when every wave of the launch is resident
    // from the start and they would otherwise march in lock step (wave_gfx950.h: kPhasePrio).  Which of the two is the launch
    // plan's decision (aecm_engine.cpp: PlanLaunch, by RotationStreamLimit of the engine's device).
    const bool phase = phase_priority;
#define AECM_LAUNCH(F, C, P) hipLaunchKernelGGL((aecm_process_kernel<F, C, P>), grid, block, lds, stream, st, io, n_streams, n_blocks, blocks_per_stream)
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

}  // namespace aecm
