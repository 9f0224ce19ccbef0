// What the wave-per-session tick units share -- aecm_kernels.hip (the dense and the sparse tick), aecm_tick_calls_kernels.hip (the
// K-call tick), aecm_tick_packets_kernels.hip (the packet tick), aecm_tick_split_kernels.hip (the split tick),
// aecm_tick_trace_kernels.hip (the traced twins of the dense, sparse and split ticks), aecm_call_trace_kernels.hip (the traced
// twins of the K-call and the packet tick): where the blocks of a
// tick or of one call fetch and deliver, how the kernels are built, and how a wavefront finds its session in a live list.  Included
// behind aecm_kernel_common.h, inside namespace aecm.  The kernels' common texts are aecm_tick_flow_body.inc and
// aecm_tick_calls_body.inc.
#ifndef AECM_AMD_TICK_UNIT_H_
#define AECM_AMD_TICK_UNIT_H_

// Where the blocks of one tick (aecm_tick_flow_body.inc) or of ONE call of a tick (aecm_tick_calls_body.inc) fetch and deliver.
template <bool kHasClean, class Append>
struct TickBlockIo {
    using E = BlockEngine<Gfx950Wave<true, true, true>, kHasClean>;
    using Regs = typename E::Regs;
    const int16_t *far_src;          // the far ring itself (direct ticks / calls) or the framed far stream
    const int16_t *nr, *cr;          // near / clean rings of this session
    int16_t *out_row;                // output stream ring
    int far_mask, mask;
    unsigned far_pos, near_pos, out_pos;      // positions of the first block in far_src / the near rings / the output ring
    const Append &append;            // the tick's (the call's) samples -> rings
    __device__ __forceinline__ int far(const Regs &r, int b) const { return far_src[(far_pos + b * kBlock + r.lane) & far_mask]; }
    __device__ __forceinline__ int near(const Regs &r, int b) const { return nr[(near_pos + b * kBlock + r.lane) & mask]; }
    __device__ __forceinline__ int clean(const Regs &r, int b) const { return cr[(near_pos + b * kBlock + r.lane) & mask]; }
    __device__ __forceinline__ void out(const Regs &r, int b, int v) const { out_row[(out_pos + b * kBlock + r.brev) & mask] = (int16_t)v; }
    // Called by the engine after it has issued its state loads: the samples go into the rings HERE (8-byte stores that, placed
    // ahead of those loads, would make the compiler fetch the scalar half of the state with vector loads: for all it knows they
    // could alias it), then this wave's fetches below must see this wave's stores -- those of this call and, in a tick of
    // several calls, those of the calls before it (far samples appended in call c are read from the ring by call c + 1).
    __device__ __forceinline__ void ready() const {
        append();
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    }
};

// Sessions per workgroup of the tick kernels.  A workgroup's waves are placed together, n / 4 per SIMD: with the 7 waves
// per SIMD the kernels are built for (below), 8-wave workgroups can only ever fill 6 of the 7 slots, 4-wave workgroups all
// of them -- at the price of one 20 KB table fill (from L2) per 4 sessions instead of per 8.  Measured, 65 536 sessions,
// ms per tick: 8 sessions 0.2356, 4 sessions 0.2251, 2 sessions 0.3153.  (Round 2, at 8 waves per SIMD, 8 per
// workgroup was the better size: profiles/r02_experiments.md.)
#ifndef AECM_TICK_FLOW_WAVES
#define AECM_TICK_FLOW_WAVES 4
#endif
#ifndef AECM_TICK_EARLY_STATE_LOAD
#define AECM_TICK_EARLY_STATE_LOAD 1      // 65 536 sessions: 0.2218 -> 0.2194 ms per tick.  (Timing probes without the two fences of the
                                          // tick -- samples into the rings before the blocks fetch them, block outputs before the
                                          // output frames read them -- moved nothing: 0.2199 / 0.2193 / 0.2199 / 0.2190 ms.)
#endif
#ifndef AECM_TICK_SPLIT_PLAN_WORDS
#define AECM_TICK_SPLIT_PLAN_WORDS 1
#endif
#ifndef AECM_TICK_FLOW_WAVES_PER_EU
#if defined(AECM_CHECKED)
#define AECM_TICK_FLOW_WAVES_PER_EU 4
#else
// 7, not 8: the scalar budget of 8 waves per SIMD (78) costs the body hundreds of scalar spills; at 94 it has 52.  With the
// uniform regions left unstructurized (build.py): 8 waves 0.272 ms per tick of 65 536 sessions, 7 waves 0.234, 6 waves 0.237
// (default pipeline: 0.241 at 8 waves, its best).
#define AECM_TICK_FLOW_WAVES_PER_EU 7
#endif
#endif
constexpr int kTickFlowWaves = AECM_TICK_FLOW_WAVES;

// The loop-form tick kernels (aecm_tick_calls_body.inc) are built like the others: four sessions per workgroup, 7 waves per SIMD,
// 4 in the audit build.  A name of their own, so that an A/B build can move the one without the other.
#ifndef AECM_TICK_CALLS_WAVES_PER_EU
#if defined(AECM_CHECKED)
#define AECM_TICK_CALLS_WAVES_PER_EU 4
#else
#define AECM_TICK_CALLS_WAVES_PER_EU 7
#endif
#endif
constexpr int kTickCallsWaves = 4;

// The session of entry wave_id of a live list of `count` ids (ascending; the planning kernels write it), declared as `s`: the id
// is wave-uniform and in a scalar register -- readfirstlane -- before anything is addressed by it, so every row offset of the
// body stays scalar and the scalar half of the state is still fetched by scalar loads.  An entry past the list's end, or an id
// that is no session's, gives s = n_streams (in scope, like the list): the wavefront serves nobody but still takes part in the
// table fill's barrier, and leaves behind it.
#define AECM_TICK_LIVE_SESSION(list, count, wave_id)                                                                          \
    const uint32_t id = (uint32_t)__builtin_amdgcn_readfirstlane((int)(list)[(wave_id) < (count) ? (wave_id) : 0]);           \
    const int64_t s = (wave_id) < (count) && id < (uint32_t)n_streams ? (int64_t)id : (int64_t)n_streams;

#endif  // AECM_AMD_TICK_UNIT_H_
