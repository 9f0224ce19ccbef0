// What the loop-form tick kernels share (aecm_tick_calls_kernels.hip: the K-call tick; aecm_tick_packets_kernels.hip: the packet tick):
// where the blocks of one call fetch and deliver, and how the kernels are built.  Included by those two units only, behind
// aecm_kernel_common.h and inside namespace aecm.  The kernels' common text is aecm_tick_calls_body.inc.
#ifndef AECM_AMD_TICK_CALLS_IO_H_
#define AECM_AMD_TICK_CALLS_IO_H_

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

#endif  // AECM_AMD_TICK_CALLS_IO_H_
