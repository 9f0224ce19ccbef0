// What the translation units that hold block kernels share (aecm_block_kernels.hip, aecm_trace_kernels.hip): the occupancy the
// one-wave-per-stream and queue kernels are built for, and the three steps of the chunk queue's claim / wait / publish protocol
// (described where the queue kernel is: aecm_block_kernels.hip).  Device code only; every function is inlined into its kernel.
#ifndef AECM_AMD_BLOCK_QUEUE_H_
#define AECM_AMD_BLOCK_QUEUE_H_

#include "aecm_kernel_common.h"

namespace aecm {

// Occupancy target: the kernel is bound by instruction issue with every wave strictly in order, so
// resident waves are what hides one wave's latencies from the VALU port.  7 waves/SIMD = 72 VGPRs; the
// fast variants need 64 / 68 (no spills).  Measured in round 1: 5 -> 6 -> 7 waves = 609 -> 657 -> 674 M frames/s.
// The hardware's ceiling is 7 as well: a CU's LDS holds seven copies of the 21 KB tables (one per 4-wave workgroup).
#ifndef AECM_WAVES_PER_EU
#if defined(AECM_CHECKED)
#define AECM_WAVES_PER_EU 4       // the audit build's checks need registers; its speed does not matter
#else
#define AECM_WAVES_PER_EU 7
#endif
#endif
#ifndef AECM_MAX_WAVES_PER_EU
#define AECM_MAX_WAVES_PER_EU 8
#endif
// The rotation variants only ever run launches of at most kRotationWavesPerEu waves per SIMD (LaunchProcessBlocks): they
// are built for that occupancy and get the larger register budget (80 VGPRs) that goes with it.
#ifndef AECM_ROTATION_WAVES_PER_EU
#if defined(AECM_CHECKED)
#define AECM_ROTATION_WAVES_PER_EU 4
#else
#define AECM_ROTATION_WAVES_PER_EU 6
#endif
#endif

#ifndef AECM_QUEUE_FENCES
#define AECM_QUEUE_FENCES 0
#endif
constexpr int kQueueAcquire = AECM_QUEUE_FENCES ? __ATOMIC_ACQUIRE : __ATOMIC_RELAXED;
constexpr int kQueueRelease = AECM_QUEUE_FENCES ? __ATOMIC_RELEASE : __ATOMIC_RELAXED;
constexpr int kQueueCtlWords = 16;          // [0] next item, then done[stream] = chunks of this launch completed
// A wait is for a wave that is running a chunk, so its bound grows with the chunk: 2^20 polls (x (s_sleep 16 = 1 024 cycles +
// one load): a second or two) or 64 polls per block of the chunk, whichever is more (a block takes a wave ~7 us on a full chip:
// ~3 polls) -- a healthy predecessor on a shared or debugged GPU is not mistaken for a hung one.
__device__ __forceinline__ uint32_t QueueMaxPolls(int chunk_blocks) {
    const uint32_t by_chunk = (uint32_t)chunk_blocks << 6;         // chunk_blocks <= 2^20 (BatchEngine::kMaxQueueChunk)
    return by_chunk > (1u << 20) ? by_chunk : (1u << 20);
}

// The three pieces the queue kernels are made of.  Every lane takes part in the queue's few memory operations with the same
// address and, for the counter, an addend that is 1 in lane 0 only: no lane-divergent control flow anywhere in the item loop.
__device__ __forceinline__ uint32_t QueueClaim(uint32_t *ctl) {
    const uint32_t one_in_lane0 = (threadIdx.x & 63u) == 0 ? 1u : 0u;
    return (uint32_t)__builtin_amdgcn_readfirstlane((int)__hip_atomic_fetch_add(ctl, one_in_lane0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
}
// Until the stream's chunks before `chunk` are done.  false: gave up -- *err is raised and every wave leaves at its next claim.
__device__ __forceinline__ bool QueueWait(const uint32_t *done, uint32_t stream, uint32_t chunk, int chunk_blocks, uint32_t *err) {
    if (chunk != 0) {
        uint32_t polls = 0;
        while ((uint32_t)__builtin_amdgcn_readfirstlane((int)__hip_atomic_load(done + stream, kQueueAcquire, __HIP_MEMORY_SCOPE_AGENT)) < chunk) {
            __builtin_amdgcn_s_sleep(16);
            if (++polls > QueueMaxPolls(chunk_blocks) ||
                ((polls & 1023u) == 0 && __builtin_amdgcn_readfirstlane((int)__hip_atomic_load(err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) != 0)) {
                __hip_atomic_store(err, 1u + stream, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                return false;
            }
        }
    }
    asm volatile("" ::: "memory");                       // the state loads stay behind the flag
    return true;
}
__device__ __forceinline__ void QueuePublish(uint32_t *done, uint32_t stream, uint32_t chunk) {
    // every store of the chunk (state, history rows: sc1, written through; output rows) has completed before the flag is raised
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    __hip_atomic_store(done + stream, chunk + 1u, kQueueRelease, __HIP_MEMORY_SCOPE_AGENT);
}

}  // namespace aecm
#endif  // AECM_AMD_BLOCK_QUEUE_H_
