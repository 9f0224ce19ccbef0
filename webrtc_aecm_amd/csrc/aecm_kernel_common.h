// Device-side pieces shared by the translation units that hold wave-level kernels: the block kernels and their traced twins
// (aecm_block_kernels.hip, aecm_trace_kernels.hip; through aecm_block_queue.h as well), the ops probe (aecm_ops_probe_kernels.hip),
// aecm_kernels.hip and the tick units (aecm_tick_calls_kernels.hip, aecm_tick_packets_kernels.hip, aecm_tick_split_kernels.hip).
#ifndef AECM_AMD_KERNEL_COMMON_H_
#define AECM_AMD_KERNEL_COMMON_H_

// The audit counters of the -DAECM_CHECKED build (aecm_ops.h counts into g_aecm_check_fail).  Device symbols are per translation
// unit (no relocatable device code), so every unit keeps a pair of its own: a unit names itself ONCE, ahead of this header,
//   #define AECM_CHECK_UNIT tick_calls
// and its pair is g_aecm_check_fail_tick_calls.  (aecm_kernels.hip names nothing: its pair is g_aecm_check_fail itself.)
#if defined(AECM_CHECKED) && defined(AECM_CHECK_UNIT)
#define AECM_CHECK_CAT_(a, b) a##b
#define AECM_CHECK_CAT(a, b) AECM_CHECK_CAT_(a, b)
#define g_aecm_check_fail AECM_CHECK_CAT(g_aecm_check_fail_, AECM_CHECK_UNIT)
#endif

#include "aecm_kernels.h"
#include "aecm_tables.h"
#include "aecm_wave.h"
#include "wave_gfx950.h"

namespace aecm {

// The LDS tables are an image inside the host-built constants blob: one coalesced copy per workgroup.
// kThreads = the workgroup size, a compile-time constant: the copy loop then needs nothing from the dispatch packet (a
// scalar load whose wait would also hold up every other scalar load in flight at kernel entry).
template <int kThreads>
__device__ __forceinline__ void FillLdsTables(const uint32_t *consts) {
    static_assert(kConstBlobWords % 4 == 0, "the constants blob is copied 16 bytes at a time");
    constexpr int kVecs = kConstBlobWords / 4, kPasses = (kVecs + kThreads - 1) / kThreads;
    const int4 *src = reinterpret_cast<const int4 *>(consts);
    int4 *dst = reinterpret_cast<int4 *>(&g_lds[0]);
    int4 tmp[kPasses];                                   // every load in flight before the first LDS store
    // Indices are clamped instead of predicated (the last vector is then copied by several threads, harmlessly): with
    // predicates the compiler sinks each load next to its store and the passes wait for each other.
#pragma unroll
    for (int k = 0; k < kPasses; ++k) {
        const int i = (int)threadIdx.x + k * kThreads;
        tmp[k] = src[i < kVecs ? i : kVecs - 1];
    }
#pragma unroll
    for (int k = 0; k < kPasses; ++k) {
        const int i = (int)threadIdx.x + k * kThreads;
        dst[i < kVecs ? i : kVecs - 1] = tmp[k];
    }
    __syncthreads();
}

// AECM_DEFINE_CHECK_COUNTERS(Reader), once per unit, inside namespace aecm: the unit's pair of audit counters and the host
// function `hipError_t Reader(uint64_t counters[2], bool reset)` (declared in aecm_kernels.h) that reads it, and zeroes it on
// request.  It does not synchronise; hipErrorNotSupported in the shipped build.
#if defined(AECM_CHECKED)
#define AECM_DEFINE_CHECK_COUNTERS(Reader)                                                           \
    __device__ unsigned long long g_aecm_check_fail[2];                                              \
    hipError_t Reader(uint64_t counters[2], bool reset) {                                            \
        unsigned long long host[2] = {0, 0};                                                         \
        hipError_t e = hipMemcpyFromSymbol(host, HIP_SYMBOL(g_aecm_check_fail), sizeof host);        \
        if (e != hipSuccess) return e;                                                               \
        counters[0] = host[0];                                                                       \
        counters[1] = host[1];                                                                       \
        if (reset) {                                                                                 \
            const unsigned long long zero[2] = {0, 0};                                               \
            e = hipMemcpyToSymbol(HIP_SYMBOL(g_aecm_check_fail), zero, sizeof zero);                 \
        }                                                                                            \
        return e;                                                                                    \
    }
#else
#define AECM_DEFINE_CHECK_COUNTERS(Reader) \
    hipError_t Reader(uint64_t *, bool) { return hipErrorNotSupported; }
#endif

}  // namespace aecm

#endif  // AECM_AMD_KERNEL_COMMON_H_
