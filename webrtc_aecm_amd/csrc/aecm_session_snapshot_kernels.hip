// gfx950 kernels of the bulk session snapshots (WebRtcAecmSessions_ExportSessions / ImportSessions): one workgroup per listed
// session gathers (scatters) its snapshot, one wavefront per snapshot says whether it may be run on.  The work itself is stated
// once, for these kernels and for the host: aecm_session_snapshot.h.  A unit of its own: the code objects of the block kernels
// and of the tick kernels do not change with it.
#include <hip/hip_runtime.h>

#include "aecm_session_snapshot.h"

namespace aecm {

constexpr int kSnapshotWorkgroup = 256;

// Workgroup b: the snapshot of session sessions[b] (first + b without a list) into blobs + b * kSessionBytes.  33 of the 34 KB
// are contiguous parts that move 16 bytes per lane (kWide: blobs is 16-byte aligned; 4 bytes per lane otherwise); the three
// tails, 384 samples, are cut out of the rings sample by sample; the 32 wrapper words are a strided read of the field-major array.
template <bool kWide>
__global__ __launch_bounds__(kSnapshotWorkgroup) void aecm_gather_sessions_kernel(SessionView view, const int32_t *sessions, int first, uint8_t *blobs) {
    const int session = sessions ? sessions[blockIdx.x] : first + (int)blockIdx.x;
    SessionGatherPart<kWide>(view, session, blobs + (size_t)blockIdx.x * kSessionBytes, (int)threadIdx.x, kSnapshotWorkgroup);
}

// The inverse: blobs + b * kSessionBytes into slot slots[b] (first + b without a list).  The slots are distinct (the host checks).
template <bool kWide>
__global__ __launch_bounds__(kSnapshotWorkgroup) void aecm_scatter_sessions_kernel(SessionView view, const int32_t *slots, int first, const uint8_t *blobs) {
    const int slot = slots ? slots[blockIdx.x] : first + (int)blockIdx.x;
    SessionScatterPart<kWide>(view, slot, blobs + (size_t)blockIdx.x * kSessionBytes, (int)threadIdx.x, kSnapshotWorkgroup);
}

// result[0] = index of the first snapshot that may not be imported (atomicMin; the caller presets 0xffffffff); info[b] = the
// rate of snapshot b | has_clean << 31, from which the host updates its mirrors.  64 threads per snapshot: thread t checks scalar
// field t and lane t of the core state, thread 0 the wrapper words too (SessionBlobDefect).
__global__ __launch_bounds__(kLanes) void aecm_validate_sessions_kernel(const uint8_t *blobs, int fs_object, int any_rate, uint32_t *result, uint32_t *info) {
    const uint8_t *blob = blobs + (size_t)blockIdx.x * kSessionBytes;
    const int t = (int)threadIdx.x;
    const int defect = SessionBlobDefect(blob, fs_object, any_rate != 0, t);
    if (__ballot(defect != 0) != 0 && t == 0) atomicMin(result, blockIdx.x);
    if (t == 0) info[blockIdx.x] = SessionBlobWord(blob, 0, 2) | (SessionBlobWord(blob, 0, 3) << 31);
}

hipError_t LaunchGatherSessions(const SessionView &view, const int32_t *sessions_dev, int first, int count, void *blobs_dev, bool wide, hipStream_t stream) {
    if (count <= 0) return hipSuccess;
    uint8_t *blobs = static_cast<uint8_t *>(blobs_dev);
    if (wide) hipLaunchKernelGGL(aecm_gather_sessions_kernel<true>, dim3(count), dim3(kSnapshotWorkgroup), 0, stream, view, sessions_dev, first, blobs);
    else hipLaunchKernelGGL(aecm_gather_sessions_kernel<false>, dim3(count), dim3(kSnapshotWorkgroup), 0, stream, view, sessions_dev, first, blobs);
    return hipGetLastError();
}

hipError_t LaunchValidateSessions(const void *blobs_dev, int count, int fs_object, bool any_rate, uint32_t *result_dev, uint32_t *info_dev, hipStream_t stream) {
    if (count <= 0) return hipSuccess;
    hipLaunchKernelGGL(aecm_validate_sessions_kernel, dim3(count), dim3(kLanes), 0, stream, static_cast<const uint8_t *>(blobs_dev), fs_object, any_rate ? 1 : 0,
                       result_dev, info_dev);
    return hipGetLastError();
}

hipError_t LaunchScatterSessions(const SessionView &view, const int32_t *slots_dev, int first, int count, const void *blobs_dev, bool wide, hipStream_t stream) {
    if (count <= 0) return hipSuccess;
    const uint8_t *blobs = static_cast<const uint8_t *>(blobs_dev);
    if (wide) hipLaunchKernelGGL(aecm_scatter_sessions_kernel<true>, dim3(count), dim3(kSnapshotWorkgroup), 0, stream, view, slots_dev, first, blobs);
    else hipLaunchKernelGGL(aecm_scatter_sessions_kernel<false>, dim3(count), dim3(kSnapshotWorkgroup), 0, stream, view, slots_dev, first, blobs);
    return hipGetLastError();
}

}  // namespace aecm
