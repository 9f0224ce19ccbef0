// The planning kernel of the K-call tick (aecm_tick_calls_kernels.hip has the tick kernel and the whole picture).  A unit of its
// own because it is built WITHOUT the flags of the tick kernels' units: -structurizecfg-skip-uniform-regions is for kernels whose
// branches are wave-uniform, and this kernel runs one LANE per session -- every branch of FlowTick diverges.  Built with that flag,
// the loop over the calls came out wrong on the MI355X: lanes that skip a call's frames (a session in its start-up phase) were
// taken for lanes with active frames at the end of FlowTick, and their F_FF_VALID was cleared (found by the 4 100-session test:
// the snapshot of a session that had not left the start-up phase differed from its twin's in that one word).
#include <initializer_list>

#include <hip/hip_runtime.h>

#include "aecm_kernels.h"

namespace aecm {

// One lane per session.  The text of aecm_flow_plan_sparse_kernel up to the planning itself: an idle lane adds the WHOLE tick
// (calls * n samples) to its session's lag; a live lane brings its session back in step once, before its first call.
static_assert(kFlowPlanBlock == 256, "the planning kernels run 256 lanes per workgroup");
__global__ __launch_bounds__(256)
void aecm_flow_plan_calls_kernel(TickFlowIo fio, TickSparseIo sp, int n, int calls, unsigned near_pos, int n_streams) {
    __shared__ uint32_t wave_counts[kFlowPlanBlock / 64];
    const int s = blockIdx.x * 256 + threadIdx.x;
    const bool in_range = s < n_streams;
    const int flags = !in_range ? kFlowIdle : fio.flags_per_session ? (int)fio.flags_per_session[s] : fio.flags;
    const bool live = (flags & kFlowIdle) == 0;
    {
        const uint64_t ballot = __ballot(live);
        const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
        if (lane == 0) wave_counts[wave] = (uint32_t)__builtin_popcountll(ballot);
        __syncthreads();
        const uint32_t slot = FlowLiveSlot(sp.block_base[blockIdx.x], wave_counts, wave, ballot, lane);
        if (live && slot < (uint32_t)n_streams) sp.live[slot] = (uint32_t)s;      // (the list holds n_streams entries)
    }
    if (!in_range) return;
    int32_t *lag = fio.state + (size_t)F_NEAR_LAG * n_streams + s;
    if (!live) {
        *lag = FlowIdleTick(FlowIdleTick(*lag, sp.deferred_lag), calls * n);
        return;
    }
    FlowRegs r;
    for (int k = 0; k < kFlowFieldsUsed; ++k) r.v[k] = fio.state[(size_t)k * n_streams + s];
    r.v[F_NEAR_LAG] = FlowIdleTick(r.v[F_NEAR_LAG], sp.deferred_lag);
    if (r.v[F_NEAR_LAG] != 0) {
        FlowNearMove m;
        FlowResync(r, near_pos, m);
        const uint32_t mask = (uint32_t)sp.ring_len - 1u;
        FlowMoveNear(sp.near_ring + (size_t)s * sp.ring_len, mask, m);
        if (sp.clean_ring) FlowMoveNear(sp.clean_ring + (size_t)s * sp.ring_len, mask, m);
    }
    const int ms = fio.ms_per_session ? (int)fio.ms_per_session[s] : fio.ms;
    int4 *dst = reinterpret_cast<int4 *>(fio.plans + (size_t)s * calls * kFlowPlanWords);      // [S][calls][kFlowPlanWords]
    FlowTickCalls(r, fio.fs, n, calls, ms, flags, near_pos, [&](int c, const FlowPlan &p) {
        int32_t w[kFlowPlanWords];
        FlowPackPlan(p, w);
        for (int q = 0; q < kFlowPlanWords / 4; ++q) dst[c * (kFlowPlanWords / 4) + q] = make_int4(w[4 * q], w[4 * q + 1], w[4 * q + 2], w[4 * q + 3]);
    });
    for (int k = 0; k < kFlowFieldsUsed; ++k) fio.state[(size_t)k * n_streams + s] = r.v[k];
}

hipError_t LaunchPlanCalls(const TickIo &io, const TickFlowIo &fio, const TickSparseIo &sp, int n_streams, int calls, hipStream_t stream) {
    if (n_streams <= 0) return hipSuccess;
    if (!sp.live || !sp.block_base || calls < 1 || calls > kFlowMaxTickCalls) return hipErrorInvalidValue;
    hipLaunchKernelGGL(aecm_flow_plan_calls_kernel, dim3((n_streams + 255) / 256), dim3(256), 0, stream, fio, sp, io.n, calls, (unsigned)io.near_pos, n_streams);
    return hipGetLastError();
}

}  // namespace aecm
