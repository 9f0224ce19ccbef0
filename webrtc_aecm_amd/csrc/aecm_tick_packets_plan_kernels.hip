// The planning kernel of the packet tick (aecm_tick_packets_kernels.hip has the tick kernel and the whole picture).  A unit of its
// own for the reason aecm_tick_calls_plan_kernels.hip gives: one LANE per session, every branch of FlowTick diverges, so it is built
// WITHOUT -structurizecfg-skip-uniform-regions -- and apart from that unit, so that aecm_flow_plan_calls_kernel stays, instruction
// for instruction, what it was (tests/golden/tick_calls_fingerprints.json).
#include <initializer_list>

#include <hip/hip_runtime.h>

#include "aecm_kernels.h"

namespace aecm {

// One lane per session.  The text of aecm_flow_plan_calls_kernel with two differences: the lane's rate is its session's (the core
// state's S_MULT, what the block engine itself goes by -- as aecm_flow_plan_mixed_kernel), and the planning is FlowTickPackets: the
// lane's call size is 80 where its flag byte carries kFlowHalfCall in a 160-sample tick, and what it did not consume of the tick
// becomes its lag.  An idle lane adds the WHOLE tick (calls * n samples) to its session's lag; a live lane brings its session back
// in step once, before its first call.
static_assert(kFlowPlanBlock == 256, "the planning kernels run 256 lanes per workgroup");
__global__ __launch_bounds__(256)
void aecm_flow_plan_packets_kernel(TickFlowIo fio, TickSparseIo sp, const int32_t *__restrict__ scal, int n, int calls, unsigned near_pos, int n_streams) {
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
    const int fs = scal[(size_t)s * kNumScal + S_MULT] == 2 ? 16000 : 8000;
    int4 *dst = reinterpret_cast<int4 *>(fio.plans + (size_t)s * calls * kFlowPlanWords);      // [S][calls][kFlowPlanWords]
    FlowTickPackets(r, fs, n, calls, ms, flags, near_pos, [&](int c, const FlowPlan &p) {
        int32_t w[kFlowPlanWords];
        FlowPackPlan(p, w);
        for (int q = 0; q < kFlowPlanWords / 4; ++q) dst[c * (kFlowPlanWords / 4) + q] = make_int4(w[4 * q], w[4 * q + 1], w[4 * q + 2], w[4 * q + 3]);
    });
    for (int k = 0; k < kFlowFieldsUsed; ++k) fio.state[(size_t)k * n_streams + s] = r.v[k];
}

hipError_t LaunchPlanPackets(const StatePtrs &st, const TickIo &io, const TickFlowIo &fio, const TickSparseIo &sp, int n_streams, int calls,
                             hipStream_t stream) {
    if (n_streams <= 0) return hipSuccess;
    if (!sp.live || !sp.block_base || !st.scal || calls < 1 || calls > kFlowMaxTickCalls) return hipErrorInvalidValue;
    hipLaunchKernelGGL(aecm_flow_plan_packets_kernel, dim3((n_streams + 255) / 256), dim3(256), 0, stream, fio, sp, st.scal, io.n, calls,
                       (unsigned)io.near_pos, n_streams);
    return hipGetLastError();
}

}  // namespace aecm
