// The planning kernels of a split tick (aecm_tick_split_kernels.hip has the tick kernel and the whole picture; aecm_flow_clean.h the
// two lists).  A unit of its own for the reason aecm_tick_calls_plan_kernels.hip gives: these kernels run one LANE per session, every
// branch of FlowTick diverges, and the unit is built without -structurizecfg-skip-uniform-regions.
#include <initializer_list>

#include <hip/hip_runtime.h>

#include "aecm_flow_clean.h"
#include "aecm_kernels.h"

namespace aecm {

// One lane per session.  The text of aecm_flow_plan_sparse_kernel (kMixed: of aecm_flow_plan_mixed_kernel -- the lane takes its
// session's rate from the core state and plans with FlowTickMixed), with two live lists in place of one: a calling lane's id goes to
// the list of its kind (kFlowNoClean in its flag byte: the sessions whose Process gets no clean pointer), each list ascending, the
// second starting at split.plain_start.  A session without a clean input keeps a clean ring row all the same; nothing reads it, so
// the resync may move it along with the near ring like everybody's.
static_assert(kFlowPlanBlock == 256, "the planning kernels run 256 lanes per workgroup");
template <bool kMixed>
__global__ __launch_bounds__(256)
void aecm_flow_plan_split_kernel(TickFlowIo fio, TickSparseIo sp, TickSplitIo split, const int32_t *__restrict__ scal, int n, unsigned near_pos, int n_streams) {
    __shared__ uint32_t wave_counts[2][kFlowPlanBlock / 64];
    const int s = blockIdx.x * 256 + threadIdx.x;
    const bool in_range = s < n_streams;
    const int flags = !in_range ? kFlowIdle : (int)fio.flags_per_session[s];
    const bool live = (flags & kFlowIdle) == 0, no_clean = (flags & kFlowNoClean) != 0;
    {
        const uint64_t ballot_clean = __ballot(live && !no_clean), ballot_plain = __ballot(live && no_clean);
        const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
        if (lane == 0) {
            wave_counts[0][wave] = (uint32_t)__builtin_popcountll(ballot_clean);
            wave_counts[1][wave] = (uint32_t)__builtin_popcountll(ballot_plain);
        }
        __syncthreads();
        const uint32_t slot = FlowSplitSlot(no_clean, sp.block_base[blockIdx.x], split.plain_base[blockIdx.x], split.plain_start, wave_counts, wave,
                                            ballot_clean, ballot_plain, lane);
        // (the list holds FlowSplitListEntries(n_streams); either list ends where the host counted it to end)
        const uint32_t end = no_clean ? split.plain_start + (uint32_t)split.plain_count : (uint32_t)split.clean_count;
        if (live && slot < end && slot < FlowSplitListEntries((uint32_t)n_streams)) sp.live[slot] = (uint32_t)s;
    }
    if (!in_range) return;
    int32_t *lag = fio.state + (size_t)F_NEAR_LAG * n_streams + s;
    if (!live) {
        *lag = FlowIdleTick(FlowIdleTick(*lag, sp.deferred_lag), n);
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
    FlowPlan p;
    if (kMixed) FlowTickMixed(r, scal[(size_t)s * kNumScal + S_MULT] == 2 ? 16000 : 8000, n, ms, flags, near_pos, p);
    else FlowTick(r, fio.fs, n, ms, flags, near_pos, p);
    for (int k = 0; k < kFlowFieldsUsed; ++k) fio.state[(size_t)k * n_streams + s] = r.v[k];
    int32_t w[kFlowPlanWords];
    FlowPackPlan(p, w);
    int4 *dst = reinterpret_cast<int4 *>(fio.plans + (size_t)s * kFlowPlanWords);
    for (int q = 0; q < kFlowPlanWords / 4; ++q) dst[q] = make_int4(w[4 * q], w[4 * q + 1], w[4 * q + 2], w[4 * q + 3]);
}

hipError_t LaunchPlanSplit(const StatePtrs &st, const TickIo &io, const TickFlowIo &fio, const TickSparseIo &sp, const TickSplitIo &split, int n_streams,
                           bool mixed_plan, hipStream_t stream) {
    if (n_streams <= 0) return hipSuccess;
    if (!sp.live || !sp.block_base || !split.plain_base || !fio.flags_per_session || split.clean_count < 0 || split.plain_count < 0 ||
        split.clean_count + split.plain_count > n_streams || split.plain_start != FlowPlainListStart((uint32_t)split.clean_count))
        return hipErrorInvalidValue;
    const dim3 grid((n_streams + 255) / 256), block(256);
    if (mixed_plan) hipLaunchKernelGGL((aecm_flow_plan_split_kernel<true>), grid, block, 0, stream, fio, sp, split, st.scal, io.n, (unsigned)io.near_pos, n_streams);
    else hipLaunchKernelGGL((aecm_flow_plan_split_kernel<false>), grid, block, 0, stream, fio, sp, split, st.scal, io.n, (unsigned)io.near_pos, n_streams);
    return hipGetLastError();
}

}  // namespace aecm
