// The ops probe (diagnostics; include/aecm_batch.h: WebRtcAecmBatch_DebugOps): every fixed-point primitive of aecm_ops.h, and the
// plain-integer helpers of aecm_wave.h, evaluated alone on the device over caller-given operand tuples.
//
// aecm_ops.h defines most primitives twice: a portable host branch, which the lane simulator of the test suite runs, and a device
// branch made of builtins, LLVM intrinsics reached by name, and inline assembly with operand modifiers.  The block kernels only
// ever show the two to agree on values audio produces.  This kernel runs the device branch of ONE function per launch on any
// tuples, so that a test can hold it against the host branch (tests/sim/sim_ops.cpp expands the same list, aecm_ops_table.inc)
// and against an independent definition, at the edges where an instruction and a portable definition differ by one case.
//
// Two forms:
//   0  lane form: thread i evaluates tuple i; the operands are what the thread loaded, so they sit in vector registers.
//   1  uniform form: wave w evaluates tuple w with every operand passed through v_readfirstlane, so the compiler may keep the
//      computation on the scalar unit, where the same C++ becomes other instructions (s_flbit_*, s_bfe_i32, s_lshl_b64 ...).
//      Lane 0 stores the result to out[w]; out[n + w] receives kOpsProbeNonUniform if any lane's result differs from lane 0's.
//
// A unit of its own, built with the block kernels' flags (build.py: SOURCE_FLAGS): the primitives are compiled the way they ship,
// and no other unit's instruction stream moves.
#define AECM_TABLE_ATTR __device__
#define AECM_CHECK_UNIT ops_probe      // (aecm_kernel_common.h: the unit's pair of audit counters)
#include "aecm_kernel_common.h"

#define AECM_OPS_ENGINE BlockEngine<Gfx950Wave<true>, false>
#define AECM_OPS_ENGINE_LEAN BlockEngine<Gfx950Wave<true, true, false, true, true>, false>      // aecm_process_queue_kernel's
#define AECM_OPS_VI(x) (x)
#define AECM_OPS_LANE0(x) (x)
#if defined(__HIP_DEVICE_COMPILE__)
#define AECM_OPS_UNIFORM(x) __builtin_amdgcn_readfirstlane(x)
#else
#define AECM_OPS_UNIFORM(x) (x)
#endif
#define AECM_OPS_TABLE_HELPERS
#include "aecm_ops_table.inc"
#undef AECM_OPS_TABLE_HELPERS

namespace aecm {

// This unit's share of the audit counters (see ReadCheckCounters in aecm_kernels.hip); WebRtcAecmBatch_GetCheckCounters adds it in.
AECM_DEFINE_CHECK_COUNTERS(ReadOpsProbeCheckCounters)

// ---- the table, as the host sees it --------------------------------------------------------------
namespace {
struct OpsProbeEntry {
    int id;
    const char *name;
    int arity;
};
constexpr OpsProbeEntry kOpsProbeTable[] = {
#define AECM_OP(id, name, arity, call) {id, #name, arity},
#include "aecm_ops_table.inc"
#undef AECM_OP
};
constexpr int kOpsProbeCount = (int)(sizeof(kOpsProbeTable) / sizeof(kOpsProbeTable[0]));
constexpr bool OpsProbeTableIsDense() {
    for (int i = 0; i < kOpsProbeCount; ++i)
        if (kOpsProbeTable[i].id != i || kOpsProbeTable[i].arity < 1 || kOpsProbeTable[i].arity > 3) return false;
    return true;
}
static_assert(OpsProbeTableIsDense(), "aecm_ops_table.inc: ids are dense from 0 in list order, arities 1..3");
}  // namespace

int OpsProbeCount() { return kOpsProbeCount; }
const char *OpsProbeName(int op) { return op >= 0 && op < kOpsProbeCount ? kOpsProbeTable[op].name : nullptr; }
int OpsProbeArity(int op) { return op >= 0 && op < kOpsProbeCount ? kOpsProbeTable[op].arity : 0; }

// ---- the kernel ------------------------------------------------------------------------------------
// One function of the list on one tuple.  `op` is a kernel argument, hence wave-uniform: the switch is a scalar branch.
__device__ __forceinline__ int OpsProbeEval(int op, int a, int b, int c) {
    switch (op) {
#define AECM_OP(id, name, arity, call) \
    case id:                           \
        return (call);
#include "aecm_ops_table.inc"
#undef AECM_OP
    }
    return 0;
}

__global__ __launch_bounds__(256) void aecm_ops_probe_kernel(int op, int form, const int *a, const int *b, const int *c, int *out, int n) {
    const int gid = (int)(blockIdx.x * 256u + threadIdx.x);          // the grid is sized from n <= 2^20: at most 2^26 threads
    if (form == 0) {
        if (gid >= n) return;                                        // bounds before any wave-level operation (the _uc forms' readfirstlane)
        const int x = a[gid], y = b ? b[gid] : 0, z = c ? c[gid] : 0;
        out[gid] = OpsProbeEval(op, x, y, z);
        return;
    }
    const int w = gid >> 6;                                          // the same for all 64 lanes of a wave
    if (w >= n) return;
    const int x = __builtin_amdgcn_readfirstlane(a[w]);
    const int y = __builtin_amdgcn_readfirstlane(b ? b[w] : 0);
    const int z = __builtin_amdgcn_readfirstlane(c ? c[w] : 0);
    const int r = OpsProbeEval(op, x, y, z);
    const int r0 = __builtin_amdgcn_readfirstlane(r);
    const bool differs = __ballot(r != r0) != 0;
    if ((gid & 63) == 0) {
        out[w] = r0;
        out[n + w] = differs ? kOpsProbeNonUniform : 0;
    }
}

// a, b, c: n words each (b, c may be null below the op's arity); out: n words in lane form, 2 n in uniform form.
hipError_t LaunchOpsProbe(int op, int form, const int *a_dev, const int *b_dev, const int *c_dev, int *out_dev, int n, hipStream_t stream) {
    if (op < 0 || op >= kOpsProbeCount || (form != 0 && form != 1) || n <= 0 || n > kOpsProbeMaxTuples) return hipErrorInvalidValue;
    const unsigned threads = form == 0 ? (unsigned)n : (unsigned)n * 64u;
    hipLaunchKernelGGL(aecm_ops_probe_kernel, dim3((threads + 255u) / 256u), dim3(256), 0, stream, op, form, a_dev, b_dev, c_dev, out_dev, n);
    return hipGetLastError();
}

}  // namespace aecm
