// TEST INFRASTRUCTURE -- tests/_build/libaecm_ops.so (tests/ops_sim.py): the HOST branch of every entry of
// webrtc_aecm_amd/csrc/aecm_ops_table.inc, the definitions the 64-lane simulator runs, evaluated tuple by tuple.  The device side
// of the same list is aecm_ops_probe_kernels.hip (WebRtcAecmBatch_DebugOps); tests/ops_ref.py holds a third, independent definition.
//
// A library of its own: it defines the aecm_*_violation hooks itself (the product's, aecm_host_state.cpp, abort).  The hooks are
// declared [[noreturn]] in aecm_ops.h, so they cannot come back to the primitive that called them: they throw, and the evaluation
// loop records "this tuple violates a claim of the header" (flags[i] = 1, out[i] = 0) and goes on with the next tuple.
#include <stdint.h>

#include "wave_sim.h"
#include "aecm_wave.h"

namespace {
struct ClaimViolated {};
}  // namespace

namespace aecm {
[[noreturn]] void aecm_mul24_range_violation(int, int) { throw ClaimViolated(); }
[[noreturn]] void aecm_i16_range_violation(int) { throw ClaimViolated(); }
[[noreturn]] void aecm_shift_range_violation(int) { throw ClaimViolated(); }
[[noreturn]] void aecm_nonneg_violation(int) { throw ClaimViolated(); }
}  // namespace aecm

namespace aecm {
// the simulator's policy with the lean forms of the block loop on (aecm_wave.h: PolicyLean reads W::kLean)
struct SimWaveLean : SimWave {
    static constexpr bool kLean = true;
};
}  // namespace aecm

#define AECM_OPS_ENGINE BlockEngine<SimWave, false>
#define AECM_OPS_ENGINE_LEAN BlockEngine<SimWaveLean, false>
#define AECM_OPS_VI(x) VecI(x)
#define AECM_OPS_LANE0(x) ((x).v[0])
#define AECM_OPS_UNIFORM(x) (x)
#define AECM_OPS_TABLE_HELPERS
#include "aecm_ops_table.inc"
#undef AECM_OPS_TABLE_HELPERS

namespace aecm {
static_assert(BlockEngine<SimWaveLean, false>::kLeanNarrowings && !BlockEngine<SimWave, false>::kLeanNarrowings,
              "the two engines of the table are the lean and the plain block loop");

struct OpsEntry {
    int id;
    const char *name;
    int arity;
};
static const OpsEntry kOps[] = {
#define AECM_OP(id, name, arity, call) {id, #name, arity},
#include "aecm_ops_table.inc"
#undef AECM_OP
};
static const int kOpsCount = (int)(sizeof(kOps) / sizeof(kOps[0]));

static int eval(int op, int a, int b, int c) {
    switch (op) {
#define AECM_OP(id, name, arity, call) \
    case id:                           \
        return (call);
#include "aecm_ops_table.inc"
#undef AECM_OP
    }
    return 0;
}
}  // namespace aecm

extern "C" {

int sim_ops_count() { return aecm::kOpsCount; }
const char *sim_ops_name(int op) { return op >= 0 && op < aecm::kOpsCount && aecm::kOps[op].id == op ? aecm::kOps[op].name : nullptr; }
int sim_ops_arity(int op) { return op >= 0 && op < aecm::kOpsCount ? aecm::kOps[op].arity : 0; }

// out[i] = entry op on (a[i], b[i], c[i]); b, c may be null below the op's arity.  flags (may be null): 1 where the header's own
// check of a claimed range fired.  Returns the number of such tuples, -1 for an op outside the table.
int sim_ops_eval(int op, const int32_t *a, const int32_t *b, const int32_t *c, int32_t *out, int32_t *flags, int n) {
    if (op < 0 || op >= aecm::kOpsCount) return -1;
    int violated = 0;
    for (int i = 0; i < n; ++i) {
        int f = 0;
        try {
            out[i] = aecm::eval(op, a[i], b ? b[i] : 0, c ? c[i] : 0);
        } catch (const ClaimViolated &) {
            out[i] = 0;
            f = 1;
            ++violated;
        }
        if (flags) flags[i] = f;
    }
    return violated;
}

}  // extern "C"
