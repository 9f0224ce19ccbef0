// TEST INFRASTRUCTURE -- tests/_build/libaecm_inject.so (tests/inject_sim.py): the block DSP of the product (aecm_wave.h on the 64-lane
// simulator) started from a state image given by the caller, with the claims of aecm_ops.h checked.
//
// A library of its own, like sim_ops.cpp: it defines the aecm_*_violation hooks itself (the product's, aecm_host_state.cpp, abort;
// tests/_build/libaecm_sim.so links those).  The hooks are [[noreturn]]: they throw, and sim_inject_run reports which kind of claim
// the state violated.  The same source is compiled into the stand-alone sanitizer program (tests/sim/inject_main.cpp).
#include <stdint.h>

#include "wave_sim.h"
#include "aecm_wave.h"
#include "aecm_state_check.h"

namespace {
struct ClaimViolated {
    int kind, value;
};
}  // namespace

namespace aecm {
[[noreturn]] void aecm_mul24_range_violation(int a, int) { throw ClaimViolated{1, a}; }
[[noreturn]] void aecm_i16_range_violation(int v) { throw ClaimViolated{2, v}; }
[[noreturn]] void aecm_shift_range_violation(int c) { throw ClaimViolated{3, c}; }
[[noreturn]] void aecm_nonneg_violation(int v) { throw ClaimViolated{4, v}; }
}  // namespace aecm

using namespace aecm;

extern "C" {

// One launch of n_blocks blocks on the image (vec kNumVec * 64, scal 64, hist kHistory * 64), updated in place; clean may be NULL.
// Returns 0, or the kind of the first claim violated (1 mul24, 2 as_i16, 3 shift count, 4 as_nonneg; *value, if given, is the
// offending operand) -- the image is then whatever the launch had stored before.
int sim_inject_run(uint32_t *vec, int32_t *scal, uint16_t *hist, const int16_t *far_s, const int16_t *near_s, const int16_t *clean, int n_blocks,
                   int16_t *out, int32_t *value) {
    StatePtrs st{vec, scal, hist, nullptr};
    IoView io{far_s, near_s, clean, out, 0, kBlock};
    try {
        if (clean) BlockEngine<SimWave, true>::run_stream(st, io, 0, n_blocks);
        else BlockEngine<SimWave, false>::run_stream(st, io, 0, n_blocks);
    } catch (const ClaimViolated &c) {
        if (value) *value = c.value;
        return c.kind;
    }
    return 0;
}

// n states back to back, each through the launches lens[0..n_lens) (sum = total blocks) of its own audio rows far / near / clean
// [n][total * 64]; has_clean[i] = 0: state i runs without the clean row.  kinds[i] = sim_inject_run's verdict of the first launch
// that violates a claim (the later ones of that state are not run).  Returns the number of states with a violation.
int sim_inject_run_many(int n, uint32_t *vec, int32_t *scal, uint16_t *hist, const int16_t *far_s, const int16_t *near_s, const int16_t *clean,
                        const uint8_t *has_clean, const int32_t *lens, int n_lens, int16_t *out, int32_t *kinds, int32_t *values) {
    int total = 0, bad = 0;
    for (int k = 0; k < n_lens; ++k) total += lens[k];
    for (int i = 0; i < n; ++i) {
        const int64_t row = (int64_t)i * total * kBlock;
        int done = 0;
        kinds[i] = 0;
        values[i] = 0;
        for (int k = 0; k < n_lens && !kinds[i]; ++k) {
            const int64_t at = row + (int64_t)done * kBlock;
            kinds[i] = sim_inject_run(vec + (int64_t)i * kVecWordsPerStream, scal + (int64_t)i * kNumScal, hist + (int64_t)i * kHistWordsPerStream, far_s + at,
                                      near_s + at, has_clean[i] ? clean + at : nullptr, lens[k], out + at, values + i);
            done += lens[k];
        }
        bad += kinds[i] != 0;
    }
    return bad;
}

// The product's verdict on an image that claims the rate fs: the name of the first defect (aecm_state_check.h), NULL = admitted.
const char *sim_inject_validate(const uint32_t *vec, const int32_t *scal, int fs) { return StateDefectName(StateImageDefect(vec, scal, fs)); }

}  // extern "C"
