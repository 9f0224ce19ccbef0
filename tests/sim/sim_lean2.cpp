// TEST INFRASTRUCTURE -- the decision counters of the lean block loop (aecm_wave.h: AECM_LEAN_COUNT) for the simulator
// libraries tests/test_lean_block2.py builds, one per subset of the switch's bits (-DAECM_LEAN_BLOCK=<mask>
// -DAECM_LEAN_POLICY_DEFAULT=1 -DAECM_LEAN_COUNTERS).  Slots 0..3 belong to the first set of items (tests/test_lean_block.py),
// slots 4, 5 and 7 to the second: the operands at which a shortened norm takes its special case (6 is free).
#include <string.h>

extern "C" {
long long g_aecm_lean_counters[8][2];
void sim_lean_counters(long long *out, int reset) {
    memcpy(out, g_aecm_lean_counters, sizeof(g_aecm_lean_counters));
    if (reset) memset(g_aecm_lean_counters, 0, sizeof(g_aecm_lean_counters));
}
// the switch this library was built with, so that the test can tell a library built with the wrong flags
int sim_lean_mask(void) {
#ifdef AECM_LEAN_BLOCK
    return AECM_LEAN_BLOCK;
#else
    return -1;
#endif
}
}
