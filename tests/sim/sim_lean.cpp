// TEST INFRASTRUCTURE -- the decision counters of the lean block loop (aecm_wave.h: AECM_LEAN_COUNT), for the simulator
// libraries tests/test_lean_block.py builds with -DAECM_LEAN_COUNTERS.
#include <string.h>

extern "C" {
long long g_aecm_lean_counters[8][2];
void sim_lean_counters(long long *out, int reset) {
    memcpy(out, g_aecm_lean_counters, sizeof(g_aecm_lean_counters));
    if (reset) memset(g_aecm_lean_counters, 0, sizeof(g_aecm_lean_counters));
}
}
