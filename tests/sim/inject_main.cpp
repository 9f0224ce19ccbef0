// TEST INFRASTRUCTURE -- a program of its own around tests/sim/sim_inject.cpp, built with -fsanitize=address,undefined
// (tests/inject_sim.py: build_sanitized_program) and run by tests/test_state_injection.py: the state corpus through the block DSP
// with every history-row and lane access under AddressSanitizer and every shift and conversion under UndefinedBehaviorSanitizer.
//
//   inject_main <corpus file> <result file>
// corpus file: int32 n, total_blocks, n_lens, lens[n_lens]; then vec [n][768] uint32, scal [n][64] int32, hist [n][6400] uint16,
// far / near / clean [n][total_blocks * 64] int16, has_clean [n] uint8.  result file: kinds [n] int32, out [n][total_blocks * 64]
// int16, then the three state regions as the launches left them.  Exit code 0 when every state ran without a violated claim.
#include <stdint.h>
#include <stdio.h>

#include <vector>

extern "C" int sim_inject_run_many(int n, uint32_t *vec, int32_t *scal, uint16_t *hist, const int16_t *far_s, const int16_t *near_s, const int16_t *clean,
                                   const uint8_t *has_clean, const int32_t *lens, int n_lens, int16_t *out, int32_t *kinds, int32_t *values);

template <class T> static bool get(FILE *f, std::vector<T> &v, size_t n) {
    v.resize(n);
    return fread(v.data(), sizeof(T), n, f) == n;
}
template <class T> static bool put(FILE *f, const std::vector<T> &v) { return fwrite(v.data(), sizeof(T), v.size(), f) == v.size(); }

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<int32_t> head, lens, scal, kinds, values;
    std::vector<uint32_t> vec;
    std::vector<uint16_t> hist;
    std::vector<int16_t> far_s, near_s, clean, out;
    std::vector<uint8_t> has_clean;
    if (!get(f, head, 3) || head[0] < 0 || head[1] < 0 || head[2] < 0 || !get(f, lens, (size_t)head[2])) return 2;
    const size_t n = (size_t)head[0], samples = n * (size_t)head[1] * 64;
    int total = 0;
    for (int32_t l : lens) total += l;
    if (total != head[1]) return 2;
    if (!get(f, vec, n * 768) || !get(f, scal, n * 64) || !get(f, hist, n * 6400) || !get(f, far_s, samples) || !get(f, near_s, samples) ||
        !get(f, clean, samples) || !get(f, has_clean, n))
        return 2;
    fclose(f);
    out.assign(samples, 0);
    kinds.assign(n, 0);
    values.assign(n, 0);
    const int bad = sim_inject_run_many((int)n, vec.data(), scal.data(), hist.data(), far_s.data(), near_s.data(), clean.data(), has_clean.data(), lens.data(),
                                        (int)lens.size(), out.data(), kinds.data(), values.data());
    f = fopen(argv[2], "wb");
    if (!f || !put(f, kinds) || !put(f, out) || !put(f, vec) || !put(f, scal) || !put(f, hist) || fclose(f) != 0) return 2;
    printf("%zu states, %d with a violated claim\n", n, bad);
    return bad ? 1 : 0;
}
