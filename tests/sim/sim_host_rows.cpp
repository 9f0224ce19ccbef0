// TEST INFRASTRUCTURE: the host-audio staging layer (webrtc_aecm_amd/csrc/aecm_host_rows.h: RowLayout, PackRows / UnpackRows,
// StagedIo; aecm_state.h: OffsetToStream) without a device, as a program of its own -- tests/test_host_rows.py builds it with
// AddressSanitizer and UBSan and runs it as a child process.  Every buffer is allocated to exactly its extent, so a block read or
// written one sample outside it is caught; every destination starts as a sentinel, so a block written that should not be is seen.
// Expectations are restated here sample by sample from IoView's definition (aecm_state.h): sample i of block b of stream s lives
// at s * stream_stride + b * block_stride + i, and at (s * T + b) * 64 + i of a dense plane.
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "aecm_host_rows.h"

using namespace aecm;

namespace {

constexpr int16_t kSentinel = 0x5a5a;      // the data below is 14 bits wide: never equal to it
uint64_t rng_state = 0;
int16_t NextSample() {
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (int16_t)((rng_state >> 40) & 0x3fff);
}

struct Layout {
    const char *name;
    int64_t stream_stride, block_stride;
    bool dense;
};
// (S, T) -> the five layouts.  dense: restated from ProcessBlocksHost's condition, block_stride == 64 and stream_stride == T * 64.
std::vector<Layout> Layouts(int S, int T) {
    const int64_t tick = (int64_t)S * 64, padded_tick_stream = 64 + 16;
    return {{"dense", (int64_t)T * 64, 64, true},
            {"padded stream stride", (int64_t)T * 64 + 24, 64, false},
            {"tick-major", 64, tick, S == 1 && T == 1},
            {"both padded", (int64_t)T * (64 + 8) + 40, 64 + 8, false},
            {"tick-major, both padded", padded_tick_stream, S * padded_tick_stream + 32, false}};
}
// lens modes: null, all T, mixed with zeros, all zero
std::vector<int32_t> Lens(int mode, int S, int T) {
    std::vector<int32_t> lens((size_t)S, mode == 1 ? T : 0);
    if (mode == 2)
        for (int s = 0; s < S; ++s) lens[(size_t)s] = s % 3 == 1 ? 0 : (s * 7 + T) % (T + 1);
    return lens;
}

int failures = 0;
void Expect(bool ok, const char *what, const Layout &l, int S, int T, int mode) {
    if (ok) return;
    if (++failures <= 20) printf("FAILED %s: %s, S=%d T=%d lens mode %d\n", what, l.name, S, T, mode);
}

void OneCase(const Layout &l, int S, int T, int mode) {
    const RowLayout rows{S, T, l.stream_stride, l.block_stride};
    const std::vector<int32_t> lens_v = Lens(mode, S, T);
    const int32_t *lens = mode == 0 ? nullptr : lens_v.data();
    auto live = [&](int s, int b) { return b < (lens ? lens[s] : T); };
    auto at = [&](int s, int b, int i) { return (size_t)(s * l.stream_stride + b * l.block_stride + i); };
    const size_t extent = at(S - 1, T - 1, kBlock - 1) + 1, per = (size_t)S * T * kBlock;
    Expect(rows.dense() == l.dense && rows.row() == (size_t)T * kBlock && rows.per() == per, "layout value", l, S, T, mode);

    // ---- pack: the caller's plane -> a dense plane
    std::vector<int16_t> user(extent), dense(per, kSentinel), want(per, kSentinel);
    for (int16_t &v : user) v = NextSample();
    for (int s = 0; s < S; ++s)
        for (int b = 0; b < T; ++b)
            for (int i = 0; i < kBlock; ++i)
                if (live(s, b)) want[((size_t)s * T + b) * kBlock + i] = user[at(s, b, i)];
    const std::vector<int16_t> user_before = user;
    PackRows(rows, user.data(), dense.data(), lens);
    Expect(dense == want, "PackRows: live blocks copied, the others untouched", l, S, T, mode);
    Expect(user == user_before, "PackRows: source untouched", l, S, T, mode);

    // ---- unpack: another dense plane -> a caller's plane of sentinels
    std::vector<int16_t> plane(per), back(extent, kSentinel), want_back(extent, kSentinel);
    for (int16_t &v : plane) v = NextSample();
    for (int s = 0; s < S; ++s)
        for (int b = 0; b < T; ++b)
            for (int i = 0; i < kBlock; ++i)
                if (live(s, b)) want_back[at(s, b, i)] = plane[((size_t)s * T + b) * kBlock + i];
    UnpackRows(rows, plane.data(), back.data(), lens);
    Expect(back == want_back, "UnpackRows: live blocks written, pads and blocks at or beyond the length keep the sentinel", l, S, T, mode);

    // ---- round trip: what was packed comes back where it was taken from
    std::vector<int16_t> again(extent, kSentinel);
    UnpackRows(rows, dense.data(), again.data(), lens);
    bool same = true;
    std::vector<bool> is_live(extent, false);
    for (int s = 0; s < S; ++s)
        for (int b = 0; b < T; ++b)
            for (int i = 0; i < kBlock; ++i)
                if (live(s, b)) is_live[at(s, b, i)] = true;
    for (size_t k = 0; k < extent; ++k) same = same && again[k] == (is_live[k] ? user[k] : kSentinel);
    Expect(same, "round trip", l, S, T, mode);
}

void StagedViews() {
    const Layout none{"staged view", 0, 0, false};
    for (int clean = 0; clean < 2; ++clean) {
        const size_t row = 3 * kBlock, per = 5 * row, off = 2 * row;
        std::vector<int16_t> stage(StagedSamples(per, clean != 0));
        Expect(stage.size() == per * (clean ? 4 : 3), "StagedSamples", none, 5, 3, clean);
        for (size_t o : {size_t(0), off}) {
            const IoView v = StagedIo(stage.data() + o, row, per, clean != 0);
            const int16_t *base = stage.data() + o;
            Expect(v.far == base && v.near == base + per && v.near_clean == (clean ? base + 2 * per : nullptr) &&
                       v.out == base + (clean ? 3 : 2) * per && v.stream_stride == (int64_t)row && v.block_stride == kBlock,
                   "StagedIo", none, 5, 3, clean);
        }
    }
    std::vector<uint32_t> vec(3 * kVecWordsPerStream);
    std::vector<int32_t> scal(3 * kNumScal);
    std::vector<uint16_t> hist(3 * kHistWordsPerStream);
    const uint32_t consts[1] = {0};
    const StatePtrs st{vec.data(), scal.data(), hist.data(), consts};
    const StatePtrs at2 = OffsetToStream(st, 2), at0 = OffsetToStream(st, 0);
    Expect(at2.vec == &vec[2 * kVecWordsPerStream] && at2.scal == &scal[2 * kNumScal] && at2.hist == &hist[2 * kHistWordsPerStream] && at2.consts == consts &&
               at0.vec == st.vec && at0.scal == st.scal && at0.hist == st.hist,
           "OffsetToStream", none, 3, 0, 0);
}

}  // namespace

int main() {
    int cases = 0;
    for (int S : {1, 3, 8})
        for (int T : {1, 3, 5})
            for (const Layout &l : Layouts(S, T))
                for (int mode = 0; mode < 4; ++mode) {
                    rng_state = 1000u * S + 100u * T + mode;
                    OneCase(l, S, T, mode);
                    ++cases;
                }
    StagedViews();
    printf("%d cases, %d failures\n%s\n", cases, failures, failures ? "FAILED" : "ok");
    return failures ? 1 : 0;
}
