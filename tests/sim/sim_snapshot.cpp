// TEST INFRASTRUCTURE: the CPU double of the bulk session-snapshot kernels (webrtc_aecm_amd/csrc/aecm_session_snapshot.h:
// SessionGatherPart / SessionScatterPart / SessionBlobDefect, the very routines aecm_session_snapshot_kernels.hip runs with one
// workgroup per session) on a host image of an object's device arrays, against an independent restatement of what
// SessionBatch::ExportSession / ImportSession do today: plain copies of the contiguous parts, [end - n, end) loops for the
// tails.  The restatement names the byte offsets as numbers, not through the header under test.
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "aecm_session_snapshot.h"

namespace {

using namespace aecm;

constexpr int kRingLen = 8192, kWorkers = 256;
constexpr size_t kBlobBytes = 34304;

struct Rng {
    uint64_t s;
    uint32_t next() {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        return (uint32_t)(s >> 33);
    }
    uint32_t word() { return next() ^ (next() << 16); }
};

// One object's arrays on the host, in the device's shapes.
struct Image {
    int S;
    std::vector<uint32_t> vec;
    std::vector<int32_t> scal, flow;
    std::vector<uint16_t> hist;
    std::vector<int16_t> far, near, clean, out, frames, old;
    uint32_t near_pos = 0;
    int32_t deferred_lag = 0;
    Image(int S_, bool has_clean, Rng &rng)
        : S(S_), vec((size_t)S_ * kVecWordsPerStream), scal((size_t)S_ * kNumScal), flow((size_t)S_ * kFlowFieldsUsed), hist((size_t)S_ * kHistWordsPerStream),
          far((size_t)S_ * kRingLen), near((size_t)S_ * kRingLen), clean(has_clean ? (size_t)S_ * kRingLen : 0), out((size_t)S_ * kRingLen),
          frames((size_t)S_ * kFlowFarFrameRing), old((size_t)S_ * 2 * kFlowFrame) {
        for (auto &w : vec) w = rng.word();
        for (auto &w : scal) w = (int32_t)rng.word();
        for (auto &w : hist) w = (uint16_t)rng.next();
        for (auto *ring : {&far, &near, &clean, &out, &frames, &old})
            for (auto &w : *ring) w = (int16_t)rng.next();
        for (int s = 0; s < S; ++s) {
            scal[(size_t)s * kNumScal + S_MULT] = 1 + (int)(rng.next() & 1u);
            int32_t words[kFlowWords];
            FlowInit(words);
            for (int f = 0; f < kFlowFieldsUsed; ++f) flow[(size_t)f * S + s] = words[f];
            SetPositions(s, rng.word(), 80 * (int32_t)(rng.next() % 512u), rng);
        }
    }
    // The positions a snapshot is cut by, and plausible neighbours for the rest.
    void SetPositions(int s, uint32_t blk_pos, int32_t lag, Rng &rng) {
        const auto at = [&](int f) -> int32_t & { return flow[(size_t)f * S + s]; };
        at(F_BLK_POS) = (int32_t)blk_pos;
        at(F_FRM_POS) = (int32_t)(blk_pos + rng.next() % 64u);
        at(F_OUT_RP) = (int32_t)(blk_pos - rng.next() % 100u);
        at(F_FAR_WP) = (int32_t)rng.word();
        at(F_FAR_RP) = (int32_t)((uint32_t)at(F_FAR_WP) - rng.next() % 4000u);
        at(F_NEAR_LAG) = lag;
    }
    SessionView View() {
        return SessionView{StatePtrs{vec.data(), scal.data(), hist.data(), nullptr}, flow.data(), (int64_t)S, far.data(), near.data(),
                           clean.empty() ? nullptr : clean.data(), out.data(), frames.data(), old.data(), near_pos, deferred_lag};
    }
    bool operator==(const Image &o) const {
        return vec == o.vec && scal == o.scal && flow == o.flow && hist == o.hist && far == o.far && near == o.near && clean == o.clean && out == o.out &&
               frames == o.frames && old == o.old;
    }
};

// A buffer for one snapshot, 16-byte aligned or (narrow) 4 bytes past that.
struct Blob {
    std::vector<uint8_t> store;
    uint8_t *p;
    explicit Blob(bool wide) : store(kBlobBytes + 48, 0xa5) {
        uintptr_t a = (reinterpret_cast<uintptr_t>(store.data()) + 15) & ~uintptr_t(15);
        p = reinterpret_cast<uint8_t *>(a) + (wide ? 0 : 4);
    }
};

std::vector<int> ShuffledWorkers(Rng &rng) {
    std::vector<int> order(kWorkers);
    for (int i = 0; i < kWorkers; ++i) order[i] = i;
    for (int i = kWorkers - 1; i > 0; --i) std::swap(order[i], order[rng.next() % (uint32_t)(i + 1)]);
    return order;
}

void Gather(Image &im, int session, uint8_t *blob, bool wide, Rng &rng) {
    const SessionView v = im.View();
    for (int tid : ShuffledWorkers(rng)) {
        if (wide) SessionGatherPart<true>(v, session, blob, tid, kWorkers);
        else SessionGatherPart<false>(v, session, blob, tid, kWorkers);
    }
}

void Scatter(Image &im, int slot, const uint8_t *blob, bool wide, const std::vector<int> &workers) {
    const SessionView v = im.View();
    for (int tid : workers) {
        if (wide) SessionScatterPart<true>(v, slot, blob, tid, kWorkers);
        else SessionScatterPart<false>(v, slot, blob, tid, kWorkers);
    }
}

// ---- the restatement: SessionBatch::ExportSession / ImportSession as they are, on the image ------------------------------
void ExportRestated(const Image &im, int s, uint8_t *p) {
    const uint32_t mult = (uint32_t)im.scal[(size_t)s * 64 + S_MULT];
    const uint32_t header[8] = {0x4e534541u, 1u, mult * 8000u, im.clean.empty() ? 0u : 1u, 32u, 8192u, 256u, 64u};
    memcpy(p, header, 32);
    const uint32_t core[8] = {0x53434541u, 3u, mult * 8000u, 12u, 64u, 100u, 64u, 0u};
    memcpy(p + 32, core, 32);
    memcpy(p + 64, im.vec.data() + (size_t)s * 768, 3072);
    memcpy(p + 64 + 3072, im.scal.data() + (size_t)s * 64, 256);
    memcpy(p + 64 + 3072 + 256, im.hist.data() + (size_t)s * 6400, 12800);
    int32_t flow[32] = {0};
    for (int f = 0; f < kFlowFieldsUsed; ++f) flow[f] = im.flow[(size_t)f * im.S + s];
    const uint32_t own_near_pos = im.near_pos - (uint32_t)flow[F_NEAR_LAG] - (uint32_t)im.deferred_lag;
    flow[F_NEAR_LAG] = 0;
    memcpy(p + 16192, flow, 128);
    memcpy(p + 16320, im.far.data() + (size_t)s * 8192, 16384);
    const auto tail = [](const int16_t *row, uint32_t end_pos, int n, uint8_t *dst) {
        for (int k = 0; k < n; ++k) {
            const int16_t v = row[(end_pos - (uint32_t)n + (uint32_t)k) & 8191u];
            memcpy(dst + 2 * k, &v, 2);
        }
    };
    tail(im.out.data() + (size_t)s * 8192, (uint32_t)flow[F_BLK_POS], 256, p + 32704);
    tail(im.near.data() + (size_t)s * 8192, own_near_pos, 64, p + 33216);
    if (!im.clean.empty()) tail(im.clean.data() + (size_t)s * 8192, own_near_pos, 64, p + 33344);
    else memset(p + 33344, 0, 128);
    memcpy(p + 33472, im.frames.data() + (size_t)s * 256, 512);
    memcpy(p + 33984, im.old.data() + (size_t)s * 160, 320);
}

void ImportRestated(Image &im, int s, const uint8_t *p) {
    memcpy(im.vec.data() + (size_t)s * 768, p + 64, 3072);
    memcpy(im.scal.data() + (size_t)s * 64, p + 64 + 3072, 256);
    memcpy(im.hist.data() + (size_t)s * 6400, p + 64 + 3072 + 256, 12800);
    int32_t flow[32];
    memcpy(flow, p + 16192, 128);
    flow[F_NEAR_LAG] = 0;
    for (int f = 0; f < kFlowFieldsUsed; ++f) im.flow[(size_t)f * im.S + s] = flow[f];
    memcpy(im.far.data() + (size_t)s * 8192, p + 16320, 16384);
    const uint32_t own_near_pos = im.near_pos - (uint32_t)im.deferred_lag;
    const auto place_tail = [](int16_t *row, uint32_t end_pos, int n, const uint8_t *src, bool zero_rest) {
        if (zero_rest) std::fill(row, row + 8192, (int16_t)0);
        for (int k = 0; k < n; ++k) memcpy(&row[(end_pos - (uint32_t)n + (uint32_t)k) & 8191u], src + 2 * k, 2);
    };
    place_tail(im.out.data() + (size_t)s * 8192, (uint32_t)flow[F_BLK_POS], 256, p + 32704, true);
    place_tail(im.near.data() + (size_t)s * 8192, own_near_pos, 64, p + 33216, false);
    if (!im.clean.empty()) place_tail(im.clean.data() + (size_t)s * 8192, own_near_pos, 64, p + 33344, false);
    memcpy(im.frames.data() + (size_t)s * 256, p + 33472, 512);
    memcpy(im.old.data() + (size_t)s * 160, p + 33984, 320);
}

int64_t FirstDifference(const uint8_t *a, const uint8_t *b) {
    for (size_t i = 0; i < kBlobBytes; ++i)
        if (a[i] != b[i]) return (int64_t)i;
    return -1;
}

// A snapshot every rule accepts: a session as WebRtcAecm_Init leaves its wrapper, a core state of zeros at the rate fs with the
// suppression-gain parameters of echoMode 3 (the gate admits set_config's five tuples only).
void ValidBlob(uint8_t *p, int fs, const int32_t *flow_words) {
    memset(p, 0, kBlobBytes);
    const uint32_t header[8] = {kSessionMagic, kSessionVersion, (uint32_t)fs, 0u, (uint32_t)kFlowWords, (uint32_t)kFlowFarRing, (uint32_t)kSessionOutTail,
                                (uint32_t)kSessionNearTail};
    memcpy(p, header, sizeof header);
    const uint32_t core[8] = {kSnapshotMagic, kStateLayoutVersion, (uint32_t)fs, (uint32_t)kNumVec, (uint32_t)kNumScal, (uint32_t)kHistory, (uint32_t)kLanes, 0u};
    memcpy(p + 32, core, sizeof core);
    const int32_t mult = fs / 8000;
    memcpy(p + 64 + kVecWordsPerStream * 4 + S_MULT * 4, &mult, 4);
    SupGainParams sg;
    SupGainParamsOfMode(3, &sg);
    const int32_t sg_words[4] = {sg.a, sg.d, sg.dab, sg.dbd};
    static_assert(S_SG_D == S_SG_A + 1 && S_SG_DAB == S_SG_A + 2 && S_SG_DBD == S_SG_A + 3, "the four words are neighbours");
    memcpy(p + 64 + kVecWordsPerStream * 4 + S_SG_A * 4, sg_words, sizeof sg_words);
    int32_t words[kFlowWords];
    FlowInit(words);
    memcpy(p + 16192, flow_words ? flow_words : words, sizeof words);
}

int BlobDefect(const uint8_t *p, int fs_object, bool any_rate) {
    for (int tid = 0; tid < kLanes; ++tid)
        if (const int d = SessionBlobDefect(p, fs_object, any_rate, tid)) return d;
    return 0;
}

}  // namespace

extern "C" {

size_t sim_snapshot_bytes(void) { return kSessionBytes; }

// SessionGatherPart of one session of a 3-session image (256 workers in a shuffled order) against the restatement.
// Returns -1 when every byte is equal, else the offset of the first byte that differs.
int64_t sim_snapshot_gather(uint64_t seed, int session, uint32_t blk_pos, uint32_t near_pos, int32_t lag, int32_t deferred_lag, int has_clean, int wide) {
    Rng rng{seed * 2654435761ull + 99};
    Image im(3, has_clean != 0, rng);
    im.near_pos = near_pos;
    im.deferred_lag = deferred_lag;
    im.SetPositions(session, blk_pos, lag, rng);
    Blob got(wide != 0), want(true);
    Gather(im, session, got.p, wide != 0, rng);
    ExportRestated(im, session, want.p);
    return FirstDifference(got.p, want.p);
}

// The snapshot of session `session` of a 3-session image A goes into slot `slot` of an image B of s2 sessions, another near
// position and deferred lag: SessionScatterPart (256 workers, shuffled) must leave exactly what the restatement of ImportSession
// leaves -- in EVERY session's rows (untouched near-ring samples kept, the out row zeroed, no other slot written) -- and
// gathering the slot again must reproduce the snapshot (but for the header's has_clean word when only one of the objects has a
// clean ring).  Returns 0, 1 (the images differ) or 2 + the first byte the second snapshot differs at.
int64_t sim_snapshot_scatter(uint64_t seed, int session, uint32_t blk_pos, uint32_t near_pos_a, int32_t lag, int32_t deferred_a, int clean_a, int s2, int slot,
                             uint32_t near_pos_b, int32_t deferred_b, int clean_b, int wide) {
    Rng rng{seed * 2654435761ull + 7};
    Image a(3, clean_a != 0, rng);
    a.near_pos = near_pos_a;
    a.deferred_lag = deferred_a;
    a.SetPositions(session, blk_pos, lag, rng);
    Blob blob(wide != 0), again(wide != 0);
    Gather(a, session, blob.p, wide != 0, rng);
    Image b(s2, clean_b != 0, rng);
    b.near_pos = near_pos_b;
    b.deferred_lag = deferred_b;
    Image want = b;
    Scatter(b, slot, blob.p, wide != 0, ShuffledWorkers(rng));
    ImportRestated(want, slot, blob.p);
    if (!(b == want)) return 1;
    Gather(b, slot, again.p, wide != 0, rng);
    if (clean_a != clean_b) memcpy(again.p + 12, blob.p + 12, 4);
    const int64_t d = FirstDifference(again.p, blob.p);
    return d < 0 ? 0 : 2 + d;
}

// Every element SessionScatterPart writes is written by exactly one of the 256 workers, and nothing outside the slot is written:
// each worker runs alone on two copies of an image that differ in every bit; what it wrote is where the copies agree afterwards.
// Returns 0, or 1 + the number of elements written twice, never (inside what an import writes) or outside the slot.
int64_t sim_snapshot_scatter_coverage(uint64_t seed, uint32_t blk_pos, uint32_t near_pos_b, int32_t deferred_b, int wide) {
    Rng rng{seed * 2654435761ull + 3};
    Image a(3, true, rng);
    a.SetPositions(1, blk_pos, 0, rng);
    Blob blob(wide != 0);
    Gather(a, 1, blob.p, wide != 0, rng);
    Image x(2, true, rng);
    x.near_pos = near_pos_b;
    x.deferred_lag = deferred_b;
    Image y = x;
    for (auto &w : y.vec) w = ~w;
    for (auto &w : y.scal) w = ~w;
    for (auto &w : y.flow) w = ~w;
    for (auto &w : y.hist) w = (uint16_t)~w;
    for (auto *ring : {&y.far, &y.near, &y.clean, &y.out, &y.frames, &y.old})
        for (auto &w : *ring) w = (int16_t)~w;
    // the elements an import of slot 1 writes, from the restatement: where two imports into x and y agree
    Image wx = x, wy = y;
    ImportRestated(wx, 1, blob.p);
    ImportRestated(wy, 1, blob.p);
    std::vector<int> counts;
    const auto tally = [&counts](const Image &p, const Image &q, int add) {
        size_t at = 0;
        const auto each = [&](const auto &u, const auto &v) {
            if (counts.size() < at + u.size()) counts.resize(at + u.size(), 0);
            for (size_t i = 0; i < u.size(); ++i) counts[at + i] += u[i] == v[i] ? add : 0;
            at += u.size();
        };
        each(p.vec, q.vec), each(p.scal, q.scal), each(p.flow, q.flow), each(p.hist, q.hist), each(p.far, q.far), each(p.near, q.near);
        each(p.clean, q.clean), each(p.out, q.out), each(p.frames, q.frames), each(p.old, q.old);
    };
    tally(wx, wy, -1);                                      // expected: -1, then + 1 per worker that wrote it -> 0 everywhere
    for (int tid = 0; tid < kWorkers; ++tid) {
        Image cx = x, cy = y;
        Scatter(cx, 1, blob.p, wide != 0, {tid});
        Scatter(cy, 1, blob.p, wide != 0, {tid});
        tally(cx, cy, 1);
    }
    int64_t bad = 0;
    for (int c : counts) bad += c != 0;
    return bad ? 1 + bad : 0;
}

// SessionBlobDefect on every state a session passes through in a run of n_ticks ticks with far-end bursts between them
// (tests/sim/sim_flow.cpp's scenario 13: random call sizes, underruns, split calls, msInSndCardBuf anywhere), the state right
// after a burst and before the next Process included, and with a lag word as after idle ticks now and then.  Returns -1, or the
// first tick a state was refused at; detail: [0] the defect code, [1] states checked, [2] of them right after a burst.
int64_t sim_snapshot_defect_run(uint64_t seed, int fs, int n_ticks, int64_t *detail) {
    Rng rng{seed * 2654435761ull + 12345};
    const auto range = [&rng](int lo, int hi) { return lo + (int)(rng.next() % (uint32_t)(hi - lo + 1)); };
    const auto chance = [&rng](int percent) { return (int)(rng.next() % 100u) < percent; };
    FlowRegs regs;
    int32_t words[kFlowWords];
    FlowInit(words);
    for (int k = 0; k < kFlowFieldsUsed; ++k) regs.v[k] = words[k];
    uint32_t near_pos = 0;
    detail[0] = detail[1] = detail[2] = 0;
    std::vector<uint8_t> blob(kBlobBytes);
    const auto refused = [&]() -> int {
        int32_t w[kFlowWords] = {0};
        for (int k = 0; k < kFlowFieldsUsed; ++k) w[k] = regs.v[k];
        if (chance(20)) w[F_NEAR_LAG] = 80 * range(0, kFlowLagPeriod / 80 - 1);
        ValidBlob(blob.data(), fs, w);
        ++detail[1];
        return BlobDefect(blob.data(), fs, false);
    };
    const int mult = fs == 16000 ? 2 : 1;
    for (int64_t tick = 0; tick < n_ticks; ++tick) {
        int extra = chance(30) ? range(1, 4) : 0, extra_len = chance(50) ? 80 : 160, flags = 0;
        if (chance(35)) flags |= kFlowNoFarend;
        if (chance(2)) extra = range(20, 60);
        const int ms = range(0, 300), n = chance(30) ? 80 : 160;
        if (chance(30) && n == 160) flags |= kFlowSplitCalls;
        if (extra > 0) {
            FlowBurst b;
            FlowBurstBegin(regs, extra_len, extra, b);
            for (int c = 0; c < extra; ++c) (void)FlowFarendCall(regs, mult, extra_len);
            ++detail[2];
            if (const int d = refused()) { detail[0] = d; return tick; }
        }
        FlowPlan plan;
        FlowTick(regs, fs, n, ms, flags, near_pos, plan);
        near_pos += (uint32_t)n;
        if (const int d = refused()) { detail[0] = d; return tick; }
    }
    return -1;
}

// One defect in an otherwise valid snapshot of rate fs_blob, offered to an object of rate fs_object: 0 none, 1 magic, 2 version,
// 3 lag word 81, 4 an unused wrapper word, 5 pending 64, 6 a core scalar out of range, 7 a core state of the other rate.
// Returns SessionBlobDefect's verdict: 0 or the code of the first worker that refuses.
int sim_snapshot_defect_case(int which, int fs_blob, int fs_object, int any_rate) {
    std::vector<uint8_t> blob(kBlobBytes);
    ValidBlob(blob.data(), fs_blob, nullptr);
    const auto put = [&blob](size_t at, int32_t v) { memcpy(blob.data() + at, &v, 4); };
    switch (which) {
        case 1: put(0, 0x4e534542); break;
        case 2: put(4, (int32_t)kSessionVersion + 1); break;
        case 3: put(16192 + 4 * F_NEAR_LAG, 81); break;
        case 4: put(16192 + 4 * (kFlowWords - 1), 1); break;
        case 5: put(16192 + 4 * F_FRM_POS, 64); break;
        case 6: put(64 + kVecWordsPerStream * 4 + 4 * S_STARTUP, 3); break;
        case 7: put(32 + 8, fs_blob == 8000 ? 16000 : 8000), put(64 + kVecWordsPerStream * 4 + 4 * S_MULT, fs_blob == 8000 ? 2 : 1); break;
        default: break;
    }
    return BlobDefect(blob.data(), fs_object, any_rate != 0);
}

}  // extern "C"
