// The snapshot of ONE session (WebRtcAecmSessions_ExportSession / ImportSession: aecm_sessions.h) -- its layout, and the three
// routines that write one from an object's device arrays, write one into them, and say whether one may be run on.  ONE
// statement for the host (aecm_sessions.cpp), the kernels of the bulk forms (aecm_session_snapshot_kernels.hip: one workgroup
// per session) and the CPU double of those kernels (tests/sim/sim_snapshot.cpp).
//
//   header (32 B) | block-stream blob (kStateBlobBytes, aecm_state_check.h) | wrapper state kFlowWords int32 | far ring
//   kFlowFarRing int16, as it lies | the last kSessionOutTail block-output samples before F_BLK_POS | the last kSessionNearTail
//   near-end and clean near-end samples before the session's own near position | framed-far ring | the two replay rows
//
// Every part starts at a multiple of 16 bytes and every contiguous part is a multiple of 16 bytes long: a snapshot in a
// 16-byte-aligned buffer moves as 16-byte accesses (kWide), one in a buffer that is only 4-byte aligned as 32-bit words.
#ifndef AECM_AMD_SESSION_SNAPSHOT_H_
#define AECM_AMD_SESSION_SNAPSHOT_H_

#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "aecm_flow_plan.h"
#include "aecm_state.h"
#include "aecm_state_check.h"

namespace aecm {

struct SessionSnapshotHeader {
    uint32_t magic, version, fs, has_clean, flow_words, far_ring, out_tail, near_tail;
};
constexpr uint32_t kSessionMagic = 0x4e534541u;       // "AESN"
constexpr uint32_t kSessionVersion = 1;               // bump with aecm_flow_plan.h's field list or the layout below
constexpr int kSessionOutTail = 256, kSessionNearTail = 64;
constexpr size_t kSessionHeaderBytes = sizeof(SessionSnapshotHeader);
static_assert(kSessionHeaderBytes == 32, "session snapshot header");
struct SessionOffsets {                                // byte offsets of the parts behind the header
    size_t state = kSessionHeaderBytes, flow = state + kStateBlobBytes, far = flow + kFlowWords * 4, out = far + kFlowFarRing * 2,
           near = out + kSessionOutTail * 2, clean = near + kSessionNearTail * 2, frames = clean + kSessionNearTail * 2,
           old = frames + kFlowFarFrameRing * 2, end = old + 2 * kFlowFrame * 2;
};
constexpr size_t kSessionBytes = SessionOffsets().end;
static_assert(SessionOffsets().state == 32 && SessionOffsets().flow == 16192 && SessionOffsets().far == 16320 && SessionOffsets().out == 32704 &&
                  SessionOffsets().near == 33216 && SessionOffsets().clean == 33344 && SessionOffsets().frames == 33472 &&
                  SessionOffsets().old == 33984 && SessionOffsets().end == 34304,
              "session snapshot layout");
static_assert(SessionOffsets().state % 16 == 0 && SessionOffsets().flow % 16 == 0 && SessionOffsets().far % 16 == 0 && SessionOffsets().out % 16 == 0 &&
                  SessionOffsets().near % 16 == 0 && SessionOffsets().clean % 16 == 0 && SessionOffsets().frames % 16 == 0 &&
                  SessionOffsets().old % 16 == 0 && SessionOffsets().end % 16 == 0,
              "every part of a session snapshot starts at a multiple of 16 bytes");
static_assert((kVecWordsPerStream * 4) % 16 == 0 && (kNumScal * 4) % 16 == 0 && (kHistWordsPerStream * 2) % 16 == 0 && (kFlowFarRing * 2) % 16 == 0 &&
                  (kFlowFarFrameRing * 2) % 16 == 0 && (2 * kFlowFrame * 2) % 16 == 0,
              "every contiguous part (and every row it comes from) is a multiple of 16 bytes");
static_assert((kFlowFarRing & (kFlowFarRing - 1)) == 0 && kSessionOutTail <= kFlowFarRing, "ring positions are reduced with a mask");

// One object's device arrays, as the routines below see them (the host image of tests/sim/sim_snapshot.cpp has the same shape).
struct SessionView {
    StatePtrs st;                       // core state of all S sessions (aecm_state.h)
    int32_t *flow_state;                // [kFlowFieldsUsed][S] wrapper state, field-major: flow_state[field * S + session]
    int64_t S;
    int16_t *far_ring, *near_ring, *clean_ring, *out_ring;      // [S][kFlowFarRing]; clean_ring may be null
    int16_t *far_frames;                // [S][kFlowFarFrameRing]
    int16_t *far_old;                   // [S][2 * kFlowFrame]
    uint32_t near_pos;                  // the object's near position (near-end samples ticked so far, wrapping)
    int32_t deferred_lag;               // samples of ticks nobody made that the sessions' lag words do not hold yet (FlowObjectLag)
};

// What moves bytes: 32-bit words and 16-byte quads that may alias anything (the rows are int16, uint16, int32 and uint32).
typedef uint32_t __attribute__((may_alias)) SnapWord;
typedef int16_t __attribute__((may_alias)) SnapSample;
struct __attribute__((may_alias, aligned(16))) SnapQuad {
    uint32_t w[4];
};

// bytes (a multiple of 16) from src to dst, both aligned for the unit moved: worker tid of nthreads takes every nthreads-th unit.
template <bool kWide>
AECM_FLOW_HD void SessionCopyPart(void *dst, const void *src, int bytes, int tid, int nthreads) {
    if (kWide) {
        SnapQuad *d = static_cast<SnapQuad *>(dst);
        const SnapQuad *s = static_cast<const SnapQuad *>(src);
        for (int i = tid; i < bytes / 16; i += nthreads) d[i] = s[i];
    } else {
        SnapWord *d = static_cast<SnapWord *>(dst);
        const SnapWord *s = static_cast<const SnapWord *>(src);
        for (int i = tid; i < bytes / 4; i += nthreads) d[i] = s[i];
    }
}

// The snapshot of `session` into blob, byte for byte what SessionBatch::ExportSession writes: the work of nthreads cooperating
// workers, this one being tid; no worker depends on another.  kWide: blob is 16-byte aligned (else 4-byte).
template <bool kWide>
AECM_FLOW_HD void SessionGatherPart(const SessionView &v, int session, void *blob, int tid, int nthreads) {
    const SessionOffsets at;
    uint8_t *p = static_cast<uint8_t *>(blob);
    const int64_t s = session;
    const uint32_t mask = (uint32_t)kFlowFarRing - 1u;
    const SnapWord *scal = reinterpret_cast<const SnapWord *>(v.st.scal + s * (int64_t)kNumScal);
    // the two headers
    SnapWord *head = reinterpret_cast<SnapWord *>(p);
    for (int i = tid; i < 16; i += nthreads) {
        const uint32_t fs = scal[S_MULT] * 8000u;
        const uint32_t words[16] = {kSessionMagic, kSessionVersion, fs, v.clean_ring ? 1u : 0u, (uint32_t)kFlowWords, (uint32_t)kFlowFarRing,
                                    (uint32_t)kSessionOutTail, (uint32_t)kSessionNearTail,
                                    kSnapshotMagic, kStateLayoutVersion, fs, (uint32_t)kNumVec, (uint32_t)kNumScal, (uint32_t)kHistory, (uint32_t)kLanes, 0u};
        head[i] = words[i];
    }
    // core state, as aecm_gather_states_kernel writes it: the three regions as they lie
    uint8_t *core = p + at.state + kStateHeaderBytes;
    SessionCopyPart<kWide>(core, v.st.vec + s * (int64_t)kVecWordsPerStream, (int)kVecWordsPerStream * 4, tid, nthreads);
    SessionCopyPart<kWide>(core + kVecWordsPerStream * 4, scal, kNumScal * 4, tid, nthreads);
    SessionCopyPart<kWide>(core + kVecWordsPerStream * 4 + kNumScal * 4, v.st.hist + s * (int64_t)kHistWordsPerStream, (int)kHistWordsPerStream * 2, tid, nthreads);
    // wrapper words: the snapshot is in step (lag word 0), whatever the session has sat out
    SnapWord *flow = reinterpret_cast<SnapWord *>(p + at.flow);
    for (int i = tid; i < kFlowWords; i += nthreads) flow[i] = i < kFlowFieldsUsed && i != F_NEAR_LAG ? (uint32_t)v.flow_state[(int64_t)i * v.S + s] : 0u;
    SessionCopyPart<kWide>(p + at.far, v.far_ring + s * (int64_t)kFlowFarRing, kFlowFarRing * 2, tid, nthreads);
    // the tails, by position: [end - n, end) of the ring.  The session's own near position: the object's, less what the session
    // has sat out (its lag word + the all-idle ticks not yet added to it)
    const uint32_t blk_pos = (uint32_t)v.flow_state[(int64_t)F_BLK_POS * v.S + s];
    const uint32_t own_near_pos = v.near_pos - (uint32_t)v.flow_state[(int64_t)F_NEAR_LAG * v.S + s] - (uint32_t)v.deferred_lag;
    SnapSample *out_tail = reinterpret_cast<SnapSample *>(p + at.out), *near_tail = reinterpret_cast<SnapSample *>(p + at.near),
               *clean_tail = reinterpret_cast<SnapSample *>(p + at.clean);
    const int16_t *out_row = v.out_ring + s * (int64_t)kFlowFarRing, *near_row = v.near_ring + s * (int64_t)kFlowFarRing;
    for (int k = tid; k < kSessionOutTail; k += nthreads) out_tail[k] = out_row[(blk_pos - (uint32_t)kSessionOutTail + (uint32_t)k) & mask];
    for (int k = tid; k < kSessionNearTail; k += nthreads) {
        const uint32_t at_ring = (own_near_pos - (uint32_t)kSessionNearTail + (uint32_t)k) & mask;
        near_tail[k] = near_row[at_ring];
        clean_tail[k] = v.clean_ring ? v.clean_ring[s * (int64_t)kFlowFarRing + at_ring] : (int16_t)0;
    }
    SessionCopyPart<kWide>(p + at.frames, v.far_frames + s * (int64_t)kFlowFarFrameRing, kFlowFarFrameRing * 2, tid, nthreads);
    SessionCopyPart<kWide>(p + at.old, v.far_old + s * (int64_t)(2 * kFlowFrame), 2 * kFlowFrame * 2, tid, nthreads);
}

// The inverse, into slot `slot`: what SessionBatch::ImportSession leaves (the blob has passed SessionBlobDefect).  The session
// arrives in step with this object: lag word 0, its near tails placed before the position the device takes for the object's
// (near_pos - deferred_lag); the rest of the near / clean rows stays, the rest of the out row reads as never written.  Every
// element is written by exactly one worker.
template <bool kWide>
AECM_FLOW_HD void SessionScatterPart(const SessionView &v, int slot, const void *blob, int tid, int nthreads) {
    const SessionOffsets at;
    const uint8_t *p = static_cast<const uint8_t *>(blob);
    const int64_t s = slot;
    const uint32_t mask = (uint32_t)kFlowFarRing - 1u;
    const uint8_t *core = p + at.state + kStateHeaderBytes;
    SessionCopyPart<kWide>(v.st.vec + s * (int64_t)kVecWordsPerStream, core, (int)kVecWordsPerStream * 4, tid, nthreads);
    SessionCopyPart<kWide>(v.st.scal + s * (int64_t)kNumScal, core + kVecWordsPerStream * 4, kNumScal * 4, tid, nthreads);
    SessionCopyPart<kWide>(v.st.hist + s * (int64_t)kHistWordsPerStream, core + kVecWordsPerStream * 4 + kNumScal * 4, (int)kHistWordsPerStream * 2, tid, nthreads);
    const SnapWord *flow = reinterpret_cast<const SnapWord *>(p + at.flow);
    for (int i = tid; i < kFlowFieldsUsed; i += nthreads) v.flow_state[(int64_t)i * v.S + s] = i != F_NEAR_LAG ? (int32_t)flow[i] : 0;
    SessionCopyPart<kWide>(v.far_ring + s * (int64_t)kFlowFarRing, p + at.far, kFlowFarRing * 2, tid, nthreads);
    // the out row: 16 bytes at a time where the tail is not, sample by sample where it is (the rows are 16-byte aligned whatever the blob is)
    const uint32_t out_start = (uint32_t)flow[F_BLK_POS] - (uint32_t)kSessionOutTail;
    const SnapSample *out_tail = reinterpret_cast<const SnapSample *>(p + at.out), *near_tail = reinterpret_cast<const SnapSample *>(p + at.near),
                     *clean_tail = reinterpret_cast<const SnapSample *>(p + at.clean);
    int16_t *out_row = v.out_ring + s * (int64_t)kFlowFarRing;
    for (int q = tid; q < kFlowFarRing / 8; q += nthreads) {
        const uint32_t rel0 = ((uint32_t)(8 * q) - out_start) & mask;          // where the quad's first sample lies in the tail, if it does
        if (rel0 >= (uint32_t)kSessionOutTail && rel0 <= mask - 7u) {
            reinterpret_cast<SnapQuad *>(out_row)[q] = SnapQuad{{0u, 0u, 0u, 0u}};
        } else {
            for (uint32_t j = 0; j < 8u; ++j) {
                const uint32_t rel = (rel0 + j) & mask;
                out_row[8 * q + (int)j] = rel < (uint32_t)kSessionOutTail ? (int16_t)out_tail[rel] : (int16_t)0;
            }
        }
    }
    const uint32_t own_near_pos = v.near_pos - (uint32_t)v.deferred_lag;
    for (int k = tid; k < kSessionNearTail; k += nthreads) {
        const uint32_t at_ring = (own_near_pos - (uint32_t)kSessionNearTail + (uint32_t)k) & mask;
        v.near_ring[s * (int64_t)kFlowFarRing + at_ring] = near_tail[k];
        if (v.clean_ring) v.clean_ring[s * (int64_t)kFlowFarRing + at_ring] = clean_tail[k];
    }
    SessionCopyPart<kWide>(v.far_frames + s * (int64_t)kFlowFarFrameRing, p + at.frames, kFlowFarFrameRing * 2, tid, nthreads);
    SessionCopyPart<kWide>(v.far_old + s * (int64_t)(2 * kFlowFrame), p + at.old, 2 * kFlowFrame * 2, tid, nthreads);
}

// Word i of a blob that is 4-byte aligned on the device and may lie anywhere on the host.
AECM_FLOW_HD uint32_t SessionBlobWord(const void *blob, size_t byte_offset, int i) {
#if defined(__HIP_DEVICE_COMPILE__)
    return reinterpret_cast<const SnapWord *>(static_cast<const uint8_t *>(blob) + byte_offset)[i];
#else
    uint32_t w;
    memcpy(&w, static_cast<const uint8_t *>(blob) + byte_offset + (size_t)i * 4, 4);
    return w;
#endif
}

// May this snapshot be imported into an object of rate fs_object?  Every rule of SessionBatch::ImportSession, as the work of
// kLanes workers: worker tid checks the headers, scalar field tid and lane tid of the core state, worker 0 the wrapper words and
// the core state's rules over several fields as well.  The snapshot may be run on when every worker returns 0.  any_rate: ImportSessionAnyRate's rule for the rate.
enum SessionBlobDefectCode : int {
    kSessionDefectNone = 0, kSessionDefectHeader = 1, kSessionDefectRate = 2, kSessionDefectCoreHeader = 3,
    kSessionDefectFlow = 0x100,          // + FlowStateDefect's 1-based field
    kSessionDefectCore = 0x200           // + the StateDefect
};
AECM_FLOW_HD int SessionBlobDefect(const void *blob, int fs_object, bool any_rate, int tid) {
    const SessionOffsets at;
    SessionSnapshotHeader h;
    h.magic = SessionBlobWord(blob, 0, 0); h.version = SessionBlobWord(blob, 0, 1); h.fs = SessionBlobWord(blob, 0, 2); h.has_clean = SessionBlobWord(blob, 0, 3);
    h.flow_words = SessionBlobWord(blob, 0, 4); h.far_ring = SessionBlobWord(blob, 0, 5); h.out_tail = SessionBlobWord(blob, 0, 6); h.near_tail = SessionBlobWord(blob, 0, 7);
    if (h.magic != kSessionMagic || h.version != kSessionVersion || h.has_clean > 1u || h.flow_words != (uint32_t)kFlowWords ||
        h.far_ring != (uint32_t)kFlowFarRing || h.out_tail != (uint32_t)kSessionOutTail || h.near_tail != (uint32_t)kSessionNearTail)
        return kSessionDefectHeader;
    if (any_rate ? h.fs != 8000u && h.fs != 16000u : h.fs != (uint32_t)fs_object) return kSessionDefectRate;
    if (tid == 0) {
        int32_t flow[kFlowWords];
        for (int i = 0; i < kFlowWords; ++i) flow[i] = (int32_t)SessionBlobWord(blob, at.flow, i);
        if (const int f = FlowStateDefect(flow)) return kSessionDefectFlow + f;
    }
    SnapshotHeader core;                                     // the core state must be of the session's rate
    core.magic = SessionBlobWord(blob, at.state, 0); core.version = SessionBlobWord(blob, at.state, 1); core.fs = SessionBlobWord(blob, at.state, 2);
    core.num_vec = SessionBlobWord(blob, at.state, 3); core.num_scal = SessionBlobWord(blob, at.state, 4); core.history = SessionBlobWord(blob, at.state, 5);
    core.lanes = SessionBlobWord(blob, at.state, 6); core.reserved = SessionBlobWord(blob, at.state, 7);
    if (!SnapshotHeaderOk(core) || core.fs != h.fs) return kSessionDefectCoreHeader;
    const size_t vec_at = at.state + kStateHeaderBytes, scal_at = vec_at + kVecWordsPerStream * 4;
    if (const int d = ScalarFieldDefect(tid, (int32_t)SessionBlobWord(blob, scal_at, tid), (int)core.fs)) return kSessionDefectCore + d;
    if (tid == 0)
        if (const int d = SupGainErrParamsDefect((int32_t)SessionBlobWord(blob, scal_at, S_SG_A), (int32_t)SessionBlobWord(blob, scal_at, S_SG_D),
                                                 (int32_t)SessionBlobWord(blob, scal_at, S_SG_DAB), (int32_t)SessionBlobWord(blob, scal_at, S_SG_DBD)))
            return kSessionDefectCore + d;
    if (const int d = LaneWordsDefect(tid, SessionBlobWord(blob, vec_at, V_NEARFILT * kLanes + tid), SessionBlobWord(blob, vec_at, V_NOISE * kLanes + tid),
                                      SessionBlobWord(blob, vec_at, V_MEAN * kLanes + tid), SessionBlobWord(blob, vec_at, V_M01 * kLanes + tid)))
        return kSessionDefectCore + d;
    return 0;
}

}  // namespace aecm

#if defined(__HIPCC__)
#include <hip/hip_runtime_api.h>
namespace aecm {
// Launchers of aecm_session_snapshot_kernels.hip.  blobs_dev: count snapshots back to back, anything the device can address,
// 16-byte aligned with `wide`, 4-byte aligned otherwise.  sessions_dev (device, count entries, may be null: first .. first +
// count - 1): the session each snapshot is taken from / the slot it goes into -- in range and distinct, the kernels check nothing.
// Validate: result_dev[0] (preset to 0xffffffff) becomes the index of the first snapshot SessionBlobDefect refuses; info_dev
// [count] receives every snapshot's rate | has_clean << 31.
hipError_t LaunchGatherSessions(const SessionView &view, const int32_t *sessions_dev, int first, int count, void *blobs_dev, bool wide, hipStream_t stream);
hipError_t LaunchValidateSessions(const void *blobs_dev, int count, int fs_object, bool any_rate, uint32_t *result_dev, uint32_t *info_dev, hipStream_t stream);
hipError_t LaunchScatterSessions(const SessionView &view, const int32_t *slots_dev, int first, int count, const void *blobs_dev, bool wide, hipStream_t stream);
}  // namespace aecm
#endif

#endif  // AECM_AMD_SESSION_SNAPSHOT_H_
