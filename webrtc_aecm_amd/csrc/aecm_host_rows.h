// Host audio on its way to the device and back: the caller's strided rows against the dense planes the host launches stage them
// in.  Pure host logic, no device (tests/test_host_rows.py runs it as a program of its own under sanitizers); BatchEngine's mapped
// path, chunked pipeline and ragged host form (aecm_engine.cpp) are written on top of it.
#ifndef AECM_AMD_HOST_ROWS_H_
#define AECM_AMD_HOST_ROWS_H_

#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "aecm_state.h"

namespace aecm {

// The caller's side of one plane (far, near, clean or out; IoView's strides): block b of stream s starts at
// s * stream_stride + b * block_stride.  The dense side is [streams][blocks * 64].
struct RowLayout {
    int streams = 0, blocks = 0;
    int64_t stream_stride = 0, block_stride = 0;
    size_t row() const { return (size_t)blocks * kBlock; }          // samples of a dense row
    size_t per() const { return (size_t)streams * row(); }          // samples of a dense plane
    // the caller's plane IS the dense plane: copied as one piece, and what the chunked pipeline of ProcessBlocksHost asks for
    bool dense() const { return block_stride == kBlock && stream_stride == (int64_t)blocks * kBlock; }
};

// The 64-sample blocks of a caller's plane into a dense plane, and back.  lens (may be null: every stream has all its blocks)
// limits stream s to its first lens[s] blocks; nothing else is read or written on either side -- pad samples, and blocks at or
// beyond a stream's length, stay as they are.
inline void PackRows(const RowLayout &l, const int16_t *strided, int16_t *dense, const int32_t *lens = nullptr) {
    for (int s = 0; s < l.streams; ++s)
        for (int b = 0, n = lens ? lens[s] : l.blocks; b < n; ++b)
            memcpy(dense + (size_t)s * l.row() + (size_t)b * kBlock, strided + s * l.stream_stride + b * l.block_stride, kBlock * sizeof(int16_t));
}
inline void UnpackRows(const RowLayout &l, const int16_t *dense, int16_t *strided, const int32_t *lens = nullptr) {
    for (int s = 0; s < l.streams; ++s)
        for (int b = 0, n = lens ? lens[s] : l.blocks; b < n; ++b)
            memcpy(strided + s * l.stream_stride + b * l.block_stride, dense + (size_t)s * l.row() + (size_t)b * kBlock, kBlock * sizeof(int16_t));
}

// The dense planes of one host launch on one base pointer: far | near | [clean] | out, `per` samples each, rows of `row` samples.
// (base + an offset into the far plane: the view of the streams from there on, as the chunked pipeline takes them.)
inline size_t StagedSamples(size_t per, bool has_clean) { return per * (has_clean ? 4 : 3); }
inline IoView StagedIo(int16_t *base, size_t row, size_t per, bool has_clean) {
    return IoView{base, base + per, has_clean ? base + 2 * per : nullptr, base + (has_clean ? 3 : 2) * per, (int64_t)row, kBlock};
}

}  // namespace aecm
#endif  // AECM_AMD_HOST_ROWS_H_
