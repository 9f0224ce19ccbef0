// TEST INFRASTRUCTURE -- the door of tests/test_block_trace.py, built into tests/_build/libaecm_sim_trace.so on top of
// libaecm_sim.so (tests/trace_sim.py): BlockEngine::run_stream_traced (aecm_wave.h) -- the block loop of the traced kernels
// (aecm_trace_kernels.hip), its record assembly and its index arithmetic -- on the 64-lane CPU simulator, launched the way those
// kernels launch it: one run per stream, or one run per (chunk, stream) item with the state stored and reloaded in between.
#include <stdint.h>

#include "wave_sim.h"
#include "sim_stream.h"
#include "aecm_wave.h"

using namespace aecm;

namespace {
// The simulator's policy with the one primitive the trace adds (wave_gfx950.h: store_out_u32_if -- a plain masked store).
struct TraceSimWave : SimWave {
    static void store_out_u32_if(const VecB &m, uint32_t *p, const vi &idx, const vi &val) { store_u32_if(m, p, idx, val); }
};

template <bool kHasClean>
void RunItem(SimStream *s, const IoView &io, const TraceView &tv, int64_t pos, int first, int nb) {
    using E = BlockEngine<TraceSimWave, kHasClean>;
    StatePtrs st{s->img.vec.data(), s->img.scal.data(), s->hist.data(), nullptr};
    typename E::TracedIo tio = E::traced_io(io, tv, pos, first);
    E::run_stream_traced(st, tio, 0, nb);
}
}  // namespace

extern "C" {

// One traced launch over the streams behind `handles` (sim_create): the stream at position s runs lens[s] blocks (lens NULL:
// n_blocks each).  chunk_blocks <= 0: one run per stream (aecm_trace_process_kernel); else runs of at most chunk_blocks blocks,
// chunk-major like the queue's items (aecm_trace_queue_kernel, aecm_trace_ragged_queue_kernel).  Audio and trace by their views
// (strides in samples resp. records); clean may be NULL.  Returns the number of records written.
int64_t sim_trace_launch(void **handles, int n_streams, const int32_t *lens, int n_blocks, int chunk_blocks, const int16_t *far_s, const int16_t *near_s,
                         const int16_t *clean, int16_t *out, int64_t stream_stride, int64_t block_stride, uint32_t *records,
                         int64_t trace_stream_stride, int64_t trace_block_stride) {
    const IoView io{far_s, near_s, clean, out, stream_stride, block_stride};
    const TraceView tv{records, trace_stream_stride, trace_block_stride};
    const int chunk = chunk_blocks > 0 ? chunk_blocks : (n_blocks > 0 ? n_blocks : 1);
    int64_t written = 0;
    for (int first = 0; first < n_blocks; first += chunk)
        for (int s = 0; s < n_streams; ++s) {
            const int len = lens ? lens[s] : n_blocks;
            const int nb = len - first < chunk ? len - first : chunk;
            if (nb <= 0) continue;
            if (clean) RunItem<true>((SimStream *)handles[s], io, tv, s, first, nb);
            else RunItem<false>((SimStream *)handles[s], io, tv, s, first, nb);
            written += nb;
        }
    return written;
}

}  // extern "C"
