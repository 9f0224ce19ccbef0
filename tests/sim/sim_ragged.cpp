// TEST INFRASTRUCTURE -- doors for tests/test_ragged.py, built into tests/_build/libaecm_sim_ragged.so on top of libaecm_sim.so
// (tests/ragged_sim.py): the recording schedule as arrays, and the ragged twin of sim_recordings (sim_engine.cpp) -- the
// procedure of BatchEngine::ProcessRecordingsRagged in aecm_engine.cpp with host loops instead of kernels: one common
// schedule, every stream its first blocks_after_call[calls - 1] blocks, the output assembled up to calls x frame, zeros behind.
#include <stdint.h>

#include <vector>

#include "aecm_engine.h"
#include "aecm_session_flow.h"

using namespace aecm;

extern "C" {

// Arrays sized by the caller: far_map / near_map cap_blocks x 64, out_map n_calls x frame, the per-call arrays n_calls.
// Returns the blocks of the schedule, or -1 when they do not fit cap_blocks.  *code: what the whole recording returns.
int32_t sim_schedule(int fs, int frame, int n_calls, int ms, int cap_blocks, int32_t *far_map, int32_t *near_map, int32_t *out_map,
                     int32_t *blocks_after_call, int32_t *code_after_call, int32_t *code) {
    const RecordingSchedule sch = BuildRecordingSchedule(fs, frame, n_calls, (int16_t)ms);
    if (sch.n_blocks > cap_blocks || (int)sch.blocks_after_call.size() != n_calls) return -1;
    for (size_t i = 0; i < sch.far_map.size(); ++i) far_map[i] = sch.far_map[i], near_map[i] = sch.near_map[i];
    for (size_t i = 0; i < sch.out_map.size(); ++i) out_map[i] = sch.out_map[i];
    for (int c = 0; c < n_calls; ++c) blocks_after_call[c] = sch.blocks_after_call[c], code_after_call[c] = sch.code_after_call[c];
    *code = sch.first_error ? sch.first_error : sch.warned ? kWarnBadParameter : 0;
    return sch.n_blocks;
}

int32_t sim_recordings_ragged(int n_streams, int n_samples, int fs, int frame, int cng, int echo_mode, int ms, const int16_t *far,
                              const int16_t *near, const int16_t *clean, const int32_t *calls, int16_t *out, int32_t *codes) {
    const int n_calls = n_samples / frame;
    const RecordingSchedule sch = BuildRecordingSchedule(fs, frame, n_calls, (int16_t)ms);
    if ((int)sch.blocks_after_call.size() != n_calls) return -1;
    int32_t rc = 0;
    const int16_t *pass = clean ? clean : near;
    for (int s = 0; s < n_streams; ++s) {
        const int k = calls[s];
        if (k < 0 || k > n_calls) return -1;
        const int len = k > 0 ? sch.blocks_after_call[k - 1] : 0;
        codes[s] = k > 0 ? sch.code_after_call[k - 1] : 0;
        if (rc == 0) rc = codes[s];
        const int64_t n_blk = (int64_t)len * kBlock, row = (int64_t)s * n_samples;
        std::vector<int16_t> bfar(n_blk + 1), bnear(n_blk + 1), bclean(n_blk + 1), bout(n_blk + 1, 0);
        for (int64_t j = 0; j < n_blk; ++j) {
            bfar[j] = sch.far_map[j] >= 0 ? far[row + sch.far_map[j]] : 0;
            bnear[j] = sch.near_map[j] >= 0 ? near[row + sch.near_map[j]] : 0;
            if (clean) bclean[j] = sch.near_map[j] >= 0 ? clean[row + sch.near_map[j]] : 0;
        }
        if (len > 0) {
            BatchEngine *e = BatchEngine::Create(1, 0);           // one stream of the simulated engine, its own length
            e->Init(fs);
            e->SetConfig(cng, echo_mode, 0, 1);
            IoView io{bfar.data(), bnear.data(), clean ? bclean.data() : nullptr, bout.data(), n_blk, kBlock};
            e->ProcessBlocksHost(io, len);
            delete e;
        }
        for (int64_t j = 0; j < n_samples; ++j) {
            const int32_t v = j < (int64_t)n_calls * frame ? sch.out_map[j] : -1;
            int16_t r = 0;
            if (j < (int64_t)k * frame) {
                if (v >= 0) r = v < n_blk ? bout[v] : (int16_t)0;     // (never beyond the stream's own blocks: the prefix property)
                else if (v <= -2) r = pass[row + (-(int64_t)v - 2)];
            }
            out[row + j] = r;
        }
    }
    return rc;
}

}  // extern "C"
