// TEST INFRASTRUCTURE -- builds tests/_build/libaecm_sim.so: the product's block-DSP source
// (webrtc_aecm_amd/csrc/aecm_wave.h) instantiated on the 64-lane CPU simulator policy.
#include <stdint.h>
#include <string.h>

#include <vector>

#include "wave_sim.h"
#include "sim_stream.h"
#include "aecm_wave.h"

using namespace aecm;

extern "C" {

void *sim_create(int fs, int cng_mode, int echo_mode) {
    SimStream *s = new SimStream();
    if (!BuildInitImage(fs, &s->img) || !ApplyConfig(s->img.scal.data(), cng_mode, echo_mode)) {
        delete s;
        return nullptr;
    }
    return s;
}
void sim_free(void *h) { delete (SimStream *)h; }
void sim_control(void *h, int fixed_delay, int nlp_flag) { ApplyControl(((SimStream *)h)->img.scal.data(), fixed_delay, nlp_flag); }
void sim_set_echo_path(void *h, const int16_t *path) {
    SimStream *s = (SimStream *)h;
    SetEchoPath(s->img.vec.data(), s->img.scal.data(), path);
}
void sim_get_echo_path(void *h, int16_t *path) {
    SimStream *s = (SimStream *)h;
    GetEchoPath(s->img.vec.data(), s->img.scal.data(), path);
}

// n_blocks consecutive blocks; clean may be NULL.
void sim_process(void *h, const int16_t *far_s, const int16_t *near_s, const int16_t *clean, int16_t *out, int n_blocks) {
    SimStream *s = (SimStream *)h;
    StatePtrs st{s->img.vec.data(), s->img.scal.data(), s->hist.data(), nullptr};
    IoView io{far_s, near_s, clean, out, 0, kBlock};
    if (clean) BlockEngine<SimWave, true>::run_stream(st, io, 0, n_blocks);
    else BlockEngine<SimWave, false>::run_stream(st, io, 0, n_blocks);
}

// The constants blob the HOST builds for the GPU kernels, next to the same quantities evaluated from
// their definitions in aecm_wave.h / the simulator policy (rows: LaneConstRow order, then twiddles).
void sim_constants(uint32_t *blob_out, uint32_t *defined_lane_rows, uint32_t *defined_twiddles) {
    std::vector<uint32_t> blob;
    BuildKernelConstants(&blob);
    memcpy(blob_out, blob.data(), blob.size() * 4);
    BlockEngine<SimWave, false>::Regs r;
    BlockEngine<SimWave, false>::init_lane_constants(r, nullptr);
    for (int k = 0; k < kLaneConstRows; ++k)
        for (int t = 0; t < kLanes; ++t) defined_lane_rows[k * kLanes + t] = (uint32_t)r.lc[k].v[t];
    VecI wre, wim;
    uint32_t *o = defined_twiddles;
    VecI nwre, nwim, sre, cre, sim_, cim;
#define SIM_TW(S) SimWave::inv_twiddles<S>(wre, wim, nwre, nwim); for (int t = 0; t < kLanes; ++t) { *o++ = (uint32_t)wre.v[t]; *o++ = (uint32_t)wim.v[t]; *o++ = (uint32_t)nwre.v[t]; *o++ = (uint32_t)nwim.v[t]; }
    SIM_TW(0) SIM_TW(1) SIM_TW(2) SIM_TW(3) SIM_TW(4) SIM_TW(5) SIM_TW(6)
#undef SIM_TW
#define SIM_FT(S) SimWave::fwd_twiddles<S>(wre, wim, nwre, nwim); for (int t = 0; t < kLanes; ++t) { *o++ = (uint32_t)wre.v[t]; *o++ = (uint32_t)wim.v[t]; *o++ = (uint32_t)nwre.v[t]; *o++ = (uint32_t)nwim.v[t]; }
    SIM_FT(1) SIM_FT(2) SIM_FT(3) SIM_FT(4) SIM_FT(5) SIM_FT(6)
#undef SIM_FT
#define SIM_FO(S) SimWave::fwd_offsets<S>(sre, cre, sim_, cim); for (int t = 0; t < kLanes; ++t) { *o++ = (uint32_t)sre.v[t]; *o++ = (uint32_t)cre.v[t]; *o++ = (uint32_t)sim_.v[t]; *o++ = (uint32_t)cim.v[t]; }
    SIM_FO(2) SIM_FO(4) SIM_FO(6)
#undef SIM_FO
}

// One 128-point transform of the kernel's fft128 on natural-order data (re/im in, re/im out): lane t
// starts with points t and t + 64 and ends with bins bitrev6(t) and bitrev6(t) + 64.  variant:
// 0 = forward of real input (im ignored), 1 = forward complex, 2 = inverse.  The last stage only
// produces what its caller consumes: forward -> im of bins >= 64 is not computed (returned as 0),
// inverse -> real parts only.  Returns the inverse transform's accumulated scale (0 for forward).
int sim_fft128(int16_t *re, int16_t *im, int variant) {
    using E = BlockEngine<SimWave, false>;
    VecI a, b;
    for (int t = 0; t < kLanes; ++t) {
        const int im_a = variant == 0 ? 0 : im[t], im_b = variant == 0 ? 0 : im[t + 64];
        a.v[t] = (re[t] & 0xffff) | (int)((unsigned)im_a << 16);
        b.v[t] = (re[t + 64] & 0xffff) | (int)((unsigned)im_b << 16);
    }
    int scale = 0;
    const VecI kp = SimWave::opaque_const(32770);
    if (variant == 0) scale = E::fft128<false, true>(a, b, kp);
    else if (variant == 1) scale = E::fft128<false, false>(a, b, kp);
    else {
        scale = E::fft128<true, false>(a, b, kp);
        for (int t = 0; t < kLanes; ++t) {          // the inverse transform hands its real parts on in the upper halves
            a.v[t] >>= 16;
            b.v[t] >>= 16;
        }
    }
    for (int t = 0; t < kLanes; ++t) {
        int r = 0;
        for (int k = 0; k < 6; ++k) r |= ((t >> k) & 1) << (5 - k);
        re[r] = (int16_t)a.v[t];
        re[r + 64] = (int16_t)b.v[t];
        im[r] = variant == 2 ? (int16_t)0 : (int16_t)(a.v[t] >> 16);
        im[r + 64] = 0;
    }
    return scale;
}

// The whole state image (aecm_state.h): vec kNumVec * 64 words, scal 64 words, hist kHistory * 64 uint16.
void sim_get_image(void *h, uint32_t *vec, int32_t *scal, uint16_t *hist) {
    SimStream *s = (SimStream *)h;
    memcpy(vec, s->img.vec.data(), s->img.vec.size() * 4);
    memcpy(scal, s->img.scal.data(), s->img.scal.size() * 4);
    memcpy(hist, s->hist.data(), s->hist.size() * 2);
}
void sim_set_image(void *h, const uint32_t *vec, const int32_t *scal, const uint16_t *hist) {
    SimStream *s = (SimStream *)h;
    memcpy(s->img.vec.data(), vec, s->img.vec.size() * 4);
    memcpy(s->img.scal.data(), scal, s->img.scal.size() * 4);
    memcpy(s->hist.data(), hist, s->hist.size() * 2);
}

void sim_digest(void *h, uint32_t *digest) {
    SimStream *s = (SimStream *)h;
    ComputeDigest(s->img.vec.data(), s->img.scal.data(), s->hist.data(), digest);
}

}  // extern "C"
