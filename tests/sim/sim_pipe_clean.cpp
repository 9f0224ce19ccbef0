// TEST INFRASTRUCTURE -- a door for tests/test_pipelined_clean.py, built into tests/_build/libaecm_sim_pipe_clean.so on top of
// libaecm_sim.so (tests/pipe_clean_sim.py): ONE WORKGROUP of the pipelined kernel for launches with a clean near-end input
// (aecm_pipelined_body.inc: kClean) on the lane simulator.  Four streams whose state lives on between launches; a launch runs the
// roles of the sixteen-wave shape (front, delay, channel, gain, tail) or of the six-wave shape (front, back) in lock step, one
// "barrier" per step, with either order of producers and consumers inside a step.  With a clean input the three spectra travel
// from the front role to the others through BlockEngine::pack_clean_hand_over / unpack_clean_hand_over -- the functions the kernel
// calls on both sides of its PipeCleanSlot -- and the clean input's last block reaches the role that stores V_OUTBUF the way the
// kernel does it: the front role leaves it in a row of its own in its last, otherwise empty step, the storing role picks it up
// behind the launch's last barrier.  Without a clean input the same roles run the two-signal block and c_old stays what it was.
#include <stdint.h>
#include <string.h>

#include <vector>

#include "wave_sim.h"
#include "aecm_host_state.h"
#include "aecm_wave.h"

using namespace aecm;

namespace {
constexpr int kStreams = 4;

struct Stream {
    StreamImage img;
    std::vector<uint16_t> hist = std::vector<uint16_t>(kHistWordsPerStream, 0);
};
struct Workgroup {
    Stream s[kStreams];
};

// One launch of one stream's roles; every stream of the workgroup is stepped by the caller's loop, step by step.
template <bool kClean>
struct Roles {
    using E = BlockEngine<SimWave, kClean>;
    struct Slot {
        typename E::Spectrum xf, df;          // without a clean input: the spectra as they are (PipeSlot carries what the roles read of them)
        typename E::CleanHandOver packed;     // with one: the packed hand-over, and nothing else
    };
    Stream &st;
    const bool deep;
    const int n_blocks, n_slots;
    typename E::StridedIo sio;
    typename E::Regs rf, rd, rc, rg, rt;      // front, delay, channel (or back), gain, tail
    VecI x_old, d_old, c_prev, ovl, c_old;
    VecI c_last;                              // the kernel's PipeCleanLast row of this stream
    bool c_last_written = false;
    int hist_pos = 0;
    Slot slots[4];
    int delays[2] = {0, 0};
    VecI far_rows[2];
    typename E::GainInput gains[2];
    typename E::TailInput tails[2];
    int barriers[5] = {0, 0, 0, 0, 0};

    Roles(Stream &stream, bool deep_shape, int blocks, const IoView &io, int64_t base)
        : st(stream), deep(deep_shape), n_blocks(blocks), n_slots(deep_shape ? 4 : 2), sio{io, base} {
        for (typename E::Regs *r : {&rf, &rd, &rc, &rg, &rt}) E::init_lane_constants(*r, nullptr);
        uint32_t *vec = st.img.vec.data();
        int32_t *scal = st.img.scal.data();
        E::load_time_state(vec, rf.lane, x_old, d_old);
        if (kClean) {                                                     // the front wave's half of V_OUTBUF's word
            VecI unused;
            E::load_tail_state(vec, rf.lane, unused, c_prev);
        }
        E::load_state(rc, vec, scal);
        if (deep) {
            E::load_delay_state(rd, vec, scal);
            hist_pos = scal[S_HISTPOS];
            rd.u.fixed_delay = scal[S_FIXED_DELAY];
            E::load_state(rg, vec, scal);
            E::load_tail_state(vec, rt.lane, ovl, c_old);
        }
    }
    bool has(int b) const { return b >= 0 && b < n_blocks; }
    // what a role behind the front reads of a slot
    void read(const Slot &sl, typename E::Spectrum &xf, typename E::Spectrum &df, typename E::Spectrum &cf) const {
        if (kClean) {
            E::unpack_clean_hand_over(sl.packed, xf, df, cf);
        } else {
            xf = sl.xf;
            df = sl.df;
            cf = sl.df;
        }
    }
    void front(int b) {
        if (has(b)) {
            const VecI far_new = sio.far(rf, b), near_new = sio.near(rf, b);
            Slot &sl = slots[b % n_slots];
            typename E::Spectrum cf;
            if (kClean) {
                const VecI clean_new = sio.clean(rf, b);
                typename E::Spectrum xf, df;
                E::front_block(rf, x_old, far_new, d_old, near_new, c_prev, clean_new, xf, df, cf);
                sl.packed = E::pack_clean_hand_over(xf, df, cf);
                c_prev = clean_new;
            } else {
                E::front_block(rf, x_old, far_new, d_old, near_new, VecI(0), VecI(0), sl.xf, sl.df, cf);
            }
            x_old = far_new;
            d_old = near_new;
        } else if (kClean && b == n_blocks) {                            // the front wave's last step
            c_last = c_prev;
            c_last_written = true;
        }
        barriers[0] += 1;
    }
    void delay(int b) {
        if (has(b)) {
            typename E::Spectrum xf, df, cf;
            read(slots[b % n_slots], xf, df, cf);
            const int estimate = E::delay_block(rd, xf, df);
            delays[b & 1] = estimate;
            hist_pos = hist_pos + 1 >= kHistory ? 0 : hist_pos + 1;
            const int d = E::effective_delay(rd.u, estimate);
            if (d != 0) {
                if (d == 1 && b > 0) {
                    typename E::Spectrum pxf, pdf, pcf;
                    read(slots[(b - 1) % n_slots], pxf, pdf, pcf);
                    far_rows[b & 1] = pxf.mag;
                } else {
                    far_rows[b & 1] = SimWave::load_u16(st.hist.data() + E::aligned_slot(hist_pos, d) * kLanes, rd.lane);
                }
            }
        }
        barriers[1] += 1;
    }
    void channel(int b) {
        if (has(b)) {
            typename E::Spectrum xf, df, cf;
            read(slots[b % n_slots], xf, df, cf);
            E::update_startup(rc.u);
            E::track_q(rc.u, df, cf);
            gains[b & 1] = E::template channel_block<true>(rc, st.hist.data(), xf, df, delays[b & 1], far_rows[b & 1]);
        }
        barriers[2] += 1;
    }
    void gain(int b) {
        if (has(b)) {
            typename E::Spectrum xf, df, cf;
            read(slots[b % n_slots], xf, df, cf);
            E::track_q(rg.u, df, cf);
            tails[b & 1] = E::gain_block(rg, df, cf, gains[b & 1]);
        }
        barriers[3] += 1;
    }
    void tail(int b) {
        if (has(b)) {
            const typename E::TailInput &t = tails[b & 1];
            rt.out_ovl = ovl;
            const VecI o = E::tail_block(rt, t.a, t.b, t.clean_q);
            ovl = rt.out_ovl;
            sio.out(rt, b, o);
        }
        barriers[4] += 1;
    }
    void back(int b) {                                                    // the six-wave shape's back wave
        if (has(b)) {
            typename E::Spectrum xf, df, cf;
            read(slots[b % n_slots], xf, df, cf);
            E::update_startup(rc.u);
            const typename E::TailInput t = E::template middle_block<false>(rc, st.hist.data(), xf, df, cf, 0, VecI(0));
            const VecI o = E::tail_block(rc, t.a, t.b, t.clean_q);
            sio.out(rc, b, o);
        }
        barriers[2] += 1;
    }
    // behind the last barrier: every role stores its part of the state.  false: the hand-over of c_old was not there.
    bool store() {
        uint32_t *vec = st.img.vec.data();
        int32_t *scal = st.img.scal.data();
        if (kClean && !c_last_written) return false;
        if (deep) {
            rc.b.echo_filt = rg.b.echo_filt; rc.b.near_filt = rg.b.near_filt; rc.b.low_ctr = rg.b.low_ctr; rc.b.high_ctr = rg.b.high_ctr;
            rc.b.noise_est = rg.b.noise_est;
            rc.u.seed = rg.u.seed; rc.u.sup_gain = rg.u.sup_gain; rc.u.sup_gain_old = rg.u.sup_gain_old; rc.u.noise_ctr = rg.u.noise_ctr;
            rc.b64.echo_filt = rg.b64.echo_filt; rc.b64.near_filt = rg.b64.near_filt; rc.b64.noise_est = rg.b64.noise_est;
            rc.b64.low_ctr = rg.b64.low_ctr; rc.b64.high_ctr = rg.b64.high_ctr;
            E::template store_state<false, false, false>(rc, vec, scal);
            E::store_time_state(vec, rf.lane, x_old, d_old);
            if (kClean) c_old = c_last;
            E::store_tail_state(vec, rt.lane, ovl, c_old);
            E::store_delay_state(rd, vec, scal);
        } else {
            if (kClean) rc.c_old = c_last;
            E::template store_state<false, true, true>(rc, vec, scal);
            E::store_time_state(vec, rf.lane, x_old, d_old);
        }
        return true;
    }
};

template <bool kClean>
int Launch(Workgroup &wg, bool deep, int order, int n_blocks, int64_t stride, const int16_t *far_s, const int16_t *near_s, const int16_t *clean_s,
           int16_t *out) {
    const IoView io{far_s, near_s, clean_s, out, stride, kBlock};
    std::vector<Roles<kClean>> r;
    r.reserve(kStreams);
    for (int k = 0; k < kStreams; ++k) r.emplace_back(wg.s[k], deep, n_blocks, io, (int64_t)k * stride);
    const int steps = n_blocks + (deep ? 4 : 1);
    for (int step = 0; step < steps; ++step) {
        for (int i = 0; i < kStreams; ++i) {
            Roles<kClean> &x = r[order == 0 ? i : kStreams - 1 - i];
            if (deep) {
                if (order == 0) { x.tail(step - 4); x.gain(step - 3); x.channel(step - 2); x.delay(step - 1); x.front(step); }
                else { x.front(step); x.delay(step - 1); x.channel(step - 2); x.gain(step - 3); x.tail(step - 4); }
            } else {
                if (order == 0) { x.back(step - 1); x.front(step); }
                else { x.front(step); x.back(step - 1); }
            }
        }
    }
    for (int k = 0; k < kStreams; ++k) {
        if (!r[k].store()) return -1;
        for (int role : {0, 2})
            if (r[k].barriers[role] != steps) return -1;
        if (deep)
            for (int role : {1, 3, 4})
                if (r[k].barriers[role] != steps) return -1;
    }
    return steps;
}
}  // namespace

extern "C" {

// cng / echo_mode: [4].  NULL for bad parameters.
void *sim_pipe_clean_create(int fs, const int32_t *cng, const int32_t *echo_mode) {
    Workgroup *wg = new Workgroup();
    for (int k = 0; k < kStreams; ++k) {
        if (!BuildInitImage(fs, &wg->s[k].img) || !ApplyConfig(wg->s[k].img.scal.data(), cng[k], echo_mode[k])) {
            delete wg;
            return nullptr;
        }
    }
    return wg;
}
void sim_pipe_clean_free(void *h) { delete (Workgroup *)h; }

// One launch of n_blocks blocks: far / near / clean / out [4][stride]; clean may be NULL (a launch without a clean input).
// deep != 0: the role set of the sixteen-wave shape, else of the six-wave shape.  order 0: consumers first inside a step, 1: producers
// first.  Returns the barriers every role executed (-1: not all the same number, or c_old's hand-over was missing), -2: bad arguments.
int32_t sim_pipe_clean_launch(void *h, int deep, int order, int n_blocks, int64_t stride, const int16_t *far_s, const int16_t *near_s,
                              const int16_t *clean_s, int16_t *out) {
    if (!h || n_blocks <= 0 || (int64_t)n_blocks * kBlock > stride || !far_s || !near_s || !out) return -2;
    Workgroup &wg = *(Workgroup *)h;
    return clean_s ? Launch<true>(wg, deep != 0, order, n_blocks, stride, far_s, near_s, clean_s, out)
                   : Launch<false>(wg, deep != 0, order, n_blocks, stride, far_s, near_s, nullptr, out);
}

void sim_pipe_clean_digests(void *h, uint32_t *digests) {
    Workgroup &wg = *(Workgroup *)h;
    for (int k = 0; k < kStreams; ++k)
        ComputeDigest(wg.s[k].img.vec.data(), wg.s[k].img.scal.data(), wg.s[k].hist.data(), digests + (size_t)k * kDigestWords);
}

}  // extern "C"
