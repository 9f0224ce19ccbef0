// TEST INFRASTRUCTURE -- part of tests/_build/libaecm_sim.so: ONE WORKGROUP of the pipelined kernels' body
// (webrtc_aecm_amd/csrc/aecm_pipelined_body.inc, all three of its forms) on the lane simulator.  Up to four slots, each a sim_create
// stream with a length of its own; the roles of the sixteen-wave shape (front, delay, channel, gain, tail -- each with registers of
// its own, one step apart) or of the six-wave shape (front, back) march in lock step: the SAME BlockEngine functions, the same
// state ownership (which role loads and stores what), the same slot rings and the same rule for the far-history row.  The
// workgroup's steps are counted by the LONGEST of its lengths; in a step a role works for its slot only while the block it is at
// lies below the slot's own length (the kernel's "blk < len"; equal lengths are the special case), and every role executes one
// "barrier" per step.  order 0: inside a step the consumers run first (what a barrier guarantees: nobody sees this step's
// writes); order 1: the producers run first -- a role that read something written in the same step would now see other data, so
// the two orders (and the plain engine) must agree.
// Between the roles travel the words the kernel's LDS slots hold and nothing else, through the functions the kernel calls on both
// sides of them: pack_ / unpack_hand_over or, with a clean input, pack_ / unpack_clean_hand_over for the spectra, and pack_ /
// unpack_gain_state for the gain role's part of the state.  With a clean input its last block reaches the role that stores
// V_OUTBUF as in the kernel: the front role leaves it in a row of its own in the workgroup's last, otherwise empty step.
#include <stdint.h>

#include <algorithm>
#include <type_traits>
#include <vector>

#include "wave_sim.h"
#include "sim_stream.h"
#include "aecm_wave.h"

using namespace aecm;

namespace {
constexpr int kSlotsPerWorkgroup = 4;

// The roles of one slot; the workgroup's loop steps every slot's, step by step.
template <bool kClean>
struct Roles {
    using E = BlockEngine<SimWave, kClean>;
    using Spectrum = typename E::Spectrum;
    using Packed = typename std::conditional<kClean, typename E::CleanHandOver, typename E::HandOver>::type;
    SimStream *const st;                      // null: an empty slot
    const bool deep;
    const int len, longest, n_slots;
    typename E::StridedIo sio;
    typename E::Regs rf, rd, rc, rg, rt;      // front, delay, channel (or back), gain, tail
    VecI x_old, d_old, c_prev, ovl, c_old;
    VecI c_last;                              // the kernel's PipeCleanLast row of this slot
    bool c_last_written = false;
    int hist_pos = 0;
    Packed slots[4];
    int delays[2] = {0, 0};
    VecI far_rows[2];
    typename E::GainInput gains[2];
    typename E::TailInput tails[2];
    int barriers[5] = {0, 0, 0, 0, 0};
    int64_t hand_over_writes = 0, out_blocks = 0, input_rows = 0;

    Roles(SimStream *stream, bool deep_shape, int blocks, int longest_of_the_workgroup, const IoView &io, int64_t base)
        : st(blocks > 0 ? stream : nullptr), deep(deep_shape), len(blocks), longest(longest_of_the_workgroup), n_slots(deep_shape ? 4 : 2),
          sio{io, base} {
        for (typename E::Regs *r : {&rf, &rd, &rc, &rg, &rt}) E::init_lane_constants(*r, nullptr);
        if (!st) return;                                                  // an empty or zero-length slot: neither state nor rows are touched
        uint32_t *vec = st->img.vec.data();
        int32_t *scal = st->img.scal.data();
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
    // a role's test: "this slot's stream still has the block this role works on in this step"
    bool has(int b) const { return st && b >= 0 && b < len; }
    // what a role behind the front reads of a slot
    static void read(const typename E::CleanHandOver &h, Spectrum &xf, Spectrum &df, Spectrum &cf) { E::unpack_clean_hand_over(h, xf, df, cf); }
    static void read(const typename E::HandOver &h, Spectrum &xf, Spectrum &df, Spectrum &cf) {
        E::unpack_hand_over(h, xf, df);
        cf = df;
    }
    static Packed pack(const Spectrum &xf, const Spectrum &df, const Spectrum &cf) {
        if constexpr (kClean) return E::pack_clean_hand_over(xf, df, cf);
        else return E::pack_hand_over(xf, df);
    }
    void front(int b) {
        if (has(b)) {
            const VecI far_new = sio.far(rf, b), near_new = sio.near(rf, b);      // (never a row at or beyond the stream's length)
            const VecI clean_new = kClean ? sio.clean(rf, b) : VecI(0);
            input_rows += 1;
            Spectrum xf, df, cf;
            E::front_block(rf, x_old, far_new, d_old, near_new, c_prev, clean_new, xf, df, cf);
            slots[b % n_slots] = pack(xf, df, cf);
            hand_over_writes += 1;
            x_old = far_new;
            d_old = near_new;
            c_prev = clean_new;
        } else if (kClean && st && b == longest) {                       // the front wave's last step
            c_last = c_prev;
            c_last_written = true;
        }
        barriers[0] += 1;
    }
    void delay(int b) {
        if (has(b)) {
            Spectrum xf, df, cf;
            read(slots[b % n_slots], xf, df, cf);
            const int estimate = E::delay_block(rd, xf, df);
            delays[b & 1] = estimate;
            hist_pos = hist_pos + 1 >= kHistory ? 0 : hist_pos + 1;
            const int d = E::effective_delay(rd.u, estimate);
            if (d != 0) {
                if (d == 1 && b > 0) {
                    Spectrum pxf, pdf, pcf;
                    read(slots[(b - 1) % n_slots], pxf, pdf, pcf);
                    far_rows[b & 1] = pxf.mag;
                } else {
                    far_rows[b & 1] = SimWave::load_u16(st->hist.data() + E::aligned_slot(hist_pos, d) * kLanes, rd.lane);
                }
            }
        }
        barriers[1] += 1;
    }
    void channel(int b) {
        if (has(b)) {
            Spectrum xf, df, cf;
            read(slots[b % n_slots], xf, df, cf);
            E::update_startup(rc.u);
            E::track_q(rc.u, df, cf);
            gains[b & 1] = E::template channel_block<true>(rc, st->hist.data(), xf, df, delays[b & 1], far_rows[b & 1]);
        }
        barriers[2] += 1;
    }
    void gain(int b) {
        if (has(b)) {
            Spectrum xf, df, cf;
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
            out_blocks += 1;
        }
        barriers[4] += 1;
    }
    void back(int b) {                                                    // the six-wave shape's back wave: everything behind the transforms
        if (has(b)) {
            Spectrum xf, df, cf;
            read(slots[b % n_slots], xf, df, cf);
            E::update_startup(rc.u);
            const typename E::TailInput t = E::template middle_block<false>(rc, st->hist.data(), xf, df, cf, 0, VecI(0));
            const VecI o = E::tail_block(rc, t.a, t.b, t.clean_q);
            sio.out(rc, b, o);
            out_blocks += 1;
        }
        barriers[2] += 1;
    }
    // behind the last barrier: every role stores its part of the state, once.  false: the hand-over of c_old was not there.
    bool store() {
        if (!st) return true;
        uint32_t *vec = st->img.vec.data();
        int32_t *scal = st->img.scal.data();
        if (kClean && !c_last_written) return false;
        if (deep) {
            E::unpack_gain_state(E::pack_gain_state(rg), rc);             // the gain wave's part goes to the channel wave, which stores the state
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
int Launch(SimStream *const *streams, const int32_t *lens, bool deep, int order, const IoView &io, int64_t *counts) {
    const int longest = *std::max_element(lens, lens + kSlotsPerWorkgroup);
    std::vector<Roles<kClean>> r;
    r.reserve(kSlotsPerWorkgroup);
    for (int k = 0; k < kSlotsPerWorkgroup; ++k) r.emplace_back(streams[k], deep, lens[k], longest, io, (int64_t)k * io.stream_stride);
    const int steps = longest + (deep ? 4 : 1);
    for (int step = 0; step < steps; ++step) {
        for (int i = 0; i < kSlotsPerWorkgroup; ++i) {
            Roles<kClean> &x = r[order == 0 ? i : kSlotsPerWorkgroup - 1 - i];
            if (deep) {                                                   // front: block step, delay: step - 1, channel: - 2, gain: - 3, tail: - 4
                if (order == 0) { x.tail(step - 4); x.gain(step - 3); x.channel(step - 2); x.delay(step - 1); x.front(step); }
                else { x.front(step); x.delay(step - 1); x.channel(step - 2); x.gain(step - 3); x.tail(step - 4); }
            } else {
                if (order == 0) { x.back(step - 1); x.front(step); }
                else { x.front(step); x.back(step - 1); }
            }
        }
    }
    bool ok = true;
    for (int k = 0; k < kSlotsPerWorkgroup; ++k) {
        ok = r[k].store() && ok;
        for (int role = 0; role < 5; ++role)
            if ((deep || role == 0 || role == 2) && r[k].barriers[role] != steps) ok = false;
        if (counts) {
            counts[k * 3 + 0] = r[k].hand_over_writes;
            counts[k * 3 + 1] = r[k].out_blocks;
            counts[k * 3 + 2] = r[k].input_rows;
        }
    }
    return ok ? steps : -1;
}
}  // namespace

extern "C" {

// One launch of one workgroup.  streams[4]: sim_create handles (state lives in them: launches continue one another and alternate with
// sim_process), null = an empty slot; lens[4]: blocks per slot (0: the slot touches nothing).  far / near / clean / out:
// [4][stride] samples, clean may be NULL (a launch without a clean input).  deep != 0: the role set of the sixteen-wave shape, else
// of the six-wave shape.  counts[4][3] (may be NULL): per slot, hand-over slots written by its front role, output blocks written,
// input rows loaded.  Returns the steps every role executed (-1: not all the same number, or c_old's hand-over was missing), -2:
// bad arguments.
int32_t sim_roles_launch(void *const *streams, const int32_t *lens, int deep, int order, int64_t stride, const int16_t *far_s, const int16_t *near_s,
                         const int16_t *clean_s, int16_t *out, int64_t *counts) {
    if (!streams || !lens || !far_s || !near_s || !out) return -2;
    for (int k = 0; k < kSlotsPerWorkgroup; ++k) {
        if (lens[k] < 0 || (int64_t)lens[k] * kBlock > stride || (lens[k] > 0 && !streams[k])) return -2;
        for (int j = 0; j < k; ++j)
            if (streams[k] && streams[j] == streams[k]) return -2;
    }
    const IoView io{far_s, near_s, clean_s, out, stride, kBlock};
    SimStream *const *s = reinterpret_cast<SimStream *const *>(streams);
    return clean_s ? Launch<true>(s, lens, deep != 0, order, io, counts) : Launch<false>(s, lens, deep != 0, order, io, counts);
}

}  // extern "C"
