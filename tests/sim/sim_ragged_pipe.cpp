// TEST INFRASTRUCTURE -- a door for tests/test_ragged_pipelined.py, built into tests/_build/libaecm_sim_ragged_pipe.so on top of
// libaecm_sim.so (tests/ragged_pipe_sim.py): ONE WORKGROUP of the ragged pipelined kernel (aecm_pipelined_body.inc: kRagged) on the
// lane simulator.  Four slots, each with a stream and a length of its own (0 = empty slot); the roles of the sixteen-wave shape
// (front, delay, channel, gain, tail -- sim_lib.cpp: sim_process_roles, per slot) or of the six-wave shape (front, back) march in
// lock step: every role executes one "barrier" per step of the workgroup, the steps are counted by the LONGEST of the four lengths,
// and in a step a role works for a slot only while the block it is at lies below that slot's own length -- what the kernel's
// "blk < len" tests say.  A slot past its length writes no hand-over slot and no output; its state is stored once, at the end.
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "wave_sim.h"
#include "aecm_host_state.h"
#include "aecm_wave.h"

using namespace aecm;

namespace {
using E = BlockEngine<SimWave, false>;
constexpr int kStreams = 4;

struct Slot { E::Spectrum xf, df; };
struct SlotState {                        // one slot of the workgroup: its stream, its roles' registers, its hand-over rings
    int len = 0;
    StreamImage img;
    std::vector<uint16_t> hist = std::vector<uint16_t>(kHistWordsPerStream, 0);
    E::Regs rf, rd, rc, rg, rt;           // front, delay, channel (or back), gain, tail
    VecI x_old, d_old, ovl, c_old;
    int hist_pos = 0;
    Slot slots[4];
    int delays[2] = {0, 0};
    VecI far_rows[2];
    E::GainInput gains[2];
    E::TailInput tails[2];
    int64_t hand_over_writes = 0, out_blocks = 0, input_rows = 0;
};
}  // namespace

extern "C" {

// far / near / out: [4][stride] samples.  deep != 0: the role set of the sixteen-wave shape, else of the six-wave shape.
// order: as sim_process_roles (0 = consumers first inside a step, 1 = producers first).  digests: [4][kDigestWords].
// counts[4][3]: per slot, hand-over slots written by its front role, output blocks written, input rows loaded.
// Returns the barriers every role executed (all roles the same number, or -1), -2 for bad arguments.
int32_t sim_ragged_pipe_workgroup(int fs, int cng, int echo_mode, int deep, int order, const int32_t *lens, int64_t stride, const int16_t *far_s,
                                  const int16_t *near_s, int16_t *out, uint32_t *digests, int64_t *counts) {
    std::vector<SlotState> wg(kStreams);
    int longest = 0;
    for (int k = 0; k < kStreams; ++k) {
        SlotState &s = wg[k];
        s.len = lens[k];
        if (s.len < 0 || (int64_t)s.len * kBlock > stride) return -2;
        longest = std::max(longest, s.len);
        if (!BuildInitImage(fs, &s.img) || !ApplyConfig(s.img.scal.data(), cng, echo_mode)) return -2;
        for (E::Regs *r : {&s.rf, &s.rd, &s.rc, &s.rg, &s.rt}) E::init_lane_constants(*r, nullptr);
        if (s.len == 0) continue;                                         // an empty slot: neither state nor rows are touched
        uint32_t *vec = s.img.vec.data();
        int32_t *scal = s.img.scal.data();
        E::load_time_state(vec, s.rf.lane, s.x_old, s.d_old);
        E::load_state(s.rc, vec, scal);
        if (deep) {
            E::load_delay_state(s.rd, vec, scal);
            s.hist_pos = scal[S_HISTPOS];
            s.rd.u.fixed_delay = scal[S_FIXED_DELAY];
            E::load_state(s.rg, vec, scal);
            E::load_tail_state(vec, s.rt.lane, s.ovl, s.c_old);
        }
    }
    const int kSlots = deep ? 4 : 2;
    const IoView io{far_s, near_s, nullptr, out, stride, kBlock};
    auto io_of = [&](int k) { return E::StridedIo{io, (int64_t)k * stride}; };
    // a role's test: "this slot's stream still has the block this role works on in this step"
    auto has = [&](const SlotState &s, int b) { return b >= 0 && b < s.len; };
    auto front = [&](int k, int b) {
        SlotState &s = wg[k];
        if (!has(s, b)) return;
        E::StridedIo sio = io_of(k);
        const VecI far_new = sio.far(s.rf, b), near_new = sio.near(s.rf, b);      // (never a row at or beyond the stream's length)
        s.input_rows += 1;
        E::Spectrum cf;
        Slot &sl = s.slots[b % kSlots];
        E::front_block(s.rf, s.x_old, far_new, s.d_old, near_new, VecI(0), VecI(0), sl.xf, sl.df, cf);
        s.hand_over_writes += 1;
        s.x_old = far_new;
        s.d_old = near_new;
    };
    auto delay = [&](int k, int b) {
        SlotState &s = wg[k];
        if (!has(s, b)) return;
        const Slot &sl = s.slots[b % kSlots];
        const int estimate = E::delay_block(s.rd, sl.xf, sl.df);
        s.delays[b & 1] = estimate;
        s.hist_pos = s.hist_pos + 1 >= kHistory ? 0 : s.hist_pos + 1;
        const int d = E::effective_delay(s.rd.u, estimate);
        if (d != 0) {
            if (d == 1 && b > 0) s.far_rows[b & 1] = s.slots[(b - 1) % kSlots].xf.mag;
            else s.far_rows[b & 1] = SimWave::load_u16(s.hist.data() + E::aligned_slot(s.hist_pos, d) * kLanes, s.rd.lane);
        }
    };
    auto channel = [&](int k, int b) {
        SlotState &s = wg[k];
        if (!has(s, b)) return;
        const Slot &sl = s.slots[b % kSlots];
        E::update_startup(s.rc.u);
        E::track_q(s.rc.u, sl.df, sl.df);
        s.gains[b & 1] = E::channel_block<true>(s.rc, s.hist.data(), sl.xf, sl.df, s.delays[b & 1], s.far_rows[b & 1]);
    };
    auto gain = [&](int k, int b) {
        SlotState &s = wg[k];
        if (!has(s, b)) return;
        const Slot &sl = s.slots[b % kSlots];
        E::track_q(s.rg.u, sl.df, sl.df);
        s.tails[b & 1] = E::gain_block(s.rg, sl.df, sl.df, s.gains[b & 1]);
    };
    auto tail = [&](int k, int b) {
        SlotState &s = wg[k];
        if (!has(s, b)) return;
        const E::TailInput &t = s.tails[b & 1];
        s.rt.out_ovl = s.ovl;
        const VecI o = E::tail_block(s.rt, t.a, t.b, t.clean_q);
        s.ovl = s.rt.out_ovl;
        E::StridedIo sio = io_of(k);
        sio.out(s.rt, b, o);
        s.out_blocks += 1;
    };
    auto back = [&](int k, int b) {                                       // the six-wave shape's back wave: everything behind the transforms
        SlotState &s = wg[k];
        if (!has(s, b)) return;
        const Slot &sl = s.slots[b % kSlots];
        E::update_startup(s.rc.u);
        const E::TailInput t = E::middle_block<false>(s.rc, s.hist.data(), sl.xf, sl.df, sl.df, 0, VecI(0));
        const VecI o = E::tail_block(s.rc, t.a, t.b, t.clean_q);
        E::StridedIo sio = io_of(k);
        sio.out(s.rc, b, o);
        s.out_blocks += 1;
    };
    // the steps of the WORKGROUP: counted by its longest stream, one barrier per step for every role of every slot
    const int lag = deep ? 4 : 1;
    int barriers[5] = {0, 0, 0, 0, 0};                                    // front, delay, channel / back, gain, tail
    for (int step = 0; step < longest + lag; ++step) {
        for (int i = 0; i < kStreams; ++i) {
            const int k = order == 0 ? i : kStreams - 1 - i;
            if (deep) {
                if (order == 0) { tail(k, step - 4); gain(k, step - 3); channel(k, step - 2); delay(k, step - 1); front(k, step); }
                else { front(k, step); delay(k, step - 1); channel(k, step - 2); gain(k, step - 3); tail(k, step - 4); }
            } else {
                if (order == 0) { back(k, step - 1); front(k, step); }
                else { front(k, step); back(k, step - 1); }
            }
        }
        for (int &b : barriers) b += 1;
    }
    for (int k = 0; k < kStreams; ++k) {
        SlotState &s = wg[k];
        uint32_t *vec = s.img.vec.data();
        int32_t *scal = s.img.scal.data();
        if (s.len > 0) {                                                  // the state: once, at the end, by the role that owns each part
            if (deep) {
                E::Regs &rc = s.rc, &rg = s.rg;
                rc.b.echo_filt = rg.b.echo_filt; rc.b.near_filt = rg.b.near_filt; rc.b.low_ctr = rg.b.low_ctr; rc.b.high_ctr = rg.b.high_ctr;
                rc.b.noise_est = rg.b.noise_est;
                rc.u.seed = rg.u.seed; rc.u.sup_gain = rg.u.sup_gain; rc.u.sup_gain_old = rg.u.sup_gain_old; rc.u.noise_ctr = rg.u.noise_ctr;
                rc.b64.echo_filt = rg.b64.echo_filt; rc.b64.near_filt = rg.b64.near_filt; rc.b64.noise_est = rg.b64.noise_est;
                rc.b64.low_ctr = rg.b64.low_ctr; rc.b64.high_ctr = rg.b64.high_ctr;
                E::store_state<false, false, false>(rc, vec, scal);
                E::store_time_state(vec, s.rf.lane, s.x_old, s.d_old);
                E::store_tail_state(vec, s.rt.lane, s.ovl, s.c_old);
                E::store_delay_state(s.rd, vec, scal);
            } else {
                E::store_state<false, true, true>(s.rc, vec, scal);
                E::store_time_state(vec, s.rf.lane, s.x_old, s.d_old);
            }
        }
        ComputeDigest(vec, scal, s.hist.data(), digests + (size_t)k * kDigestWords);
        counts[k * 3 + 0] = s.hand_over_writes;
        counts[k * 3 + 1] = s.out_blocks;
        counts[k * 3 + 2] = s.input_rows;
    }
    for (int r = 1; r < 5; ++r)
        if (barriers[r] != barriers[0]) return -1;
    return barriers[0];
}

}  // extern "C"
