// TEST INFRASTRUCTURE: packet ticks (WebRtcAecmSessions_TickPackets) on sample TAGS -- the method of sim_mixed.cpp, whose whole
// OBJECT of sessions of both rates this unit takes over.  The device side is what the host's tick planner (packets), the planning
// kernels (aecm_flow_plan_packets_kernel: FlowTickPackets at the lane's rate; aecm_flow_plan_calls_kernel where the routing falls
// back to the K-call tick) and aecm_tick_packets_kernel do, in the kernel's own order per call -- spill, far framing (fresh samples
// from call c's piece of the PACKED row, everything older from the ring), append of the call's n_s samples at near position
// near_pos + c n_s, blocks, output frames.  It is compared with
//   - the reference side, one SessionFlow<T> per session at the session's rate, called K times with the session's size: every
//     block input and every output sample;
//   - a twin object of the device model of ordinary mixed ticks (sim_mixed.cpp: planning + Session::TickBody), ticked K times on
//     re-laid rows (ordinary tick c gets row[c n_s .. c n_s + n_s) at the start of an n-sample row, junk behind it): the flow words
//     except F_NEAR_LAG after every tick, every output, and the snapshot models (what ExportSession writes) byte for byte.
// Stand-alone (main below): g++ -fsanitize=address,undefined tests/sim/sim_packets.cpp -Iwebrtc_aecm_amd/csrc && ./a.out
#include "sim_mixed.cpp"       // Session (rings, TickBody, BufferFarend), Rng, the tags (its anonymous namespace: this unit's too)

namespace {

struct Object {
    std::vector<std::unique_ptr<Session>> ss;
    TickObject host;               // what the host keeps for the object (aecm_tick_plan.h)
    bool has_clean = false;
};

// The host's side of a tick: check, plan, commit.  False: refused.  *tick_pos: the object's near position before the tick.
bool HostTick(Object &o, int n, int calls, bool packets, const uint8_t *flags, TickPlan *plan, uint32_t *tick_pos) {
    TickArgs a;
    a.flags_per_session = flags;
    a.n = n;
    a.calls = calls;
    a.packets = packets;
    a.has_clean = o.has_clean;
    *plan = o.host.Tick(a, tick_pos);
    return plan->code == 0;
}

enum PacketsDetail : int {
    P_WHAT = 0, P_SESSION, P_FIELD, P_BLOCKS, P_PACKET_TICKS, P_CALLS_SHAPED, P_ORDINARY, P_BURSTS, P_NOBODY, P_LONGEST_IDLE, P_HALF_SPILL_LATER,
    P_STARTUP_END_LATER, P_RESYNC_AFTER_IDLE, P_HALF_AND_FULL, P_HALF_PACKETS, P_NONDIRECT_LATER, P_NO_BLOCK_CALLS, P_FULL_8K_PACKETS, kPacketsDetail
};

struct Rows {                  // one session's rows of one tick (width samples) and what the device delivered
    std::vector<int64_t> far, near, clean, out;
    std::vector<int64_t> bfar, bnear, bclean;      // block inputs, in order
};

struct Fail {
    int what = 0, session = -1, field = 0;
    explicit operator bool() const { return what != 0; }
};

// One ORDINARY tick of the object: the host's plan (calls == 1) and the three planning kernels + the tick kernels' body, as
// sim_mixed.cpp's fuzz does it.  rows[s]: n samples.
Fail OrdinaryTick(Object &o, int n, const uint8_t *flags, const int *ms, std::vector<Rows> &rows, int64_t *detail) {
    const int S = (int)o.ss.size();
    TickPlan plan;
    uint32_t tick_pos;
    if (!HostTick(o, n, 1, false, flags, &plan, &tick_pos)) return Fail{11, -1, 0};
    const bool mixed_plan = plan.mixed_plan;
    const FlowTickRoute route = plan.route;
    if (!route.launch) {
        if (detail) detail[P_NOBODY]++;
        return Fail{};
    }
    for (int s = 0; s < S; ++s) {
        Session &q = *o.ss[s];
        const bool idle = (flags[s] & kFlowIdle) != 0, half = !idle && (flags[s] & kFlowHalfCall) != 0;
        FlowPlan planned;
        if (!route.sparse_plan) {
            if (q.regs.v[F_NEAR_LAG] != 0 || idle || half || q.fs != o.host.fs) return Fail{8, s, 0};
            FlowRegs r = q.regs;
            FlowTick(r, o.host.fs, n, ms[s], flags[s], tick_pos, planned);
            for (int k = 0; k < kFlowTickFields; ++k) q.regs.v[k] = r.v[k];
        } else if (idle) {
            q.regs.v[F_NEAR_LAG] = FlowIdleTick(FlowIdleTick(q.regs.v[F_NEAR_LAG], route.deferred_lag), n);
            continue;
        } else {
            if (!mixed_plan && (half || q.fs != o.host.fs)) return Fail{8, s, 0};
            q.regs.v[F_NEAR_LAG] = FlowIdleTick(q.regs.v[F_NEAR_LAG], route.deferred_lag);
            if (q.regs.v[F_NEAR_LAG] != 0) {
                FlowNearMove m;
                FlowResync(q.regs, tick_pos, m);
                FlowMoveNear(q.near_ring.data(), (uint32_t)(kRingLen - 1), m);
                if (o.has_clean) FlowMoveNear(q.clean_ring.data(), (uint32_t)(kRingLen - 1), m);
            }
            if (mixed_plan) FlowTickMixed(q.regs, q.fs, n, ms[s], flags[s], tick_pos, planned);
            else FlowTick(q.regs, o.host.fs, n, ms[s], flags[s], tick_pos, planned);
        }
        if (const int field = q.StateDefect()) return Fail{100, s, field};
        Rows &w = rows[s];
        q.TickBody(planned, o.has_clean, n, tick_pos, w.far.data(), w.near.data(), w.clean.data(), w.out.data(), &w.bfar, &w.bnear, &w.bclean);
    }
    return Fail{};
}

// aecm_tick_packets_kernel for one session: K plans, rows packed at c * n_s, n_s from the plan.
void PacketBody(Session &q, bool has_clean, int calls, const int32_t (*words)[kFlowPlanWords], uint32_t tick_pos, Rows &w, bool half, int64_t *detail) {
    const int64_t mask = kRingLen - 1;
    for (int c = 0; c < calls; ++c) {
        FlowPlan p;
        FlowUnpackPlan(words[c], p);
        const int n = p.n_frames * kFlowFrame;
        const int64_t *fin = w.far.data() + c * n, *nin = w.near.data() + c * n, *cin = w.clean.data() + c * n;
        int64_t *out = w.out.data() + c * n;
        const uint32_t npos = tick_pos + (uint32_t)(c * n);
        if ((p.spill[0] | p.spill[1]) && c > 0 && half) detail[P_HALF_SPILL_LATER]++;
        for (int i = 0; i < 2; ++i)
            if (p.spill[i])
                for (int j = 0; j < kFlowFrame; ++j) q.far_old[i * kFlowFrame + j] = q.far_ring[(p.spill_pos[i] + (uint32_t)j) & mask];
        const bool active = p.frame[0].active | p.frame[1].active;
        if (c > 0 && active && !p.direct) detail[P_NONDIRECT_LATER]++;
        if (!p.direct && active) {
            const auto far_stream = [&](uint32_t x) -> int64_t {
                const int r0 = (int)(x - p.far[0].pos);
                return r0 >= 0 && r0 < p.far[0].count ? fin[r0] : q.far_ring[x & mask];
            };
            int64_t left[kFlowBlock], frames[2][kFlowFrame];
            for (int j = 0; j < p.left_count; ++j) left[j] = q.far_ring[(p.blk_pos0 + p.left_delta + (uint32_t)j) & mask];
            for (int f = 0; f < 2; ++f) {
                const FlowFrame &fr = p.frame[f];
                if (!fr.active) continue;
                for (int j = 0; j < kFlowFrame; ++j) frames[f][j] = fr.far_from_stream ? far_stream(fr.far_pos + (uint32_t)j) : q.far_old[fr.old_idx * kFlowFrame + j];
            }
            for (int j = 0; j < p.left_count; ++j) q.far_frames[(p.blk_pos0 + (uint32_t)j) & (kFlowFarFrameRing - 1)] = left[j];
            for (int f = 0; f < 2; ++f) {
                const FlowFrame &fr = p.frame[f];
                if (!fr.active) continue;
                for (int j = 0; j < kFlowFrame; ++j) q.far_frames[(fr.frm_pos + (uint32_t)j) & (kFlowFarFrameRing - 1)] = frames[f][j];
            }
        }
        for (int j = 0; j < n; ++j) {                                        // the append: the call's n_s samples, nothing behind them
            if (j < p.far[0].count) q.far_ring[(p.far[0].pos + (uint32_t)j) & mask] = fin[j];
            q.near_ring[(npos + (uint32_t)j) & mask] = nin[j];
            if (has_clean) q.clean_ring[(npos + (uint32_t)j) & mask] = cin[j];
        }
        if (p.n_blocks == 0) detail[P_NO_BLOCK_CALLS]++;
        for (int b = 0; b < p.n_blocks; ++b, ++q.blocks_done)
            for (int t = 0; t < kFlowBlock; ++t) {
                const uint32_t x = p.blk_pos0 + (uint32_t)(b * kFlowBlock + t);
                w.bfar.push_back(p.direct ? q.far_ring[(x + p.far_delta) & mask] : q.far_frames[x & (kFlowFarFrameRing - 1)]);
                w.bnear.push_back(q.near_ring[(p.near_base + x) & mask]);
                if (has_clean) w.bclean.push_back(q.clean_ring[(p.near_base + x) & mask]);
                q.out_ring[x & mask] = kOutTagBase + q.blocks_done * kFlowBlock + t;
            }
        const int64_t *pass = has_clean ? cin : nin;
        for (int f = 0; f < p.n_frames; ++f)
            for (int j = 0; j < kFlowFrame; ++j)
                out[f * kFlowFrame + j] = p.frame[f].active ? q.out_ring[(p.frame[f].out_pos + (uint32_t)j) & mask] : pass[f * kFlowFrame + j];
    }
}

// One PACKET tick of the object: the host's plan with `packets`, then the planning and tick kernels it names.
// rows[s]: calls * n samples, packed.  idle_before[s]: the session sat out the tick before this one.
Fail PacketTick(Object &o, int n, int calls, const uint8_t *flags, const int *ms, std::vector<Rows> &rows, const std::vector<int> &idle_before,
                int64_t *detail) {
    if (calls == 1) return OrdinaryTick(o, n, flags, ms, rows, detail);       // the same launches, the same kernels
    const int S = (int)o.ss.size(), span = calls * n;
    TickPlan plan;
    uint32_t tick_pos;
    if (!HostTick(o, n, calls, true, flags, &plan, &tick_pos) || plan.span != span) return Fail{11, -1, 0};
    const bool mixed_plan = plan.mixed_plan;
    const FlowTickRoute route = plan.route;
    if (!route.launch) {
        detail[P_NOBODY]++;
        return Fail{};
    }
    if (!route.sparse_plan || !route.sparse_tick || plan.family != (mixed_plan ? kTickFamily_packets : kTickFamily_calls)) return Fail{12, -1, 0};      // a K-call tick always goes by the live list
    detail[mixed_plan ? P_PACKET_TICKS : P_CALLS_SHAPED]++;
    bool live_half = false, live_full = false;
    for (int s = 0; s < S; ++s) {
        Session &q = *o.ss[s];
        const bool idle = (flags[s] & kFlowIdle) != 0, half = !idle && (flags[s] & kFlowHalfCall) != 0;
        if (idle) {
            q.regs.v[F_NEAR_LAG] = FlowIdleTick(FlowIdleTick(q.regs.v[F_NEAR_LAG], route.deferred_lag), span);
            continue;
        }
        (half ? live_half : live_full) = true;
        q.regs.v[F_NEAR_LAG] = FlowIdleTick(q.regs.v[F_NEAR_LAG], route.deferred_lag);
        if (q.regs.v[F_NEAR_LAG] != 0) {
            FlowNearMove m;
            FlowResync(q.regs, tick_pos, m);
            FlowMoveNear(q.near_ring.data(), (uint32_t)(kRingLen - 1), m);
            if (o.has_clean) FlowMoveNear(q.clean_ring.data(), (uint32_t)(kRingLen - 1), m);
            if (mixed_plan && idle_before[s] && m.count > 0) detail[P_RESYNC_AFTER_IDLE]++;
        }
        int32_t words[kFlowMaxTickCalls][kFlowPlanWords];
        int defect = 0;
        bool startup_before = q.regs.v[F_EC_STARTUP] != 0;
        const auto sink = [&](int c, const FlowPlan &p) {
            FlowPackPlan(p, words[c]);
            FlowRegs between = q.regs;                                        // a state BETWEEN two calls: the lag is still to come
            int32_t w[kFlowWords] = {0};
            for (int k = 0; k < kFlowFieldsUsed; ++k) w[k] = between.v[k];
            if (const int field = FlowStateDefect(w)) defect = defect ? defect : field;
            const bool startup_now = q.regs.v[F_EC_STARTUP] != 0;
            if (c > 0 && startup_before && !startup_now && mixed_plan) detail[P_STARTUP_END_LATER]++;
            startup_before = startup_now;
        };
        if (mixed_plan) {
            FlowTickPackets(q.regs, q.fs, n, calls, ms[s], flags[s], tick_pos, sink);
        } else {
            if (half || q.fs != o.host.fs) return Fail{8, s, 0};
            FlowTickCalls(q.regs, o.host.fs, n, calls, ms[s], flags[s], tick_pos, sink);
        }
        if (defect) return Fail{100, s, defect};
        if (const int field = q.StateDefect()) return Fail{100, s, field};
        detail[P_HALF_PACKETS] += half && mixed_plan;
        detail[P_FULL_8K_PACKETS] += !half && mixed_plan && q.fs == 8000 && n == 160;
        PacketBody(q, o.has_clean, calls, words, tick_pos, rows[s], half, detail);
    }
    if (mixed_plan && live_half && live_full) detail[P_HALF_AND_FULL]++;        // (fewer than 64 sessions: one planning wavefront)
    return Fail{};
}

// What ExportSession writes of a session (aecm_sessions.cpp): the flow words with the lag as 0, the far ring, the last 256 block
// outputs before F_BLK_POS, the last 64 near-end (and clean) samples before the session's OWN position, framed-far ring, replay rows.
std::vector<int64_t> SnapshotModel(const Object &o, const Session &q) {
    std::vector<int64_t> v;
    for (int k = 0; k < kFlowFieldsUsed; ++k) v.push_back(k == F_NEAR_LAG ? 0 : q.regs.v[k]);
    v.insert(v.end(), q.far_ring.begin(), q.far_ring.end());
    const uint32_t own = (uint32_t)o.host.near_pos - (uint32_t)q.regs.v[F_NEAR_LAG] - (uint32_t)o.host.lag.deferred_lag, mask = (uint32_t)(kRingLen - 1);
    for (uint32_t k = 0; k < 256; ++k) v.push_back(q.out_ring[((uint32_t)q.regs.v[F_BLK_POS] - 256u + k) & mask]);
    for (uint32_t k = 0; k < 64; ++k) v.push_back(q.near_ring[(own - 64u + k) & mask]);
    for (uint32_t k = 0; k < 64; ++k) v.push_back(o.has_clean ? q.clean_ring[(own - 64u + k) & mask] : 0);
    v.insert(v.end(), q.far_frames.begin(), q.far_frames.end());
    v.insert(v.end(), q.far_old.begin(), q.far_old.end());
    return v;
}

}  // namespace

extern "C" {

int sim_packets_detail_words(void) { return kPacketsDetail; }

// An object of n_sessions sessions through n_ticks ticks.  rates_mode 0: both rates at random; 1: every session at the object's
// rate (packet ticks without half flags fall back to the K-call tick there: "TickCalls-shaped").  The object's rate, the clean
// input and the start position (wrapping) come from the seed.  Every tick is drawn from: packet ticks (K = 1 .. 6, half flags per
// session in stretches, so that a session makes more than 98 calls of 80 samples in a row), ordinary ticks (half and split calls),
// bursts before some ticks, idle sessions and idle stretches longer than the ring, ticks nobody makes.  Returns -1 when everything
// agreed, else the first tick that did not; detail[P_WHAT]: 1 block count, 2 far block tags, 3 near block tags, 4 clean block
// tags, 5 output tags against the reference, 6 the twin's outputs or block inputs differ, 7 out row written past the calls, 8 a
// planning kernel met a session it cannot plan, 9 lag no multiple of 80 below the period or not the distance to the session's own
// position, 11 the host refused the flags, 12 routing, 20 flow words differ from the twin's (detail[P_FIELD] = field), 21 the
// snapshot models differ, 100: FlowStateDefect refused a state (P_FIELD), also one between two calls.
int64_t sim_packets_fuzz(uint64_t seed, int n_sessions, int n_ticks, int rates_mode, int64_t *detail) {
    Rng rng{seed * 2654435761ull + 777};
    for (int i = 0; i < kPacketsDetail; ++i) detail[i] = 0;
    Object dev, twin;
    const uint32_t starts[3] = {0u, 0xffffffffu - 0xffffffffu % 80u - 800u, (uint32_t)kFlowLagPeriod * 1000u - 400u};
    const int S = n_sessions;
    for (Object *o : {&dev, &twin}) {
        o->host.Init(n_sessions, (seed & 1) ? 16000 : 8000);
        o->has_clean = (seed & 2) != 0;
        o->host.near_pos = starts[(seed / 4) % 3];
    }
    for (int s = 0; s < S; ++s) {
        const int fs = rates_mode == 0 ? (rng.chance(50) ? 16000 : 8000) : dev.host.fs;
        const uint32_t p0 = rng.chance(50) ? 0u : rng.next() * 7u;
        for (Object *o : {&dev, &twin}) {
            o->host.SetRate(s, fs);
            o->ss.emplace_back(new Session(fs));
            Session &q = *o->ss.back();
            q.regs.v[F_FAR_RP] = q.regs.v[F_FAR_WP] = (int32_t)p0;
            q.regs.v[F_FRM_POS] = q.regs.v[F_BLK_POS] = q.regs.v[F_OUT_RP] = (int32_t)(p0 * 3u);
        }
    }
    std::vector<int64_t> far_offered((size_t)S, 0), near_offered((size_t)S, 0), idle_samples((size_t)S, 0);
    std::vector<int> half_mode((size_t)S, 0), half_left((size_t)S, 0), forced((size_t)S, 0), idle_before((size_t)S, 0), ms((size_t)S, 40);
    std::vector<uint8_t> flags((size_t)S);
    const auto fail = [&](const Fail &f) { detail[P_WHAT] = f.what; detail[P_SESSION] = f.session; detail[P_FIELD] = f.field; };
    for (int64_t tick = 0; tick < n_ticks; ++tick) {
        // the object's tick size: an 8 kHz object mostly ticks 80, a 16 kHz object mostly 160
        const int n = rng.chance(dev.host.fs == 16000 ? 90 : 30) ? 160 : 80;
        int calls = rng.range(1, kFlowMaxTickCalls);
        const bool ordinary = rng.chance(25);
        if (ordinary) calls = 1;
        // ---- a far-end burst before the tick
        if (rng.chance(12)) {
            const int len = rng.chance(50) ? 80 : 160;
            for (int s = 0; s < S; ++s) {
                const int c = rng.chance(50) ? 0 : rng.range(1, rng.chance(5) ? 40 : 3);
                if (!c) continue;
                std::vector<int64_t> burst((size_t)c * len);
                for (size_t j = 0; j < burst.size(); ++j) burst[j] = far_offered[s] + (int64_t)j;
                far_offered[s] += (int64_t)burst.size();
                for (Object *o : {&dev, &twin}) o->ss[s]->BufferFarend(len, c, burst.data());
                for (int k = 0; k < c; ++k) dev.ss[s]->ref.BufferFarend(burst.data() + (size_t)k * len, (size_t)len);
                detail[P_BURSTS]++;
            }
        }
        // ---- the tick's flags and rows
        const bool all_idle = rng.chance(3);
        std::vector<Rows> rows((size_t)S), trows((size_t)S);
        std::vector<int> n_s((size_t)S, 0);
        for (int s = 0; s < S; ++s) {
            if (half_left[s]-- <= 0) {                                         // half calls come in stretches
                half_mode[s] = rng.range(0, 2);
                half_left[s] = rng.range(30, 90);
            }
            uint8_t f = 0;
            if (rng.chance(12)) f |= kFlowNoFarend;
            if (n == 160) {
                if (rates_mode != 1 || !rng.chance(50) || ordinary) {
                    if (half_mode[s] == 1 || (half_mode[s] == 2 && rng.chance(50))) f |= kFlowHalfCall;
                }
                if (rates_mode == 1 && !ordinary && rng.chance(40)) f &= (uint8_t)~kFlowHalfCall;
                if (ordinary && !(f & kFlowHalfCall) && dev.ss[s]->fs == 16000 && rng.chance(25)) f |= kFlowSplitCalls;
            }
            if (forced[s] == 0 && rng.chance(1)) forced[s] = rng.chance(30) ? rng.range(20, 40) : rng.range(1, 6);      // x up to 960 samples: longer than the ring
            bool idle = all_idle || forced[s] > 0 || rng.chance(8);
            if (forced[s] > 0) --forced[s];
            if (idle) f = (uint8_t)(kFlowIdle | (rng.next() & 11u));
            flags[s] = f;
            if (rng.chance(10)) ms[s] = rng.chance(50) ? rng.range(0, 60) : rng.range(250, 400);
            else if (rng.chance(30)) ms[s] = ms[s] + rng.range(-10, 10);
            n_s[s] = idle ? 0 : FlowPacketCallSize(n, f);
        }
        if (rates_mode == 1 && !ordinary && calls > 1 && rng.chance(50))         // a uniform object, nobody half: the K-call tick's launches
            for (int s = 0; s < S; ++s) {
                if (flags[s] & kFlowIdle) continue;
                flags[s] &= (uint8_t)~kFlowHalfCall;
                n_s[s] = n;
            }
        std::vector<int> ms_now = ms;
        for (int s = 0; s < S; ++s)
            if (rng.chance(3)) ms_now[s] = rng.chance(50) ? -300 : 700;
        const int span = calls * n;
        for (int s = 0; s < S; ++s) {
            Rows &w = rows[s];
            w.far.assign((size_t)span, kJunk); w.near.assign((size_t)span, kJunk); w.clean.assign((size_t)span, kJunk); w.out.assign((size_t)span, kSentinel);
            const int mine = calls * n_s[s];
            for (int j = 0; j < mine; ++j) {
                w.far[j] = far_offered[s] + j;
                w.near[j] = kNearTagBase + near_offered[s] + j;
                w.clean[j] = kCleanTagBase + near_offered[s] + j;
            }
            far_offered[s] += mine;
            near_offered[s] += mine;
            if (n_s[s] == 0) {
                idle_samples[s] += span;
                if (idle_samples[s] > detail[P_LONGEST_IDLE]) detail[P_LONGEST_IDLE] = idle_samples[s];
            } else {
                idle_samples[s] = 0;
            }
        }
        // ---- the device: one packet tick (or one ordinary tick)
        if (ordinary) detail[P_ORDINARY]++;
        if (const Fail f = PacketTick(dev, n, calls, flags.data(), ms_now.data(), rows, idle_before, detail)) { fail(f); return tick; }
        // ---- the twin: K ordinary ticks on re-laid rows
        std::vector<Rows> tall((size_t)S);
        for (int s = 0; s < S; ++s) tall[s].out.assign((size_t)span, kSentinel);
        for (int c = 0; c < calls; ++c) {
            for (int s = 0; s < S; ++s) {
                Rows &w = trows[s];
                w.far.assign((size_t)n, kJunk); w.near.assign((size_t)n, kJunk); w.clean.assign((size_t)n, kJunk); w.out.assign((size_t)n, kSentinel);
                for (int j = 0; j < n_s[s]; ++j) {
                    w.far[j] = rows[s].far[c * n_s[s] + j];
                    w.near[j] = rows[s].near[c * n_s[s] + j];
                    w.clean[j] = rows[s].clean[c * n_s[s] + j];
                }
            }
            if (const Fail f = OrdinaryTick(twin, n, flags.data(), ms_now.data(), trows, nullptr)) { fail(Fail{f.what + 1000, f.session, f.field}); return tick; }
            for (int s = 0; s < S; ++s) {
                for (int j = 0; j < n_s[s]; ++j) tall[s].out[c * n_s[s] + j] = trows[s].out[j];
                for (int j = n_s[s]; j < n; ++j)
                    if (trows[s].out[j] != kSentinel) { fail(Fail{7, s, 1}); return tick; }
                tall[s].bfar.insert(tall[s].bfar.end(), trows[s].bfar.begin(), trows[s].bfar.end());
                tall[s].bnear.insert(tall[s].bnear.end(), trows[s].bnear.begin(), trows[s].bnear.end());
                tall[s].bclean.insert(tall[s].bclean.end(), trows[s].bclean.begin(), trows[s].bclean.end());
                trows[s].bfar.clear(); trows[s].bnear.clear(); trows[s].bclean.clear();
            }
        }
        // ---- per session: the reference, the twin, the state
        for (int s = 0; s < S; ++s) {
            Session &q = *dev.ss[s], &t = *twin.ss[s];
            Rows &w = rows[s];
            const int32_t l = q.regs.v[F_NEAR_LAG];
            if (l < 0 || l >= kFlowLagPeriod || l % kFlowFrame != 0) { fail(Fail{9, s, 0}); return tick; }
            if (const int field = q.StateDefect()) { fail(Fail{100, s, field}); return tick; }
            for (int k = 0; k < kFlowTickFields; ++k)
                if (q.regs.v[k] != t.regs.v[k]) { fail(Fail{20, s, k + 1}); return tick; }
            if (dev.host.near_pos != twin.host.near_pos) { fail(Fail{20, s, F_NEAR_LAG + 1}); return tick; }
            if (SnapshotModel(dev, q) != SnapshotModel(twin, t)) { fail(Fail{21, s, 0}); return tick; }
            if (w.out != tall[s].out || w.bfar != tall[s].bfar || w.bnear != tall[s].bnear || w.bclean != tall[s].bclean) { fail(Fail{6, s, 0}); return tick; }
            idle_before[s] = n_s[s] == 0;
            if (n_s[s] == 0) {
                for (int j = 0; j < span; ++j)
                    if (w.out[j] != kSentinel) { fail(Fail{7, s, 0}); return tick; }
                continue;
            }
            const bool split = (flags[s] & kFlowSplitCalls) != 0 && calls == 1 && n_s[s] == 160;
            const int n_calls = split ? 2 : calls, len = split ? 80 : n_s[s];
            std::vector<int64_t> rfar, rnear, rclean, out_ref((size_t)span, kSentinel);
            for (int c = 0; c < n_calls; ++c) {
                if (!(flags[s] & kFlowNoFarend)) q.ref.BufferFarend(w.far.data() + c * len, (size_t)len);
                (void)q.ref.Process(w.near.data() + c * len, dev.has_clean ? w.clean.data() + c * len : nullptr, out_ref.data() + c * len, (size_t)len,
                                    (int16_t)ms_now[s], [&](const int64_t *fb, const int64_t *nb, const int64_t *cb, int64_t *ob, int nblk) {
                                        rfar.insert(rfar.end(), fb, fb + nblk * kFlowBlock);
                                        rnear.insert(rnear.end(), nb, nb + nblk * kFlowBlock);
                                        if (cb) rclean.insert(rclean.end(), cb, cb + nblk * kFlowBlock);
                                        for (int j = 0; j < nblk * kFlowBlock; ++j) ob[j] = kOutTagBase + q.ref_blocks * kFlowBlock + j;
                                        q.ref_blocks += nblk;
                                        return true;
                                    });
            }
            detail[P_BLOCKS] += (int64_t)rfar.size() / kFlowBlock;
            int what = 0;
            if (w.bfar.size() != rfar.size()) what = 1;
            else if (w.bfar != rfar) what = 2;
            else if (w.bnear != rnear) what = 3;
            else if (w.bclean != rclean) what = 4;
            else if (w.out != out_ref) what = 5;                               // (the sentinels behind the calls included: never written)
            if (what) { fail(Fail{what, s, 0}); return tick; }
        }
    }
    return -1;
}

// Lag arithmetic: a session that makes T all-half packet ticks of K calls in ticks of 160 from lag 0, WITHOUT the resync of the next
// tick (what F_NEAR_LAG would read if nothing brought the session back in step), through FlowTickPackets itself.
int32_t sim_packets_lag_after(int64_t ticks, int calls) {
    FlowRegs r;
    int32_t words[kFlowWords];
    FlowInit(words);
    for (int k = 0; k < kFlowFieldsUsed; ++k) r.v[k] = words[k];
    uint32_t near_pos = 0;
    for (int64_t t = 0; t < ticks; ++t, near_pos += (uint32_t)(calls * 160))
        FlowTickPackets(r, 8000, 160, calls, 40, kFlowHalfCall | kFlowNoFarend, near_pos, [](int, const FlowPlan &) {});
    return r.v[F_NEAR_LAG];
}

// The recipe of the GPU test of a replay-row spill inside a packet of half calls: a session at fs with msInSndCardBuf 40 makes
// pre_ticks ordinary ticks of 160 samples, then packets of `calls` half calls until a plan spills a replay row (at most max_ticks).
// result = {packet tick of the spill (0-based), call c of the spill, replay row}; returns 0, or -1 when no spill happened.
int sim_packets_spill_recipe(int fs, int pre_ticks, int calls, int max_ticks, int32_t *result) {
    FlowRegs r;
    int32_t words[kFlowWords];
    FlowInit(words);
    for (int k = 0; k < kFlowFieldsUsed; ++k) r.v[k] = words[k];
    uint32_t near_pos = 0;
    for (int t = 0; t < pre_ticks; ++t, near_pos += 160) {
        FlowPlan p;
        FlowTick(r, fs, 160, 40, 0, near_pos, p);
    }
    for (int t = 0; t < max_ticks; ++t, near_pos += (uint32_t)(calls * 160)) {
        int at = -1, row = -1;
        if (r.v[F_NEAR_LAG] != 0) {
            FlowNearMove m;
            FlowResync(r, near_pos, m);
        }
        FlowTickPackets(r, fs, 160, calls, 40, kFlowHalfCall, near_pos, [&](int c, const FlowPlan &p) {
            if (at < 0 && (p.spill[0] | p.spill[1])) { at = c; row = p.spill[1] ? 1 : 0; }
        });
        if (at >= 0) {
            result[0] = t; result[1] = at; result[2] = row;
            return 0;
        }
    }
    return -1;
}

}  // extern "C"

#if !defined(AECM_SIM_PACKETS_NO_MAIN)
int main() {
    int64_t detail[kPacketsDetail];
    for (uint64_t seed = 0; seed < 8; ++seed) {
        const int64_t tick = sim_packets_fuzz(seed, 6, 200, seed >= 6 ? 1 : 0, detail);
        if (tick != -1) {
            printf("seed %llu: tick %lld what %lld session %lld field %lld\n", (unsigned long long)seed, (long long)tick, (long long)detail[0],
                   (long long)detail[1], (long long)detail[2]);
            return 1;
        }
    }
    int32_t res[3];
    if (sim_packets_spill_recipe(8000, 12, 6, 40, res) != 0 || res[1] <= 0) return 2;
    if (sim_packets_lag_after(7, 3) != (7 * 3 * 80) % 40960) return 3;
    printf("ok\n");
    return 0;
}
#endif
