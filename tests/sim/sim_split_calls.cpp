// TEST INFRASTRUCTURE: K-call and packet ticks with a clean near-end input PER SESSION (WebRtcAecmSessions_SetSplitCallTicks;
// AECM_SESSION_NO_CLEAN with calls > 1) on sample TAGS -- the whole OBJECT of sim_packets.cpp, which this unit takes over, with the
// host's switch on.  The device side is what the host's tick planner (family split with k_calls), the planning kernels of
// aecm_tick_split_calls_plan_kernels.hip (the two-list first lines of aecm_flow_plan_split_list.inc lane by lane, then FlowTickCalls /
// FlowTickPackets per lane) and the tick kernels of aecm_tick_split_calls_kernels.hip do: the loop body (sim_packets.cpp: PacketBody)
// once per list, with a clean input over live[0 .. clean_count), without over live[plain_start .. + plain_count).  Compared with
//   - the reference side, one SessionFlow<T> per session, called K times with the clean pointer or NULL by the session's kind: every
//     block input and every output sample (a flagged session's clean rows hold junk in all K pieces: any use would show);
//   - a twin object of the device model of ORDINARY split ticks, ticked K times on the same (half calls: re-laid) rows: flow words,
//     outputs, block inputs and the snapshot models byte for byte.
// Also the host's planner with the switch and a call trace as a table can ask it (tests/split_calls_sim.py: Object).
// Stand-alone (-DSIM_SPLIT_CALLS_MAIN): g++ -fsanitize=address,undefined tests/sim/sim_split_calls.cpp -Iwebrtc_aecm_amd/csrc && ./a.out
#define AECM_SIM_PACKETS_NO_MAIN
#include "sim_packets.cpp"      // Object, HostTick, Rows, Fail, PacketBody, SnapshotModel; sim_mixed.cpp: Session, Rng, the tags

namespace {

enum SplitCallsDetail : int {
    SC_WHAT = 0, SC_SESSION, SC_FIELD, SC_BLOCKS, SC_SPLIT_CALLS_TICKS, SC_SPLIT_PACKET_TICKS, SC_ALL_CLEAN_TICKS, SC_ALL_PLAIN_TICKS, SC_ORDINARY_SPLIT,
    SC_NOBODY, SC_CLEAN_MULT4, SC_CLEAN_OTHER, SC_REINIT, SC_HALF_PLAIN, SC_STARTUP_PLAIN_CALLS, SC_BURSTS, kSplitCallsDetail
};

// Does session's WebRtcAecm_Process get a clean pointer in this tick: its own kind in a split tick, else the tick's.
bool TakesClean(const TickPlan &plan, uint8_t f) { return plan.split_tick ? (f & kFlowNoClean) == 0 : plan.clean_plane; }

// aecm_flow_plan_split_list.inc, lane by lane, on the bases the host's plan left (TickObject::Bases): list = FlowSplitListEntries(S)
// entries preset to 0xffffffff.  False: a store fell outside its list.
bool SplitLists(const TickObject &host, const TickPlan &plan, const uint8_t *flags, std::vector<uint32_t> &list) {
    const int32_t S = host.n_sessions, blocks = (int32_t)host.live_bases.size();
    const uint32_t *clean_bases = host.Bases(plan).data(), *plain_bases = clean_bases + blocks;
    const uint32_t plain_start = FlowPlainListStart((uint32_t)plan.clean_count);
    list.assign(FlowSplitListEntries((uint32_t)S), 0xffffffffu);
    for (int32_t b = 0; b < blocks; ++b) {
        uint32_t wave_counts[2][kFlowPlanBlock / 64];
        uint64_t ballots[2][kFlowPlanBlock / 64];
        const auto flag_of = [&](int t) { const int32_t s = b * kFlowPlanBlock + t; return s < S ? (int)flags[s] : kFlowIdle; };
        for (int w = 0; w < kFlowPlanBlock / 64; ++w) {
            ballots[0][w] = ballots[1][w] = 0;
            for (int lane = 0; lane < 64; ++lane) {
                const int f = flag_of(w * 64 + lane);
                const bool live = (f & kFlowIdle) == 0, no_clean = (f & kFlowNoClean) != 0;
                if (live && !no_clean) ballots[0][w] |= uint64_t(1) << lane;
                if (live && no_clean) ballots[1][w] |= uint64_t(1) << lane;
            }
            wave_counts[0][w] = (uint32_t)__builtin_popcountll(ballots[0][w]);
            wave_counts[1][w] = (uint32_t)__builtin_popcountll(ballots[1][w]);
        }
        for (int t = 0; t < kFlowPlanBlock; ++t) {
            const int f = flag_of(t), w = t >> 6, lane = t & 63;
            const bool live = (f & kFlowIdle) == 0, no_clean = (f & kFlowNoClean) != 0;
            if (!live) continue;
            const uint32_t slot = FlowSplitSlot(no_clean, clean_bases[b], plain_bases[b], plain_start, wave_counts, w, ballots[0][w], ballots[1][w], lane);
            const uint32_t end = no_clean ? plain_start + (uint32_t)plan.plain_count : (uint32_t)plan.clean_count;
            if (!(slot < end && slot < FlowSplitListEntries((uint32_t)S))) return false;
            list[slot] = (uint32_t)(b * kFlowPlanBlock + t);
        }
    }
    return true;
}

// One ORDINARY tick of the object with a clean plane, whatever kinds call: sim_packets.cpp's OrdinaryTick with the clean input per
// session (the split tick's kernels run the tick body with or without one by the list a session is on).
Fail SplitOrdinaryTick(Object &o, int n, const uint8_t *flags, const int *ms, std::vector<Rows> &rows, int64_t *detail) {
    const int S = (int)o.ss.size();
    TickPlan plan;
    uint32_t tick_pos;
    if (!HostTick(o, n, 1, false, flags, &plan, &tick_pos)) return Fail{11, -1, 0};
    const FlowTickRoute route = plan.route;
    if (!route.launch) return Fail{};
    if (plan.split_tick && (plan.family != kTickFamily_split || !route.sparse_plan)) return Fail{12, -1, 0};
    if (detail && plan.split_tick) detail[SC_ORDINARY_SPLIT]++;
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
            if (!plan.mixed_plan && (half || q.fs != o.host.fs)) return Fail{8, s, 0};
            q.regs.v[F_NEAR_LAG] = FlowIdleTick(q.regs.v[F_NEAR_LAG], route.deferred_lag);
            if (q.regs.v[F_NEAR_LAG] != 0) {
                FlowNearMove m;
                FlowResync(q.regs, tick_pos, m);
                FlowMoveNear(q.near_ring.data(), (uint32_t)(kRingLen - 1), m);
                FlowMoveNear(q.clean_ring.data(), (uint32_t)(kRingLen - 1), m);      // (the object has a clean ring: everybody's row moves)
            }
            if (plan.mixed_plan) FlowTickMixed(q.regs, q.fs, n, ms[s], flags[s], tick_pos, planned);
            else FlowTick(q.regs, o.host.fs, n, ms[s], flags[s], tick_pos, planned);
        }
        if (const int field = q.StateDefect()) return Fail{100, s, field};
        Rows &w = rows[s];
        q.TickBody(planned, TakesClean(plan, flags[s]), n, tick_pos, w.far.data(), w.near.data(), w.clean.data(), w.out.data(), &w.bfar, &w.bnear, &w.bclean);
    }
    return Fail{};
}

// One tick of `calls` call pairs of the object with the switch on: the host's plan, the planning launch (one lane per session), the
// tick launches (one per list).  rows[s]: calls * n samples, packed for half calls.
Fail SplitCallsTick(Object &o, int n, int calls, bool packets, const uint8_t *flags, const int *ms, std::vector<Rows> &rows, int64_t *detail) {
    if (calls == 1) return SplitOrdinaryTick(o, n, flags, ms, rows, detail);      // the same launches, the same kernels
    const int S = (int)o.ss.size(), span = calls * n;
    TickPlan plan;
    uint32_t tick_pos;
    if (!HostTick(o, n, calls, packets, flags, &plan, &tick_pos) || plan.span != span) return Fail{11, -1, 0};
    const FlowTickRoute route = plan.route;
    if (!route.launch) {
        detail[SC_NOBODY]++;
        return Fail{};
    }
    const TickFamily want = plan.split_tick ? kTickFamily_split : plan.mixed_plan ? kTickFamily_packets : kTickFamily_calls;
    if (!route.sparse_plan || !route.sparse_tick || !plan.k_calls || plan.family != want || (plan.mixed_plan && !packets)) return Fail{12, -1, 0};
    if (plan.split_tick) {
        detail[plan.mixed_plan ? SC_SPLIT_PACKET_TICKS : SC_SPLIT_CALLS_TICKS]++;
        detail[plan.clean_count % kFlowSplitGroup == 0 ? SC_CLEAN_MULT4 : SC_CLEAN_OTHER]++;
    } else {
        detail[plan.clean_plane ? SC_ALL_CLEAN_TICKS : SC_ALL_PLAIN_TICKS]++;
    }
    // ---- the planning launch
    std::vector<int32_t> words((size_t)S * kFlowMaxTickCalls * kFlowPlanWords, 0);
    const auto words_of = [&](int s) { return reinterpret_cast<int32_t(*)[kFlowPlanWords]>(words.data() + (size_t)s * kFlowMaxTickCalls * kFlowPlanWords); };
    for (int s = 0; s < S; ++s) {
        Session &q = *o.ss[s];
        const bool idle = (flags[s] & kFlowIdle) != 0, half = !idle && (flags[s] & kFlowHalfCall) != 0;
        if (idle) {
            q.regs.v[F_NEAR_LAG] = FlowIdleTick(FlowIdleTick(q.regs.v[F_NEAR_LAG], route.deferred_lag), span);
            continue;
        }
        q.regs.v[F_NEAR_LAG] = FlowIdleTick(q.regs.v[F_NEAR_LAG], route.deferred_lag);
        if (q.regs.v[F_NEAR_LAG] != 0) {
            FlowNearMove m;
            FlowResync(q.regs, tick_pos, m);
            FlowMoveNear(q.near_ring.data(), (uint32_t)(kRingLen - 1), m);
            FlowMoveNear(q.clean_ring.data(), (uint32_t)(kRingLen - 1), m);
        }
        int defect = 0, startup_calls = 0;
        const auto sink = [&](int c, const FlowPlan &p) {
            FlowPackPlan(p, words_of(s)[c]);
            int32_t w[kFlowWords] = {0};                                          // a state BETWEEN two calls must be a valid one too
            for (int k = 0; k < kFlowFieldsUsed; ++k) w[k] = q.regs.v[k];
            if (const int field = FlowStateDefect(w)) defect = defect ? defect : field;
            startup_calls += p.n_blocks == 0;
        };
        if (plan.mixed_plan) {
            FlowTickPackets(q.regs, q.fs, n, calls, ms[s], flags[s], tick_pos, sink);
        } else {
            if (half || q.fs != o.host.fs) return Fail{8, s, 0};
            FlowTickCalls(q.regs, o.host.fs, n, calls, ms[s], flags[s], tick_pos, sink);
        }
        if (defect) return Fail{100, s, defect};
        if (const int field = q.StateDefect()) return Fail{100, s, field};
        if (plan.split_tick && (flags[s] & kFlowNoClean)) {
            detail[SC_HALF_PLAIN] += half;
            detail[SC_STARTUP_PLAIN_CALLS] += startup_calls;
        }
    }
    // ---- the tick launch(es): wavefront w of a launch serves entry w of its list
    int64_t scratch[kPacketsDetail] = {0};
    std::vector<int> served((size_t)S, 0);
    const auto serve = [&](uint32_t s, bool has_clean) {
        if (s >= (uint32_t)S) return false;
        served[s]++;
        PacketBody(*o.ss[s], has_clean, calls, words_of((int)s), tick_pos, rows[s], (flags[s] & kFlowHalfCall) != 0, scratch);
        return true;
    };
    if (plan.split_tick) {
        std::vector<uint32_t> list;
        if (!SplitLists(o.host, plan, flags, list)) return Fail{13, -1, 0};
        const uint32_t plain_start = FlowPlainListStart((uint32_t)plan.clean_count);
        for (int32_t i = 0; i < plan.clean_count; ++i)
            if (!serve(list[(size_t)i], true)) return Fail{13, i, 1};
        for (int32_t i = 0; i < plan.plain_count; ++i)
            if (!serve(list[plain_start + (size_t)i], false)) return Fail{13, i, 2};
    } else {
        for (int s = 0; s < S; ++s)
            if (!(flags[s] & kFlowIdle)) serve((uint32_t)s, plan.clean_plane);
    }
    for (int s = 0; s < S; ++s)
        if (served[s] != ((flags[s] & kFlowIdle) ? 0 : 1)) return Fail{13, s, 3};
    // every session on the list of its kind
    return Fail{};
}

}  // namespace

extern "C" {

int sim_split_calls_detail_words(void) { return kSplitCallsDetail; }

// An object of n_sessions sessions through n_ticks ticks, every tick with a clean plane.  rates_mode 0: both rates at random (every
// K-call tick is a packet tick); 1: every session at the object's rate (TickCalls and TickPackets forms at random, half calls in the
// latter).  Every session is of one kind (flagged AECM_SESSION_NO_CLEAN or not) until it is initialised anew, which switches it; with
// more than 64 sessions the first wavefront is all of one kind.  Ticks: K = 1 .. 6, about 30 % idle, ticks in which only flagged /
// only unflagged sessions call, ticks nobody makes, NO_FAREND, msInSndCardBuf anywhere, bursts.  Returns -1 when everything agreed,
// else the first tick that did not; detail[SC_WHAT] as sim_packets_fuzz's, and 13: a live list served a session twice, never, or one
// that is none (SC_FIELD: 1 clean list, 2 plain list, 3 the count).
int64_t sim_split_calls_fuzz(uint64_t seed, int n_sessions, int n_ticks, int rates_mode, int64_t *detail) {
    Rng rng{seed * 2654435761ull + 3333};
    for (int i = 0; i < kSplitCallsDetail; ++i) detail[i] = 0;
    Object dev, twin;
    const uint32_t starts[3] = {0u, 0xffffffffu - 0xffffffffu % 80u - 800u, (uint32_t)kFlowLagPeriod * 1000u - 400u};
    const int S = n_sessions;
    for (Object *o : {&dev, &twin}) {
        o->host.Init(n_sessions, (seed & 1) ? 16000 : 8000);
        o->has_clean = true;
        o->host.near_pos = starts[(seed / 4) % 3];
    }
    dev.host.split_call_ticks = true;                                          // (the twin never makes a tick that needs it)
    std::vector<uint8_t> kind((size_t)S, 0), flags((size_t)S);
    for (int s = 0; s < S; ++s) {
        const int fs = rates_mode == 0 ? (rng.chance(50) ? 16000 : 8000) : dev.host.fs;
        kind[s] = (s < 64 && S > 64) ? ((seed & 8) ? kFlowNoClean : 0) : (rng.chance(50) ? kFlowNoClean : 0);
        const uint32_t p0 = rng.chance(50) ? 0u : rng.next() * 7u;
        for (Object *o : {&dev, &twin}) {
            o->host.SetRate(s, fs);
            o->ss.emplace_back(new Session(fs));
            Session &q = *o->ss.back();
            q.regs.v[F_FAR_RP] = q.regs.v[F_FAR_WP] = (int32_t)p0;
            q.regs.v[F_FRM_POS] = q.regs.v[F_BLK_POS] = q.regs.v[F_OUT_RP] = (int32_t)(p0 * 3u);
        }
    }
    std::vector<int64_t> far_offered((size_t)S, 0), near_offered((size_t)S, 0);
    std::vector<int> half((size_t)S, 0), ms((size_t)S, 40);
    const auto fail = [&](const Fail &f) { detail[SC_WHAT] = f.what; detail[SC_SESSION] = f.session; detail[SC_FIELD] = f.field; };
    for (int64_t tick = 0; tick < n_ticks; ++tick) {
        const int n = rng.chance(dev.host.fs == 16000 ? 90 : 30) ? 160 : 80;
        const int calls = rng.chance(20) ? 1 : rng.range(2, kFlowMaxTickCalls);
        const bool packets = rates_mode == 0 || rng.chance(50);
        // ---- one session initialised anew, of the other kind from now on
        if (rng.chance(2)) {
            const int s = rng.range(0, S - 1);
            kind[s] ^= (uint8_t)kFlowNoClean;
            for (Object *o : {&dev, &twin}) {
                o->ss[s].reset(new Session(o->ss[s]->fs));
                o->host.InitSession(s, o->ss[s]->fs);
            }
            detail[SC_REINIT]++;
        }
        // ---- a far-end burst before the tick
        if (rng.chance(10)) {
            const int len = rng.chance(50) ? 80 : 160;
            for (int s = 0; s < S; ++s) {
                const int c = rng.chance(60) ? 0 : rng.range(1, 3);
                if (!c) continue;
                std::vector<int64_t> burst((size_t)c * len);
                for (size_t j = 0; j < burst.size(); ++j) burst[j] = far_offered[s] + (int64_t)j;
                far_offered[s] += (int64_t)burst.size();
                for (Object *o : {&dev, &twin}) o->ss[s]->BufferFarend(len, c, burst.data());
                for (int k = 0; k < c; ++k) dev.ss[s]->ref.BufferFarend(burst.data() + (size_t)k * len, (size_t)len);
                detail[SC_BURSTS]++;
            }
        }
        // ---- the tick's flags and rows
        const int who = rng.chance(3) ? 3 : rng.chance(8) ? 1 : rng.chance(8) ? 2 : 0;      // 3 nobody, 1 only flagged, 2 only unflagged sessions call
        std::vector<int> n_s((size_t)S, 0), ms_now((size_t)S);
        for (int s = 0; s < S; ++s) {
            if (rng.chance(5)) half[s] = rng.chance(40);
            uint8_t f = kind[s];
            if (rng.chance(12)) f |= kFlowNoFarend;
            if (n == 160 && packets && half[s]) f |= kFlowHalfCall;
            const bool idle = who == 3 || (who == 1 && !kind[s]) || (who == 2 && kind[s]) || rng.chance(30);
            if (idle) f = (uint8_t)(kFlowIdle | (rng.next() & 27u));                          // an idle session's other bits mean nothing
            flags[s] = f;
            if (rng.chance(10)) ms[s] = rng.chance(50) ? rng.range(0, 60) : rng.range(250, 400);
            ms_now[s] = rng.chance(3) ? (rng.chance(50) ? -300 : 700) : ms[s];
            n_s[s] = idle ? 0 : FlowPacketCallSize(n, f);
        }
        const int span = calls * n;
        std::vector<Rows> rows((size_t)S), trows((size_t)S), tall((size_t)S);
        for (int s = 0; s < S; ++s) {
            Rows &w = rows[s];
            w.far.assign((size_t)span, kJunk); w.near.assign((size_t)span, kJunk); w.clean.assign((size_t)span, kJunk); w.out.assign((size_t)span, kSentinel);
            const int mine = calls * n_s[s];
            for (int j = 0; j < mine; ++j) {
                w.far[j] = far_offered[s] + j;
                w.near[j] = kNearTagBase + near_offered[s] + j;
                if (!kind[s]) w.clean[j] = kCleanTagBase + near_offered[s] + j;               // a flagged session's clean row: junk, all K pieces
            }
            far_offered[s] += mine;
            near_offered[s] += mine;
            tall[s].out.assign((size_t)span, kSentinel);
        }
        // ---- the device: one tick of K calls
        if (const Fail f = SplitCallsTick(dev, n, calls, packets, flags.data(), ms_now.data(), rows, detail)) { fail(f); return tick; }
        // ---- the twin: K ordinary (split) ticks on re-laid rows
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
            if (const Fail f = SplitOrdinaryTick(twin, n, flags.data(), ms_now.data(), trows, nullptr)) { fail(Fail{f.what + 1000, f.session, f.field}); return tick; }
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
        // ---- per session: the twin, the state, the reference
        for (int s = 0; s < S; ++s) {
            Session &q = *dev.ss[s], &t = *twin.ss[s];
            Rows &w = rows[s];
            const int32_t l = q.regs.v[F_NEAR_LAG];
            if (l < 0 || l >= kFlowLagPeriod || l % kFlowFrame != 0) { fail(Fail{9, s, 0}); return tick; }
            for (int k = 0; k < kFlowTickFields; ++k)
                if (q.regs.v[k] != t.regs.v[k]) { fail(Fail{20, s, k + 1}); return tick; }
            if (dev.host.near_pos != twin.host.near_pos) { fail(Fail{20, s, F_NEAR_LAG + 1}); return tick; }
            if (dev.host.history.Get(s) != twin.host.history.Get(s)) { fail(Fail{22, s, 0}); return tick; }
            if (SnapshotModel(dev, q) != SnapshotModel(twin, t)) { fail(Fail{21, s, 0}); return tick; }
            if (w.out != tall[s].out || w.bfar != tall[s].bfar || w.bnear != tall[s].bnear || w.bclean != tall[s].bclean) { fail(Fail{6, s, 0}); return tick; }
            if (n_s[s] == 0) {
                for (int j = 0; j < span; ++j)
                    if (w.out[j] != kSentinel) { fail(Fail{7, s, 0}); return tick; }
                continue;
            }
            const bool takes_clean = !kind[s];
            std::vector<int64_t> rfar, rnear, rclean, out_ref((size_t)span, kSentinel);
            for (int c = 0; c < calls; ++c) {
                if (!(flags[s] & kFlowNoFarend)) q.ref.BufferFarend(w.far.data() + c * n_s[s], (size_t)n_s[s]);
                (void)q.ref.Process(w.near.data() + c * n_s[s], takes_clean ? w.clean.data() + c * n_s[s] : nullptr, out_ref.data() + c * n_s[s], (size_t)n_s[s],
                                    (int16_t)ms_now[s], [&](const int64_t *fb, const int64_t *nb, const int64_t *cb, int64_t *ob, int nblk) {
                                        rfar.insert(rfar.end(), fb, fb + nblk * kFlowBlock);
                                        rnear.insert(rnear.end(), nb, nb + nblk * kFlowBlock);
                                        if (cb) rclean.insert(rclean.end(), cb, cb + nblk * kFlowBlock);
                                        for (int j = 0; j < nblk * kFlowBlock; ++j) ob[j] = kOutTagBase + q.ref_blocks * kFlowBlock + j;
                                        q.ref_blocks += nblk;
                                        return true;
                                    });
            }
            detail[SC_BLOCKS] += (int64_t)rfar.size() / kFlowBlock;
            int what = 0;
            if (w.bfar.size() != rfar.size()) what = 1;
            else if (w.bfar != rfar) what = 2;
            else if (w.bnear != rnear) what = 3;
            else if (w.bclean != rclean) what = 4;
            else if (w.out != out_ref) what = 5;
            if (what) { fail(Fail{what, s, 0}); return tick; }
        }
    }
    return -1;
}

// ---- the host's planner with the switch, for a table of plans (tests/test_split_calls.py) ----------------------------------------
void *sim_split_calls_object_new(int32_t n_sessions, int32_t fs) {
    TickObject *o = new TickObject();
    o->Init(n_sessions, fs);
    return o;
}
void sim_split_calls_object_free(void *o) { delete static_cast<TickObject *>(o); }
void sim_split_calls_object_init(void *o) {
    TickObject *p = static_cast<TickObject *>(o);
    p->Init(p->n_sessions, p->fs);
}
void sim_split_calls_object_init_session(void *o, int32_t session, int32_t fs) { static_cast<TickObject *>(o)->InitSession(session, fs); }
void sim_split_calls_object_switch(void *o, int32_t on) { static_cast<TickObject *>(o)->split_call_ticks = on != 0; }
int32_t sim_split_calls_object_get_switch(void *o) { return static_cast<TickObject *>(o)->split_call_ticks; }
int32_t sim_split_calls_object_call_trace(void *o, int32_t on) { return static_cast<TickObject *>(o)->AttachCallTrace(on != 0); }
int32_t sim_split_calls_object_session_trace(void *o, int32_t on) { return static_cast<TickObject *>(o)->AttachTrace(on != 0); }
// args = {n, calls, packets, has_clean, fast variant}; plan = {family, live, span, k_calls, mixed_plan, split_tick, clean_plane,
// clean_count, plain_count, sparse_tick, half_calls, checked}.  Returns the code; an accepted tick is committed.
int32_t sim_split_calls_object_tick(void *o, const uint8_t *flags, const int32_t *args, int32_t *plan) {
    TickObject &obj = *static_cast<TickObject *>(o);
    TickArgs a;
    a.flags_per_session = flags;
    a.n = args[0];
    a.calls = args[1];
    a.packets = args[2] != 0;
    a.has_clean = args[3] != 0;
    TickPlan p;
    p.code = obj.CheckArgs(true, true, flags, 0, (size_t)a.n, a.calls, (int64_t)a.n * a.calls, a.packets, false, args[4] != 0);
    if (!p.code) p = obj.Plan(a);
    if (p.code) return p.code;
    obj.Commit(p);
    const int32_t v[12] = {(int32_t)p.family, p.live, p.span, p.k_calls, p.mixed_plan, p.split_tick, p.clean_plane, p.clean_count, p.plain_count,
                           p.route.sparse_tick, p.half_calls, p.clean_tick.checked};
    for (int i = 0; i < 12; ++i) plan[i] = v[i];
    return 0;
}
const char *sim_split_calls_family_name(int32_t family) { return TickFamilyName(family); }
// rest = {near_pos, split_used, call_trace_calls, deferred_lag}
void sim_split_calls_object_state(void *o, uint8_t *modes, int64_t *rest) {
    TickObject *p = static_cast<TickObject *>(o);
    for (int32_t s = 0; s < p->n_sessions; ++s) modes[s] = p->history.Get(s);
    rest[0] = p->near_pos;
    rest[1] = p->history.split_used;
    rest[2] = p->call_trace_calls;
    rest[3] = p->lag.deferred_lag;
}

}  // extern "C"

#if defined(SIM_SPLIT_CALLS_MAIN)
int main() {
    int64_t detail[kSplitCallsDetail];
    const int sizes[4] = {6, 11, 70, 300};
    for (uint64_t seed = 0; seed < 8; ++seed) {
        const int S = sizes[seed % 4];
        const int64_t tick = sim_split_calls_fuzz(seed, S, S > 64 ? 20 : 150, seed % 3 == 2 ? 1 : 0, detail);
        if (tick != -1) {
            printf("seed %llu: tick %lld what %lld session %lld field %lld\n", (unsigned long long)seed, (long long)tick, (long long)detail[SC_WHAT],
                   (long long)detail[SC_SESSION], (long long)detail[SC_FIELD]);
            return 1;
        }
    }
    // the switch: off, a split tick of two calls is unsupported and changes nothing; on, it is planned; under a call trace it is not
    TickObject o;
    o.Init(8, 16000);
    const uint8_t mixed[8] = {0, 16, 0, 16, 4, 4 | 16, 0, 16};
    TickArgs a;
    a.flags_per_session = mixed;
    a.calls = 2;
    a.has_clean = true;
    if (o.Tick(a).code != kTickUnsupported || o.near_pos != 0) return 2;
    o.split_call_ticks = true;
    const TickPlan p = o.Tick(a);
    if (p.code || p.family != kTickFamily_split || !p.k_calls || p.mixed_plan || p.span != 320 || o.near_pos != 320) return 3;
    if (!o.AttachCallTrace(true) || o.Tick(a).code != kTickUnsupported || o.near_pos != 320 || o.call_trace_calls != 0) return 4;
    printf("ok\n");
    return 0;
}
#endif
