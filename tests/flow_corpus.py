"""TEST INFRASTRUCTURE: the session-flow decision corpus.  Seeded, deterministic scenarios for the session wrapper's decision path
(webrtc_aecm_amd/csrc/aecm_flow_plan.h: FlowTick, FlowStartup, FlowEstBufDelay, FlowDelayComp, FlowMoveFarReadPtr, FlowFarendCall,
FlowBurstBegin, FlowResync, FlowMoveNear, FlowTickMixed / Calls / Packets, FlowLiveSlot), laid out over the 300 sessions of one object
so that the 64 sessions of a planning wavefront sit in different scenarios and phases: session s runs scenario s mod M, started
s div M ticks late (idle ticks where the entry point has them, a start-up history of alternating msInSndCardBuf where it has not).
300 sessions are two planning workgroups (256 + 44 lanes: the last wavefront is partial) and 75 tick workgroups.

A scenario is a few lines: rate, call size, and per call of its own the msInSndCardBuf, the flags (NO_FAREND, SPLIT_CALLS, for a
16 kHz session of a mixed object HALF_CALL), far-end calls made before it (bursts), optionally an imported start state (a start-up
phase that has run for `preroll` calls without a far end; position counters standing short of 2^31 / 2^32).  `schedule(family)`
turns the scenarios an entry point admits into the arrays of one object's run: tools/flow_coverage.py measures them on the host
(tests/sim/sim_flowcov.cpp), tests/test_gpu_flow_corpus.py runs them on the device and on the reference."""
from __future__ import annotations

import numpy as np

NO_FAREND, SPLIT_CALLS, IDLE, HALF_CALL = 1, 2, 4, 8
S = 300
T_OWN = 140                                     # calls of its own every session makes
IDLE_SLACK = 30                                 # idle ticks every session of an entry point with idle ticks gets on top of its late start
GAP_AT = 60                                     # ... and from this tick on a stretch of ticks NOBODY makes (nothing is launched: the lag is
                                                # deferred), family["gap"] ticks long
IMPORT_ROWS = 2                                 # sessions s div M < IMPORT_ROWS carry their scenario's imported start state


def _const(v):
    return lambda T, rng: np.full(T, v, dtype=np.int64)


def _zeros(T, rng):
    return np.zeros(T, dtype=np.int64)


def _sc(name, fs, n, ms, flags=_zeros, burst=_zeros, half=None, preroll=0, preroll_ms=40, far_off=0, frm_off=0, seed=0):
    return dict(name=name, fs=fs, n=n, ms=ms, flags=flags, burst=burst, half=half, preroll=preroll, preroll_ms=preroll_ms, far_off=far_off,
                frm_off=frm_off, seed=seed)


def _ranges(*spans):
    """spans: (first, last, value) -> fn(T, rng) that is 0 elsewhere."""
    def fn(T, rng):
        a = np.zeros(T, dtype=np.int64)
        for first, last, v in spans:
            a[first:last] |= v
        return a
    return fn


def _steps_ms(*spans, base=40):
    def fn(T, rng):
        a = np.full(T, base, dtype=np.int64)
        for first, last, v in spans:
            a[first:last] = v
        return a
    return fn


def _random_ms(lo, hi, wild=0.0, walk=False):
    def fn(T, rng):
        if walk:
            a = np.clip(40 + np.cumsum(rng.integers(-6, 7, T)), 0, 500)
        else:
            a = rng.integers(lo, hi + 1, T)
        w = rng.random(T) < wild
        a[w] = np.where(rng.random(int(w.sum())) < 0.5, -300, 700)
        return a.astype(np.int64)
    return fn


def _random_flags(p_nofar, p_split=0.0, runs=()):
    def fn(T, rng):
        a = (rng.random(T) < p_nofar).astype(np.int64) * NO_FAREND | (rng.random(T) < p_split).astype(np.int64) * SPLIT_CALLS
        for first, last, v in runs:
            a[first:last] |= v
        return a
    return fn


def _random_burst(p, hi, big=()):
    def fn(T, rng):
        a = np.where(rng.random(T) < p, rng.integers(1, hi + 1, T), 0).astype(np.int64)
        for t, v in big:
            a[t] = v
        return a
    return fn


def scenarios(without=()):
    """The corpus.  What each scenario is there for stands next to it; tools/flow_coverage.py --without NAME shows what depends on it."""
    near31, near32 = (1 << 31) - 1000, (1 << 32) - 1400
    sc = [
        # the reference CLI's cadence: start-up by the counter limit, filled < / == bufSizeStart, direct ticks, one and two blocks per frame
        _sc("cli16", 16000, 160, _const(40), far_off=near32, frm_off=near31),
        _sc("cli8", 8000, 80, _const(40), far_off=near31, frm_off=near32),
        # msInSndCardBuf that fails the start-up tolerance by either operand until checkBufSizeCtr runs out (> 50), the last value high
        # enough for the min(., 50) clamp; out-of-range values; then underruns
        _sc("jumpy16", 16000, 160, _steps_ms((0, 60, -1), (56, 58, 700), (90, 100, -300)), _ranges((70, 85, NO_FAREND)), seed=1),
        _sc("jumpy8", 8000, 80, _steps_ms((0, 60, -1), (80, 84, 700)), _ranges((100, 130, NO_FAREND)), seed=2),
        # a high constant delay: the mean clamps to 50 frames, the jitter buffer fills to its capacity (calls truncated to nothing),
        # delay compensation fires against a full buffer (n_add at its floor, the read pointer move clamped by what is free)
        _sc("high_ms16", 16000, 160, _const(450), _ranges((60, 64, NO_FAREND))),
        _sc("high_ms8", 8000, 160, _const(470), _ranges((75, 80, NO_FAREND))),
        # delay steps 10 <-> 480 ms: delay compensation at its ceiling, every arm of the delay estimator's diff test, timeForDelayChange
        # past 25 on the way up (knownDelay > 0) and on the way down (max(filtDelay - 160, 0) = 0)
        _sc("delay_step16", 16000, 160, _steps_ms((8, 52, 480), (52, 96, 10), (96, 126, 300), base=10), _random_flags(0.02), seed=3),
        _sc("delay_step8", 8000, 80, _steps_ms((8, 50, 480), (50, 100, 0), (100, 125, 250), base=10), _random_flags(0.03), seed=4),
        # two 80-sample calls per tick leave replay slot 1 unused until its frame is about to leave the far ring (the spill), then a run
        # of underruns replays both slots: slot 0 from the ring, slot 1 from its row; in the second the slot is refreshed in the spill's tick
        _sc("spill_row16", 16000, 160, _random_ms(35, 45), _ranges((12, 78, SPLIT_CALLS), (70, 100, NO_FAREND)), seed=5),
        _sc("spill_refresh16", 16000, 160, _random_ms(35, 45), _ranges((12, 56, SPLIT_CALLS), (100, 112, NO_FAREND)), seed=6),
        # ... and in the third a far-end burst laps the slot's frame first (FlowBurstBegin moves it to its row)
        _sc("spill_burst16", 16000, 160, _random_ms(35, 45), _ranges((12, 90, SPLIT_CALLS)), _ranges((46, 47, 30)), seed=14),
        # a start-up phase that waits for 50 buffered frames in two 80-sample calls per tick and ends in a tick's FIRST call: frame 0 is
        # the start-up copy, frame 1 is active
        _sc("split_startup16", 16000, 160, _const(450), _ranges((7, 60, SPLIT_CALLS)), _ranges((7, 8, 1)), seed=15),
        # 16 kHz in 80-sample calls (nBlocks10ms = 0: neither start-up limit fires), imported with counters a few calls short of 32 767:
        # they wrap, then 160-sample calls compare them as size_t; the calls of 80 are half calls of a mixed object
        _sc("wrap_counter16", 16000, 160, _steps_ms(base=41), half=_ranges((0, 90, 1)), preroll=32700, preroll_ms=41, seed=7),
        # far-end bursts: the jitter buffer overflows (calls truncated to fewer samples than offered), replay frames are lapped
        _sc("bursty16", 16000, 160, _random_ms(0, 300), _random_flags(0.35, 0.3), _random_burst(0.3, 4, big=((60, 30), (100, 60))), seed=8),
        _sc("bursty8", 8000, 80, _random_ms(0, 200, wild=0.03), _random_flags(0.3), _random_burst(0.25, 3, big=((70, 55),)), seed=9),
        # everything at random
        _sc("random16", 16000, 160, _random_ms(0, 500, wild=0.03), _random_flags(0.3, 0.3), half=lambda T, rng: (rng.random(T) < 0.3).astype(np.int64), seed=10),
        _sc("walk16", 16000, 160, _random_ms(0, 0, walk=True), _random_flags(0.08, 0.5), seed=11),
        _sc("random8", 8000, 160, _random_ms(0, 200), _random_flags(0.25), seed=12),
        # a delay that ramps up while timeForDelayChange runs out and then drops: diff < 96 with knownDelay > 0 right after diff > 224
        _sc("ramp16", 16000, 160, lambda T, rng: np.where(np.arange(T) < 56, np.clip(60 + 9 * (np.arange(T) - 8), 10, 500), 0).astype(np.int64), seed=16),
        _sc("ramp8", 8000, 80, lambda T, rng: np.where(np.arange(T) < 62, np.clip(40 + 8 * (np.arange(T) - 6), 10, 500), 0).astype(np.int64), seed=17),
        # the delay step again, later: its way up meets delay_step8's way down in the same ticks (the two sides of max(filtDelay - 160, 0))
        _sc("delay_step16b", 16000, 160, _steps_ms((48, 100, 480), base=10), seed=18),
        # no delay at all at 8 kHz: bufSizeStart is 0, the start-up phase ends on an EMPTY jitter buffer and the first frames are replays
        # of rows nothing was ever copied to
        _sc("zero_delay8", 8000, 80, _const(0), _ranges((0, 100, NO_FAREND)), seed=19),
        # a 16 kHz session on half calls for so long that replay slot 1 leaves the far ring inside the mixed and the packets planner
        _sc("half_spill16", 16000, 160, _random_ms(38, 44), _ranges((132, 140, NO_FAREND)), half=_ranges((24, 132, 1)), seed=20),
        # ... and one whose first full call comes in the very tick the slot has aged: the spill and the refresh in one tick
        _sc("half_refresh16", 16000, 160, _const(40), half=_ranges((24, 112, 1)), seed=21),
        _sc("underrun8", 8000, 80, _random_ms(0, 80), _random_flags(0.0, runs=((30, 40, NO_FAREND), (80, 90, NO_FAREND))), seed=13),
    ]
    assert len({c["name"] for c in sc}) == len(sc)
    return [c for c in sc if c["name"] not in without]


# family: object rate, tick samples, kind 0 tick / 1 calls / 2 packets, K, idle ticks, forced sparse, which scenarios it admits.  gap: the
# ticks nobody makes.  Every seventh session sits out the two ticks before them too; where its calls are 80 samples that is a lag of
# 16 400 (205 x 80 at 8 kHz; 80 + 102 x 160 after a half call; 239 x 240 = 16 400 + 40 960 on three calls of 80) -- a ring distance of
# 16, fewer than the 32 or 48 pending samples such a session can have: the backward copy of FlowMoveNear.  (Pending samples come in
# multiples of 16 and lags in multiples of 80: a ring distance below 48 needs a lag of 16 400 or 32 800.)
FAMILIES = {
    "dense16": dict(fs=16000, n=160, kind=0, K=1, idle=False, force=False, admits=lambda c: c["fs"] == 16000 and c["half"] is None),
    "dense8": dict(fs=8000, n=80, kind=0, K=1, idle=False, force=False, admits=lambda c: c["fs"] == 8000 and c["n"] == 80),
    "sparse16": dict(gap=100, fs=16000, n=160, kind=0, K=1, idle=True, force=False, admits=lambda c: c["fs"] == 16000 and c["half"] is None),
    "forced8": dict(gap=203, fs=8000, n=80, kind=0, K=1, idle=True, force=True, admits=lambda c: c["fs"] == 8000 and c["n"] == 80),
    "mixed": dict(gap=100, fs=16000, n=160, kind=0, K=1, idle=True, force=False, admits=lambda c: True),
    "calls2": dict(gap=100, fs=16000, n=160, kind=1, K=2, idle=True, force=False, admits=lambda c: c["fs"] == 16000 and c["half"] is None),
    "calls3": dict(gap=237, fs=8000, n=80, kind=1, K=3, idle=True, force=False, admits=lambda c: c["fs"] == 8000 and c["n"] == 80),
    "calls6": dict(gap=100, fs=16000, n=160, kind=1, K=6, idle=True, force=False, admits=lambda c: c["fs"] == 16000 and c["half"] is None),
    "packets2": dict(gap=100, fs=16000, n=160, kind=2, K=2, idle=True, force=False, admits=lambda c: True),
}


def schedule(family, without=(), sessions=S, t_own=T_OWN):
    """The run of one object: dict(fs, n, K, kind, force, T, rates[S], flags[T, S] uint8, ms[T, S] int16, burst[T, S] uint8, burst_len,
    preroll[S], preroll_ms[S], far_off[S], frm_off[S] uint32, names[S]).  A K-call entry point takes K of a scenario's calls per tick with
    the first one's msInSndCardBuf and flags (NO_FAREND and HALF_CALL only: its documented refusals); SPLIT_CALLS goes where the tick is
    160 samples and the session's call fills it."""
    fam = FAMILIES[family]
    sc = [c for c in scenarios(without) if fam["admits"](c)]
    M, K, n = len(sc), fam["K"], fam["n"]
    ticks_own = t_own // K
    late = (sessions - 1) // M
    T = ticks_own + late + (IDLE_SLACK + fam["gap"] if fam["idle"] else 0)
    rates = np.array([sc[s % M]["fs"] for s in range(sessions)], dtype=np.int32)
    flags = np.zeros((T, sessions), dtype=np.uint8)
    ms = np.full((T, sessions), 40, dtype=np.int16)
    burst = np.zeros((T, sessions), dtype=np.uint8)
    preroll, preroll_ms = np.zeros(sessions, dtype=np.int32), np.full(sessions, 40, dtype=np.int16)
    far_off, frm_off = np.zeros(sessions, dtype=np.uint32), np.zeros(sessions, dtype=np.uint32)
    idle_rng = np.random.default_rng(977)
    for s in range(sessions):
        c, d = sc[s % M], s // M
        rng = np.random.default_rng(1000 * c["seed"] + 17)
        c_ms, c_flags, c_burst = c["ms"](t_own, rng), c["flags"](t_own, rng), c["burst"](t_own, rng)
        c_half = c["half"](t_own, rng) if c["half"] is not None else np.zeros(t_own, dtype=np.int64)
        if d < IMPORT_ROWS:
            preroll[s], preroll_ms[s] = c["preroll"], c["preroll_ms"]
            far_off[s] = (c["far_off"] - 160 * d) & 0xffffffff if c["far_off"] else 0
            frm_off[s] = (c["frm_off"] - 64 * d) & 0xffffffff if c["frm_off"] else 0
        first = c_ms[0]
        # -1: the alternating history -- per TICK of this entry point (the K calls of a tick share their msInSndCardBuf), so that the
        # counter never reaches 6 and checkBufSizeCtr runs out instead, in the tick that holds call 50
        c_ms = np.where(c_ms == -1, np.where((np.arange(t_own) // K) % 2 == 0, 40, 100 + 20 * (s % 5)), c_ms)
        if first == -1:
            c_ms[50 // K * K:50 // K * K + K] = 40 if d % 2 else 480   # what checkBufSizeCtr > 50 takes: below and above the min(., 50) clamp
        own_n = c["n"]                                             # the session's full call; a mixed object's tick is 160 for everybody
        half_always = own_n < n                                    # an 80-sample caller in a 160-sample tick: half calls throughout
        if fam["idle"]:
            # late by d idle ticks, then idle at random; everybody sits out the gap, every seventh session the two ticks before it too
            own_ticks = np.ones(T, dtype=bool)
            own_ticks[:d] = False
            own_ticks[GAP_AT:GAP_AT + fam["gap"]] = False
            if s % 7 == 3:
                own_ticks[GAP_AT - 2:GAP_AT] = False
            extra = int(own_ticks.sum()) - ticks_own
            own_ticks[idle_rng.choice(np.flatnonzero(own_ticks)[1:], size=extra, replace=False)] = False
            flags[~own_ticks, s] = IDLE
            where = np.flatnonzero(own_ticks)
            assert where.size == ticks_own
        else:
            # late by d ticks of a start-up history that never settles (no far end, msInSndCardBuf alternating)
            where = np.arange(d, d + ticks_own)
            for t in range(d):
                flags[t, s], ms[t, s] = NO_FAREND, (40 if t % 2 == 0 else 300)
            flags[d + ticks_own:, s] = NO_FAREND
        for k, t in enumerate(where):
            j = k * K
            f = int(c_flags[j]) & NO_FAREND
            if K == 1 and n == 160 and own_n == 160 and not c_half[j]:
                f |= int(c_flags[j]) & SPLIT_CALLS
            if half_always or (c_half[j] and fam["kind"] != 1 and family in ("mixed", "packets2")):
                f |= HALF_CALL
            flags[t, s] = f
            ms[t, s] = c_ms[j]
            burst[t, s] = min(int(c_burst[j:j + K].sum()), 255)
    return dict(family=family, fs=fam["fs"], n=n, K=K, kind=fam["kind"], force=fam["force"], T=T, rates=rates, flags=flags, ms=ms, burst=burst,
                burst_len=80, preroll=preroll, preroll_ms=preroll_ms, far_off=far_off, frm_off=frm_off,
                names=[sc[s % M]["name"] for s in range(sessions)], M=M)


REFRESH_AT = 21                                 # (found with tools/flow_coverage.py: the tick in which some sessions' slot has just aged)


def schedule_calls_spill(sessions=S):
    """The replay-row spill INSIDE a K-call tick (calls_helpers.SPILL_RECIPE), divergently: a 16 kHz object makes ordinary ticks of 160
    samples (a session joins 0 .. 11 ticks late: its start-up phase ends, farendOld[1] lives in the far ring), then 24 ticks of six, five or
    four calls of 80 samples (one of them two calls of 160: whose slot aged right then has it refreshed in the same call) (only farendOld[0] is refreshed; after some 98 calls of 80 -- fewer for who joined early, more for who idled or had
    no far end -- the ring's write position laps farendOld[1], which moves to its row in the middle of a tick's calls), then
    ticks of 160 without a far end that replay both slots.  The same dict as schedule(), n and kind per tick."""
    pre, k_ticks, post = 24, 24, 8
    T = pre + k_ticks + post
    rng = np.random.default_rng(4242)
    flags = np.zeros((T, sessions), dtype=np.uint8)
    ms = np.broadcast_to((35 + np.arange(sessions) % 11).astype(np.int16), (T, sessions)).copy()
    late = (np.arange(sessions) // 7) % 12
    flags[np.arange(T)[:, None] < late[None, :]] = IDLE
    mid = slice(pre, pre + k_ticks)
    flags[mid] |= (rng.random((k_ticks, sessions)) < 0.1).astype(np.uint8) * NO_FAREND
    flags[mid] |= (rng.random((k_ticks, sessions)) < 0.1).astype(np.uint8) * IDLE
    flags[pre + k_ticks:] = NO_FAREND
    # every fifth session reports no delay at all: its bufSizeStart is ONE frame, its jitter buffer holds one frame between calls, and it
    # makes the refreshing tick without a far end -- frame 1 of that call is a replay, its aged slot is NOT refreshed there
    shallow = np.arange(sessions) % 5 == 2
    ms[:, shallow] = 0
    flags[pre + REFRESH_AT, shallow] = NO_FAREND
    n = np.where((np.arange(T) >= pre) & (np.arange(T) < pre + k_ticks), 80, 160)
    calls = np.where(n == 80, 6 - np.arange(T) % 3, 1)      # 6, 5, 4 calls in turn: the slot's age at a tick's start takes every residue
    n[pre + REFRESH_AT], calls[pre + REFRESH_AT] = 160, 2            # two calls of 160 in the tick in which the slot of some sessions has just aged: refreshed
    z = np.zeros(sessions, dtype=np.int32)
    return dict(family="calls6_spill", fs=16000, n=n, K=calls, kind=(calls > 1).astype(np.int32), force=False, T=T, rates=np.full(sessions, 16000, dtype=np.int32),
                flags=flags, ms=ms, burst=np.zeros((T, sessions), dtype=np.uint8), burst_len=80, preroll=z, preroll_ms=np.full(sessions, 40, dtype=np.int16),
                far_off=z.astype(np.uint32), frm_off=z.astype(np.uint32), names=["calls_spill"] * sessions, M=1)


def schedules(without=()):
    """Every object of the corpus."""
    return [schedule(f, without=without) for f in FAMILIES] + ([] if "calls_spill" in without else [schedule_calls_spill()])


# ---- the corpus as audio: signals, the layout of a tick, one WebRtcAecm_* instance per session -------------------------------------
GOLDEN_NAMES = {f: f"sessflow_{f}" for f in list(FAMILIES) + ["calls6_spill"]}      # tools/gen_golden.py: the unmodified reference's runs


def family_schedule(family):
    return schedule_calls_spill() if family == "calls6_spill" else schedule(family)


def tick_layout(sch, t):
    """(n, K, kind, n_s[S]: samples of ONE call of each session (0: it sits the tick out), calls[S]: call pairs it makes)."""
    T, sessions = sch["flags"].shape
    n, K, kind = (int(np.broadcast_to(sch[k], T)[t]) for k in ("n", "K", "kind"))
    K = K if kind else 1
    fl = sch["flags"][t]
    n_s = np.where((fl & HALF_CALL) != 0, 80, n)
    n_s[(fl & IDLE) != 0] = 0
    return n, K, kind, n_s, np.where(n_s > 0, K, 0)


def signals(sch):
    """far[S, L], near[S, L] int16 for a schedule: noise, the near end an echo of it plus a talker of its own -- cheap, different for
    every session, long enough for every call and burst of the run."""
    T, sessions = sch["flags"].shape
    need = np.zeros(sessions, dtype=np.int64)
    for t in range(T):
        _, _, _, n_s, calls = tick_layout(sch, t)
        need += n_s * calls
    L = int((need + sch["burst"].astype(np.int64).sum(axis=0) * sch["burst_len"]).max()) + 160
    rng = np.random.default_rng(31337 + len(sch["family"]) + T)
    far = rng.integers(-6000, 6000, (sessions, L), dtype=np.int16)
    near = (np.roll(far, 37, axis=1) // 2 + rng.integers(-900, 900, (sessions, L), dtype=np.int16)).astype(np.int16)
    return far, near


def drive_reference(sch, far, near, make_session, workers=16):
    """Every session of the schedule on a WebRtcAecm_* instance of its own (make_session(fs)): its preroll (Process calls of 80 samples
    without a far end -- the state the device session is imported with), then tick by tick its bursts and its call pairs, at its own
    rate and call size; an idle tick is no call.  Returns (out: per session the samples its calls delivered, in order, [S, max] zero
    padded; codes[T, S]: the first non-zero return code of a tick; paths[S, 65])."""
    from concurrent.futures import ThreadPoolExecutor
    T, sessions = sch["flags"].shape
    layouts = [tick_layout(sch, t) for t in range(T)]
    total = np.zeros(sessions, dtype=np.int64)
    for _, _, _, n_s, calls in layouts:
        total += n_s * calls
    out = np.zeros((sessions, int(total.max())), dtype=np.int16)
    codes = np.zeros((T, sessions), dtype=np.int32)
    paths = np.zeros((sessions, 65), dtype=np.int16)
    blen = int(sch["burst_len"])

    def one(s):
        sess = make_session(int(sch["rates"][s]))
        junk = np.full(80, -12345, dtype=np.int16)
        for _ in range(int(sch["preroll"][s])):
            sess.process(junk, None, int(sch["preroll_ms"][s]))
        cf = cn = 0
        for t, (n, K, kind, n_s, calls) in enumerate(layouts):
            for _ in range(int(sch["burst"][t, s])):
                assert sess.buffer_farend(far[s, cf:cf + blen]) == 0
                cf += blen
            if not calls[s]:
                continue
            f, ms, k = int(sch["flags"][t, s]), int(sch["ms"][t, s]), int(n_s[s])
            pairs = [(80, 2)] if (f & SPLIT_CALLS) and k == 160 and not kind else [(k, int(calls[s]))]
            for ln, cnt in pairs:
                for _ in range(cnt):
                    if not f & NO_FAREND:
                        assert sess.buffer_farend(far[s, cf:cf + ln]) == 0
                        cf += ln
                    rc, o = sess.process(near[s, cn:cn + ln], None, ms)
                    out[s, cn:cn + ln] = o
                    cn += ln
                    codes[t, s] = codes[t, s] or rc
        rc, paths[s] = sess.get_echo_path()
        assert rc == 0 and cn == total[s]
    with ThreadPoolExecutor(max_workers=workers) as ex:
        list(ex.map(one, range(sessions)))
    return out, codes, paths


def summary(out, codes, paths):
    """What a fixture keeps of the reference's run: a SHA-256 of every session's output, the (tick, session, code) triples of the
    non-zero codes, the final echo paths."""
    import hashlib
    t, s = np.nonzero(codes)
    return dict(sha256=np.array([hashlib.sha256(np.ascontiguousarray(row).tobytes()).hexdigest() for row in out]),
                codes=np.stack([t, s, codes[t, s]], axis=1).astype(np.int32), paths=np.asarray(paths, dtype=np.int16))
