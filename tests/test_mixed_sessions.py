"""Objects of mixed sampling rates and call sizes without a GPU (WebRtcAecmSessions_InitRates / InitSessionRate /
GetSessionRate / ImportSessionAnyRate, AECM_SESSION_HALF_CALL): the object model on sample tags against one generic wrapper per
session at its own rate and call sizes (tests/sim/sim_mixed.cpp), the launch routing (an object that uses none of it routes as
before), the host's argument checks, the exported interface, and the recorded reference runs tests/golden/sessmixed_*.npz."""
import subprocess

import numpy as np
import pytest

import mixed_helpers as mh
import mixed_sim

LAG_PERIOD = 40960
STARTS = (0, 0xffffffff - 0xffffffff % 80 - 800, (LAG_PERIOD * 1000 - 400) & 0xffffffff)      # 0, just below 2^32, just below a multiple of the lag period


def test_mixed_object_equals_one_wrapper_per_session_on_sample_tags():
    """48 seeds x 600 ticks x 6 sessions (mixed_sim.FUZZ_PLAN): 24 seeds of objects that hold both rates, 12 of uniform objects whose
    sessions make half calls, 12 of uniform objects without (the parent's routes) -- and EACH of the three from each start of the
    object's near position: 0, just below 2^32, just below a multiple of kFlowLagPeriod, with either object rate and with and without
    a clean input.  Per session and tick at random 8 kHz / half, 8 kHz / 160, 16 kHz / half, 16 kHz / 160, 16 kHz / split, idle ticks,
    NO_FAREND, far-end bursts with per-session call counts, msInSndCardBuf anywhere; ticks of 160 and 80.  Every block's far, near and
    clean tags, every output tag and every code equal the per-session wrapper's; a half call's row is not written past its 80
    samples; every state passed through is one FlowStateDefect accepts; the lag is always a multiple of 80 below kFlowLagPeriod; no
    planning kernel ever meets a session it cannot plan."""
    seen = dict.fromkeys(mixed_sim.DETAIL, 0)
    per_start = {}                                  # (mode, start) -> half calls, mixed planning ticks, resyncs that moved samples
    for mode, first, count in mixed_sim.FUZZ_PLAN:
        for seed in range(first, first + count):
            idle_percent = 30 if seed % 4 == 3 else 10
            start = ((seed - first) // 4) % 3
            tick, d = mixed_sim.fuzz(seed, 6, 600, mode, idle_percent, STARTS[start])
            assert tick == -1, (seed, mode, start, tick, d)
            assert d["max_lag"] % 80 == 0 and d["max_lag"] < LAG_PERIOD
            if mode == mixed_sim.UNIFORM:
                # a dense tick: all six sessions call in this tick and in the one before (0.9^12 of 600 ticks at 10 % idle: ~170)
                assert d["mixed_ticks"] == 0 and d["half_calls"] == 0 and (d["dense_ticks"] > 50 or idle_percent > 10), (seed, d)
            else:
                assert d["half_calls"] > 500 and d["resyncs"] > 300 and d["mixed_ticks"] > 300, (seed, d)
            acc = per_start.setdefault((mode, start), [0, 0, 0, 0])
            for i, k in enumerate(("half_calls", "mixed_ticks", "resyncs")):
                acc[i] += d[k]
            acc[3] += 1
            for k in seen:
                seen[k] += d[k]
    # every mode from every start; the modes that exercise the feature made half calls, took the mixed planning launch and moved
    # pending samples from each of them -- across the 2^32 wrap and across the lag period too
    assert sorted(per_start) == sorted((m, s) for m in (0, 1, 2) for s in range(3))
    for (mode, start), (half, mixed, resyncs, seeds) in per_start.items():
        assert seeds >= (8 if mode == mixed_sim.MIXED_RATES else 4), (mode, start, seeds)
        if mode != mixed_sim.UNIFORM:
            assert half > 2000 and mixed > 1200 and resyncs > 1200, (mode, start, half, mixed, resyncs)
    assert seen["blocks"] > 100000
    assert seen["half_calls"] > 20000 and seen["half_calls_16k"] > 4000 and seen["full_calls_8k"] > 10000 and seen["split_calls"] > 6000
    assert seen["resyncs"] > 20000 and seen["moved_samples"] > seen["resyncs"]       # pending samples did move behind the object's position
    assert seen["mixed_ticks"] > 10000 and seen["dense_ticks"] > 500 and seen["nobody_ticks"] > 100
    assert seen["idle"] > 5000 and seen["bursts"] > 3000 and seen["warnings"] > 1000
    assert seen["max_lag"] > 0


def test_uniform_object_routes_as_before():
    """FlowRouteTickMixed for an object without half calls and without sessions of another rate IS FlowRouteTick: the same
    FlowTickRoute, field by field, and the same bookkeeping after every one of 20 000 random ticks per seed (nobody, everybody and
    some of the sessions live, both tick sizes, the diagnostics switch) -- and never the mixed planning launch."""
    l = mixed_sim.lib()
    for seed in range(10):
        for S in (1, 9, 1000):
            assert l.sim_mixed_route_uniform(seed, S, 20000) == -1, (seed, S)


def test_half_calls_and_other_rates_take_the_mixed_planning_launch():
    r = mixed_sim.Router(9)
    dense = dict(launch=1, sparse_plan=0, sparse_tick=0, deferred_lag=0, mixed_plan=0, may_lag=0)
    assert r.tick(9, 160) == dense
    # a half call: the planning launch that knows call sizes and lags, the dense tick launch; the object is out of step afterwards ...
    assert r.tick(9, 160, half_calls=True) == dict(dense, sparse_plan=1, mixed_plan=1, may_lag=1)
    # ... so the next tick, without a half call, resyncs through the sparse planning launch (as after an idle tick) -- and then
    # the object is what it was before
    assert r.tick(9, 160) == dict(dense, sparse_plan=1)
    assert r.tick(9, 160) == dense
    # half calls next to idle sessions: the live list too; ticks nobody makes are deferred to the next planning launch
    assert r.tick(5, 160, half_calls=True) == dict(dense, sparse_plan=1, sparse_tick=1, mixed_plan=1, may_lag=1)
    assert r.tick(0, 160, half_calls=True) == dict(launch=0, sparse_plan=0, sparse_tick=0, deferred_lag=0, mixed_plan=0, may_lag=1)
    assert r.tick(0, 80) ["launch"] == 0
    assert r.tick(9, 160, half_calls=True) == dict(dense, sparse_plan=1, deferred_lag=240, mixed_plan=1, may_lag=1)
    # an object that holds a session of another rate plans every tick per session, in step or not; without half calls it stays in step
    r = mixed_sim.Router(9)
    for _ in range(3):
        assert r.tick(9, 160, other_rates=True) == dict(dense, sparse_plan=1, mixed_plan=1)
    assert r.tick(9, 80, other_rates=True) == dict(dense, sparse_plan=1, mixed_plan=1)
    assert r.tick(9, 160) == dense
    assert r.tick(9, 160, force_sparse=True, other_rates=True) == dict(dense, sparse_plan=1, sparse_tick=1, mixed_plan=1)


def test_tick_flag_argument_checks():
    """The host's pass over a tick's flags: HALF_CALL needs a tick of 160 samples and excludes SPLIT_CALLS -- in a session that
    calls; an idle session's byte means nothing.  The new bit does not disturb the live count or the live list's bases."""
    H, SP, I, NF = mh.HALF_CALL, mh.SPLIT_CALLS, mh.IDLE, mh.NO_FAREND
    ok = lambda flags, n: mixed_sim.check_flags(flags, n)[0] == 0
    assert ok([0, H, H | NF, SP, 0], 160) and ok([H] * 9, 160) and ok([0] * 9, 80) and ok([NF] * 3, 80)
    assert not ok([0, H, 0], 80) and not ok([0, 0, SP], 80)
    assert not ok([0, H | SP, 0], 160) and not ok([H | SP | NF], 160)
    assert ok([H, SP, H, SP], 160)                                       # the two bits in different sessions
    assert ok([I | H | SP, 0], 160) and ok([I | H, I | SP, 0], 80)       # idle sessions: ignored
    rng = np.random.default_rng(5)
    for S in (1, 255, 256, 257, 1000):
        flags = rng.integers(0, 16, S).astype(np.uint8)
        flags[(flags & (H | SP)) == (H | SP)] &= ~np.uint8(SP)
        rc, live, any_bits, bases_agree = mixed_sim.check_flags(flags, 160)
        calling = flags[(flags & I) == 0]
        assert rc == 0 and bases_agree and live == len(calling)
        assert any_bits == (int(np.bitwise_or.reduce(calling)) if len(calling) else 0)


def test_interface_is_exported():
    import webrtc_aecm_amd as aecm
    from webrtc_aecm_amd import ffi
    assert ffi.SESSION_HALF_CALL == 8 == mh.HALF_CALL
    lib = aecm.load()
    for name in ("InitRates", "InitSessionRate", "GetSessionRate", "ImportSessionAnyRate"):
        assert hasattr(lib, "WebRtcAecmSessions_" + name) and "WebRtcAecmSessions_" + name in ffi.SESSIONS_SYMBOLS
    rate = aecm.ffi.C.c_int32(0)
    assert lib.WebRtcAecmSessions_InitRates(None, 16000, None) == -1
    assert lib.WebRtcAecmSessions_InitSessionRate(None, 0, 8000) == -1
    assert lib.WebRtcAecmSessions_GetSessionRate(None, 0, rate) == -1
    assert lib.WebRtcAecmSessions_ImportSessionAnyRate(None, 0, None, 0) == -1


def test_mixed_planning_kernel_is_in_the_library():
    """The planning kernel of mixed objects is a kernel of its own next to the dense and the sparse one (whose instruction streams
    tests/test_sparse_ticks.py pins)."""
    from webrtc_aecm_amd import build, isa_census
    ours = isa_census.census_of_text(isa_census.disassemble(build.build()))
    for name in ("aecm_flow_plan_kernel", "aecm_flow_plan_sparse_kernel", "aecm_flow_plan_mixed_kernel", "aecm_broadcast_image_select_kernel"):
        assert sum(name in k for k in ours) == 1, name


def test_simulator_stand_alone_under_sanitizers():
    """tests/sim/sim_mixed.cpp as a program of its own with AddressSanitizer and UBSan (the 48 seeds x 600 ticks of mixed_sim.FUZZ_PLAN + the routing check)."""
    exe = mixed_sim.standalone(sanitize=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.returncode, r.stdout[-500:], r.stderr[-2000:])


@pytest.mark.parametrize("name", sorted(mh.GOLDEN_CASES))
def test_golden_mixed_runs_are_what_their_recipe_says(name):
    """tests/golden/sessmixed_*.npz (tools/gen_golden.py; run on the GPU by tests/test_gpu_mixed_sessions.py): arrays only, the
    pattern the recipe gives, every session past its start-up phase for at least 40 ticks, zeros where a session made no call
    (idle ticks, second halves of half calls), under 400 KB.  Where the unmodified reference is built, its instances -- one per
    session, at the session's rate, called with the session's sizes -- give exactly the stored outputs, codes and echo paths."""
    from oracle import pyoracle
    path = mh.GOLDEN_DIR / f"{name}.npz"
    assert path.stat().st_size < 400 * 1024
    g = np.load(path, allow_pickle=False)
    seed, idle_p, with_bursts = mh.GOLDEN_CASES[name]
    flags, ms = mh.mixed_pattern(seed, idle_p=idle_p)
    assert int(g["seed"]) == seed and int(g["object_fs"]) == mh.OBJECT_FS and np.array_equal(g["rates"], mh.RATES)
    assert np.array_equal(g["flags"], flags) and np.array_equal(g["ms"], ms) and flags.shape == (mh.T_MIXED, 9)
    bursts = mh.burst_pattern(seed) if with_bursts else np.zeros_like(flags)
    assert np.array_equal(g["bursts"], bursts) and bool(bursts.any()) == with_bursts
    idle, half = (flags & mh.IDLE) != 0, (flags & mh.HALF_CALL) != 0
    assert half[:, list(mh.ALWAYS_HALF)].all() and not (half & ~idle)[:, [0, 5, 6, 8]].any() and 0.15 < half[:, mh.SOMETIMES_HALF].mean() < 0.55
    assert (flags[mh.SPLIT_FROM:, mh.SPLIT] & mh.SPLIT_CALLS).all() and idle.any() == bool(idle_p)
    for key in ("", "_clean"):
        out = g["out" + key].reshape(9, mh.T_MIXED, 160)
        assert g["out" + key].dtype == np.int16 and g["paths" + key].shape == (9, 65)
        assert (g["active_from" + key] <= mh.T_MIXED - 40).all(), g["active_from" + key]
        assert not out[idle.T].any() and not out[:, :, 80:][(half & ~idle).T].any() and not g["codes" + key][idle].any()
        assert out[:, :, :80][(~idle).T].any() and 12100 in g["codes" + key]
    if pyoracle.have_reference():
        far, near, clean = mh.signals(seed, mh.RATES, mh.T_MIXED * 160, with_clean=True)
        for key, c in (("", None), ("_clean", clean)):
            o, codes, paths, _, active = mh.drive_reference(lambda fs: pyoracle.RefSession(fs, 1, 3), mh.RATES, flags, ms, 160, far, near, c, bursts,
                                                            mh.burst_signals(seed))
            assert np.array_equal(o, g["out" + key]) and np.array_equal(codes, g["codes" + key]) and np.array_equal(paths, g["paths" + key])
            assert np.array_equal(active, g["active_from" + key])
