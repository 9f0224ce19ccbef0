"""Sparse session ticks without a GPU: a session that carries AECM_SESSION_IDLE makes no call in the tick -- the wrapper's
position arithmetic with idle ticks against the generic wrapper that is simply not called (sample tags), the live list the
tick kernel's grid runs by, WebRtcAecmSessions_DescribeTickLive, the dense tick kernels' instruction streams (unchanged by
the sparse ones) and the recorded reference runs of tests/golden/sesssparse_*.npz."""
import json
from pathlib import Path

import numpy as np
import pytest

import sparse_sim

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden"


@pytest.mark.parametrize("idle_percent", [0, 30, 90])
def test_idle_ticks_equal_a_wrapper_that_is_not_called_on_sample_tags(idle_percent):
    """FlowTick + FlowIdleTick + FlowResync (what the planning kernels run) against SessionFlow<T>, which in an idle tick is
    not called: every block's 64 far / near inputs and every output sample of every call carry the expected tag; every state
    passed through -- also between an idle tick and the next call -- is one FlowStateDefect accepts.  Both rates; the plain
    cadence and 80 / 160 / split calls mixed with far-end underruns and bursts (also into idle ticks); idle stretches of 1, 2,
    3 and >= 110 ticks (longer than the 8 192-sample ring), from the first tick, in the start-up phase and on the first tick
    after it; ticks nobody makes (nothing launched: the lag is deferred); position counters that wrap.  40 seeds."""
    seen = dict.fromkeys(sparse_sim.DETAIL, 0)
    longest = 0
    for seed in range(40):
        fs = 16000 if seed % 2 else 8000
        pattern = (seed // 2) % 2
        start = (0, 0xfffff000 // 80, 0x7ffff800 // 80, 987654)[seed % 4]
        tick, d = sparse_sim.fuzz(seed, fs, 1500, pattern, idle_percent, start)
        assert tick == -1, (seed, fs, pattern, tick, d)
        for k in seen:
            seen[k] += d[k]
        longest = max(longest, d["longest_stretch"])
    assert seen["blocks"] > 2000
    assert longest >= 110 and longest * 80 > 8192                    # a stretch longer than the ring
    assert seen["resyncs"] > 50 and seen["moved_samples"] > seen["resyncs"]     # pending samples did move behind the object's position
    assert seen["nobody_ticks"] > 100 and seen["idle_in_startup"] > 20 and seen["idle_after_startup"] > 3 and seen["idle_two_block"] > 10
    if idle_percent < 90:
        assert seen["dense_ticks"] > 1000                            # ticks of an object in step took the planning kernel that knows no lags


def test_lag_word_is_whole_ticks():
    """FlowStateDefect accepts every lag an idling session passes through and refuses one that is no multiple of 80; the lag
    stays a multiple of 80 however long the stretch (it is kept modulo lcm(80, ring): 2^32 is no multiple of 80)."""
    l = sparse_sim.lib()
    field = l.sim_sparse_lag_field()
    for lag in (0, 80, 160, 8240, 40880):
        assert l.sim_sparse_lag_defect(lag) == 0, lag
    for lag in (1, 79, 81, 8192, 40960, 40961, -80, 1 << 30):
        assert l.sim_sparse_lag_defect(lag) == field, lag
    for ticks, n in ((1, 80), (103, 80), (511, 160), (512, 80), (27_000_000, 160)):     # 27 M ticks of 160: past 2^32 samples
        lag = l.sim_sparse_lag_after(ticks, n)
        assert lag == (ticks * n) % 40960 and lag % 80 == 0 and l.sim_sparse_lag_defect(lag) == 0


def test_pending_samples_move_right_when_source_and_destination_overlap():
    """FlowMoveNear: the fewer-than-one-block pending samples of a session that comes back in step move d = lag mod ring ahead in
    the ring.  d smaller than the count (a lag of 8 240 is d = 48): the ranges overlap with the destination ahead, the copy runs
    backwards; d within count of the ring's length: the destination lies behind the source, forwards; also d = 0 (nothing moves),
    clear ranges, and sources / destinations that wrap around the ring's end.  Every destination sample must hold its source
    sample's tag and nothing else may change."""
    l = sparse_sim.lib()
    ring = 8192
    for count in (63, 1, 0):
        for d in (0, 1, 48, 62, 63, 64, 80, 4096, ring - 64, ring - 63, ring - 48, ring - 1):
            for src in (0, 100, ring - 70, ring - 63, ring - 1, 0xfffffff0, 0x7fffffe0):
                assert l.sim_sparse_move_check(ring, src, d, count) == 0, (count, d, src)
    assert 8240 % ring == 48 and 40880 % ring == ring - 80


@pytest.mark.parametrize("S", [1, 4, 5, 255, 256, 257, 1000])
def test_live_list_is_the_ascending_ids_of_the_sessions_that_call(S):
    """Host half (per-workgroup prefix counts in the pass over the flags) + device half (ballot rank within the wavefront,
    counts across the workgroup's wavefronts) as the planning kernel runs them: exactly the non-idle ids, ascending; the
    other flag bits do not matter."""
    rng = np.random.default_rng(S)
    cases = [np.zeros(S, np.uint8), np.full(S, 4, np.uint8), np.full(S, 3, np.uint8), np.full(S, 7, np.uint8)]
    for p in (0.1, 0.5, 0.9, 0.99):
        cases.append(((rng.random(S) < p) * 4 + rng.integers(0, 4, S)).astype(np.uint8))
    for flags in cases:
        n, lst = sparse_sim.live_list(flags)
        expect = np.flatnonzero((flags & 4) == 0).astype(np.uint32)
        assert n == len(expect)
        assert np.array_equal(lst[:n], expect)
        assert np.all(lst[n:] == 0xffffffff)                         # nothing written past the live count


def test_describe_tick_live():
    import webrtc_aecm_amd as aecm
    for S, cus in ((9, 256), (4096, 256), (65536, 256), (65536, 64), (1000, 304)):
        dense = aecm.describe_tick(S, cus)
        assert aecm.describe_tick_live(S, S, cus) == dense                                   # field by field
        none = aecm.describe_tick_live(S, 0, cus)
        assert none["workgroups"] == 0 and none["rounds_x1000"] == 0
        prev = none
        for live in sorted({1, 2, 4, 5, S // 100 + 1, S // 10 + 1, S // 4 + 1, S // 2, S - 1, S}):
            d = aecm.describe_tick_live(S, live, cus)
            assert d["workgroups"] == -(-live // d["waves_per_workgroup"])
            assert d["workgroups"] >= prev["workgroups"] and d["rounds_x1000"] >= prev["rounds_x1000"]      # monotone in live
            assert d["waves_per_workgroup"] == dense["waves_per_workgroup"] and d["workgroups_per_cu"] == dense["workgroups_per_cu"]
            prev = d
    d = aecm.ffi.AecmLaunchDescription()
    lib = aecm.load()
    assert lib.WebRtcAecmSessions_DescribeTickLive(9, 10, 256, d) == aecm.ffi.AECM_BAD_PARAMETER_ERROR
    assert lib.WebRtcAecmSessions_DescribeTickLive(9, -1, 256, d) == aecm.ffi.AECM_BAD_PARAMETER_ERROR
    assert lib.WebRtcAecmSessions_DescribeTickLive(9, 3, 256, None) == aecm.ffi.AECM_NULL_POINTER_ERROR
    assert aecm.ffi.SESSION_IDLE == 4


def test_dense_tick_kernels_are_the_kernels_they_were():
    """The sparse tick kernels run the dense ones' body with another session id; the dense instantiations -- what every tick without an
    idle session runs -- must stay, instruction for instruction and operand for operand, the kernels of the commit before there
    was a sparse form (isa_census fingerprints of whole instruction streams; the mechanism of
    test_cmake_build_equals_the_python_recipe).  tests/golden/tick_dense_fingerprints.json holds that commit's two kernels as
    webrtc_aecm_amd/build.py built them with the compiler the file names.  It is a yardstick for one compiler: after a compiler
    upgrade, or a deliberate change of the tick kernel, re-record it -- build the commit that is to be the yardstick with
    webrtc_aecm_amd/build.py, run `python -m webrtc_aecm_amd.isa_census --all` on its library and copy fingerprint and
    n_instructions of the two `aecm_tick_flow_kernel` entries, and the first lines of
    `hipcc --version`.  (Registers, scratch, LDS and instruction classes of all four instantiations: profiles/r16_sparse_ticks.txt.)"""
    import re
    from webrtc_aecm_amd import build, isa_census
    recorded = json.loads((GOLDEN / "tick_dense_fingerprints.json").read_text())
    ours = isa_census.census_of_text(isa_census.disassemble(build.build()))
    assert sorted(recorded["kernels"]) == ["clean", "noclean"]
    for clean, key in ((0, "noclean"), (1, "clean")):
        dense = [c for k, c in ours.items() if re.search(rf"aecm_tick_flow_kernelILb{clean}EEE", k)]
        sparse = [c for k, c in ours.items() if re.search(rf"aecm_tick_flow_sparse_kernelILb{clean}EEE", k)]
        assert len(dense) == 1 and len(sparse) == 1, key
        want = recorded["kernels"][key]
        assert (dense[0]["fingerprint"], dense[0]["n_instructions"]) == (want["fingerprint"], want["n_instructions"]), (key, recorded["compiler"])
    assert any("aecm_flow_plan_sparse_kernel" in k for k in ours)


@pytest.mark.parametrize("name", ["sesssparse_fs16000_f160", "sesssparse_fs8000_f80"])
def test_golden_sparse_runs_are_what_their_recipe_says(name):
    """tests/golden/sesssparse_*.npz (tools/gen_golden.py; run on the GPU by tests/test_gpu_sparse_ticks.py): 6 sessions x 80
    ticks with the idle pattern stored -- arrays only, the pattern the recipe gives, nothing but zeros and code 0 where a
    session sat out, a slot that never called, stretches of 1, 2, 3 and 60 ticks; under 100 KB.  Where the unmodified
    reference is built, its instances -- not called in idle ticks -- give exactly the stored outputs, codes and echo paths."""
    import sparse_helpers as sh
    from oracle import pyoracle
    path = GOLDEN / f"{name}.npz"
    assert path.stat().st_size < 100 * 1024
    g = np.load(path, allow_pickle=False)
    fs, frame, seed = sh.GOLDEN_CASES[name]
    assert (int(g["fs"]), int(g["frame"]), int(g["seed"])) == (fs, frame, seed)
    flags, ms = sh.golden_pattern(fs, frame, seed)
    assert np.array_equal(g["flags"], flags) and np.array_equal(g["ms"], ms) and flags.shape == (80, 6)
    idle = (flags & sh.IDLE) != 0
    out = g["out"].reshape(6, 80, frame)
    assert not out[idle.T].any() and not g["codes"][idle].any() and idle[:, 5].all() and idle[15:75, 4].all()
    assert out[~idle.T].any() and 0.2 < idle[:, :4].mean() < 0.5 and 12100 in g["codes"]
    assert g["paths"].shape == (6, 65) and g["out"].dtype == np.int16
    if pyoracle.have_reference():
        far, near, _ = sh.signals(seed, 6, 80 * frame, fs)
        o, c, p = sh.drive_reference(lambda: pyoracle.RefSession(fs, 1, 3), fs, flags, ms, np.full(80, frame), far, near)
        assert np.array_equal(o, g["out"]) and np.array_equal(c, g["codes"]) and np.array_equal(p, g["paths"])
