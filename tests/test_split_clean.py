"""A clean near-end input per session (AECM_SESSION_NO_CLEAN) without a GPU: the two live lists of a split tick (host half +
simulated device half, tests/sim/sim_split.cpp) against a plain partition, the per-session history rule as a state machine, the
public interface, and how the new units are built.  The GPU side: tests/test_gpu_split_clean.py."""
import ctypes
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import split_sim

ROOT = Path(__file__).resolve().parent.parent
NO_FAREND, SPLIT_CALLS, IDLE, HALF_CALL, NO_CLEAN = 1, 2, 4, 8, 16
NONE, ALWAYS, NEVER, BOTH = 0, 1, 2, 3
NAMES = ["WebRtcAecmSessions_GetSessionCleanMode", "WebRtcAecmSessions_SplitCleanTwoLaunches"]
SIZES = (1, 63, 64, 65, 255, 256, 257, 300)


def _check_lists(flags):
    flags = np.asarray(flags, dtype=np.uint8)
    S = len(flags)
    calling = (flags & IDLE) == 0
    want_clean = np.flatnonzero(calling & ((flags & NO_CLEAN) == 0))
    want_plain = np.flatnonzero(calling & ((flags & NO_CLEAN) != 0))
    got, lc, lp, start, dropped = split_sim.lists(flags)
    assert (lc, lp, dropped) == (len(want_clean), len(want_plain), 0)
    assert start % 4 == 0 and lc <= start < lc + 4 and start + lp <= len(got) == S + 4      # a workgroup boundary of the tick kernel
    assert np.array_equal(got[:lc], want_clean) and np.array_equal(got[start:start + lp], want_plain)
    # nothing else was stored: every calling session exactly once, idle sessions nowhere
    stored = got[got != 0xffffffff]
    assert len(stored) == lc + lp and len(np.unique(stored)) == len(stored) and not (flags[stored] & IDLE).any()
    return lc, lp, start


@pytest.mark.parametrize("S", SIZES)
def test_two_lists_equal_a_plain_partition(S):
    """Random flag bytes (every bit of the byte, so idle sessions carry the bit too) over sizes around the wavefront and the planning
    workgroup: both lists ascending, every calling session exactly once, idle sessions nowhere, the second list at the next multiple
    of four.  Nobody clean, nobody plain, a clean count that is a multiple of four and one that is not."""
    rng = np.random.default_rng(4100 + S)
    seen_multiple = seen_other = False
    for round_ in range(40):
        flags = rng.integers(0, 32, S).astype(np.uint8)
        if round_ % 8 == 1:
            flags |= NO_CLEAN                                     # nobody clean
        if round_ % 8 == 2:
            flags &= ~np.uint8(NO_CLEAN)                          # nobody plain
        if round_ % 8 == 3:
            flags |= IDLE                                         # nobody at all
        lc, lp, start = _check_lists(flags)
        if round_ % 8 == 1:
            assert lc == 0 and start == 0
        if round_ % 8 == 2:
            assert lp == 0
        if round_ % 8 == 3:
            assert lc == lp == 0
        seen_multiple |= lc > 0 and lc % 4 == 0 and lp > 0
        seen_other |= lc % 4 != 0 and lp > 0
    if S >= 63:
        assert seen_other
    # a clean count that IS a multiple of four (the plain list starts right behind) and one that is not (it starts after a gap)
    for lc_want in (4 * (min(S, 16) // 4), 4 * (min(S, 16) // 4) + 1):
        if 0 < lc_want < S:
            flags = np.full(S, NO_CLEAN, dtype=np.uint8)
            flags[rng.choice(S, lc_want, replace=False)] = 0
            lc, lp, start = _check_lists(flags)
            assert lc == lc_want and start == -(-lc_want // 4) * 4 and lp == S - lc_want


def test_lists_across_a_planning_workgroup_boundary():
    """300 sessions: different clean and plain counts in the two planning workgroups, and a wavefront that holds only one kind."""
    flags = np.zeros(300, dtype=np.uint8)
    flags[0:64] = NO_CLEAN                    # first wavefront: all plain
    flags[64:256:3] = NO_CLEAN
    flags[100:130] |= IDLE
    flags[256:300:2] = NO_CLEAN | NO_FAREND
    flags[299] = IDLE | NO_CLEAN
    lc, lp, start = _check_lists(flags)
    assert lc % 4 != 0 and lp > 64


def test_history_rule_as_a_state_machine():
    S = 8
    o = split_sim.Object(S)
    flagged = np.array([0, NO_CLEAN, 0, NO_CLEAN, IDLE, IDLE | NO_CLEAN, 0, NO_CLEAN | NO_FAREND], dtype=np.uint8)
    # fresh -> always / never in one accepted split tick; idle sessions stay at none
    rc, route = o.tick(flagged)
    assert rc == split_sim.ACCEPTED and route == {"split": True, "clean_kernels": True, "checked": True}
    modes, pos, used = o.state()
    assert modes.tolist() == [ALWAYS, NEVER, ALWAYS, NEVER, NONE, NONE, ALWAYS, NEVER] and pos == 160 and used

    def refused(want=split_sim.BAD_PARAMETER, **kw):
        before = o.state()
        rc, _ = o.tick(**kw)
        after = o.state()
        assert rc == want and np.array_equal(before[0], after[0]) and before[1:] == after[1:]

    # always + flagged -> refused; never + unflagged -> refused, with and without a flags array, and by a tick without a clean input
    f = flagged.copy(); f[0] = NO_CLEAN
    refused(flags=f)
    f = flagged.copy(); f[1] = 0
    refused(flags=f)
    refused(flags=None)
    refused(flags=None, clean=False)                                     # the "always" sessions would get none
    refused(flags=np.zeros(S, dtype=np.uint8))
    refused(want=split_sim.UNSUPPORTED, flags=flagged, calls=2)          # K-call split ticks: unsupported
    refused(want=split_sim.BAD_PARAMETER, flags=flagged | HALF_CALL, n=80)      # the existing flag check comes first and still holds
    # the offenders idle: accepted, and an idle session is exempt whatever its byte says
    f = flagged.copy(); f[[1, 3, 7]] = IDLE
    rc, route = o.tick(f)
    assert rc == 0 and route == {"split": False, "clean_kernels": True, "checked": True}      # nobody flagged among the callers: today's tick
    f = np.full(S, IDLE, dtype=np.uint8); f[[1, 3]] = NO_CLEAN
    rc, route = o.tick(f)
    assert rc == 0 and route == {"split": False, "clean_kernels": False, "checked": True}     # everybody flagged: the tick without a clean input
    f = np.full(S, IDLE, dtype=np.uint8); f[[1, 3]] = 0
    rc, route = o.tick(f, clean=False)                                   # no clean input: the bit means nothing, "never" sessions may call
    assert rc == 0 and route["split"] is False
    assert o.state()[0].tolist() == [ALWAYS, NEVER, ALWAYS, NEVER, NONE, NONE, ALWAYS, NEVER]
    # InitSession resets one session, which may then switch kind
    o.init_session(0)
    assert o.state()[0][0] == NONE
    f = flagged.copy(); f[0] = NO_CLEAN
    assert o.tick(f)[0] == 0 and o.state()[0][0] == NEVER
    # sessions 4 and 5 made their first calls late
    f = flagged.copy(); f[0] = NO_CLEAN; f[4] = NO_CLEAN; f[5] = 0
    assert o.tick(f)[0] == 0 and o.state()[0].tolist() == [NEVER, NEVER, ALWAYS, NEVER, NEVER, ALWAYS, ALWAYS, NEVER]
    # Init forgets everything, the object is as one that never used the flag
    o.init()
    assert o.state() [1:] == (0, False) and not o.state()[0].any()


def test_an_object_that_never_uses_the_flag_is_never_refused():
    S = 5
    o = split_sim.Object(S)
    assert o.tick(None, clean=True) == (0, {"split": False, "clean_kernels": True, "checked": False})
    assert o.state()[0].tolist() == [ALWAYS] * S
    assert o.tick(None, clean=False)[0] == 0 and o.state()[0].tolist() == [BOTH] * S            # the clean input goes away: as it always was
    f = np.array([0, IDLE, NO_FAREND, IDLE | NO_CLEAN, 0], dtype=np.uint8)
    o.init_session(1)
    assert o.tick(f, clean=True)[0] == 0 and o.state()[0].tolist() == [BOTH, NONE, BOTH, BOTH, BOTH]
    f[3] = NO_CLEAN
    assert o.tick(f, clean=False) == (0, {"split": False, "clean_kernels": False, "checked": False})      # no clean input: the bit is ignored
    # ... but its first use is checked: sessions 0, 2, 4 have had both
    before = o.state()
    assert o.tick(f, clean=True)[0] == split_sim.BAD_PARAMETER
    assert np.array_equal(before[0], o.state()[0]) and before[1:] == o.state()[1:]
    # the same unflagged tick: accepted here, refused in an object that has accepted a split tick
    a, b = split_sim.Object(2), split_sim.Object(2)
    assert b.tick(np.array([0, NO_CLEAN], dtype=np.uint8))[0] == 0
    assert a.tick(np.array([0, IDLE], dtype=np.uint8), clean=False)[0] == 0 and a.tick(None, clean=False)[0] == 0
    unflagged = np.zeros(2, dtype=np.uint8)
    assert a.tick(unflagged)[0] == 0 and b.tick(unflagged)[0] == split_sim.BAD_PARAMETER
    # a tick without a flags array costs no pass over the sessions, yet is not lost: it is folded in when next looked at
    c = split_sim.Object(3)
    for _ in range(3):
        assert c.tick(None, clean=True)[0] == 0
    c.init_session(2)
    assert c.state()[0].tolist() == [ALWAYS, ALWAYS, NONE]
    assert c.tick(np.array([IDLE, NO_CLEAN, NO_CLEAN], dtype=np.uint8))[0] == split_sim.BAD_PARAMETER
    assert c.tick(np.array([IDLE, IDLE, NO_CLEAN], dtype=np.uint8))[0] == 0 and c.state()[0].tolist() == [ALWAYS, ALWAYS, NEVER]


def test_simulator_runs_stand_alone_under_sanitizers():
    """tests/sim/sim_split.cpp has a main of its own: built with AddressSanitizer and UndefinedBehaviorSanitizer into a program and
    run, on the CPU."""
    r = subprocess.run([str(split_sim.standalone())], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.stdout, r.stderr[-2000:])


def _declared_session_functions(header):
    return sorted(set(re.findall(r"^\w[\w \*]*?\b(WebRtcAecmSessions_\w+)\(", header, flags=re.M)))


def test_symbols_are_declared_exported_and_bound():
    import webrtc_aecm_amd as aecm
    from webrtc_aecm_amd import build, ffi
    header = (ROOT / "include" / "aecm_batch.h").read_text()
    lib = ctypes.CDLL(str(build.build()))
    bound = aecm.load()
    assert ffi.SESSION_NO_CLEAN == 16 and re.search(r"\bAECM_SESSION_NO_CLEAN = 16\b", header)
    declared = _declared_session_functions(header)
    assert set(NAMES) <= set(declared) and len(declared) > 40
    for name in declared:                                   # every symbol the header declares is exported
        assert hasattr(lib, name), name
    for name in NAMES:
        assert name in ffi.SESSIONS_SYMBOLS and len(getattr(bound, name).argtypes) == (3 if "Get" in name else 2)
    assert hasattr(aecm.AecmSessions, "get_session_clean_mode")
    # what can be asked without a device: no object, no call
    assert bound.WebRtcAecmSessions_GetSessionCleanMode(None, 0, None) == -1 and bound.WebRtcAecmSessions_SplitCleanTwoLaunches(None, 1) == -1
    for word in ("AECM_SESSION_NO_CLEAN", "AECM_UNSUPPORTED_FUNCTION_ERROR", "Idle sessions", "near_clean == NULL", "not supported yet"):
        assert word in header, word


def test_new_units_are_built_like_their_siblings(tmp_path):
    """Both recipes list the two new units; the tick kernel's unit gets the flags aecm_kernels.hip's tick kernels get, the planning
    kernels' unit -- one lane per session -- none of its own; the fused kernel, both per-list kernels and both planning kernels are in
    the code object; registers admit the 7 waves per SIMD the tick kernels are built for, and nothing spills to scratch memory."""
    from test_tick_packets import _kernel_metadata
    from webrtc_aecm_amd import build
    tick, plan = "aecm_tick_split_kernels.hip", "aecm_tick_split_plan_kernels.hip"
    assert tick in build.KERNEL_SOURCES and plan in build.KERNEL_SOURCES
    assert build.SOURCE_FLAGS[tick] == build.SOURCE_FLAGS["aecm_kernels.hip"] and plan not in build.SOURCE_FLAGS
    cmake = (ROOT / "CMakeLists.txt").read_text()
    assert tick in cmake and plan in cmake and re.search(r'src MATCHES "aecm_tick_split_plan_kernels"', cmake)
    meta = _kernel_metadata(tmp_path)
    assert len([k for k in meta if "aecm_tick_split_kernelE" in k]) == 1
    for clean in (0, 1):
        assert len([k for k in meta if f"aecm_tick_split_list_kernelILb{clean}E" in k]) == 1
        assert len([k for k in meta if f"aecm_flow_plan_split_kernelILb{clean}E" in k]) == 1
    for name, (sgpr, vgpr, scratch) in meta.items():
        if "aecm_tick_split_kernelE" in name or "aecm_tick_split_list_kernel" in name:
            print(name, "sgpr", sgpr, "vgpr", vgpr, "scratch", scratch)
            assert min(8, 512 // (-(-vgpr // 8) * 8), 800 // (-(-sgpr // 16) * 16 + 16)) >= 7, (sgpr, vgpr)
            assert scratch == 0
