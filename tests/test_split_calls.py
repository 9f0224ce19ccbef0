"""K-call and packet ticks with a clean near-end input per session (WebRtcAecmSessions_SetSplitCallTicks) without a GPU: the host's
plan of such ticks as a table (written from the contract in include/aecm_batch.h, not taken from the planner), whole objects on the
CPU double (tests/sim/sim_split_calls.cpp), the public interface, how the new units are built, and the golden run's recipe.  The GPU
side: tests/test_gpu_split_calls.py."""
import ctypes
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import split_calls_helpers as sch
import split_calls_sim as T
from split_calls_sim import BAD_PARAMETER, HALF_CALL, IDLE, NO_CLEAN, NO_FAREND, SPLIT_CALLS, UNSUPPORTED

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden"
S = 5
SOME_PLAIN = [0, NO_CLEAN, 0, NO_CLEAN, 0]
TWO_RATES = [16000, 16000, 8000, 16000, 16000]
NAME = "WebRtcAecmSessions_SetSplitCallTicks"


def row(name, tick, code=0, before=(), obj=None, state=None, **plan):
    return pytest.param(obj or {}, before, tick, code, plan, state or {}, id=name)


ON = dict(switch=True)
# (name, the tick, [code], [before: ticks the object has accepted first], [obj: Object's keywords + traces], [state afterwards], the plan)
TABLE = [
    # ---- the switch off: what it always was
    row("off: a split tick of K calls", dict(calls=2, flags=SOME_PLAIN), UNSUPPORTED),
    row("off: a split packet tick", dict(calls=3, packets=True, flags=[HALF_CALL, NO_CLEAN, 0, 0, 0]), UNSUPPORTED),
    row("off: every caller flagged in a K-call tick", dict(calls=2, flags=[NO_CLEAN] * S), UNSUPPORTED),
    row("off: one call is the split tick it was", dict(flags=SOME_PLAIN), family="split", k_calls=0, span=160, clean_count=3, plain_count=2),
    row("off: nobody flagged, K calls", dict(calls=2, flags=[0] * S), family="calls", k_calls=1, clean_plane=1, split_tick=0, checked=0),
    row("off: K calls, unsupported before a changed kind", dict(calls=2, flags=[NO_CLEAN, 0, 0, NO_CLEAN, 0]), UNSUPPORTED, before=[dict(flags=SOME_PLAIN)]),
    # ---- the switch on: family split with k_calls; the spans of the packet clocks
    row("on: K = 2 of 160, 20 ms at 16 kHz", dict(calls=2, flags=SOME_PLAIN), obj=ON, family="split", k_calls=1, mixed_plan=0, span=320, live=5, split_tick=1,
        clean_plane=1, clean_count=3, plain_count=2, sparse_tick=1, checked=1, state=dict(near_pos=320, modes=[1, 2, 1, 2, 1], split_used=True)),
    row("on: K = 3 of 160", dict(calls=3, flags=SOME_PLAIN), obj=ON, family="split", k_calls=1, span=480, state=dict(near_pos=480)),
    row("on: K = 6 of 160, 60 ms", dict(calls=6, flags=SOME_PLAIN), obj=ON, family="split", k_calls=1, span=960, state=dict(near_pos=960)),
    row("on: K = 6 of 80", dict(calls=6, n=80, flags=SOME_PLAIN), obj=ON, family="split", k_calls=1, span=480, mixed_plan=0),
    row("on: the packet form in a uniform object without half calls plans like TickCalls", dict(calls=2, packets=True, flags=SOME_PLAIN), obj=ON, family="split",
        k_calls=1, mixed_plan=0, span=320),
    row("on: idle sessions, junk in their bytes", dict(calls=2, flags=[0, NO_CLEAN, IDLE, IDLE | NO_CLEAN | HALF_CALL | SPLIT_CALLS, 0]), obj=ON, family="split",
        live=3, clean_count=2, plain_count=1, state=dict(modes=[1, 2, 0, 0, 1])),
    row("on: half calls in a packet tick: the packed layout", dict(calls=3, packets=True, flags=[HALF_CALL, NO_CLEAN | HALF_CALL, 0, NO_CLEAN, 0]), obj=ON,
        family="split", k_calls=1, mixed_plan=1, half_calls=1, span=480, clean_count=3, plain_count=2),
    row("on: two rates in a packet tick", dict(calls=2, packets=True, flags=SOME_PLAIN), obj=dict(switch=True, rates=TWO_RATES), family="split", k_calls=1, mixed_plan=1,
        span=320),
    row("on: one call is still the one-call split tick", dict(flags=SOME_PLAIN), obj=ON, family="split", k_calls=0, span=160),
    # ---- the degenerate ticks
    row("on: nobody who calls is flagged: the K-call tick with a clean input", dict(calls=2, flags=[0, IDLE | NO_CLEAN, 0, IDLE | NO_CLEAN, 0]), obj=ON, family="calls",
        k_calls=1, split_tick=0, clean_plane=1, live=3, checked=0, state=dict(split_used=False, modes=[1, 0, 1, 0, 1])),
    row("on: nobody flagged, half calls: the packet tick", dict(calls=2, packets=True, flags=[HALF_CALL, 0, 0, 0, 0]), obj=ON, family="packets", split_tick=0,
        clean_plane=1),
    row("on: every caller flagged: the K-call tick without a clean plane", dict(calls=2, flags=[NO_CLEAN, IDLE, NO_CLEAN, NO_CLEAN, IDLE]), obj=ON, family="calls",
        k_calls=1, split_tick=0, clean_plane=0, clean_count=0, plain_count=3, checked=1, state=dict(split_used=True, modes=[2, 0, 2, 2, 0])),
    row("on: every caller flagged, two rates: the packet tick without a clean plane", dict(calls=2, packets=True, flags=[NO_CLEAN] * S),
        obj=dict(switch=True, rates=TWO_RATES), family="packets", split_tick=0, clean_plane=0, mixed_plan=1),
    row("on: the bit without a clean plane means nothing", dict(calls=2, clean=False, flags=SOME_PLAIN), obj=ON, family="calls", split_tick=0, clean_plane=0,
        checked=0, state=dict(modes=[2] * S, split_used=False)),
    row("on: nobody calls", dict(calls=3, flags=[IDLE | NO_CLEAN] * S), obj=ON, family="nothing", span=480, state=dict(near_pos=480, deferred_lag=480, modes=[0] * S)),
    # ---- the history rule, once per tick
    row("on: a changed kind", dict(calls=2, flags=[NO_CLEAN, 0, 0, NO_CLEAN, 0]), BAD_PARAMETER, before=[dict(calls=2, flags=SOME_PLAIN)], obj=ON,
        state=dict(near_pos=320, modes=[1, 2, 1, 2, 1])),
    row("on: a kind changed after ordinary split ticks", dict(calls=3, flags=[0, 0, 0, NO_CLEAN, 0]), BAD_PARAMETER, before=[dict(flags=SOME_PLAIN)], obj=ON),
    row("on: an ordinary tick that changes a kind after a K-call split tick", dict(flags=[0] * S), BAD_PARAMETER, before=[dict(calls=2, flags=SOME_PLAIN)], obj=ON),
    row("on: the same kinds again with another K", dict(calls=6, flags=SOME_PLAIN), before=[dict(calls=2, flags=SOME_PLAIN), dict(flags=SOME_PLAIN)], obj=ON,
        family="split", k_calls=1, span=960, state=dict(near_pos=320 + 160 + 960)),
    row("on: the first use is checked against what came before", dict(calls=2, flags=SOME_PLAIN), BAD_PARAMETER, before=[dict(clean=False)], obj=ON),
    # ---- everything else TickCalls / TickPackets refuse stays refused
    row("on: split calls on a calling session", dict(calls=2, flags=[SPLIT_CALLS, NO_CLEAN, 0, 0, 0]), BAD_PARAMETER, obj=ON),
    row("on: split calls in a packet tick", dict(calls=2, packets=True, flags=[SPLIT_CALLS, NO_CLEAN, 0, 0, 0]), BAD_PARAMETER, obj=ON),
    row("on: a half call in TickCalls", dict(calls=2, flags=[HALF_CALL, NO_CLEAN, 0, 0, 0]), BAD_PARAMETER, obj=ON),
    row("on: two rates in TickCalls", dict(calls=2, flags=SOME_PLAIN), UNSUPPORTED, obj=dict(switch=True, rates=TWO_RATES)),
    row("on: the safe variant", dict(calls=2, flags=SOME_PLAIN, fast=False), UNSUPPORTED, obj=ON),
    row("on: a session trace", dict(calls=2, flags=SOME_PLAIN), UNSUPPORTED, obj=dict(switch=True, session_trace=True)),
    row("on: seven calls", dict(calls=7, flags=SOME_PLAIN), BAD_PARAMETER, obj=ON),
    # ---- the call trace: out of scope
    row("on, call-traced: a split tick of K calls", dict(calls=2, flags=SOME_PLAIN), UNSUPPORTED, obj=dict(switch=True, call_trace=True), state=dict(call_trace_calls=0)),
    row("on, call-traced: every caller flagged", dict(calls=2, flags=[NO_CLEAN] * S), UNSUPPORTED, obj=dict(switch=True, call_trace=True)),
    row("on, call-traced: nobody flagged is the traced K-call tick", dict(calls=2, flags=[0] * S), obj=dict(switch=True, call_trace=True), family="calls",
        state=dict(call_trace_calls=2)),
    row("on, call-traced: one call is the split tick", dict(flags=SOME_PLAIN), obj=dict(switch=True, call_trace=True), family="split", k_calls=0,
        state=dict(call_trace_calls=1)),
]


def _object(obj):
    obj = dict(obj)
    traces = {k: obj.pop(k, False) for k in ("call_trace", "session_trace")}
    o = T.Object(S, **obj)
    if traces["call_trace"]:
        assert o.call_trace(True)
    if traces["session_trace"]:
        assert o.session_trace(True)
    return o


@pytest.mark.parametrize("obj,before,tick,code,plan,state", TABLE)
def test_plan_table(obj, before, tick, code, plan, state):
    o = _object(obj)
    for b in before:
        assert o.tick(**b)[0] == 0, b
    was = o.state()
    rc, got = o.tick(**tick)
    assert rc == code
    if code:
        assert o.state() == was, "a refused tick changes nothing"
    assert {k: got[k] for k in plan} == plan
    now = o.state()
    assert {k: now[k] for k in state} == state


def test_the_switch_is_the_objects_not_the_sessions():
    """Off in a new object; Init keeps it (the lifetime of force_sparse); switching off brings the refusal back."""
    o = T.Object(S)
    assert not o.switched() and o.tick(calls=2, flags=SOME_PLAIN)[0] == UNSUPPORTED
    o.switch(True)
    assert o.tick(calls=2, flags=SOME_PLAIN)[0] == 0
    o.init()
    assert o.switched() and o.state()["near_pos"] == 0 and o.tick(calls=2, flags=[NO_CLEAN, 0, NO_CLEAN, 0, 0])[0] == 0
    o.switch(False)
    assert o.tick(calls=2, flags=[NO_CLEAN, 0, NO_CLEAN, 0, 0])[0] == UNSUPPORTED and o.tick(flags=[NO_CLEAN, 0, NO_CLEAN, 0, 0])[0] == 0


@pytest.mark.parametrize("n_sessions,ticks", [(5, 400), (11, 400), (257, 40), (300, 40)])
@pytest.mark.parametrize("rates_mode", [0, 1])
def test_whole_objects_on_the_cpu_double(n_sessions, ticks, rates_mode):
    """Objects of both kinds of session through K-call / packet ticks with the switch on: every block input and output sample equals one
    SessionFlow per session called K times with or without the clean pointer; flow words, outputs and snapshot models equal a twin's
    that makes K ordinary split ticks; every live list serves every caller exactly once."""
    tick, d = T.fuzz(7000 + n_sessions + rates_mode, n_sessions, ticks, rates_mode)
    assert tick == -1, d
    split = d["split_calls_ticks"] + d["split_packet_ticks"]
    assert split > ticks // 4 and d["blocks"] > 0 and d["clean_other"] > 0 and d["startup_plain_calls"] > 0, d
    if rates_mode == 1:
        assert d["split_calls_ticks"] > 0, d
    if ticks >= 400:
        assert d["all_clean_ticks"] > 0 and d["all_plain_ticks"] > 0 and d["reinit"] > 0 and d["half_plain"] > 0 and d["nobody"] > 0, d
    if n_sessions == 11:                                  # (five sessions rarely have four callers with a clean input and one without)
        assert d["clean_mult4"] > 0, d


def test_simulator_runs_stand_alone_under_sanitizers():
    """tests/sim/sim_split_calls.cpp has a main of its own: built with AddressSanitizer and UndefinedBehaviorSanitizer into a program
    and run, on the CPU (nothing sanitized is loaded into python)."""
    r = subprocess.run([str(T.standalone())], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.stdout, r.stderr[-2000:])


def test_symbols_are_declared_exported_and_bound():
    import webrtc_aecm_amd as aecm
    from webrtc_aecm_amd import build, ffi
    header = (ROOT / "include" / "aecm_batch.h").read_text()
    lib = ctypes.CDLL(str(build.build()))
    bound = aecm.load()
    assert re.search(rf"\bint32_t {NAME}\(AecmSessions \*s, int32_t on\);", header)
    assert NAME in ffi.SESSIONS_SYMBOLS and hasattr(lib, NAME) and len(getattr(bound, NAME).argtypes) == 2
    assert hasattr(aecm.AecmSessions, "set_split_call_ticks")
    assert getattr(bound, NAME)(None, 1) == -1 and getattr(bound, NAME)(None, 0) == -1      # no object: no device needed
    # both sections say that the call-traced case stays refused; the lifetime of the switch is documented
    assert header.count(NAME) >= 3 and "keeps its value across Init" in header
    for word in ("not supported yet", "While a call trace is attached", "ticks are not call-traced"):
        assert word in header, word


def test_new_units_are_built_like_their_siblings(tmp_path):
    """Both recipes list the two new units; the tick kernels' unit gets the flags of aecm_tick_calls_kernels.hip, the planning kernels'
    unit -- one lane per session, every branch divergent -- none of its own; all six kernels are in the code object; registers and
    scratch of the four tick kernels are no more than those of aecm_tick_calls_kernel<clean> / aecm_tick_packets_kernel<clean> of the
    same build."""
    from test_tick_packets import _kernel_metadata
    from webrtc_aecm_amd import build
    tick, plan = "aecm_tick_split_calls_kernels.hip", "aecm_tick_split_calls_plan_kernels.hip"
    assert tick in build.KERNEL_SOURCES and plan in build.KERNEL_SOURCES
    assert build.SOURCE_FLAGS[tick] == build.SOURCE_FLAGS["aecm_tick_calls_kernels.hip"] == build.UNIFORM_BRANCH_FLAGS and plan not in build.SOURCE_FLAGS
    cmake = (ROOT / "CMakeLists.txt").read_text()
    assert tick in cmake and plan in cmake and re.search(r'src MATCHES "aecm_tick_split_calls_plan_kernels"', cmake)
    meta = _kernel_metadata(tmp_path)
    for name in ("aecm_flow_plan_split_calls_kernelE", "aecm_flow_plan_split_packets_kernelE"):
        assert len([k for k in meta if name in k]) == 1, name
    for kind in ("calls", "packets"):
        for clean in (0, 1):
            (name, ours), = [(k, v) for k, v in meta.items() if f"aecm_tick_split_{kind}_kernelILb{clean}E" in k]
            (_, sibling), = [(k, v) for k, v in meta.items() if f"aecm_tick_{kind}_kernelILb{clean}E" in k]
            print(name, "sgpr, vgpr, scratch", ours, "sibling", sibling)
            assert all(a <= b for a, b in zip(ours, sibling)), (name, ours, sibling)


@pytest.mark.parametrize("name", sorted(sch.GOLDEN_CASES))
def test_golden_run_is_what_its_recipe_says(name):
    """tests/golden/sesssplitcalls_*.npz (tools/gen_golden.py; run on the GPU by tests/test_gpu_split_calls.py): arrays only, the
    pattern the recipe gives, zeros and code 0 where a session sat out; where the unmodified reference is built, its instances --
    the flagged sessions' called without a clean pointer -- give exactly the stored outputs, codes and echo paths."""
    import calls_helpers as ch
    import sparse_helpers as sh
    import split_helpers as sph
    from oracle import pyoracle
    path = GOLDEN / f"{name}.npz"
    assert path.stat().st_size < 150 * 1024
    g = np.load(path, allow_pickle=False)
    fs, n, K, seed = sch.GOLDEN_CASES[name]
    assert sorted(g.files) == sorted(["seed", "fs", "frame", "calls", "never", "flags", "ms", "out", "codes", "paths"])
    assert (int(g["fs"]), int(g["frame"]), int(g["calls"]), int(g["seed"])) == (fs, n, K, seed) and g["never"].tolist() == list(sph.NEVER11)
    flags, ms = sch.golden_pattern(K, seed)
    Tn = sch.GOLDEN_CALLS // K
    assert np.array_equal(g["flags"], flags) and np.array_equal(g["ms"], ms) and flags.shape == (Tn, sph.S11)
    idle = (flags & IDLE) != 0
    assert not (flags & (SPLIT_CALLS | HALF_CALL)).any() and (flags[:, list(sph.NEVER11)][~idle[:, list(sph.NEVER11)]] & NO_CLEAN).all()
    kinds = [((flags[t] & NO_CLEAN) != 0)[~idle[t]] for t in range(Tn)]
    assert all(k.any() and not k.all() for k in kinds), "every tick has callers of both kinds"
    counts = {int((~k).sum()) % 4 == 0 for k in kinds}
    assert counts == {True, False}, "clean counts that are a multiple of four and that are not"
    out = g["out"].reshape(sph.S11, Tn, K * n)
    assert g["out"].dtype == np.int16 and not out[idle.T].any() and not g["codes"][idle].any() and out[~idle.T].any()
    assert 0.1 < idle.mean() < 0.35 and 12100 in g["codes"] and g["paths"].shape == (sph.S11, 65)
    if pyoracle.have_reference():
        far, near, clean = sh.signals(seed, sph.S11, sch.GOLDEN_CALLS * n, fs, with_clean=True)
        refs = sch.reference_sessions(lambda rate: pyoracle.RefSession(rate, 1, 3), [fs] * sph.S11, sph.NEVER11)
        eout, ecodes, _ = ch.run_reference(None, ch.calls_ops(K, n, flags, ms), ch.Feed(far, near, sph.object_clean(clean, sph.NEVER11)), sessions=refs)
        assert np.array_equal(eout, g["out"]) and np.array_equal(ecodes, g["codes"])
        assert np.array_equal(np.stack([r.get_echo_path()[1] for r in refs]), g["paths"])
        # the kinds matter: with a clean pointer for everybody the flagged sessions' outputs differ
        plain, _, _ = ch.run_reference(lambda: pyoracle.RefSession(fs, 1, 3), ch.calls_ops(K, n, flags, ms), ch.Feed(far, near, clean))
        assert all(not np.array_equal(plain[s], eout[s]) for s in sph.NEVER11)
        assert all(np.array_equal(plain[s], eout[s]) for s in range(sph.S11) if s not in sph.NEVER11)
