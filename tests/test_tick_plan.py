"""The host's plan of a session tick (webrtc_aecm_amd/csrc/aecm_tick_plan.h) without a GPU: which ticks are refused and with which code,
which kernels an accepted tick takes, what it hands the planning launch and what it leaves in the object.  The expectations of the two
tables are written from the contract of SessionBatch::Tick (aecm_sessions.h) and of FlowRouteTick[Mixed] (aecm_flow_plan.h), not taken
from the planner; the random run compares it with the one restatement from the primitives (tests/sim/sim_tickplan.cpp)."""
import subprocess

import pytest

import tickplan_sim as T
from tickplan_sim import BAD_PARAMETER, HALF_CALL, IDLE, NO_CLEAN, NO_FAREND, NULL_POINTER, SPLIT_CALLS, UNINITIALIZED, UNSPECIFIED, UNSUPPORTED

S = 5
ALL_IDLE = [IDLE] * S
SOME_IDLE = [0, IDLE, 0, 0, IDLE]
SOME_PLAIN = [0, NO_CLEAN, 0, NO_CLEAN, 0]
TWO_RATES = [16000, 16000, 8000, 16000, 16000]
JUNK = IDLE | HALF_CALL | SPLIT_CALLS | NO_FAREND | NO_CLEAN | 0xe0


def row(name, tick, code=0, before=(), obj=None, state=None, **plan):
    return pytest.param(obj or {}, before, tick, code, plan, state or {}, id=name)


# (name, the tick, [code], [before: ticks the object has accepted first], [obj: Object's keywords], [state: the object afterwards], the plan)
TABLE = [
    # ---- every family, and what decides between them
    row("dense: everybody calls, everybody in step", dict(), family="dense", live=5, span=160, sparse_plan=0, sparse_tick=0, deferred_lag=0, need_slot=0,
        state=dict(near_pos=160, deferred_lag=0, may_lag=False)),
    row("dense of 80 samples", dict(n=80), family="dense", span=80, state=dict(near_pos=80)),
    row("dense with per-session ms: a slot", dict(ms_per_session=True), family="dense", need_slot=1),
    row("dense with a flags array nobody uses: a slot", dict(flags=[0] * S), family="dense", live=5, need_slot=1, sparse_tick=0),
    row("two calls of 80 in 160 samples are an ordinary tick", dict(flags=[SPLIT_CALLS, 0, 0, 0, 0]), family="dense", live=5),
    row("sparse: somebody sits out", dict(flags=SOME_IDLE), family="sparse", live=3, sparse_plan=1, sparse_tick=1, deferred_lag=0, need_slot=1, mixed_plan=0,
        state=dict(near_pos=160, may_lag=True, deferred_lag=0)),
    row("nobody calls: nothing launched, the lag deferred", dict(flags=ALL_IDLE), family="nothing", live=0, need_slot=0, sparse_tick=0, deferred_lag=0,
        state=dict(near_pos=160, deferred_lag=160, may_lag=True, modes=[0] * S)),
    row("nobody calls, a lag already deferred", dict(flags=ALL_IDLE, n=80), before=[dict(flags=ALL_IDLE)], family="nothing", live=0, deferred_lag=0,
        state=dict(near_pos=240, deferred_lag=240, may_lag=True)),
    row("nobody calls a K-call tick: the whole span is deferred", dict(flags=ALL_IDLE, calls=2), family="nothing", span=320, need_slot=0,
        state=dict(near_pos=320, deferred_lag=320)),
    row("everybody calls after an all-idle tick: sparse plan, dense tick", dict(), before=[dict(flags=ALL_IDLE)], family="sparse", live=5, sparse_plan=1,
        sparse_tick=0, deferred_lag=160, need_slot=0, state=dict(near_pos=320, deferred_lag=0, may_lag=False)),
    row("everybody calls after a sparse tick: sparse plan, dense tick", dict(), before=[dict(flags=SOME_IDLE)], family="sparse", sparse_plan=1, sparse_tick=0,
        deferred_lag=0, state=dict(may_lag=False)),
    row("and the tick after that is dense again", dict(), before=[dict(flags=SOME_IDLE), dict()], family="dense", sparse_plan=0),
    row("somebody calls after two all-idle ticks: both handed over", dict(flags=SOME_IDLE), before=[dict(flags=ALL_IDLE), dict(flags=ALL_IDLE, n=80)], family="sparse",
        sparse_tick=1, deferred_lag=240, state=dict(near_pos=400, deferred_lag=0, may_lag=True)),
    row("force_sparse: the live list although everybody calls", dict(), obj=dict(force_sparse=True), family="sparse", live=5, sparse_plan=1, sparse_tick=1, need_slot=1,
        state=dict(may_lag=False)),
    row("a half call with everyone live: mixed plan, object out of step", dict(flags=[HALF_CALL, 0, 0, 0, 0]), family="mixed", live=5, sparse_plan=1, sparse_tick=0,
        mixed_plan=1, half_calls=1, need_slot=1, state=dict(may_lag=True, near_pos=160)),
    row("after a half call the next full tick still plans sparse", dict(), before=[dict(flags=[HALF_CALL, 0, 0, 0, 0])], family="sparse", sparse_tick=0, mixed_plan=0,
        state=dict(may_lag=False)),
    row("a half call among idle sessions", dict(flags=[HALF_CALL, IDLE, 0, 0, 0]), family="mixed", live=4, sparse_tick=1, mixed_plan=1),
    row("an object of two rates plans every tick per session", dict(), obj=dict(rates=TWO_RATES), family="mixed", sparse_plan=1, sparse_tick=0, mixed_plan=1, need_slot=0,
        state=dict(other_rates=1, may_lag=False)),
    row("two rates, K calls, no packets", dict(calls=2), UNSUPPORTED, obj=dict(rates=TWO_RATES)),
    row("two rates, K calls, packets", dict(calls=2, packets=True), obj=dict(rates=TWO_RATES), family="packets", span=320, sparse_tick=1, mixed_plan=1, need_slot=1,
        state=dict(near_pos=320)),
    row("K calls in a uniform object: always by the live list", dict(calls=3), family="calls", span=480, live=5, sparse_plan=1, sparse_tick=1, need_slot=1, mixed_plan=0,
        state=dict(near_pos=480, may_lag=False)),
    row("K calls of 80 samples, somebody idle", dict(calls=6, n=80, flags=SOME_IDLE), family="calls", span=480, live=3, state=dict(may_lag=True)),
    row("a packet tick in a uniform object without half calls IS the K-call tick", dict(calls=2, packets=True, flags=[NO_FAREND, 0, 0, 0, 0]), family="calls",
        mixed_plan=0, sparse_tick=1),
    row("a packet tick with a half call", dict(calls=2, packets=True, flags=[HALF_CALL, 0, 0, 0, 0]), family="packets", mixed_plan=1, half_calls=1, span=320,
        state=dict(may_lag=True)),
    row("a packet of one call is the ordinary tick", dict(calls=1, packets=True), family="dense"),
    row("a half call in a K-call tick without packets", dict(calls=2, flags=[HALF_CALL, 0, 0, 0, 0]), BAD_PARAMETER),
    row("split calls in a K-call tick", dict(calls=2, flags=[SPLIT_CALLS, 0, 0, 0, 0]), BAD_PARAMETER),
    row("split calls in a packet tick", dict(calls=2, packets=True, flags=[SPLIT_CALLS, 0, 0, 0, 0]), BAD_PARAMETER),
    row("split calls for everybody in a K-call tick", dict(calls=2, all_flags=SPLIT_CALLS), BAD_PARAMETER),
    # ---- the clean input per session
    row("no caller flagged: the tick with a clean input", dict(clean=True, flags=[0] * S), family="dense", clean_plane=1, split_tick=0, checked=0,
        state=dict(modes=[1] * S, split_used=False)),
    row("every caller flagged: the launches of the tick without one", dict(clean=True, flags=[NO_CLEAN] * S), family="dense", clean_plane=0, split_tick=0, clean_count=0,
        plain_count=5, checked=1, state=dict(modes=[2] * S, split_used=True)),
    row("every caller flagged, somebody idle", dict(clean=True, flags=[NO_CLEAN, IDLE, NO_CLEAN, NO_CLEAN, IDLE | 3]), family="sparse", clean_plane=0, split_tick=0,
        plain_count=3, state=dict(modes=[2, 0, 2, 2, 0])),
    row("some callers flagged: the split tick, by the two lists", dict(clean=True, flags=SOME_PLAIN), family="split", live=5, clean_plane=1, split_tick=1, clean_count=3,
        plain_count=2, sparse_tick=1, sparse_plan=1, need_slot=1, checked=1, state=dict(modes=[1, 2, 1, 2, 1], split_used=True, may_lag=False)),
    row("a split tick with idle sessions", dict(clean=True, flags=[0, NO_CLEAN, IDLE, IDLE | NO_CLEAN, 0]), family="split", live=3, clean_count=2, plain_count=1,
        state=dict(modes=[1, 2, 0, 0, 1], may_lag=True)),
    row("a split tick with a half call", dict(clean=True, flags=[HALF_CALL, NO_CLEAN, 0, 0, 0]), family="split", mixed_plan=1, half_calls=1, clean_count=4, plain_count=1),
    row("a split tick of K calls", dict(clean=True, calls=2, flags=SOME_PLAIN), UNSUPPORTED),
    row("the bit without a clean plane means nothing", dict(flags=SOME_PLAIN), family="dense", clean_plane=0, split_tick=0, clean_count=0, plain_count=0, checked=0,
        state=dict(modes=[2] * S, split_used=False)),
    row("the bit in the one byte for everybody means nothing", dict(clean=True, all_flags=NO_CLEAN), family="dense", clean_plane=1, split_tick=0, checked=0,
        state=dict(modes=[1] * S)),
    row("a kind changed after a split tick", dict(clean=True, flags=[NO_CLEAN, 0, 0, NO_CLEAN, 0]), BAD_PARAMETER, before=[dict(clean=True, flags=SOME_PLAIN)],
        state=dict(near_pos=160, modes=[1, 2, 1, 2, 1])),
    row("after a split tick a tick without flags gives everybody a clean input", dict(clean=True), BAD_PARAMETER, before=[dict(clean=True, flags=SOME_PLAIN)]),
    row("after a split tick a tick without a clean plane", dict(), BAD_PARAMETER, before=[dict(clean=True, flags=SOME_PLAIN)]),
    row("after a split tick: the same kinds again, idle bytes junk", dict(clean=True, flags=[JUNK, NO_CLEAN, 0, NO_CLEAN, JUNK]), before=[dict(clean=True, flags=SOME_PLAIN)],
        family="split", live=3, clean_count=1, plain_count=2, checked=1),
    row("after a split tick: only the sessions without call, the plain launches", dict(clean=True, flags=[IDLE, NO_CLEAN, IDLE, NO_CLEAN, IDLE]),
        before=[dict(clean=True, flags=SOME_PLAIN)], family="sparse", clean_plane=0, split_tick=0, plain_count=2, live=2),
    row("the same change before any split tick: accepted, unchecked", dict(), before=[dict(clean=True)], family="dense", checked=0,
        state=dict(modes=[3] * S, split_used=False)),
    row("a kind changed per session before any split tick: unchecked", dict(clean=True, flags=[0] * S), before=[dict()], family="dense", checked=0, state=dict(modes=[3] * S)),
    # ---- flags that need 160 samples or exclude each other; idle bytes
    row("split calls in 80 samples", dict(n=80, flags=[0, SPLIT_CALLS, 0, 0, 0]), BAD_PARAMETER),
    row("split calls for everybody in 80 samples", dict(n=80, all_flags=SPLIT_CALLS), BAD_PARAMETER),
    row("a half call in 80 samples", dict(n=80, flags=[0, 0, HALF_CALL, 0, 0]), BAD_PARAMETER),
    row("half and split on one session", dict(flags=[0, 0, HALF_CALL | SPLIT_CALLS, 0, 0]), BAD_PARAMETER),
    row("half on one session, split on another", dict(flags=[HALF_CALL, SPLIT_CALLS, 0, 0, 0]), family="mixed", mixed_plan=1),
    row("idle sessions whose other bits are junk, 80 samples", dict(n=80, flags=[JUNK, 0, JUNK, 0, 0]), family="sparse", live=3, half_calls=0, mixed_plan=0, split_tick=0),
    row("idle junk with a clean plane is no split tick", dict(clean=True, flags=[JUNK, 0, 0, 0, 0]), family="sparse", split_tick=0, clean_plane=1, checked=0),
    # ---- pointers and scalars
    row("near or out null", dict(near_out=False), NULL_POINTER),
    row("far null while everybody buffers", dict(far=False), NULL_POINTER),
    row("far null while one session buffers", dict(far=False, flags=[NO_FAREND, IDLE, NO_FAREND, 0, IDLE]), NULL_POINTER),
    row("far null, nobody buffers (one byte)", dict(far=False, all_flags=NO_FAREND), family="dense"),
    row("far null, nobody buffers (per session)", dict(far=False, flags=[NO_FAREND, IDLE, NO_FAREND, NO_FAREND | SPLIT_CALLS, IDLE]), family="sparse", live=3),
    row("not initialised", dict(), UNINITIALIZED, obj=dict(fs=0)),
    row("81 samples", dict(n=81), BAD_PARAMETER),
    row("2^32 + 80 samples", dict(n=2**32 + 80, stride=2**33), BAD_PARAMETER),
    row("no calls", dict(calls=0), BAD_PARAMETER),
    row("seven calls", dict(calls=7), BAD_PARAMETER),
    row("rows shorter than the tick", dict(calls=2, stride=319), BAD_PARAMETER),
    row("poisoned", dict(poisoned=True), UNSPECIFIED),
    row("the safe variant", dict(fast=False), UNSUPPORTED),
    # ---- host output
    row("host output, everybody calls: nothing to zero", dict(host=True), family="dense", zero_out=0),
    row("host output, somebody idle: zeros first", dict(host=True, flags=SOME_IDLE), family="sparse", zero_out=1),
    row("host output, a half call: zeros first", dict(host=True, flags=[HALF_CALL, 0, 0, 0, 0]), family="mixed", zero_out=1),
    row("host output, nobody calls: zeros", dict(host=True, flags=ALL_IDLE), family="nothing", zero_out=1),
    row("device output is never zeroed", dict(flags=SOME_IDLE), family="sparse", zero_out=0),
]


@pytest.mark.parametrize("obj,before,tick,code,plan,state", TABLE)
def test_table(obj, before, tick, code, plan, state):
    o = T.Object(S, **obj)
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


def test_table_covers_every_family_and_code():
    assert {p.values[4].get("family") for p in TABLE} >= set(T.families())
    assert {p.values[3] for p in TABLE} >= {0, UNSPECIFIED, UNSUPPORTED, UNINITIALIZED, NULL_POINTER, BAD_PARAMETER}
    assert 40 <= len(TABLE)


def test_family_names():
    assert T.families() == ["nothing", "dense", "sparse", "mixed", "calls", "packets", "split"]


@pytest.mark.parametrize("n_sessions", [5, 257])
@pytest.mark.parametrize("case", T.COINCIDING, ids=lambda c: c["name"])
def test_coinciding_defects(case, n_sessions):
    """Two adjacent checks tripped at once: the earlier one's code, and nothing changed."""
    o = T.Object(n_sessions, fs=0 if case.get("uninit") else 16000, rates=T.pattern(n_sessions, *case["rates"]) if "rates" in case else None)
    if case.get("after_split"):
        assert o.tick(**dict(T.SPLIT_FIRST, flags=T.pattern(n_sessions, *T.SPLIT_FIRST["flags"])))[0] == 0
    tick = dict(case["tick"])
    if "flags" in tick:
        tick["flags"] = T.pattern(n_sessions, *tick["flags"])
    was = o.state()
    assert o.tick(**tick)[0] == case["code"]
    assert o.state() == was


def test_planning_is_pure():
    """Planning the same tick twice without a commit gives equal plans and leaves the object alone."""
    o = T.Object(S)
    assert o.tick(flags=ALL_IDLE)[0] == 0 and o.tick(clean=True, flags=[0, NO_CLEAN, IDLE, 0, 0])[0] == 0
    was = o.state()
    for tick in (dict(clean=True, flags=SOME_PLAIN), dict(flags=ALL_IDLE), dict(clean=True, flags=[0, NO_CLEAN, 0, IDLE, HALF_CALL]), dict(clean=True)):
        first = o.tick(commit=False, **tick)
        assert o.tick(commit=False, **tick) == first and o.state() == was


def test_codes():
    """The warning for an msInSndCardBuf outside 0 .. 500, per session; a session that sits out has no code."""
    assert T.codes(40, None, S) == (0, [0] * S)
    assert T.codes(501, None, S) == (T.WARNING, [T.WARNING] * S)
    assert T.codes(-1, SOME_IDLE, S) == (T.WARNING, [T.WARNING, 0, T.WARNING, T.WARNING, 0])
    assert T.codes([0, 500, 40, 40, 40], None, S) == (0, [0] * S)
    assert T.codes([40, 501, 40, -1, 40], None, S) == (T.WARNING, [0, T.WARNING, 0, T.WARNING, 0])
    assert T.codes([40, 501, 40, -1, 900], SOME_IDLE, S) == (T.WARNING, [0, 0, 0, T.WARNING, 0])
    assert T.codes([40, 501, 40, 40, 900], SOME_IDLE, S) == (0, [0] * S)


@pytest.mark.parametrize("n_sessions", [1, 5, 256, 257, 600])
def test_random_ticks_against_the_primitives(n_sessions):
    """10^4 random ticks (flags, calls, packets, n, clean, sessions initialised anew in between): every plan field and the object after
    every tick equal the restatement's; a refused tick leaves the object as it was; planning twice gives one plan."""
    at, what, seen = T.fuzz(1000 + n_sessions, n_sessions, 10_000)
    assert (at, what) == (-1, 0), seen
    assert all(seen[f] > 0 for f in seen if not (f == "split" and n_sessions == 1)), seen      # (one session cannot be of both kinds)


def test_standalone_under_sanitizers():
    """The same run as a program of its own under AddressSanitizer and UBSan (nothing sanitized is loaded into python)."""
    run = subprocess.run([str(T.standalone())], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and run.stdout.strip().endswith("ok"), run.stdout + run.stderr
