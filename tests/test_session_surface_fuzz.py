"""The session surface fuzz without a device (tests/surface_fuzz.py): the programs are deterministic, they cover what they claim to
cover, and the host planner (aecm_tick_plan.h compiled for the CPU: tickplan_sim.Object) answers every tick of every program with the
code of the rule table and keeps the model's clean modes.

The reference side of a case (the whole program on one reference instance per slot), measured on the build machine:
small-16k 0.4 s, small-8k 0.3 s, wave-mixed 1.8 s, group-mixed 3.9 s."""
import json
from collections import Counter
from pathlib import Path

import numpy as np
import pytest

import surface_fuzz as sf
import tickplan_sim as T
from oracle import pyoracle

GOLDEN = Path(__file__).resolve().parent / "golden" / "session_surface_fuzz.json"
CASE_NAMES = sorted(sf.CASES)
needs_ref = pytest.mark.skipif(not pyoracle.have_reference(), reason="oracle/_ref/libaecm_ref.so not built")
_programs, _models = {}, {}


def program(case):
    if case not in _programs:
        _programs[case] = sf.generate(case)
    return _programs[case]


def model(case):
    """The program on the reference, once per case."""
    if case not in _models:
        _models[case] = sf.run_reference(case, program(case))
    return _models[case]


@pytest.mark.parametrize("case", CASE_NAMES)
def test_program_is_deterministic(case):
    """Two generations give the same program, a prefix is the program's prefix, and its SHA-256 is the pinned one."""
    again = sf.generate(case)
    assert again == program(case) and sf.generate(case, 25) == program(case)[:25]
    assert sf.program_sha256(program(case)) == json.loads(GOLDEN.read_text())[case]["program"]


@needs_ref
@pytest.mark.parametrize("case", CASE_NAMES)
def test_expected_outputs_are_pinned(case):
    """The reference's codes, outputs and echo paths over the program: their SHA-256 is the pinned one (tools/gen_golden.py)."""
    assert model(case).digest.hexdigest() == json.loads(GOLDEN.read_text())[case]["expected"]


@pytest.mark.parametrize("case", CASE_NAMES)
def test_program_covers_the_surface(case):
    """Conditions on the program, not measurements: every op kind at least 5 times, every flag at least 20 times on a calling session,
    every K in 2 .. 6 at least 3 times through TickCalls (where the object holds one rate) and TickPackets, at least 10 migrations and
    3 of them between a burst and the session's next Process call, every refusal rule at least once, about one op in eight refused,
    an Async chain that ends in an export without Synchronize, every form of every entry point."""
    prog = program(case)
    c = sf.CASES[case]
    cov = Counter(op.get("cov") for op in prog)
    assert all(cov[k] >= 5 for k in sf.KINDS), {k: cov[k] for k in sf.KINDS if cov[k] < 5}
    ticks = [op for op in prog if op["kind"] == "tick" and "rule" not in op]
    flags = Counter()
    for op in ticks:
        for f in op["flags"] or []:
            for bit in sf.FLAG_NAMES:
                flags[bit] += bool(f & bit) and (bit == sf.IDLE or not f & sf.IDLE)
    assert all(flags[bit] >= 20 for bit in sf.FLAG_NAMES), flags
    ks = Counter((op["entry"], op["K"]) for op in ticks)
    entries = ("TickCalls", "TickPackets") if c["rates"] == "uniform" else ("TickPackets",)       # (an object of two rates refuses TickCalls with K > 1)
    assert all(ks[(e, k)] >= 3 for e in entries for k in range(2, 7)), ks
    forms = Counter((op["entry"], op["form"]) for op in ticks)
    assert all(forms[(e, f)] >= 1 for e, fs in sf.FORMS.items() for f in fs), forms
    assert {80, 160} == {op["n"] for op in ticks} and any(op["clean"] for op in ticks) and any(not op["clean"] for op in ticks)
    assert any(isinstance(op["ms"], int) for op in ticks) and any(isinstance(op["ms"], list) for op in ticks)
    assert sum(op.get("expect") == sf.WARNING for op in ticks) >= 3
    assert any(op["kind"] == "burst" and op["calls"] == 40 for op in prog)
    # migrations, and those of a session with far frames buffered and no Process call since
    sh, moved, pending = sf.Shadow(case), 0, 0
    for op in prog:
        if op["kind"] in ("migrate", "migrate_bulk") and "rule" not in op:
            moved += 1
            pending += any(sh.ob[op["obj"]].pending[s] for s in ([op["s"]] if op["kind"] == "migrate" else op["ss"]))
        sh.apply(op)
    assert moved >= 10 and pending >= 3, (moved, pending)
    assert any(op["kind"] == "migrate" and not op["sync_before"] for op in prog)
    rules = Counter(op["rule"] for op in prog if "rule" in op)
    assert all(rules[name] >= 1 for name in sf.RULE_NAMES), rules
    assert len(prog) / 12 <= sum(rules.values()) <= len(prog) / 5, (sum(rules.values()), len(prog))
    traced = Counter()
    sh = sf.Shadow(case)
    for op in prog:
        if op["kind"] == "trace" and op["which"]:
            traced[(op["which"], op["ring"], op["layout"])] += 1
        sh.apply(op)
    assert {k[0] for k in traced} == {"session", "call"} and {k[1] for k in traced} == {1, 3} and len({k[2] for k in traced}) == 2, traced
    if sf.special_slots(case):                             # the single-slot ops of the larger cases: mostly at the lanes that matter
        single = [op["s"] for op in prog if "s" in op and "rule" not in op]
        assert sum(s in sf.special_slots(case) for s in single) >= len(single) // 2


def test_every_refusal_rule_occurs():
    """All rows of the refusal table occur over the cases (each occurs in each: test_program_covers_the_surface)."""
    seen = set()
    for case in CASE_NAMES:
        seen |= {op["rule"] for op in program(case) if "rule" in op}
    assert seen == set(sf.RULE_NAMES)


@needs_ref
@pytest.mark.parametrize("case", CASE_NAMES)
def test_the_canceller_works(case):
    """At least a quarter of all compared session-calls give an output that is not the copy of their input: past start-up."""
    m = model(case)
    assert m.compared > 0 and 4 * m.working >= m.compared, (m.working, m.compared)


@pytest.mark.parametrize("case", CASE_NAMES)
def test_planner_twin_agrees(case):
    """Every tick and Process op of the program through the host planner twin: its code is the rule table's (refused ticks included; an
    accepted tick's is 0 -- the msInSndCardBuf warning is not the planner's), its clean modes are the model's after EVERY op, its trace
    counts are the model's, and the families it names over the case are the list written next to the case.
    SetSplitCallTicks, ForceSparseTicks, the two traces and the safe variant are inputs of the planner and are passed through.
    WebRtcAecmSessions_SplitCleanTwoLaunches is not: the planner takes no such input on the host (SessionBatch decides the launch count
    of a split tick behind the plan), so "two_launches" ops are not given to the twin -- no tick is excluded for it.  Far-end bursts,
    set_config_session, the echo-path ops and Synchronize do not reach the planner either."""
    prog = program(case)
    sh = sf.Shadow(case)
    twin = [T.Object(ob.S, ob.fs, rates=ob.rates) for ob in sh.ob]
    families = set()
    for op in prog:
        o, k = op["obj"], op["kind"]
        ob, tw = sh.ob[o], twin[o]
        refused = op.get("expect", 0) not in (0, sf.WARNING)
        if k in ("tick", "process"):
            common = dict(n=op["n"], calls=op.get("K", 1), stride=op["stride"], clean=op["clean"], host=op["form"] == "host",
                          ms_per_session=isinstance(op["ms"], list), fast=not ob.safe)
            if k == "process":
                rc, plan = tw.tick(all_flags=sf.NO_FAREND, far=False, **common)
            else:
                rc, plan = tw.tick(flags=op["flags"], packets=op["entry"] == "TickPackets", **common)
            assert rc == (op["expect"] if refused else 0), (case, sf.describe(op), rc)
            if not refused:
                families.add(plan["family"])
        elif refused:
            pass
        elif k == "init_session":
            tw.init_session(op["s"], ob.fs)
        elif k == "init_session_rate":
            tw.init_session(op["s"], op["rate"])
        elif k in ("migrate", "migrate_bulk"):
            pairs = [(op["s"], op["j"])] if k == "migrate" else zip(op["ss"], op["js"])
            for s, j in pairs:
                twin[op["dst"]].init_session(j, ob.rates[s])
        elif k == "force_sparse":
            tw.force_sparse(op["on"])
        elif k == "split_call_ticks":
            tw.split_call_ticks(op["on"])
        elif k == "trace":
            if op["which"] is None:
                assert tw.attach_trace(ob.trace, False)
            else:
                assert tw.attach_trace(op["which"], True)
        sh.apply(op)
        for x in range(2):
            assert twin[x].state()["modes"] == sh.ob[x].mode, (case, sf.describe(op), x)
            want = sh.ob[x].trace_count
            assert twin[x].trace_counts() == (want if sh.ob[x].trace == "session" else 0, want if sh.ob[x].trace == "call" else 0), (case, sf.describe(op))
            assert twin[x].state()["other_rates"] == sh.ob[x].other_rates()
    assert sorted(families) == sf.CASES[case]["families"], sorted(families)


def test_listing(capsys):
    """python -m surface_fuzz --case .. --until .. --print: one line per op, a refusal with its rule."""
    sf.main(["--case", "small-16k", "--until", "60", "--print"])
    out = capsys.readouterr().out.splitlines()
    assert len(out) == 61 and out[0].startswith("small-16k: 60 ops")
    prog = program("small-16k")[:60]
    assert all(("refused: " + op["rule"]) in line for op, line in zip(prog, out[1:]) if "rule" in op)
    sf.main(["--case", "small-16k", "--until", "60", "--session", "A3", "--print"])
    assert 1 < len(capsys.readouterr().out.splitlines()) <= 61
