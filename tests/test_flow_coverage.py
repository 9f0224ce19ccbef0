"""The session-flow corpus (tests/flow_corpus.py) stays decision-complete, and divergently so: tools/flow_coverage.py builds the
host harness over aecm_flow_plan.h and SessionFlow<T> (tests/sim/sim_flowcov.cpp) with -O0 --coverage and the header's decision
markers on, drives every object of the corpus through it the way the planning kernels do and reads gcov's branch counts and the
markers' record of outcomes per tick and session.  Three sets must be exactly what tests/flow_allowlist.json lists and argues:
the decisions taken one way only, the decisions never taken divergently within a wavefront by any planner, and -- every planner
being a compilation of its own -- the (decision, planner) pairs in which a planner evaluates a decision but never divergently.  The
harness's plans and wrapper states must move the sample tags SessionFlow<T> moves, for every session and tick of the corpus.
(profiles/r23_flow_decision_coverage.txt has the same measurement for what the suite fed before the corpus.)"""
import importlib.util
import json
import re
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
ALLOWLIST = ROOT / "tests" / "flow_allowlist.json"
_spec = importlib.util.spec_from_file_location("flow_coverage", ROOT / "tools" / "flow_coverage.py")
F = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(F)

pytestmark = pytest.mark.skipif(bool(F.tools_missing()), reason=f"not installed: {F.tools_missing()}")

# the decisions the corpus was written for (the issue's list), by marker: each must go both ways AND diverge within a wavefront
MUST_DIVERGE = ("SU_COUNTER_ZERO", "SU_TOL_ABS", "SU_TOL_REL", "SU_COUNTER_LIMIT", "SU_CTR_LIMIT", "SU_CLAMP_MEAN", "SU_CLAMP_LAST", "SU_FILLED_EQ",
                "SU_FILLED_GT", "DC_FIRES", "DC_NADD_FLOOR", "DC_NADD_CEILING", "MRP_BY_READABLE", "MRP_BY_FREE", "FC_TRUNCATED", "FC_NOTHING_FITS",
                "T_NO_FAREND", "EB_SHORT", "EB_ACC_NOT_POSITIVE", "EB_DIFF_HIGH", "EB_HIGH_LAST_LOW", "EB_DIFF_LOW", "EB_KNOWN_POSITIVE",
                "EB_LOW_LAST_HIGH", "EB_CHANGE", "EB_KNOWN_FLOOR", "T_FRESH", "T_REPLAY_IN_RING", "T_NEW_RUN", "T_TWO_BLOCKS", "T_STUFF", "T_SPILL_SET",
                "T_SPILL_NOT_REFRESHED", "T_DIRECT", "T_FF_WAS_DIRECT", "T_LEFT_PENDING", "T_MS_NEGATIVE", "T_MS_HIGH", "T_SPLIT_FLAG", "K_RESYNC",
                "MN_BACKWARDS", "TM_HALF_FLAG", "PK_HALF_FLAG", "K_LIVE", "T_STARTUP", "T_ACTIVE1")
# the kinds of argument an entry may rest on: a kernel argument or another value that is the same for every lane of the launch, a
# range that excludes one side, a refusal of the entry points, a test every caller has made already -- never "no scenario reaches it"
REASON_KINDS = re.compile(r"kernel argument|dead by range|dead in these|refus|a constant in|one session per wavefront|wave-uniform|every caller|under its own", re.I)


@pytest.fixture(scope="module")
def report():
    return F.measure("corpus")


@pytest.fixture(scope="module")
def allow():
    return json.loads(ALLOWLIST.read_text())


def _compare(got, listed, what):
    new, gone = sorted(set(got) - set(listed)), sorted(set(listed) - set(got))
    assert not new, f"{what} that the allowlist does not have (a scenario was lost?):\n  " + "\n  ".join(map(str, new))
    assert not gone, f"allowlist entries ({what}) that no longer hold (or are spelled differently): take them off the list:\n  " + "\n  ".join(map(str, gone))


def test_one_way_decisions_are_exactly_the_allowlist(report, allow):
    got = F.one_way_branches(report) + ["marker " + n for n in F.one_way_markers(report)]
    _compare(got, [e["key"] for e in allow["one_way"]], "decisions the corpus takes one way only")


def test_decisions_never_divergent_within_a_wavefront_are_exactly_the_allowlist(report, allow):
    _compare(["marker " + n for n in F.never_divergent(report)], [e["key"] for e in allow["never_divergent"]],
             "decisions that go both ways but never divergently within a wavefront")


def test_per_planner_exceptions_are_exactly_the_allowlist(report, allow):
    got = [f"marker {n} in {p.split(':')[0]}" for n, planners in F.undiverged_by_planner(report).items() for p in planners]
    listed = [f"{e['key']} in {p}" for e in allow["per_planner"] for p in e["planners"]]
    _compare(got, listed, "(decision, planner) pairs in which the planner evaluates the decision but never divergently")


def test_the_allowlist_is_argued(allow):
    assert set(allow) == {"one_way", "never_divergent", "per_planner"}
    for section, entries in allow.items():
        assert len({e["key"] for e in entries}) == len(entries), section
        for e in entries:
            assert set(e) == ({"key", "planners", "reason"} if section == "per_planner" else {"key", "reason"}), e
            assert len(e["reason"]) > 60 and REASON_KINDS.search(e["reason"]), (section, e["key"])
            assert not re.search(r"not (found|reached)", e["reason"].lower()), (section, e["key"])
            if section == "per_planner":
                assert e["planners"] and set(e["planners"]) <= set(F.PLANNERS), e
            if e["key"].startswith("marker "):
                assert e["key"][7:] in report_names(), e["key"]
            else:
                assert F.CSRC.joinpath("aecm_flow_plan.h").read_text().count(e["key"].split("|")[2][:40]) >= 1, e["key"]


def report_names():
    text = F.CSRC.joinpath("aecm_flow_plan.h").read_text()
    return set(re.findall(r"X\((\w+)\)", text))


def test_the_decisions_the_corpus_is_there_for_diverge(report):
    for n in MUST_DIVERGE:
        v = report["markers"][n]
        assert v["false"] > 0 and v["true"] > 0 and v["divergent"], (n, v)
    assert len(report["branches"]) >= 55 and len(report["markers"]) == len(report_names())
    # the two data-dependent loops: one and two blocks per frame; calls left by the start-up `continue`: none, some and all of a launch's
    loops = {tuple(x) for x in report["call_loop"]}
    for k in (1, 2, 3, 6):
        assert (k, 0) in loops and (k, k) in loops, (k, sorted(loops))
    assert any(0 < c < k for k, c in loops if k > 2), sorted(loops)


def test_every_decision_line_carries_a_marker(report):
    """A conditional added to a Flow* function without its AECM_FLOW_MARK would be invisible to the divergence record."""
    assert F.unmarked_lines(report["lines"]) == []
    text = F.CSRC.joinpath("aecm_flow_plan.h").read_text()
    assert "#define AECM_FLOW_MARK(id, outcome) ((void)0)" in text and "#define AECM_FLOW_MARK_IF(guard, id, outcome) ((void)0)" in text


def test_the_harness_reproduces_session_flow(report):
    """Every object of the corpus: the plans executed as the tick kernels execute them move the tags SessionFlow<T> moves (block
    inputs, outputs, return codes), the live lists are the ascending ids, every state is one FlowStateDefect admits."""
    from flow_corpus import S, schedules
    runs = report["run"]["runs"]
    assert sorted(r["family"] for r in runs) == sorted(s["family"] for s in schedules())
    for r in runs:
        assert r["first_difference"] == -1, r
        assert r["sessions"] == S == 300
    launched = {k for r in runs for k in r["kernels"]}
    assert {"dense", "sparse", "mixed", "calls", "packets"} <= launched, launched
