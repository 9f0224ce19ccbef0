"""The block corpus (tests/block_corpus.py) stays decision-complete: tools/decision_coverage.py builds the oracle and the lane
simulator's block DSP (lean forms off and on, with and without a clean input) with -O0 --coverage, runs the corpus through them in
a child process and reads gcov's branch counts.  The conditionals of the block path that went one way only must be exactly the
entries of tests/decision_allowlist.json -- each with the families it is one-way in and the reason why no input reaches it -- and
the coverage libraries must reproduce the oracle's outputs and digests on every case, so the run is a parity run too.
(profiles/r21_decision_coverage.txt has the same measurement for what the GPU block tests fed before the corpus.)"""
import importlib.util
import json
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
ALLOWLIST = ROOT / "tests" / "decision_allowlist.json"
_spec = importlib.util.spec_from_file_location("decision_coverage", ROOT / "tools" / "decision_coverage.py")
D = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(D)

pytestmark = pytest.mark.skipif(bool(D.tools_missing()), reason=f"not installed: {D.tools_missing()}")

# The oracle's entries may only be the decisions the corpus was written against and could not reach (aecm_oracle_fft128's clamp of
# the stage maximum, calc_step_size's min >= max, the two clamps of hnl that are dead by range) and the guards inside its
# division helpers (a zero divisor): (function, text of the line).
ORACLE_MAY_STAY = {
    ("aecm_oracle_fft128", "if (m > 32767) m = 32767;"),
    ("calc_step_size", "if (o->far_energy_min >= o->far_energy_max) {"),
    ("aecm_oracle_process_block", "if (hnl[i] < 0) hnl[i] = 0;"),
    ("aecm_oracle_process_block", "if (hnl[i] > NLP_COMP_HIGH) hnl[i] = ONE_Q14;"),
    ("div_w32_w16", "return den != 0 ? num / den : (int32_t)0x7FFFFFFF;"),
    ("div_u32_u16", "return den != 0 ? num / den : 0xFFFFFFFFu;"),
}
# reached by the corpus and by nothing the GPU block tests fed before it, or by one kernel family only (the issue's list): these
# must be two-way in every library that has them
MUST_BE_TWO_WAY = ("if (o->noise_est[i] < (1 << min_track)) {", "if (o->noise_high_ctr[i] >= 5) {",
                   "((best < o->minimum_probability) || (best < o->last_delay_probability));")


@pytest.fixture(scope="module")
def report():
    return D.measure("corpus")


def test_one_way_decisions_are_exactly_the_allowlist(report):
    allow = {e["key"]: sorted(e["families"]) for e in json.loads(ALLOWLIST.read_text())}
    got = {k: sorted(v) for k, v in D.one_way_entries(report).items()}
    new = {k: v for k, v in got.items() if allow.get(k) != v}
    gone = {k: v for k, v in allow.items() if got.get(k) != v}
    assert not new, "decisions the corpus takes one way only and the allowlist does not have (a case was lost?):\n" + "\n".join(
        f"  {k}  in {v}: counts {[report['families'][f][k] for f in v]}" for k, v in new.items())
    assert not gone, "allowlist entries that are two-way now (or are spelled differently): take them off the list:\n" + "\n".join(f"  {k}  {v}" for k, v in gone.items())


def test_the_allowlist_is_argued():
    entries = json.loads(ALLOWLIST.read_text())
    assert len({e["key"] for e in entries}) == len(entries)
    for e in entries:
        assert set(e) == {"key", "families", "reason"} and e["families"] and set(e["families"]) <= {"oracle", *D.FAMILIES}, e
        assert len(e["reason"]) > 60 and "not reached yet" not in e["reason"].lower(), e["key"]
        name, fn, text = D.split_key(e["key"])[:3]
        if "oracle" in e["families"]:
            assert e["families"] == ["oracle"] and name == "aecm_oracle.c" and (fn, text) in ORACLE_MAY_STAY, e["key"]
        else:
            assert name in D.KERNEL_FILES, e["key"]


def test_the_decisions_the_corpus_is_there_for_are_two_way(report):
    oracle = report["families"]["oracle"]
    for text in MUST_BE_TWO_WAY:
        keys = [k for k in oracle if D.split_key(k)[2].startswith(text)]
        assert keys, text
        for k in keys:
            assert min(oracle[k]) > 0, (k, oracle[k])
    # the kernel's side of the noise decrement and of the stored delay estimate, in every instantiation family
    for fam in D.FAMILIES:
        dec = report["families"][fam]
        assert len(dec) > 100, (fam, len(dec))
        for k, v in dec.items():
            if "BlockEngine::process_binary|if (best < u.last_prob) u.last_prob = best;" in k:
                assert min(v) > 0, (fam, k, v)


def test_coverage_libraries_reproduce_the_oracle(report):
    """Every corpus case through the simulator libraries built for coverage (plain and lean for a case without a clean input, clean
    for one with; one to three launches per case): outputs and 24-word digests equal the oracle's."""
    run = report["run"]
    from block_corpus import corpus_cases
    cases = corpus_cases()
    assert run["cases"] == [c["name"] for c in cases]
    assert run["sim_runs"] == sum(1 if c["clean"] is not None else 2 for c in cases)
    assert run["mismatches"] == [], run["mismatches"]
