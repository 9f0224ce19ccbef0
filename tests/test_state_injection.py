"""The import gate's promise, on the CPU: every state image the gate admits (webrtc_aecm_amd/csrc/aecm_state_check.h) runs on the
block DSP with every claim of aecm_ops.h holding and equals the oracle, output sample for sample and state word for word; every
state it refuses is refused for the reason the hand-written restatement (tests/state_corpus.py: STATE_RULES) gives.

The GPU counterpart (tests/test_gpu_state_injection.py) imports only states that have passed what this module checks."""
import subprocess

import numpy as np
import pytest

import inject_sim
import simlib
import state_corpus as sc
from block_corpus import configure, corpus_cases
from oracle import pyoracle

N_MUTATIONS = 20000                # admitted single-field mutations that are run (more are generated: the refused ones are judged only)
CHUNK = 2500


def oracle_run(state, far, near, clean):
    """(out, image) of the oracle started from the state: the launches do not matter to it, it runs block by block."""
    o = pyoracle.OracleStream(state.fs).import_image(*state.image)
    out = o.process_blocks(far, near, clean if state.clean else None)
    return out, o.export_image()


def run_and_compare(states, first_index=0):
    """The states (all admitted) through sc.LAUNCHES on the simulator with the claims checked, and through the oracle.  Returns the
    failures as text, one per state: a violated claim, an output sample or a state word that differs."""
    vec, scal, hist = sc.stack(states)
    audio = [sc.continuation_audio(first_index + i) for i in range(len(states))]
    far, near, clean = (np.ascontiguousarray(np.stack([a[k] for a in audio])) for k in range(3))
    kinds, values, out = inject_sim.run_many(vec, scal, hist, far, near, clean, [s.clean for s in states], sc.LAUNCHES)
    failures = []
    for i, s in enumerate(states):
        if kinds[i]:
            failures.append(f"{s.name}: {inject_sim.KINDS[int(kinds[i])]} claim violated ({int(values[i])})")
            continue
        exp_out, exp_img = oracle_run(s, far[i], near[i], clean[i])
        if not np.array_equal(out[i], exp_out):
            at = int(np.flatnonzero(out[i] != exp_out)[0])
            failures.append(f"{s.name}: output differs from the oracle's from block {at // 64} sample {at % 64}: {int(out[i][at])} != {int(exp_out[at])}")
            continue
        diff = sc.describe_image_diff((vec[i], scal[i], hist[i]), exp_img)
        if diff:
            failures.append(f"{s.name}: state after the launches differs from the oracle's: {diff}")
    return failures


def _report(failures, n):
    assert not failures, f"{len(failures)} of {n} admitted states fail:\n" + "\n".join(failures[:40])


# ---- the oracle's image door, pinned on reachable states -------------------------------------------------------------------------
def test_oracle_image_door_on_every_block_corpus_case():
    """For every case of the block corpus, at blocks 0, 1, 192 and at its end: the simulator's image imported into a fresh oracle
    has the simulator's digest, exports the simulator's image on every live word (the first comparison of WHOLE images the project
    has: S_DFACLEANQ, S_DFACLEANQ_OLD, dBufClean and the configuration words are not in the digest), and continues like the
    simulator for 64 blocks (the case's own audio, from its beginning again behind its end), with the clean input where the case
    has one.  On the way every state the simulator passes through -- after every single block -- is admitted by the gate."""
    for c in corpus_cases():
        s = configure(simlib.SimStream(c["fs"], c["cng"], c["echo_mode"]), c)
        n = c["n_blocks"]
        cuts = sorted({0, 1, min(192, n), n})
        for b in range(n + 1):
            img = s.image()
            defect = inject_sim.validate(img[0], img[1], c["fs"])
            assert defect is None, f"{c['name']} block {b}: the gate refuses a state the algorithm reached ({defect})"
            assert sc.restated_defect(img[0], img[1], c["fs"]) is None, (c["name"], b)
            if b in cuts:
                o = pyoracle.OracleStream(c["fs"]).import_image(*img)
                assert np.array_equal(o.digest(), s.digest()), (c["name"], b)
                diff = sc.describe_image_diff(o.export_image(), img)
                assert not diff, f"{c['name']} block {b}: export_image(import_image(x)) != x: {diff}"
                idx = (np.arange(b * 64, (b + 64) * 64) % (n * 64))
                far, near = c["far"][idx], c["near"][idx]
                clean = None if c["clean"] is None else c["clean"][idx]
                twin = simlib.SimStream(c["fs"])
                twin.set_image(*img)
                assert np.array_equal(twin.process(far, near, clean), o.process_blocks(far, near, clean)), (c["name"], b)
                diff = sc.describe_image_diff(o.export_image(), twin.image())
                assert not diff, f"{c['name']} 64 blocks after block {b}: {diff}"
            if b < n:
                sl = slice(b * 64, (b + 1) * 64)
                s.process(c["far"][sl], c["near"][sl], None if c["clean"] is None else c["clean"][sl])


def test_the_gate_admits_every_state_the_flow_corpus_passes_through():
    """The session-flow corpus as audio, one simulated session (the product's Session class over the simulated engine) per corpus
    session: the core state after every launch a session makes -- every cut of its stream -- passes the gate."""
    import flow_corpus as fc

    def make(fs):
        s = simlib.SimSession()
        assert s.init(fs) == 0
        return s
    simlib.engine_gate_counts(reset=True)
    launches = 0
    for sch in fc.schedules():
        far, near = fc.signals(sch)
        fc.drive_reference(sch, far, near, make)
        checked, refused = simlib.engine_gate_counts()
        assert refused == 0, (sch["family"], refused, checked)
        assert checked > launches + 100 * sch["flags"].shape[1], (sch["family"], checked)
        launches = checked


def test_export_writes_zero_into_dead_words():
    vm, sm = sc.live_masks()
    for b in sc.base_states()[::7]:
        dirty = b.copy()
        dirty.vec |= ~vm                                   # set every dead bit: the gate says nothing about them
        dirty.scal[sc.N_SCAL_USED:] = -1
        assert dirty.expected_defect() is None and inject_sim.validate(dirty.vec, dirty.scal, dirty.fs) is None
        vec, scal, hist = pyoracle.OracleStream(b.fs).import_image(*dirty.image).export_image()
        assert not np.any(vec & ~vm) and not np.any(scal.view(np.uint32) & ~sm)
        assert not sc.describe_image_diff((vec, scal, hist), b.image, live_only=False)


# ---- restatement = product -------------------------------------------------------------------------------------------------------
def test_corpus_has_what_it_promises():
    names = [s.name for s in sc.corpus()]
    assert len(set(names)) == len(names)
    assert all(b.expected_defect() is None for b in sc.base_states())
    admitted = [s for s in sc.corpus() if s.expected_defect() is None]
    for field, value in sc.INDEX_PROBES:                           # the index-like fields at both ends, among the states that are run
        assert any(int(s.scal[sc.S[field]]) == value for s in admitted), (field, value)
    probes = {fs: list(sc.rule_probes(fs)) for fs in (8000, 16000)}
    for r in sc.STATE_RULES:                                       # every rule is probed on both sides of both of its bounds it has
        mine = [(v, ok) for rr, _, v, ok in probes[16000] if rr is r]
        assert any(ok for _, ok in mine) and any(not ok for _, ok in mine), r.name
    for r in sc.LANE_RULES:
        assert {lane for rr, lane, _, _ in probes[16000] if rr is r} == {t for t in sc.RULE_LANES if r.applies(t)}
    assert sum(ok for _, ok in sc.sg_probes()) == 5
    assert {s.fs for s in sc.base_states()} == {8000, 16000} and any(s.clean for s in sc.base_states())


def test_restated_rules_equal_the_product_on_every_blob():
    """STATE_RULES and the product's gate give the same verdict, by name, on every state of the corpus and on seeded single-field
    mutations, admitted or refused; and a probe of a rule is refused for THAT rule."""
    wrong = []
    for s in list(sc.corpus()) + sc.single_field_mutations(777, 6000):
        got, exp = inject_sim.validate(s.vec, s.scal, s.fs), s.expected_defect()
        if got != exp:
            wrong.append(f"{s.name}: product {got!r}, restatement {exp!r}")
    assert not wrong, "\n".join(wrong[:40])
    k = 0
    for fs in (16000, 8000):
        for r, lane, value, ok in sc.rule_probes(fs):
            st = sc.rule_mutations()[k]
            k += 1
            if not ok:
                assert inject_sim.validate(st.vec, st.scal, st.fs) == r.defect, st.name
    for st, (tup, ok) in zip(sc.rule_mutations()[k:], sc.sg_probes()):
        assert inject_sim.validate(st.vec, st.scal, st.fs) == (None if ok else sc.SG_DEFECT), st.name


# ---- every admitted state runs exactly -------------------------------------------------------------------------------------------
def test_every_admitted_corpus_state_runs_with_every_claim_holding_and_equals_the_oracle():
    """Base states, every rule at its bounds, every unchecked word at its type's extremes, combinations: launches of 1, 2 and 3
    blocks.  No state is left out."""
    admitted = [s for s in sc.corpus() if s.expected_defect() is None]
    assert len(admitted) >= 800
    assert sum(s.clean for s in admitted) * 5 >= len(admitted)
    _report(run_and_compare(admitted), len(admitted))


def test_admitted_single_field_mutations_run_with_every_claim_holding_and_equal_the_oracle():
    """At least N_MUTATIONS seeded single-field mutations that the gate admits, a third of them with a clean input."""
    failures, done, seed = [], 0, 1000
    with_clean = 0
    while done < N_MUTATIONS:
        batch = [s for s in sc.single_field_mutations(seed, CHUNK) if s.expected_defect() is None]
        assert len(batch) > CHUNK // 2
        for s in batch:
            assert inject_sim.validate(s.vec, s.scal, s.fs) is None, s.name
        failures += run_and_compare(batch, first_index=100000 + done)
        with_clean += sum(s.clean for s in batch)
        done += len(batch)
        seed += 1
    assert with_clean * 4 >= done
    _report(failures, done)


# ---- the same under sanitizers, as a program of its own ---------------------------------------------------------------------------
def test_admitted_corpus_under_asan_and_ubsan_in_a_program_of_its_own(tmp_path):
    """tests/sim/inject_main.cpp (its own main, never loaded into an interpreter) built with -fsanitize=address,undefined runs the
    admitted corpus: a far-history row or a lane word addressed outside its array at the bounds of S_HISTPOS, S_LAST_DELAY or
    S_FIXED_DELAY, or a shift by a count outside the type, ends it.  Its results equal the unsanitized library's."""
    probe = subprocess.run(["g++", "-fsanitize=address,undefined", "-x", "c++", "-", "-o", str(tmp_path / "probe")], input="int main() { return 0; }",
                           capture_output=True, text=True)
    if probe.returncode != 0:
        pytest.skip("g++ cannot link the sanitizer runtimes here")
    exe = inject_sim.build_sanitized_program()
    admitted = [s for s in sc.corpus() if s.expected_defect() is None]
    vec, scal, hist = sc.stack(admitted)
    audio = [sc.continuation_audio(i) for i in range(len(admitted))]
    far, near, clean = (np.ascontiguousarray(np.stack([a[k] for a in audio])) for k in range(3))
    has_clean = np.array([s.clean for s in admitted], dtype=np.uint8)
    lens = np.array(sc.LAUNCHES, dtype=np.int32)
    with open(tmp_path / "corpus.bin", "wb") as f:
        f.write(np.array([len(admitted), int(lens.sum()), lens.size], dtype=np.int32).tobytes() + lens.tobytes())
        for a in (vec, scal, hist, far, near, clean, has_clean):
            f.write(a.tobytes())
    r = subprocess.run([str(exe), str(tmp_path / "corpus.bin"), str(tmp_path / "result.bin")], capture_output=True, text=True, timeout=1200,
                       env={"ASAN_OPTIONS": "detect_leaks=0:abort_on_error=0", "UBSAN_OPTIONS": "halt_on_error=1:print_stacktrace=1"})     # (the leak checker needs ptrace rights a sandbox may not give)
    log = r.stdout + r.stderr
    assert r.returncode == 0 and "runtime error" not in log and "AddressSanitizer" not in log, log[-4000:]
    kinds, values, out = inject_sim.run_many(vec, scal, hist, far, near, clean, has_clean, lens)
    assert not kinds.any()
    raw = (tmp_path / "result.bin").read_bytes()
    expected = np.zeros(len(admitted), np.int32).tobytes() + out.tobytes() + vec.tobytes() + scal.tobytes() + hist.tobytes()
    assert raw == expected
