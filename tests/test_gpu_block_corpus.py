"""The decision-complete block corpus (tests/block_corpus.py) through every device kernel family: one wavefront per stream in
the fast and the safe variant, the chunk queue (the family with the lean forms), the ragged queue, ragged pipelined, the
pipelined shapes, the clean instantiations of each (for the cases that carry a clean input), the checked build, and the
session kernels (ordinary ticks, ticks of K calls, packet ticks of a mixed-rate object with half calls, sparse ticks).  One
stream per case with the case's configuration, echo path and control settings, for the whole length of the case, so that the
decisions the corpus is there for -- the comfort-noise decrement, the delay estimator's second validity operand, the start-up
states -- happen inside each of these kernels.  Every test asserts the launch form first, then every output sample and every
24-word state digest, bit-exact against the CPU checker."""
import functools
import os
import subprocess
import sys
import textwrap
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import test_gpu_pipelined_clean as P
import test_gpu_ragged as R
import webrtc_aecm_amd as aecm
from block_corpus import configure, corpus_cases
from helpers import GOLDEN, describe_digest_diff, process_clean
from oracle import pyoracle

pytestmark = pytest.mark.gpu
T_MID = 192
RATES = (16000, 8000)
SETS = [(fs, clean) for fs in RATES for clean in (False, True)]
SET_IDS = [f"{fs}{'-clean' if clean else ''}" for fs, clean in SETS]
CLEAN_BIT = P.CLEAN_BIT
LONG = 1200                                      # cases longer than this go through the sixteen- and the six-wave shape only


def _checker_stream(cls, c):
    return configure(cls(c["fs"], c["cng"], c["echo_mode"]), c)


def _process(o, c, first, last):
    if last == first:
        return np.zeros(0, np.int16)
    if c["clean"] is None:
        return o.process(c["far"][first * 64:last * 64], c["near"][first * 64:last * 64])
    return process_clean(o, c["far"], c["near"], c["clean"], first, last)


@functools.lru_cache(maxsize=None)
def _expected(checker="OracleStream"):
    """{case name: (out, digest after min(T_MID, n) blocks, digest at the end)} of the whole corpus on a CPU checker, once."""
    cls = getattr(pyoracle, checker)

    def one(c):
        o = _checker_stream(cls, c)
        mid_at = min(T_MID, c["n_blocks"])
        a = _process(o, c, 0, mid_at)
        mid = o.digest()
        b = _process(o, c, mid_at, c["n_blocks"])
        out = np.concatenate([a, b])
        out.flags.writeable = False
        return c["name"], (out, mid, o.digest())
    with ThreadPoolExecutor() as ex:
        return dict(ex.map(one, corpus_cases()))


@functools.lru_cache(maxsize=None)
def _groups(fs, clean):
    """[(n_blocks, cases, far[S, n], near, clean or None)] of a rate: the cases of one length are the streams of one batch."""
    res = []
    cases = corpus_cases(fs=fs, clean=clean)
    for n in sorted({c["n_blocks"] for c in cases}):
        sel = [c for c in cases if c["n_blocks"] == n]
        res.append((n, sel, *(np.stack([c[k] for c in sel]) if (k != "clean" or clean) else None for k in ("far", "near", "clean"))))
    assert res, (fs, clean)
    return res


def _batch(cases, fs, variant=aecm.KERNEL_FAST):
    b = aecm.AecmBatch(len(cases), fs, variant=variant)
    for k, c in enumerate(cases):
        b.set_config(c["cng"], c["echo_mode"], k, 1)
        if c["path"] is not None:
            b.init_echo_path(k, c["path"])
        if c["control"] is not None:
            b.control(*c["control"], k, 1)
    return b


def _cut(a, first, last):
    return None if a is None else np.ascontiguousarray(a[:, first * 64:last * 64])


def _check_out(cases, out, first, exp, what):
    for s, c in enumerate(cases):
        e = exp[c["name"]][0][first * 64:first * 64 + out.shape[1]]
        bad = np.nonzero((out[s] != e).reshape(-1, 64).any(axis=1))[0]
        assert bad.size == 0, f"{what}: output of case {c['name']} differs first in block {first + int(bad[0])}"


def _check_digests(cases, b, exp, which, what):
    for s, c in enumerate(cases):
        d, e = b.digest(s), exp[c["name"]][which]
        assert np.array_equal(d, e), f"{what}: state of case {c['name']}: {describe_digest_diff(d, e)}"


def _run_launches(b, cases, far, near, clean, n, want, exp, what, cuts=None):
    """Launches over [0, n) cut at `cuts` (default: T_MID), each described first; outputs of every launch, digests at T_MID and n."""
    cuts = [x for x in (cuts or [0, T_MID]) if x < n] + [n]
    for first, last in zip(cuts, cuts[1:]):
        assert b.describe_launch(last - first, clean=clean is not None) == want, (what, first, last, b.describe_launch(last - first, clean=clean is not None))
        out = b.process_host(_cut(far, first, last), _cut(near, first, last), _cut(clean, first, last))
        _check_out(cases, out, first, exp, f"{what}, blocks {first}..{last}")
        if last in (T_MID, n):
            _check_digests(cases, b, exp, 2 if last == n else 1, f"{what}, after block {last}")


def _one_wavefront(fs, clean, variant, checker):
    exp = _expected(checker)
    for n, cases, far, near, cl in _groups(fs, clean):
        b = _batch(cases, fs, variant)
        b.set_launch_pipelining(0)
        _run_launches(b, cases, far, near, cl, n, (0, 0), exp, f"one wavefront per stream, {n} blocks")
        b.close()


@pytest.mark.parametrize("fs,clean", SETS, ids=SET_IDS)
@pytest.mark.parametrize("variant", [aecm.KERNEL_FAST, aecm.KERNEL_SAFE], ids=["fast", "safe"])
def test_one_wavefront_per_stream(variant, fs, clean):
    """aecm_process_kernel, two launches that continue each other (192 blocks and the rest of the case)."""
    _one_wavefront(fs, clean, variant, "OracleStream")


@R._needs_ref
@pytest.mark.parametrize("fs,clean", SETS, ids=SET_IDS)
def test_one_wavefront_per_stream_against_the_reference(fs, clean):
    _one_wavefront(fs, clean, aecm.KERNEL_FAST, "RefCoreStream")


@pytest.mark.parametrize("fs,clean", SETS, ids=SET_IDS)
@pytest.mark.parametrize("chunk", [4, 32])
def test_chunk_queue(chunk, fs, clean):
    """aecm_process_queue_kernel forced by policy (without a clean input: the family that takes the lean forms): a stream's
    state is handed from wave to wave through memory every `chunk` blocks, for the whole case."""
    exp = _expected()
    for n, cases, far, near, cl in _groups(fs, clean):
        b = _batch(cases, fs)
        b.set_launch_chunking(chunk, 0)
        _run_launches(b, cases, far, near, cl, n, (2, chunk), exp, f"chunk queue {chunk}, {n} blocks")
        b.close()


@functools.lru_cache(maxsize=None)
def _ragged(fs, clean):
    """All cases of a set as one ragged batch: rows padded to the longest case; lengths 0, 1, random and full among them (every
    case longer than LONG at its full length).  Returns (cases, far, near, clean, lens, T, expected {s: (out, digest)})."""
    cases = corpus_cases(fs=fs, clean=clean)
    T = max(c["n_blocks"] for c in cases)
    rs = np.random.RandomState(fs // 1000 + clean)
    lens = np.array([c["n_blocks"] if c["n_blocks"] > LONG or k % 2 == 0 else rs.randint(0, c["n_blocks"] + 1) for k, c in enumerate(cases)], dtype=np.int32)
    short = [k for k, c in enumerate(cases) if c["n_blocks"] <= LONG]
    if len(short) >= 3:
        lens[short[-1]], lens[short[-2]] = 0, 1
    pad = lambda c, k: np.concatenate([c[k], np.full((T - c["n_blocks"]) * 64, 12345, np.int16)])
    far, near = (np.stack([pad(c, k) for c in cases]) for k in ("far", "near"))
    cl = np.stack([pad(c, "clean") for c in cases]) if clean else None
    full = _expected()

    def one(k):
        c = cases[k]
        if lens[k] == c["n_blocks"]:
            return full[c["name"]][0], full[c["name"]][2]
        o = _checker_stream(pyoracle.OracleStream, c)
        return _process(o, c, 0, int(lens[k])), o.digest()
    with ThreadPoolExecutor() as ex:
        exp = dict(enumerate(ex.map(one, range(len(cases)))))
    return cases, far, near, cl, lens, T, exp


@pytest.mark.parametrize("fs,clean", SETS, ids=SET_IDS)
def test_ragged_queue(fs, clean):
    """aecm_process_ragged_queue_kernel, chunks of 8 blocks: every case of the set in one batch at its own length; out rows past
    each length keep the sentinel, a stream of length 0 keeps its configured state."""
    cases, far, near, cl, lens, T, exp = _ragged(fs, clean)
    b = _batch(cases, fs)
    b.set_launch_chunking(8, 0)
    d = b.describe_ragged_launch(lens, clean)
    assert (d["form"], d["chunk_blocks"]) == (2, 8) and d["items"] == int(np.sum(-(-lens.astype(np.int64) // 8))), d
    out = R._run_device(b, far, near, lens, T, cl)
    R._check(b, out, lens, exp, fs, None)
    b.close()


@pytest.mark.parametrize("fs,clean", SETS, ids=SET_IDS)
@pytest.mark.parametrize("shape", ["sixteen waves (42240)", "six waves (20)"])
def test_ragged_pipelined(shape, fs, clean):
    """The ragged pipelined kernels, by opt-in (SetRaggedPipelining / SetRaggedCleanPipelining), in the deepest and the
    shallowest shape."""
    wishes, bits, waves = P.SHAPES[shape]
    cases, far, near, cl, lens, T, exp = _ragged(fs, clean)
    b = _batch(cases, fs)
    b.set_launch_policy(pipelined_min_streams=1, pipelined_min_blocks=1, **wishes)
    b.set_ragged_pipelining(True)
    if clean:
        b.set_ragged_clean_pipelining(True)
    d = b.describe_ragged_launch(lens, clean)
    assert (d["form"], d["shape"] & ~CLEAN_BIT, d["waves_per_workgroup"]) == (3, bits, waves) and bool(d["shape"] & CLEAN_BIT) == clean, d
    out = R._run_device(b, far, near, lens, T, cl)
    R._check(b, out, lens, exp, fs, None)
    b.close()


@pytest.mark.parametrize("fs,clean", SETS, ids=SET_IDS)
@pytest.mark.parametrize("shape", [None, *list(P.SHAPES)[1:]], ids=["sixteen waves by size", *list(P.SHAPES)[1:]])
def test_pipelined_shapes(shape, fs, clean):
    """The pipelined kernels: the sixteen-wave shape by size, the twelve-, eight- and six-wave shapes by wish.  Launches of 1, 2
    and 3 blocks (shorter than the pipeline is deep), then up to block 192, then the rest; the cases longer than 1 200 blocks go
    through the sixteen- and the six-wave shape only."""
    exp = _expected()
    bits, waves = (0x1a02, 16) if shape is None else P.SHAPES[shape][1:]
    for n, cases, far, near, cl in _groups(fs, clean):
        if n > LONG and waves not in (16, 6):
            continue
        b = _batch(cases, fs)
        b.set_launch_policy(pipelined_min_streams=1, pipelined_min_blocks=1, **({} if shape is None else P.SHAPES[shape][0]))
        if clean:
            b.set_clean_pipelining(True)
        _run_launches(b, cases, far, near, cl, n, (3, bits | (CLEAN_BIT if clean else 0)), exp, f"pipelined {waves} waves, {n} blocks", cuts=[0, 1, 3, 6, T_MID])
        b.close()


def test_checked_build_counts_nothing(tmp_path):
    """libaecm_mi355x_checked.so (-DAECM_CHECKED: every "provably fits" claim of aecm_ops.h counted on the device), in a child
    process: the whole corpus as one wavefront per stream, through the chunk queue and pipelined.  Both counters stay 0 and
    the outputs equal the oracle's."""
    from webrtc_aecm_amd import build
    assert build.LIB_CHECKED.exists()
    script = tmp_path / "audit_corpus.py"
    script.write_text(textwrap.dedent("""
        import numpy as np
        import webrtc_aecm_amd as aecm
        import test_gpu_block_corpus as T
        assert aecm.check_counters(0, reset=True) is not None
        exp = T._expected()
        for fs, clean in T.SETS:
            for n, cases, far, near, cl in T._groups(fs, clean):
                for form in (0, 2, 3):
                    b = T._batch(cases, fs)
                    if form == 0:
                        b.set_launch_pipelining(0)
                    elif form == 2:
                        b.set_launch_chunking(32, 0)
                    else:
                        b.set_launch_policy(pipelined_min_streams=1, pipelined_min_blocks=1)
                        b.set_clean_pipelining(True)
                    assert b.describe_launch(n, clean=clean)[0] == form, (fs, clean, n, form)
                    out = b.process_host(far, near, cl)
                    T._check_out(cases, out, 0, exp, f"checked build, form {form}")
                    T._check_digests(cases, b, exp, 2, f"checked build, form {form}")
                    b.close()
        c = aecm.check_counters(0)
        print("AUDIT", int(c[0]), int(c[1]))
    """))
    env = dict(os.environ, AECM_LIB_PATH=str(build.LIB_CHECKED),
               PYTHONPATH=os.pathsep.join([str(GOLDEN.parent.parent), str(GOLDEN.parent), os.environ.get("PYTHONPATH", "")]))
    r = subprocess.run([sys.executable, str(script)], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("AUDIT")]
    assert line and line[-1].split()[1:] == ["0", "0"], r.stdout[-500:]


# ---- sessions: one session per case, for the whole length of the case -------------------------------------------------------
import corpus_sessions as cs  # noqa: E402
import packets_helpers as ph  # noqa: E402
import sparse_helpers as sh  # noqa: E402


def _reference_sessions(cases):
    """One WebRtcAecm_* instance per case: the unmodified reference where oracle/_ref travelled, else the single-session ABI."""
    res = []
    for c in cases:
        if pyoracle.have_reference():
            s = pyoracle.RefSession(c["fs"], 1, 3)
        else:
            s = aecm.Aecm()
            assert s.init(c["fs"]) == 0
        res.append(cs.configure_session(s, c))
    return res


def _object(cases, object_fs, rates):
    mixed = len(set(rates.tolist())) > 1
    return cs.configure_object(aecm.AecmSessions(len(cases), object_fs, 1, 3, rates=rates if mixed else None), cases)


def _run_sessions(cases, object_fs, K, kind, form="host", idle_stretches=False, seed=0, fixture=None):
    ops, far, near, rates = cs.plan(cases, object_fs, K, kind, idle_stretches, seed)
    exp_out, exp_codes, refs = ph.run_reference(None, rates, ops, ph.Feed(far, near), sessions=_reference_sessions(cases))
    paths = np.stack([r.get_echo_path()[1] for r in refs])
    if fixture is not None:                               # the unmodified reference's run, recorded: holds where oracle/_ref did not travel
        g, mine = np.load(GOLDEN / f"{fixture}.npz"), cs.summary(cases, exp_out, exp_codes, paths)
        assert str(g["sha256"]) == mine["sha256"] and all(np.array_equal(g[k], mine[k]) for k in ("tail", "codes", "paths")), fixture
    sb = _object(cases, object_fs, rates)
    if idle_stretches:
        assert sb.force_sparse_ticks(True) == 0
    out, codes = ph.run_object(sb, ops, ph.Feed(far, near), form=form)
    assert np.array_equal(codes, exp_codes), (kind, K)
    bad = np.argwhere(out != exp_out)
    assert bad.size == 0, (kind, K, "first difference: case, sample", cases[int(bad[0][0])]["name"], int(bad[0][1]))
    twin = None
    if K > 1 or idle_stretches:                           # K ordinary ticks per K-call tick; dense ticks for the sparse form
        twin = _object(cases, object_fs, rates)
        tout, tcodes = ph.run_object(twin, ops, ph.Feed(far, near), as_single_ticks=True)
        assert np.array_equal(tcodes, exp_codes) and np.array_equal(tout, exp_out), (kind, K, "the twin itself")
    for s, c in enumerate(cases):
        rc, path = sb.get_echo_path(s)
        assert rc == 0 and np.array_equal(path, paths[s]), (kind, K, "echo path", c["name"])
        if twin is not None:
            a, b = sb.export_session(s), twin.export_session(s)
            assert a[0] == 0 and b[0] == 0 and sh.snapshot_state(a[1]) == sh.snapshot_state(b[1]), (kind, K, "state of session", c["name"])
    sb.close()
    if twin is not None:
        twin.close()
    return len(ops)


@pytest.mark.parametrize("fs", RATES)
def test_sessions_ordinary_ticks(fs):
    """aecm_tick_flow_kernel: every case of the rate, long ones included; the reference's run is also pinned by the fixture."""
    _run_sessions(cs.session_cases(fs), fs, 1, "tick", fixture=f"sesscorpus_fs{fs}")


@pytest.mark.parametrize("fs", RATES)
@pytest.mark.parametrize("K", [2, 3, 6])
def test_sessions_tick_calls(K, fs):
    """WebRtcAecmSessions_TickCalls (aecm_tick_calls_body.inc keeps the core state in registers across the K calls): start-up
    states 1 and 2 inside the kernel for every K; the cases longer than 1 200 blocks (the noise decrement, the delay estimator's
    second operand) with K = 3."""
    _run_sessions(cs.session_cases(fs, long_cases=K == 3), fs, K, "calls", seed=K)


@pytest.mark.parametrize("K", [2, 3])
def test_sessions_tick_packets_mixed_rates(K):
    """WebRtcAecmSessions_TickPackets on a 16 kHz object that holds the cases of both rates: the 8 kHz sessions make half calls.
    The long cases with K = 2."""
    _run_sessions(cs.session_cases(long_cases=K == 2), 16000, K, "packets", form="device", seed=20 + K)


@pytest.mark.parametrize("fs", RATES)
def test_sessions_sparse_ticks(fs):
    """The sparse form (live list + sparse tick kernel, forced), sessions idle for stretches of 1 .. 39 ticks; the twin ticks densely."""
    _run_sessions(cs.session_cases(fs, long_cases=fs == 16000), fs, 1, "tick", idle_stretches=True, seed=40)
