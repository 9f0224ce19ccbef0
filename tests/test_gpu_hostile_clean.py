"""Hostile clean near-end inputs (helpers.adversarial_clean_cases: ten kinds of nearendClean that are no scaled copy of the near
end, over hostile and over converging far / near pairs) through every device kernel that takes a clean input: one wavefront
per stream in the fast and the safe variant, the chunk queue, the ragged chunk queue, the four pipelined clean shapes, and the
session tick kernel.  One stream per case, 20 streams per rate, each with its case's configuration and echo path; every test
asserts the launch form first, then all outputs and all 24-word state digests, bit-exact against the CPU checker."""
import functools
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import test_gpu_pipelined_clean as P
import test_gpu_ragged as R
import webrtc_aecm_amd as aecm
from helpers import adversarial_clean_cases, call_pattern, describe_digest_diff, drive_session, process_clean
from oracle import pyoracle

pytestmark = pytest.mark.gpu
T_FULL, T_MID = 1100, 192                      # past CONV_LEN2 = 1 024 (all three start-up states); the first digest
RATES = (16000, 8000)
CLEAN_BIT = P.CLEAN_BIT


def _stream(cls, c):
    o = cls(c["fs"], c["cng"], c["echo_mode"])
    if c["path"] is not None:
        o.init_echo_path(c["path"])
    return o


@functools.lru_cache(maxsize=None)
def _cases(fs):
    """The 20 cases of a rate and their signals as [20, T_FULL * 64] arrays (read-only: shared by every test)."""
    cases = [c for c in adversarial_clean_cases(T_FULL) if c["fs"] == fs]
    assert len(cases) == 20
    arrays = tuple(np.stack([c[k] for c in cases]) for k in ("far", "near", "clean"))
    for a in arrays:
        a.flags.writeable = False
    return cases, arrays


@functools.lru_cache(maxsize=None)
def _expected(fs, checker="OracleStream"):
    """(out[20, T_FULL * 64], digests after T_MID blocks, digests after T_FULL blocks) of the rate's cases on a CPU checker."""
    cases, _ = _cases(fs)
    cls = getattr(pyoracle, checker)

    def one(c):
        o = _stream(cls, c)
        a = process_clean(o, c["far"], c["near"], c["clean"], 0, T_MID)
        mid = o.digest()
        b = process_clean(o, c["far"], c["near"], c["clean"], T_MID, T_FULL)
        return np.concatenate([a, b]), mid, o.digest()
    with ThreadPoolExecutor() as ex:
        res = list(ex.map(one, cases))
    out = tuple(np.stack([r[k] for r in res]) for k in range(3))
    for a in out:
        a.flags.writeable = False
    return out


def _digests_at(fs, lens):
    """State digests of the rate's cases after lens[s] blocks with the clean input (0: the configured, untouched stream)."""
    cases, _ = _cases(fs)

    def one(k):
        o = _stream(pyoracle.OracleStream, cases[k])
        process_clean(o, cases[k]["far"], cases[k]["near"], cases[k]["clean"], 0, int(lens[k]))
        return o.digest()
    with ThreadPoolExecutor() as ex:
        return np.stack(list(ex.map(one, range(len(cases)))))


def _batch(fs, variant=aecm.KERNEL_FAST):
    cases, _ = _cases(fs)
    b = aecm.AecmBatch(len(cases), fs, variant=variant)
    for k, c in enumerate(cases):
        b.set_config(c["cng"], c["echo_mode"], k, 1)
        if c["path"] is not None:
            b.init_echo_path(k, c["path"])
    return b


def _cut(a, first, last):
    return np.ascontiguousarray(a[:, first * 64:last * 64])


def _check(fs, b, out, first, exp_out, exp_dig, what=""):
    """out: the device's output of blocks [first, first + out.shape[1] / 64) of every stream; exp_dig: the digests behind them."""
    cases, _ = _cases(fs)
    exp = exp_out[:, first * 64:first * 64 + out.shape[1]]
    for s, c in enumerate(cases):
        bad = np.nonzero((out[s] != exp[s]).reshape(-1, 64).any(axis=1))[0]
        assert bad.size == 0, f"{what}: output of stream {s} (kind {c['kind']}, base {c['base']}) differs first in block {first + int(bad[0])}"
    for s, c in enumerate(cases):
        d = b.digest(s)
        assert np.array_equal(d, exp_dig[s]), f"{what}: state of stream {s} (kind {c['kind']}, base {c['base']}): {describe_digest_diff(d, exp_dig[s])}"


def _one_wavefront(fs, variant, checker):
    _, (far, near, clean) = _cases(fs)
    exp_out, mid, end = _expected(fs, checker)
    b = _batch(fs, variant)
    for first, last, dig in ((0, T_MID, mid), (T_MID, T_FULL, end)):
        assert b.describe_launch(last - first, clean=True) == (0, 0)
        out = P._run(b, _cut(far, first, last), _cut(near, first, last), _cut(clean, first, last), last - first)
        _check(fs, b, out, first, exp_out, dig, f"blocks {first}..{last}")
    b.close()


@pytest.mark.parametrize("fs", RATES)
@pytest.mark.parametrize("variant", [aecm.KERNEL_FAST, aecm.KERNEL_SAFE], ids=["fast", "safe"])
def test_one_wavefront_per_stream(variant, fs):
    """aecm_process_kernel with kHasClean, 1 100 blocks as launches of 192 and 908."""
    _one_wavefront(fs, variant, "OracleStream")


@R._needs_ref
@pytest.mark.parametrize("fs", RATES)
def test_one_wavefront_per_stream_against_the_reference(fs):
    _one_wavefront(fs, aecm.KERNEL_FAST, "RefCoreStream")


@pytest.mark.parametrize("fs", RATES)
@pytest.mark.parametrize("chunk", [4, 32])
def test_chunk_queue(chunk, fs):
    """aecm_process_queue_kernel<true> forced onto 20 streams: a stream's state (c_old with it) is handed from wave to wave
    through memory every `chunk` blocks; two launches of 96 blocks continue each other."""
    _, (far, near, clean) = _cases(fs)
    exp_out, mid, _ = _expected(fs)
    half = T_MID // 2
    b = _batch(fs)
    b.set_launch_chunking(chunk, 0)
    assert b.describe_launch(half, True) == (2, chunk)
    out = np.concatenate([b.process_host(_cut(far, k, k + half), _cut(near, k, k + half), _cut(clean, k, k + half)) for k in (0, half)], axis=1)
    _check(fs, b, out, 0, exp_out, mid, f"chunk {chunk}")
    b.close()


def _ragged_lengths(fs):
    lens = np.random.RandomState(fs // 1000).randint(0, T_MID + 1, size=20).astype(np.int32)
    lens[[2, 9, 17]] = (0, T_MID, 1)
    return lens


def _check_ragged(fs, b, out, lens):
    cases, _ = _cases(fs)
    exp_out = _expected(fs)[0]
    digests = _digests_at(fs, lens)
    for s, c in enumerate(cases):
        n = int(lens[s]) * 64
        assert np.array_equal(out[s][:n], exp_out[s][:n]), f"output of stream {s} (kind {c['kind']}, base {c['base']}, length {lens[s]}) differs"
        assert (out[s][n:] == R.SENTINEL).all(), f"stream {s}: out blocks beyond its length {lens[s]} were written"
        d = b.digest(s)
        assert np.array_equal(d, digests[s]), f"state of stream {s} (kind {c['kind']}, base {c['base']}, length {lens[s]}): {describe_digest_diff(d, digests[s])}"


@pytest.mark.parametrize("fs", RATES)
def test_ragged_queue(fs):
    """aecm_process_ragged_queue_kernel<true>: chunks of 8 blocks, lengths random in [0, 192] with 0, 1 and 192 among them; out
    rows past each length keep the sentinel, and a stream of length 0 keeps its configured state."""
    _, (far, near, clean) = _cases(fs)
    lens = _ragged_lengths(fs)
    b = _batch(fs)
    b.set_launch_chunking(8, 0)
    d = b.describe_ragged_launch(lens, True)
    assert (d["form"], d["chunk_blocks"]) == (2, 8) and d["items"] == int(np.sum(-(-lens.astype(np.int64) // 8)))
    out = R._run_device(b, _cut(far, 0, T_MID), _cut(near, 0, T_MID), lens, T_MID, _cut(clean, 0, T_MID))
    _check_ragged(fs, b, out, lens)
    b.close()


@pytest.mark.parametrize("fs", RATES)
def test_ragged_launch_with_both_pipelining_switches_keeps_its_form(fs):
    """No pipelined kernel takes a ragged launch with a clean input: with both switches on (and a policy that would pipeline
    a batch of any size) it is described and run as with both off -- one wavefront per stream here -- while the same lengths
    without a clean input are pipelined."""
    _, (far, near, clean) = _cases(fs)
    lens = _ragged_lengths(fs)
    b = _batch(fs)
    before = b.describe_ragged_launch(lens, True)
    b.set_launch_policy(pipelined_min_streams=1, pipelined_min_blocks=1)
    b.set_ragged_pipelining(True)
    b.set_clean_pipelining(True)
    d = b.describe_ragged_launch(lens, True)
    assert d["form"] == 0 and d["shape"] == 0 and d == before, (d, before)
    assert b.describe_ragged_launch(lens, False)["form"] == 3
    out = R._run_device(b, _cut(far, 0, T_MID), _cut(near, 0, T_MID), lens, T_MID, _cut(clean, 0, T_MID))
    _check_ragged(fs, b, out, lens)
    b.close()


def _pipelined_batch(fs, shape):
    b = _batch(fs)
    if shape is not None:
        b.set_launch_policy(pipelined_min_streams=1, pipelined_min_blocks=1, **P.SHAPES[shape][0])
    b.set_clean_pipelining(True)
    return b


@pytest.mark.parametrize("fs", RATES)
@pytest.mark.parametrize("shape", list(P.SHAPES))
def test_pipelined_clean_shapes(shape, fs):
    """aecm_process_pipelined_clean_kernel in its four shapes.  Launches of 1, 2 and 3 blocks (shorter than the pipeline is deep:
    prologue and drain only) and the rest up to block 192; the sixteen- and the six-wave shape go on to block 1 100."""
    _, (far, near, clean) = _cases(fs)
    exp_out, mid, end = _expected(fs)
    bits, waves = P.SHAPES[shape][1:]
    b = _pipelined_batch(fs, shape)
    cuts = [0, 1, 3, 6, T_MID] + ([T_FULL] if waves in (16, 6) else [])
    for first, last in zip(cuts, cuts[1:]):
        assert b.describe_launch(last - first, clean=True) == (3, bits | CLEAN_BIT), (first, last)
        out = P._run(b, _cut(far, first, last), _cut(near, first, last), _cut(clean, first, last), last - first)
        exp = exp_out[:, first * 64:last * 64]
        bad = np.nonzero((out != exp).any(axis=1))[0]
        assert bad.size == 0, f"blocks {first}..{last}: outputs of streams {bad.tolist()} differ"
        if last in (T_MID, T_FULL):
            _check(fs, b, out, first, exp_out, mid if last == T_MID else end, f"blocks {first}..{last}")
    b.close()


_SEQUENCE = ((37, True), (11, False), (23, True), (40, True))       # (blocks, with the clean input) of the launches continuing each other


@functools.lru_cache(maxsize=None)
def _expected_sequence(fs):
    """[(out, digests)] per launch of _SEQUENCE: the second launch has no clean input, so this is no prefix of _expected."""
    cases, _ = _cases(fs)
    oracles = [_stream(pyoracle.OracleStream, c) for c in cases]
    res, at = [], 0
    for n, with_clean in _SEQUENCE:
        sl = slice(at * 64, (at + n) * 64)
        out = np.stack([process_clean(o, c["far"], c["near"], c["clean"], at, at + n) if with_clean else o.process(c["far"][sl], c["near"][sl])
                        for o, c in zip(oracles, cases)])
        res.append((out, np.stack([o.digest() for o in oracles])))
        at += n
    return res


@pytest.mark.parametrize("fs", RATES)
@pytest.mark.parametrize("shape", list(P.SHAPES))
def test_launches_of_every_kind_continue_each_other(shape, fs):
    """A clean pipelined launch, a pipelined launch without a clean input (c_old must come through untouched while d_old moves
    on), a clean launch with the switch off (one wavefront per stream), a clean pipelined launch again."""
    cases, (far, near, clean) = _cases(fs)
    bits = P.SHAPES[shape][1]
    b = _pipelined_batch(fs, shape)
    at = 0
    for (n, with_clean), switch, (exp_out, exp_dig) in zip(_SEQUENCE, (True, True, False, True), _expected_sequence(fs)):
        b.set_clean_pipelining(switch)
        want = (3, bits | (CLEAN_BIT if with_clean else 0)) if switch else (0, 0)
        assert b.describe_launch(n, clean=with_clean) == want, (at, b.describe_launch(n, clean=with_clean))
        out = P._run(b, _cut(far, at, at + n), _cut(near, at, at + n), _cut(clean, at, at + n) if with_clean else None, n)
        for s, c in enumerate(cases):
            assert np.array_equal(out[s], exp_out[s]), f"launch at block {at}: output of stream {s} (kind {c['kind']}, base {c['base']}) differs"
            d = b.digest(s)
            assert np.array_equal(d, exp_dig[s]), f"launch at block {at}: state of stream {s}: {describe_digest_diff(d, exp_dig[s])}"
        at += n
    b.close()


@pytest.mark.parametrize("fs", RATES)
@pytest.mark.parametrize("shape", [None, "six waves (20)"], ids=["default shape", "six waves"])
def test_output_in_place_of_the_clean_input(shape, fs):
    """out_dev = near_clean_dev: no clean row may be read after an output row of the launch has been written -- a hostile clean
    input differs from the output everywhere, so a late read cannot go unnoticed."""
    _, (far, near, clean) = _cases(fs)
    exp_out, mid, _ = _expected(fs)
    b = _pipelined_batch(fs, shape)
    form, detail = b.describe_launch(T_MID, clean=True)
    assert form == 3 and detail & CLEAN_BIT and (shape is None or detail == P.SHAPES[shape][1] | CLEAN_BIT), (form, detail)
    out = P._run(b, _cut(far, 0, T_MID), _cut(near, 0, T_MID), _cut(clean, 0, T_MID), T_MID, in_place=True)
    _check(fs, b, out, 0, exp_out, mid, "in place")
    b.close()


# ---- sessions: the clean input on every call, on the converging (base B) case of every kind --------------------------------
N_CALLS = 120


def _session_cases(fs, frame):
    cases = [c for c in _cases(fs)[0] if c["base"] == "B"]
    assert len(cases) == 10 and all(c["near"].size >= N_CALLS * frame for c in cases)
    return cases


@R._needs_ref
@pytest.mark.parametrize("fs,frame", [(16000, 160), (8000, 80)])
def test_single_session_abi_against_reference_sessions(fs, frame):
    """WebRtcAecm_* (aecm.Aecm) call by call against the reference's own session ABI: jittering and out-of-range
    msInSndCardBuf, far-end underruns, nearendClean on every call."""
    n = N_CALLS * frame
    for k, c in enumerate(_session_cases(fs, frame)):
        ms_seq, far_present = call_pattern(300 + k, N_CALLS)
        r = pyoracle.RefSession(fs, c["cng"], c["echo_mode"])
        s = aecm.Aecm()
        assert s.init(fs) == 0 and s.set_config(c["cng"], c["echo_mode"]) == 0
        exp, exp_codes = drive_session(r, c["far"][:n], c["near"][:n], frame, ms_seq, far_present, c["clean"][:n])
        got, codes = drive_session(s, c["far"][:n], c["near"][:n], frame, ms_seq, far_present, c["clean"][:n])
        s.close()
        assert np.array_equal(codes, exp_codes), (c["kind"], fs)
        assert np.array_equal(got, exp), (c["kind"], fs, int(np.nonzero(got != exp)[0][0]) // frame)


@R._needs_ref
@pytest.mark.parametrize("fs,frame", [(16000, 160), (8000, 80)])
def test_session_batch_against_reference_sessions(fs, frame):
    """WebRtcAecmSessions_* (aecm_tick_flow_kernel<true>): one session per kind, every session its own msInSndCardBuf and
    underruns, against one reference session each."""
    cases = _session_cases(fs, frame)
    S = len(cases)
    far, near, clean = (np.stack([c[k][:N_CALLS * frame] for c in cases]) for k in ("far", "near", "clean"))
    pats = [call_pattern(400 + k, N_CALLS) for k in range(S)]
    refs = [pyoracle.RefSession(fs, c["cng"], c["echo_mode"]) for c in cases]
    sb = aecm.AecmSessions(S, fs, 1, 3)
    for k, c in enumerate(cases):
        assert sb.set_config_session(k, c["cng"], c["echo_mode"]) == 0
    for i in range(N_CALLS):
        sl = slice(i * frame, (i + 1) * frame)
        ms = np.array([pats[k][0][i] for k in range(S)], dtype=np.int16)
        fl = np.array([0 if pats[k][1][i] else aecm.ffi.SESSION_NO_FAREND for k in range(S)], dtype=np.uint8)
        rc, out, codes = sb.tick_host_per_session(far[:, sl], near[:, sl], ms, clean[:, sl], flags=fl)
        for k in range(S):
            if not fl[k]:
                assert refs[k].buffer_farend(far[k, sl]) == 0
            rc1, o1 = refs[k].process(near[k, sl], clean[k, sl], int(ms[k]))
            assert codes[k] == rc1, (fs, frame, i, k)
            assert np.array_equal(out[k], o1), (fs, frame, i, cases[k]["kind"])
    sb.close()


@pytest.mark.parametrize("fs,frame", [(16000, 160), (8000, 80)])
def test_recordings_with_the_switch_on_equal_the_switch_off(fs, frame):
    _, (far, near, clean) = _cases(fs)
    n = N_CALLS * frame
    res = []
    for on in (False, True):
        b = _batch(fs)
        b.set_clean_pipelining(on)
        assert b.describe_launch(n // 64, clean=True)[0] == (3 if on else 0)
        rc, out = b.process_recordings_host(far[:, :n], near[:, :n], frame, 40, clean[:, :n])
        res.append((rc, out, np.stack([b.digest(s) for s in range(20)])))
        b.close()
    assert res[0][0] == res[1][0] == 0
    assert np.array_equal(res[0][1], res[1][1]) and np.array_equal(res[0][2], res[1][2])
    assert not np.array_equal(res[0][1], near[:, :n])                        # the recordings were processed, not passed through
