"""Pipelined launches for ragged batches with a clean near-end input on the device (WebRtcAecmBatch_SetRaggedCleanPipelining):
every carried shape at sizes from two streams to more than a thousand, bit-exact (outputs and 24-word state digests) against the
CPU checker run over each stream's own first len[s] blocks with its clean input, nothing read or written behind a stream's end,
the clean input's carried-over block of streams that end before their workgroup does, and no result depending on the switch."""
import functools
import hashlib

import numpy as np
import pytest

import test_gpu_hostile_clean as H
import test_gpu_pipelined_clean as P
import test_gpu_ragged as R
import webrtc_aecm_amd as aecm
from helpers import GOLDEN, describe_digest_diff, process_clean, synth_streams
from oracle import pyoracle
from test_gpu_ragged_pipelined import _lengths
from webrtc_aecm_amd.synth import synth_pair

pytestmark = pytest.mark.gpu
SENTINEL = R.SENTINEL
CLEAN_BIT = P.CLEAN_BIT
SHAPES = P.SHAPES          # the shapes that are both ragged and clean shapes: wishes, shape bits (without 0x2000), waves


def _batch(S, fs, shape=None, any_size=True, **kw):
    """A batch with test_gpu_ragged's per-stream configurations and the new switch on (and, with a shape, a policy that pipelines
    a launch of any size in it)."""
    b = aecm.AecmBatch(S, fs, **kw)
    cfgs = R._configure(b, S)
    if shape is not None:
        b.set_launch_policy(pipelined_min_streams=1, pipelined_min_blocks=1, **SHAPES[shape][0])
    elif any_size:
        b.set_launch_policy(pipelined_min_streams=1, pipelined_min_blocks=1)
    b.set_ragged_clean_pipelining(True)
    return b, cfgs


def _every_shape_case(shape, S, fs):
    wishes, bits, waves = SHAPES[shape]
    T = 60 if S > 100 else 90
    rs = np.random.RandomState(S * 100 + bits + fs // 1000 + 7)
    lens = _lengths(rs, S, T)
    far, near = synth_streams(list(range(5400, 5400 + S)), T, fs)
    clean = P._clean_of(far, near)
    b, cfgs = _batch(S, fs, shape)
    b.set_ragged_clean_pipelining(False)
    assert b.describe_ragged_launch(lens, True)["form"] == 0              # the default: off
    b.set_ragged_clean_pipelining(True)
    d = b.describe_ragged_launch(lens, True)
    live = int((lens > 0).sum())
    assert (d["form"], d["shape"], d["waves_per_workgroup"]) == (3, bits | CLEAN_BIT, waves), d
    assert -(-live // 4) <= d["workgroups"] <= live, d
    out = R._run_device(b, far, near, lens, T, clean)
    R._check(b, out, lens, R._expected(pyoracle.OracleStream, fs, cfgs, far, near, lens, clean), fs, cfgs)
    fresh = {cfg: pyoracle.OracleStream(fs, *cfg).digest() for cfg in set(cfgs)}
    for s in np.nonzero(lens == 0)[0]:
        assert np.array_equal(b.digest(int(s)), fresh[cfgs[s]]), f"zero-length stream {s} was touched"
    b.close()


@pytest.mark.parametrize("fs", [16000, 8000])
@pytest.mark.parametrize("S", [2, 3, 5, 37, 300])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_every_shape_random_lengths(shape, S, fs):
    _every_shape_case(shape, S, fs)


@pytest.mark.parametrize("shape", ["sixteen waves (42240)", "six waves (20)"])
def test_more_than_a_thousand_streams(shape):
    _every_shape_case(shape, 1030, 16000)


@pytest.mark.parametrize("shape", ["sixteen waves (42240)", "six waves (20)"])
def test_one_live_stream_next_to_an_empty_one(shape):
    """The smallest ragged launch: one workgroup, one live slot."""
    bits = SHAPES[shape][1]
    fs, T = 16000, 40
    lens = np.array([0, 17], dtype=np.int32)
    far, near = synth_streams([1, 2], T, fs)
    clean = P._clean_of(far, near)
    b, cfgs = _batch(2, fs, shape)
    d = b.describe_ragged_launch(lens, True)
    assert (d["form"], d["shape"], d["workgroups"]) == (3, bits | CLEAN_BIT, 1), d
    out = R._run_device(b, far, near, lens, T, clean)
    R._check(b, out, lens, R._expected(pyoracle.OracleStream, fs, cfgs, far, near, lens, clean), fs, cfgs)
    b.close()


def test_two_ragged_clean_launches_equal_one_launch_of_the_summed_lengths():
    """A stream whose first length is 0, one whose second is 0 and one of length 1 among them: the second launch's first block
    starts with the clean samples the first ended on -- c_old of a stream that ended before its workgroup did."""
    S, T, fs = 300, 120, 16000
    rs = np.random.RandomState(5)
    total = rs.randint(2, T + 1, size=S).astype(np.int32)
    a = (total * rs.rand(S)).astype(np.int32)
    a[:3] = (0, total[1], 1)
    far, near = synth_streams(list(range(6100, 6100 + S)), T, fs)
    clean = P._clean_of(far, near)
    one, cfgs = _batch(S, fs)
    assert one.describe_ragged_launch(total, True)["form"] == 3
    ref = one.process_ragged_host(far, near, total, clean)
    exp = R._expected(pyoracle.OracleStream, fs, cfgs, far, near, total, clean, streams=range(0, S, 10))
    two, _ = _batch(S, fs)
    assert two.describe_ragged_launch(a, True)["form"] == 3 and two.describe_ragged_launch(total - a, True)["form"] == 3
    first = two.process_ragged_host(far, near, a, clean)
    far2, near2, clean2 = np.zeros_like(far), np.zeros_like(near), np.zeros_like(clean)
    for s in range(S):
        n = (total[s] - a[s]) * 64
        for dst, src in ((far2, far), (near2, near), (clean2, clean)):
            dst[s, :n] = src[s, a[s] * 64:total[s] * 64]
    second = two.process_ragged_host(far2, near2, total - a, clean2)
    for s in range(S):
        got = np.concatenate([first[s, :a[s] * 64], second[s, :(total[s] - a[s]) * 64]])
        assert np.array_equal(got, ref[s, :total[s] * 64]), s
        assert np.array_equal(two.digest(s), one.digest(s)), (s, describe_digest_diff(two.digest(s), one.digest(s)))
        if s in exp:
            assert np.array_equal(got, exp[s][0]) and np.array_equal(one.digest(s), exp[s][1]), s
    one.close()
    two.close()


@pytest.mark.parametrize("shape", [None, *SHAPES])
def test_launches_of_every_kind_in_a_row_on_one_batch(shape):
    """Ragged clean pipelined, ragged without a clean input (pipelined; c_old must come through untouched), ragged clean with the
    new switch off (one wavefront per stream), ragged clean pipelined again -- each continues every stream where its own last
    launch ended; after each, outputs and digests equal the oracle run over the same sequence."""
    S, fs, L = 300, 16000, 40
    rs = np.random.RandomState(12)
    far, near = synth_streams(list(range(6500, 6500 + S)), 4 * L, fs)
    clean = P._clean_of(far, near)
    b, cfgs = _batch(S, fs, shape)
    b.set_ragged_pipelining(True)
    oracles = [pyoracle.OracleStream(fs, *cfg) for cfg in cfgs]
    at = np.zeros(S, dtype=np.int64)
    for launch, (with_clean, switch, form) in enumerate(((True, True, 3), (False, True, 3), (True, False, 0), (True, True, 3))):
        lens = _lengths(rs, S, L)
        rs.shuffle(lens)
        b.set_ragged_clean_pipelining(switch)
        d = b.describe_ragged_launch(lens, with_clean)
        assert d["form"] == form and bool(d["shape"] & CLEAN_BIT) == (with_clean and switch), (launch, d)
        f, n, c = (np.stack([x[s, at[s] * 64:(at[s] + L) * 64] for s in range(S)]) for x in (far, near, clean))
        out = R._run_device(b, f, n, lens, L, c if with_clean else None)
        for s, o in enumerate(oracles):
            k = int(lens[s])
            exp = process_clean(o, f[s], n[s], c[s], 0, k) if with_clean else (o.process(f[s][:k * 64], n[s][:k * 64]) if k else np.zeros(0, np.int16))
            assert np.array_equal(out[s][:k * 64], exp), f"launch {launch}: output of stream {s} (length {k}) differs"
            assert (out[s][k * 64:] == SENTINEL).all(), f"launch {launch}: stream {s} was written behind its length {k}"
            assert np.array_equal(b.digest(s), o.digest()), f"launch {launch}: state of stream {s}: {describe_digest_diff(b.digest(s), o.digest())}"
        at += lens
    b.close()


@pytest.mark.parametrize("shape", [None, "six waves (20)"], ids=["default shape", "six waves"])
def test_output_in_place_of_the_clean_input(shape):
    """out_dev = near_clean_dev: results as the oracle's, and the rows at and beyond len[s] x 64 still hold the clean input's
    samples -- no clean row is read after an output row of the launch has been written, none behind a length is written."""
    import torch
    S, T, fs = 300, 60, 16000
    rs = np.random.RandomState(41)
    lens = _lengths(rs, S, T)
    far, near = synth_streams(list(range(8800, 8800 + S)), T, fs)
    clean = P._clean_of(far, near)
    b, cfgs = _batch(S, fs, shape)
    assert b.describe_ragged_launch(lens, True)["form"] == 3
    dev = torch.device("cuda", 0)
    tf, tn, tc = (torch.from_numpy(x).to(dev) for x in (far, near, clean))
    torch.cuda.synchronize()
    b.process_ragged_device(tf.data_ptr(), tn.data_ptr(), tc.data_ptr(), far.shape[1], 64, T, lens, tc.data_ptr())
    b.synchronize()
    out = tc.cpu().numpy()
    exp = R._expected(pyoracle.OracleStream, fs, cfgs, far, near, lens, clean)
    for s in range(S):
        n = int(lens[s]) * 64
        assert np.array_equal(out[s][:n], exp[s][0]), f"output of stream {s} (length {lens[s]}) differs"
        assert np.array_equal(out[s][n:], clean[s][n:]), f"stream {s}: rows behind its length {lens[s]} no longer hold the clean input"
        assert np.array_equal(b.digest(s), exp[s][1]), f"state of stream {s}: {describe_digest_diff(b.digest(s), exp[s][1])}"
    b.close()


@pytest.mark.parametrize("fs", H.RATES)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_hostile_clean_inputs_with_ragged_lengths(shape, fs):
    """helpers.adversarial_clean_cases (20 streams per rate, each with its case's configuration and echo path; 40 in all) with
    test_gpu_hostile_clean's ragged lengths -- 0, 1 and 192 among them -- through the four shapes."""
    _, (far, near, clean) = H._cases(fs)
    lens = H._ragged_lengths(fs)
    bits = SHAPES[shape][1]
    b = H._batch(fs)
    b.set_launch_policy(pipelined_min_streams=1, pipelined_min_blocks=1, **SHAPES[shape][0])
    b.set_ragged_clean_pipelining(True)
    d = b.describe_ragged_launch(lens, True)
    assert (d["form"], d["shape"]) == (3, bits | CLEAN_BIT), d
    out = R._run_device(b, H._cut(far, 0, H.T_MID), H._cut(near, 0, H.T_MID), lens, H.T_MID, H._cut(clean, 0, H.T_MID))
    H._check_ragged(fs, b, out, lens)
    b.close()


@functools.lru_cache(maxsize=None)
def _form_independence_inputs(S):
    T, fs, K = 512, 16000, 32
    rs = np.random.RandomState(S + 1)
    lens = rs.randint(T // 4, T + 1, size=S).astype(np.int32)
    lens[5], lens[6] = T, T // 4
    pairs = [synth_pair(1900 + k, T, fs) for k in range(K)]
    idx = np.arange(S) % K
    far = np.stack([p[0] for p in pairs])[idx]
    near = np.stack([p[1] for p in pairs])[idx]
    clean = P._clean_of(far, near)
    sample = sorted({5, 6, int(np.argmax(lens)), int(np.argmin(lens)), 0, S - 1, *rs.randint(0, S, size=18).tolist()})[:24]
    return T, fs, lens, far, near, clean, sample


def _form_independence(S, with_reference):
    T, fs, lens, far, near, clean, sample = _form_independence_inputs(S)
    digests, outs = [], []
    for on in (True, False):
        b = aecm.AecmBatch(S, fs)
        cfgs = R._configure(b, S)
        b.set_ragged_clean_pipelining(on)
        d = b.describe_ragged_launch(lens, True)
        assert (d["form"] == 3 and d["shape"] & CLEAN_BIT) if on else (d["form"] == 0 and d["shape"] == 0), (on, d)
        out = R._run_device(b, far, near, lens, T, clean)
        if on:
            cls = pyoracle.RefCoreStream if with_reference else pyoracle.OracleStream
            R._check(b, out, lens, R._expected(cls, fs, cfgs, far, near, lens, clean, streams=sample), fs, cfgs, sample)
        digests.append(np.stack([b.digest(s) for s in range(S)]))
        outs.append(out)
        b.close()
    bad = np.nonzero((digests[0] != digests[1]).any(axis=1))[0]
    assert bad.size == 0, f"state depends on the launch form in streams {bad[:8].tolist()}"
    assert np.array_equal(outs[0], outs[1])
    assert (outs[0][lens[:, None] * 64 <= np.arange(T * 64)[None, :]] == SENTINEL).all()


@pytest.mark.parametrize("S", [1024, 4096])
def test_switch_on_against_switch_off_under_the_shipped_policy(S):
    """Lengths uniform in [T/4, T], T = 512, the shipped policy: switch on (form 3) against switch off (one wavefront per
    stream) -- all outputs and all state digests equal; a sample of 24 streams against the oracle."""
    _form_independence(S, False)


@R._needs_ref
def test_switch_on_sample_against_the_reference():
    _form_independence(1024, True)


def test_policy_fuzz_never_changes_results():
    """Random pipe_rot / pipe_prio / pipe_spread / pipe_wgs_per_cu: scheduling only."""
    S, T, fs = 200, 50, 16000
    rs = np.random.RandomState(22)
    lens = _lengths(rs, S, T)
    far, near = synth_streams(list(range(7100, 7100 + S)), T, fs)
    clean = P._clean_of(far, near)
    want = None
    for trial in range(10):
        b = aecm.AecmBatch(S, fs)
        cfgs = R._configure(b, S)
        fields = {}
        if trial:
            wishes = list(SHAPES.values())[rs.randint(len(SHAPES))][0]
            fields = dict(wishes, pipe_rot=int(rs.randint(0, 1024)), pipe_prio=int(rs.randint(0, 256)), pipe_spread=int(rs.randint(0, 2)),
                          pipe_wgs_per_cu=int(rs.randint(0, 3)))
        b.set_launch_policy(**fields)
        b.set_ragged_clean_pipelining(True)
        d = b.describe_ragged_launch(lens, True)
        assert d["form"] == 3 and d["shape"] & CLEAN_BIT, (trial, fields, d)
        out = R._run_device(b, far, near, lens, T, clean)
        dig = np.stack([b.digest(s) for s in range(S)])
        if want is None:
            R._check(b, out, lens, R._expected(pyoracle.OracleStream, fs, cfgs, far, near, lens, clean), fs, cfgs)
            want = (out, dig)
        else:
            assert np.array_equal(out, want[0]) and np.array_equal(dig, want[1]), (trial, fields)
        b.close()


def test_the_safe_variant_is_never_pipelined():
    """A batch on the safe variant with the switch on: described as one wavefront per stream -- by the engine's own rule -- and
    its results equal the oracle's; the same batch on the fast variant is pipelined: the variant is what decided."""
    S, T, fs = 300, 60, 16000
    rs = np.random.RandomState(32)
    lens = _lengths(rs, S, T)
    far, near = synth_streams(list(range(8200, 8200 + S)), T, fs)
    clean = P._clean_of(far, near)
    b, cfgs = _batch(S, fs, variant=aecm.KERNEL_SAFE)
    d = b.describe_ragged_launch(lens, True)
    assert d["form"] == 0 and d["shape"] == 0, d
    out = R._run_device(b, far, near, lens, T, clean)
    R._check(b, out, lens, R._expected(pyoracle.OracleStream, fs, cfgs, far, near, lens, clean), fs, cfgs)
    b.close()
    b, _ = _batch(S, fs)
    assert b.describe_ragged_launch(lens, True)["form"] == 3
    b.set_ragged_clean_pipelining(False)
    assert b.describe_ragged_launch(lens, True)["form"] == 0
    b.close()


def test_sparse_batch_of_8192_streams_with_100_live():
    S, T, fs, L = 8192, 100, 16000, 100
    rs = np.random.RandomState(10)
    live = np.sort(rs.choice(S, size=L, replace=False))
    lens = np.zeros(S, dtype=np.int32)
    lens[live] = rs.randint(1, T + 1, size=L)
    lens[live[0]] = T
    pairs = [synth_pair(300 + k, T, fs) for k in range(16)]
    idx = np.arange(S) % 16
    far, near = np.stack([p[0] for p in pairs])[idx], np.stack([p[1] for p in pairs])[idx]
    clean = P._clean_of(far, near)
    b = aecm.AecmBatch(S, fs)
    cfgs = R._configure(b, S)
    b.set_ragged_clean_pipelining(True)
    d = b.describe_ragged_launch(lens, True)
    assert d["form"] == 3 and d["shape"] & CLEAN_BIT and d["workgroups"] <= L, d
    idle = lens == 0
    states_before = np.asarray(b.export_states(0, S))[idle]
    out = R._run_device(b, far, near, lens, T, clean)
    R._check(b, out, lens, R._expected(pyoracle.OracleStream, fs, cfgs, far, near, lens, clean, streams=live.tolist()), fs, cfgs, live.tolist())
    assert np.array_equal(states_before, np.asarray(b.export_states(0, S))[idle]), "the state of a stream without blocks is not bit-identical"
    assert (out[idle] == SENTINEL).all()
    b.close()


def test_recordings_with_the_switch_on_equal_the_switch_off():
    fs, frame, n, S = 16000, 160, 60, 40
    rs = np.random.RandomState(3)
    calls = rs.randint(0, n + 1, size=S).astype(np.int32)
    calls[:3] = (0, n, 1)
    far, near = synth_streams(list(range(360, 360 + S)), n * frame // 64 + 1, fs)
    far, near = np.ascontiguousarray(far[:, :n * frame]), np.ascontiguousarray(near[:, :n * frame])
    clean = P._clean_of(far, near)
    res = []
    for on in (False, True):
        b = aecm.AecmBatch(S, fs, 1, 3)
        b.set_ragged_clean_pipelining(on)
        rc, out, codes = b.process_recordings_ragged_host(far, near, frame, calls, 40, clean)
        res.append((rc, out, codes, np.stack([b.digest(s) for s in range(S)])))
        b.close()
    assert res[0][0] == res[1][0] and np.array_equal(res[0][2], res[1][2])
    assert np.array_equal(res[0][1], res[1][1]) and np.array_equal(res[0][3], res[1][3])
    for s, k in enumerate(calls.tolist()):
        assert not res[1][1][s][k * frame:].any(), s


@pytest.mark.parametrize("shape", [None, *SHAPES])
def test_committed_ragged_clean_golden_is_reproduced(shape):
    """tests/golden/ragged_clean_16k.npz (tools/gen_golden.py: seeds, lengths, configurations, per-stream output hashes and
    digests from the unmodified reference with a clean input) -- runs where the reference does not exist."""
    g = np.load(GOLDEN / "ragged_clean_16k.npz")
    fs, T, lens, seeds = int(g["fs"]), int(g["n_blocks"]), g["lens"].astype(np.int32), g["seeds"].tolist()
    S = lens.size
    far, near = synth_streams(seeds, T, fs)
    clean = P._clean_of(far, near)
    b = aecm.AecmBatch(S, fs)
    for s in range(S):
        b.set_config(int(g["cng"][s]), int(g["echo_mode"][s]), s, 1)
    if shape is not None:
        b.set_launch_policy(**SHAPES[shape][0])
    b.set_ragged_clean_pipelining(True)
    d = b.describe_ragged_launch(lens, True)
    assert d["form"] == 3 and d["shape"] & CLEAN_BIT and (shape is None or d["shape"] == SHAPES[shape][1] | CLEAN_BIT), d
    out = R._run_device(b, far, near, lens, T, clean)
    for s in range(S):
        n = int(lens[s]) * 64
        assert hashlib.sha256(out[s][:n].tobytes()).hexdigest() == str(g["sha256"][s]), s
        assert (out[s][n:] == SENTINEL).all(), s
        assert np.array_equal(b.digest(s), g["digests"][s]), s
    b.close()
