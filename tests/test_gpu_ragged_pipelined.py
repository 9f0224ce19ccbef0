"""Pipelined launches for ragged batches on the device (WebRtcAecmBatch_SetRaggedPipelining): every carried shape at sizes from
one stream to more than a thousand, bit-exact (outputs and 24-word state digests) against the CPU checker run over each stream's
own first len[s] blocks, nothing written behind a stream's end, and no result depending on the form."""
import hashlib
import subprocess

import numpy as np
import pytest

import test_gpu_ragged as R
import webrtc_aecm_amd as aecm
from helpers import GOLDEN, synth_streams
from oracle import pyoracle
from webrtc_aecm_amd.synth import synth_pair

pytestmark = pytest.mark.gpu
SENTINEL = R.SENTINEL
# the unbalanced shapes the ragged form carries: the policy's wishes that force each, and the shape bits describe_ragged_launch reports
SHAPES = {
    "sixteen waves (42240)": (dict(pipe_tail_waves=2, pipe_front_waves=4, pipe_raw=0, pipe_delay_waves=2, pipe_gain_waves=4), 0x1a02, 16),
    "twelve waves (4220)": (dict(pipe_tail_waves=2, pipe_front_waves=2, pipe_raw=0, pipe_delay_waves=4, pipe_gain_waves=0), 0x802, 12),
    "ten waves (241)": (dict(pipe_tail_waves=2, pipe_front_waves=4, pipe_raw=1, pipe_delay_waves=0, pipe_gain_waves=0), 0x602, 10),
    "eight waves, raw (221)": (dict(pipe_tail_waves=2, pipe_front_waves=2, pipe_raw=1, pipe_delay_waves=0, pipe_gain_waves=0), 0x402, 8),
    "eight waves (220)": (dict(pipe_tail_waves=2, pipe_front_waves=2, pipe_raw=0, pipe_delay_waves=0, pipe_gain_waves=0), 0x002, 8),
    "six waves (20)": (dict(pipe_tail_waves=0, pipe_front_waves=2, pipe_raw=0, pipe_delay_waves=0, pipe_gain_waves=0), 0x000, 6),
}


def _lengths(rs, S, T):
    """Random in [0, T] with 0, 1 and T among them (S = 2: T and 1; S = 1: one length, which is the equal-length launch)."""
    lens = rs.randint(0, T + 1, size=S).astype(np.int32)
    special = {1: (T - 1,), 2: (T, 1)}.get(S, (0, T, 1))
    lens[:len(special)] = special
    return lens


@pytest.mark.parametrize("fs", [16000, 8000])
@pytest.mark.parametrize("S", [1, 2, 3, 5, 37, 300, 1030])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_every_shape_random_lengths(shape, S, fs):
    wishes, bits, waves = SHAPES[shape]
    T = 60 if S > 100 else 90
    rs = np.random.RandomState(S * 100 + bits + fs // 1000)
    lens = _lengths(rs, S, T)
    far, near = synth_streams(list(range(5000, 5000 + S)), T, fs)
    b = aecm.AecmBatch(S, fs)
    cfgs = R._configure(b, S)
    b.set_launch_policy(pipelined_min_streams=1, pipelined_min_blocks=1, **wishes)
    b.set_ragged_pipelining(True)
    d = b.describe_ragged_launch(lens)
    live = int((lens > 0).sum())
    # (one stream has one length: every length equal is the equal-length launch -- pipelined in the forced shape as well)
    assert (d["form"], d["shape"], d["waves_per_workgroup"]) == (3, bits, waves), d
    assert -(-live // 4) <= d["workgroups"] <= live
    out = R._run_device(b, far, near, lens, T)
    R._check(b, out, lens, R._expected(pyoracle.OracleStream, fs, cfgs, far, near, lens), fs, cfgs)
    fresh = {cfg: pyoracle.OracleStream(fs, *cfg).digest() for cfg in set(cfgs)}
    for s in np.nonzero(lens == 0)[0]:
        assert np.array_equal(b.digest(int(s)), fresh[cfgs[s]]), f"zero-length stream {s} was touched"
    b.close()


@pytest.mark.parametrize("shape", ["sixteen waves (42240)", "six waves (20)"])
def test_single_stream_batch_with_a_zero_length_neighbour(shape):
    """S = 1 cannot be ragged on its own (one length is all-equal): the smallest ragged launches -- one live stream next to an
    empty one, in a batch of one stream's worth of work."""
    wishes, bits, _ = SHAPES[shape]
    fs, T = 16000, 40
    lens = np.array([0, 17], dtype=np.int32)
    far, near = synth_streams([1, 2], T, fs)
    b = aecm.AecmBatch(2, fs)
    cfgs = R._configure(b, 2)
    b.set_launch_policy(pipelined_min_streams=1, pipelined_min_blocks=1, **wishes)
    b.set_ragged_pipelining(True)
    d = b.describe_ragged_launch(lens)
    assert (d["form"], d["shape"], d["workgroups"]) == (3, bits, 1), d
    out = R._run_device(b, far, near, lens, T)
    R._check(b, out, lens, R._expected(pyoracle.OracleStream, fs, cfgs, far, near, lens), fs, cfgs)
    b.close()


def _form_independence(S, with_reference):
    T, fs, K = 512, 16000, 32
    rs = np.random.RandomState(S)
    lens = rs.randint(T // 4, T + 1, size=S).astype(np.int32)
    lens[5], lens[6] = T, T // 4
    pairs = [synth_pair(900 + k, T, fs) for k in range(K)]
    idx = np.arange(S) % K
    far = np.stack([p[0] for p in pairs])[idx]
    near = np.stack([p[1] for p in pairs])[idx]
    sample = sorted({5, 6, int(np.argmax(lens)), int(np.argmin(lens)), 0, S - 1, *rs.randint(0, S, size=18).tolist()})[:24]
    digests, outs = [], []
    for on in (True, False):
        b = aecm.AecmBatch(S, fs)
        cfgs = R._configure(b, S)
        b.set_ragged_pipelining(on)
        d = b.describe_ragged_launch(lens)
        assert d["form"] == (3 if on else 0), d
        out = R._run_device(b, far, near, lens, T)
        if on:
            cls = pyoracle.RefCoreStream if with_reference else pyoracle.OracleStream
            R._check(b, out, lens, R._expected(cls, fs, cfgs, far, near, lens, streams=sample), fs, cfgs, sample)
        digests.append(np.stack([b.digest(s) for s in range(S)]))
        outs.append(out)
        b.close()
    bad = np.nonzero((digests[0] != digests[1]).any(axis=1))[0]
    assert bad.size == 0, f"state depends on the launch form in streams {bad[:8].tolist()}"
    assert np.array_equal(outs[0], outs[1])
    assert (outs[0][lens[:, None] * 64 <= np.arange(T * 64)[None, :]] == SENTINEL).all()


@pytest.mark.parametrize("S", [1024, 4096])
def test_form_independence_under_the_shipped_policy(S):
    """Lengths uniform in [T/4, T], T = 512, the shipped policy: switch on (form 3) against switch off (one wavefront per
    stream) -- all outputs and all state digests equal; a sample of 24 streams against the oracle."""
    _form_independence(S, False)


@R._needs_ref
def test_form_independence_sample_against_the_reference():
    _form_independence(1024, True)


def test_the_safe_variant_is_never_pipelined():
    """A batch on the safe variant with the switch on: described as one wavefront per stream -- by the engine's own rule -- and
    its results equal the switch-off run and the oracle."""
    S, T, fs = 300, 60, 16000
    rs = np.random.RandomState(31)
    lens = _lengths(rs, S, T)
    far, near = synth_streams(list(range(8000, 8000 + S)), T, fs)
    res = []
    for on in (True, False):
        b = aecm.AecmBatch(S, fs, variant=aecm.KERNEL_SAFE)
        cfgs = R._configure(b, S)
        b.set_ragged_pipelining(on)
        d = b.describe_ragged_launch(lens)
        assert d["form"] == 0 and d["shape"] == 0, d
        out = R._run_device(b, far, near, lens, T)
        if on:
            R._check(b, out, lens, R._expected(pyoracle.OracleStream, fs, cfgs, far, near, lens), fs, cfgs)
        res.append((out, np.stack([b.digest(s) for s in range(S)])))
        b.close()
    assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1])
    # the same batch on the fast variant is pipelined: the variant is what decided
    b = aecm.AecmBatch(S, fs)
    b.set_ragged_pipelining(True)
    assert b.describe_ragged_launch(lens)["form"] == 3
    b.set_ragged_pipelining(False)
    assert b.describe_ragged_launch(lens)["form"] == 0
    b.close()


def test_two_ragged_pipelined_launches_equal_one_launch_of_the_summed_lengths():
    S, T, fs = 300, 120, 16000
    rs = np.random.RandomState(4)
    total = rs.randint(2, T + 1, size=S).astype(np.int32)
    a = (total * rs.rand(S)).astype(np.int32)
    a[:3] = (0, total[1], 1)
    total[2] = max(total[2], 2)
    far, near = synth_streams(list(range(6000, 6000 + S)), T, fs)
    one = aecm.AecmBatch(S, fs)
    R._configure(one, S)
    one.set_ragged_pipelining(True)
    assert one.describe_ragged_launch(total)["form"] == 3
    ref = one.process_ragged_host(far, near, total)
    two = aecm.AecmBatch(S, fs)
    R._configure(two, S)
    two.set_ragged_pipelining(True)
    assert two.describe_ragged_launch(a)["form"] == 3 and two.describe_ragged_launch(total - a)["form"] == 3
    first = two.process_ragged_host(far, near, a)
    far2, near2 = np.zeros_like(far), np.zeros_like(near)
    for s in range(S):
        n = (total[s] - a[s]) * 64
        far2[s, :n], near2[s, :n] = far[s, a[s] * 64:total[s] * 64], near[s, a[s] * 64:total[s] * 64]
    second = two.process_ragged_host(far2, near2, total - a)
    for s in range(S):
        got = np.concatenate([first[s, :a[s] * 64], second[s, :(total[s] - a[s]) * 64]])
        assert np.array_equal(got, ref[s, :total[s] * 64]), s
        assert np.array_equal(two.digest(s), one.digest(s)), s
    one.close()
    two.close()


def test_sparse_batch_of_8192_streams_with_100_live():
    S, T, fs, L = 8192, 100, 16000, 100
    rs = np.random.RandomState(9)
    live = np.sort(rs.choice(S, size=L, replace=False))
    lens = np.zeros(S, dtype=np.int32)
    lens[live] = rs.randint(1, T + 1, size=L)
    lens[live[0]] = T
    pairs = [synth_pair(300 + k, T, fs) for k in range(16)]
    idx = np.arange(S) % 16
    far, near = np.stack([p[0] for p in pairs])[idx], np.stack([p[1] for p in pairs])[idx]
    b = aecm.AecmBatch(S, fs)
    cfgs = R._configure(b, S)
    b.set_ragged_pipelining(True)
    d = b.describe_ragged_launch(lens)
    assert d["form"] == 3 and d["workgroups"] <= L, d
    idle = lens == 0
    states_before = np.asarray(b.export_states(0, S))[idle]
    out = R._run_device(b, far, near, lens, T)
    R._check(b, out, lens, R._expected(pyoracle.OracleStream, fs, cfgs, far, near, lens, streams=live.tolist()), fs, cfgs, live.tolist())
    assert np.array_equal(states_before, np.asarray(b.export_states(0, S))[idle]), "the state of a stream without blocks is not bit-identical"
    assert (out[idle] == SENTINEL).all()
    b.close()


def test_policy_fuzz_never_changes_results():
    """Random pipe_rot / pipe_prio / pipe_spread / pipe_wgs_per_cu: scheduling only."""
    S, T, fs = 200, 50, 16000
    rs = np.random.RandomState(21)
    lens = _lengths(rs, S, T)
    far, near = synth_streams(list(range(7000, 7000 + S)), T, fs)
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
        b.set_ragged_pipelining(True)
        assert b.describe_ragged_launch(lens)["form"] == 3, (trial, fields)
        out = R._run_device(b, far, near, lens, T)
        dig = np.stack([b.digest(s) for s in range(S)])
        if want is None:
            R._check(b, out, lens, R._expected(pyoracle.OracleStream, fs, cfgs, far, near, lens), fs, cfgs)
            want = (out, dig)
        else:
            assert np.array_equal(out, want[0]) and np.array_equal(dig, want[1]), (trial, fields)
        b.close()


def test_recordings_with_the_switch_on_equal_the_switch_off():
    fs, frame, n, S = 16000, 160, 60, 40
    rs = np.random.RandomState(2)
    calls = rs.randint(0, n + 1, size=S).astype(np.int32)
    calls[:3] = (0, n, 1)
    far, near = synth_streams(list(range(300, 300 + S)), n * frame // 64 + 1, fs)
    far, near = np.ascontiguousarray(far[:, :n * frame]), np.ascontiguousarray(near[:, :n * frame])
    res = []
    for on in (False, True):
        b = aecm.AecmBatch(S, fs, 1, 3)
        b.set_ragged_pipelining(on)
        rc, out, codes = b.process_recordings_ragged_host(far, near, frame, calls, 40)
        res.append((rc, out, codes, np.stack([b.digest(s) for s in range(S)])))
        b.close()
    assert res[0][0] == res[1][0] and np.array_equal(res[0][2], res[1][2])
    assert np.array_equal(res[0][1], res[1][1]) and np.array_equal(res[0][3], res[1][3])
    for s, k in enumerate(calls.tolist()):
        assert not res[1][1][s][k * frame:].any(), s


def test_cli_batch_with_ragged_pipelining_writes_the_same_bytes(tmp_path):
    import wave
    from webrtc_aecm_amd import build
    build.build()

    def write(path, x):
        with wave.open(str(path), "wb") as w:
            w.setnchannels(1)
            w.setsampwidth(2)
            w.setframerate(16000)
            w.writeframes(np.asarray(x, dtype="<i2").tobytes())
    sizes = (48000 + 57, 16000, 32000 + 3, 8000)
    for k, n in enumerate(sizes):
        far, near = synth_pair(40 + k, n // 64 + 1, 16000, "mixed")
        write(tmp_path / f"f{k}.wav", far[:n])
        write(tmp_path / f"n{k}.wav", near[:n])
    (tmp_path / "pairs.txt").write_text("".join(f"{tmp_path}/f{k}.wav {tmp_path}/n{k}.wav\n" for k in range(len(sizes))))
    written = []
    for flags in ([], ["--ragged-pipelining"], ["--devices", "0", "--ragged-pipelining"]):
        r = subprocess.run([str(build.CLI), "--batch", str(tmp_path / "pairs.txt"), *flags], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and "time interval" in r.stdout, r.stdout + r.stderr
        written.append([(tmp_path / f"n{k}_out.wav").read_bytes() for k in range(len(sizes))])
        for k in range(len(sizes)):
            (tmp_path / f"n{k}_out.wav").unlink()
    assert written[0] == written[1] == written[2]


@pytest.mark.parametrize("shape", [None, *SHAPES])
def test_committed_ragged_golden_is_reproduced_in_the_pipelined_form(shape):
    """tests/golden/ragged_16k.npz (per-stream output hashes and digests from the unmodified reference) -- runs where the
    reference does not exist."""
    g = np.load(GOLDEN / "ragged_16k.npz")
    fs, T, lens, seeds = int(g["fs"]), int(g["n_blocks"]), g["lens"].astype(np.int32), g["seeds"].tolist()
    S = lens.size
    far, near = synth_streams(seeds, T, fs)
    b = aecm.AecmBatch(S, fs)
    for s in range(S):
        b.set_config(int(g["cng"][s]), int(g["echo_mode"][s]), s, 1)
    if shape is not None:
        b.set_launch_policy(**SHAPES[shape][0])
    b.set_ragged_pipelining(True)
    d = b.describe_ragged_launch(lens)
    assert d["form"] == 3 and (shape is None or d["shape"] == SHAPES[shape][1]), d
    out = R._run_device(b, far, near, lens, T)
    for s in range(S):
        n = int(lens[s]) * 64
        assert hashlib.sha256(out[s][:n].tobytes()).hexdigest() == str(g["sha256"][s]), s
        assert (out[s][n:] == SENTINEL).all(), s
        assert np.array_equal(b.digest(s), g["digests"][s]), s
    b.close()
