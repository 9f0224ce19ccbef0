"""Ragged batches on the device: WebRtcAecmBatch_ProcessBlocksRagged / ProcessRecordingsRagged through every launch form they
can take, bit-exact (outputs and 24-word state digests) against the CPU checker run over each stream's own first len[s] blocks."""
import hashlib
import subprocess
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import webrtc_aecm_amd as aecm
from helpers import GOLDEN, describe_digest_diff, stream_config, synth_streams
from oracle import pyoracle
from webrtc_aecm_amd.synth import synth_clean, synth_pair

pytestmark = pytest.mark.gpu
SENTINEL = 0x5A5A
_needs_ref = pytest.mark.skipif(not pyoracle.have_reference(), reason="prebuilt oracle/_ref/libaecm_ref.so not present")


def _checker_run(cls, fs, cfg, far, near, n_blocks, clean=None):
    """(out[:n_blocks * 64], digest) of one stream's first n_blocks blocks on a CPU checker."""
    o = cls(fs, cfg[0], cfg[1])
    if n_blocks == 0:
        return np.zeros(0, np.int16), o.digest()
    if clean is None:
        return o.process(far[:n_blocks * 64], near[:n_blocks * 64]), o.digest()
    out = np.concatenate([o.process_block_clean(far[b * 64:(b + 1) * 64], near[b * 64:(b + 1) * 64], clean[b * 64:(b + 1) * 64])
                          for b in range(n_blocks)])
    return out, o.digest()


def _expected(cls, fs, cfgs, far, near, lens, clean=None, streams=None):
    streams = list(range(len(lens))) if streams is None else list(streams)
    with ThreadPoolExecutor() as ex:
        res = list(ex.map(lambda s: _checker_run(cls, fs, cfgs[s], far[s], near[s], int(lens[s]), None if clean is None else clean[s]), streams))
    return dict(zip(streams, res))


def _run_device(b, far, near, lens, T, clean=None):
    """WebRtcAecmBatch_ProcessBlocksRagged on device tensors; the out tensor starts as SENTINEL everywhere."""
    import torch
    dev = torch.device("cuda", 0)
    tf, tn = torch.from_numpy(far).to(dev), torch.from_numpy(near).to(dev)
    tc = torch.from_numpy(clean).to(dev) if clean is not None else None
    out = torch.full_like(tn, SENTINEL)
    torch.cuda.synchronize()
    b.process_ragged_device(tf.data_ptr(), tn.data_ptr(), out.data_ptr(), far.shape[1], 64, T, lens, tc.data_ptr() if tc is not None else None)
    b.synchronize()
    return out.cpu().numpy()


def _check(b, out, lens, exp, fs, cfgs, streams=None):
    for s in (range(len(lens)) if streams is None else streams):
        n = int(lens[s]) * 64
        assert np.array_equal(out[s][:n], exp[s][0]), f"output of stream {s} (length {lens[s]}) differs"
        assert (out[s][n:] == SENTINEL).all(), f"stream {s}: out blocks beyond its length {lens[s]} were written"
        d = b.digest(s)
        assert np.array_equal(d, exp[s][1]), f"state digest of stream {s} (length {lens[s]}): {describe_digest_diff(d, exp[s][1])}"


def _configure(b, S):
    cfgs = [stream_config(s) for s in range(S)]
    for s, (cng, em) in enumerate(cfgs):
        b.set_config(cng, em, s, 1)
    return cfgs


def _forced_queue_case(cls, S, chunk, fs, with_clean, T=200):
    rs = np.random.RandomState(S * 1000 + chunk + fs // 1000 + with_clean)
    lens = rs.randint(0, T + 1, size=S).astype(np.int32)
    lens[:3] = (0, T, 1)
    far, near = synth_streams(list(range(4000, 4000 + S)), T, fs)
    clean = synth_clean(near) if with_clean else None
    b = aecm.AecmBatch(S, fs)
    cfgs = _configure(b, S)
    b.set_launch_chunking(chunk, 0)
    d = b.describe_ragged_launch(lens, with_clean)
    assert (d["form"], d["chunk_blocks"]) == (2, chunk) and d["items"] == int(np.sum(-(-lens.astype(np.int64) // chunk)))
    out = _run_device(b, far, near, lens, T, clean)
    _check(b, out, lens, _expected(cls, fs, cfgs, far, near, lens, clean), fs, cfgs)
    fresh = {cfg: cls(fs, *cfg).digest() for cfg in set(cfgs)}
    for s in np.nonzero(lens == 0)[0]:
        assert np.array_equal(b.digest(int(s)), fresh[cfgs[s]]), f"zero-length stream {s} was touched"
    b.close()


@pytest.mark.parametrize("with_clean", [False, True])
@pytest.mark.parametrize("fs", [16000, 8000])
@pytest.mark.parametrize("S", [37, 300])
@pytest.mark.parametrize("chunk", [8, 32])
def test_forced_queue_form_random_lengths(chunk, S, fs, with_clean):
    """The ragged chunk queue forced at small sizes, lengths random in [0, T] (zero, one and T among them)."""
    _forced_queue_case(pyoracle.OracleStream, S, chunk, fs, with_clean)


@_needs_ref
def test_forced_queue_form_against_the_reference():
    _forced_queue_case(pyoracle.RefCoreStream, 37, 8, 16000, False)


def test_default_policy_full_size_and_form_independence():
    """8 192 streams, lengths uniform in [T/4, T], T = 512, the shipped policy: the chunk queue.  A sample of 24 streams against
    the oracle; the state of ALL streams (digests, and outputs) against a second run of the same batch with one wavefront per
    stream -- results may not depend on the form."""
    S, T, fs, K = 8192, 512, 16000, 32
    rs = np.random.RandomState(77)
    lens = rs.randint(T // 4, T + 1, size=S).astype(np.int32)
    lens[5], lens[6] = T, T // 4
    pairs = [synth_pair(900 + k, T, fs) for k in range(K)]
    idx = np.arange(S) % K
    far = np.stack([p[0] for p in pairs])[idx]
    near = np.stack([p[1] for p in pairs])[idx]
    sample = sorted({5, 6, int(np.argmax(lens)), int(np.argmin(lens)), 0, S - 1, *rs.randint(0, S, size=18).tolist()})
    digests = []
    outs = []
    for chunking in (None, 0):
        b = aecm.AecmBatch(S, fs)
        cfgs = _configure(b, S)
        if chunking is not None:
            b.set_launch_chunking(chunking)
        d = b.describe_ragged_launch(lens)
        assert d["form"] == (2 if chunking is None else 1), d
        if chunking is None:
            assert d["chunk_blocks"] == 128 and d["sum_blocks"] == int(lens.sum()) and d["max_blocks"] == T
        out = _run_device(b, far, near, lens, T)
        if chunking is None:
            _check(b, out, lens, _expected(pyoracle.OracleStream, fs, cfgs, far, near, lens, streams=sample), fs, cfgs, sample)
        digests.append(np.stack([b.digest(s) for s in range(S)]))
        outs.append(out)
        b.close()
    bad = np.nonzero((digests[0] != digests[1]).any(axis=1))[0]
    assert bad.size == 0, f"state depends on the launch form in streams {bad[:8].tolist()}"
    assert np.array_equal(outs[0], outs[1])


def test_two_ragged_launches_equal_one_equal_length_launch():
    """Continuation: a ragged launch, then a second ragged launch with the remaining blocks of every stream."""
    S, T, fs = 300, 200, 16000
    rs = np.random.RandomState(3)
    a = rs.randint(0, T + 1, size=S).astype(np.int32)
    a[:2] = (0, T)
    far, near = synth_streams(list(range(6000, 6000 + S)), T, fs)
    one = aecm.AecmBatch(S, fs)
    _configure(one, S)
    ref = one.process_host(far, near)
    two = aecm.AecmBatch(S, fs)
    _configure(two, S)
    two.set_launch_chunking(8, 0)
    first = two.process_ragged_host(far, near, a)
    far2, near2 = np.zeros_like(far), np.zeros_like(near)
    for s in range(S):
        far2[s, :(T - a[s]) * 64], near2[s, :(T - a[s]) * 64] = far[s, a[s] * 64:], near[s, a[s] * 64:]
    second = two.process_ragged_host(far2, near2, T - a)
    for s in range(S):
        got = np.concatenate([first[s, :a[s] * 64], second[s, :(T - a[s]) * 64]])
        assert np.array_equal(got, ref[s]), s
        assert not first[s, a[s] * 64:].any() and not second[s, (T - a[s]) * 64:].any(), s
        assert np.array_equal(two.digest(s), one.digest(s)), s
    with pytest.raises(aecm.AecmError) as e:
        two.process_ragged_host(far, near, np.full(S, T + 1))
    assert e.value.code == aecm.ffi.AECM_BAD_PARAMETER_ERROR
    assert np.array_equal(two.digest(7), one.digest(7))                  # refused: nothing changed


@pytest.mark.parametrize("with_clean", [False, True])
@pytest.mark.parametrize("fs,frame", [(16000, 160), (8000, 80), (16000, 80), (8000, 160)])
def test_ragged_recordings_equal_single_sessions(fs, frame, with_clean):
    """Every row equals a single aecm.Aecm session fed that many calls, zeros behind it, codes equal; all-equal call counts
    equal process_recordings_host.  ms = 40, and once out of range (every call then returns the warning)."""
    n = 90
    calls = np.array([0, 1, 7, 33, n // 2, n], dtype=np.int32)
    S = calls.size
    far, near = synth_streams(list(range(300, 300 + S)), n * frame // 64 + 1, fs)
    far, near = np.ascontiguousarray(far[:, :n * frame]), np.ascontiguousarray(near[:, :n * frame])
    clean = synth_clean(near) if with_clean else None
    for ms in (40, 700) if frame == 160 and not with_clean else (40,):
        b = aecm.AecmBatch(S, fs, 1, 3)
        rc, out, codes = b.process_recordings_ragged_host(far, near, frame, calls, ms, clean)
        for s, k in enumerate(calls.tolist()):
            sess = aecm.Aecm()
            assert sess.init(fs) == 0 and sess.set_config(1, 3) == 0
            got_codes = []
            for i in range(k):
                sl = slice(i * frame, (i + 1) * frame)
                assert sess.buffer_farend(far[s][sl]) == 0
                code, exp = sess.process(near[s][sl], None if clean is None else clean[s][sl], ms)
                got_codes.append(code)
                assert np.array_equal(out[s][sl], exp), f"ms {ms}: row {s} ({k} calls) differs from the single session in call {i}"
            assert not out[s][k * frame:].any(), f"ms {ms}: row {s} is not zero behind its {k} calls"
            assert codes[s] == next((c for c in got_codes if c != 0), 0), f"ms {ms}: code of row {s}: {codes[s]} vs {got_codes}"
            sess.close()
        assert rc == next((c for c in codes.tolist() if c != 0), 0), f"ms {ms}: return code {rc} vs codes {codes.tolist()}"
        b2, b3 = aecm.AecmBatch(S, fs, 1, 3), aecm.AecmBatch(S, fs, 1, 3)
        rc2, out2, codes2 = b2.process_recordings_ragged_host(far, near, frame, np.full(S, n), ms, clean)
        rc3, out3 = b3.process_recordings_host(far, near, frame, ms, clean)
        assert rc2 == rc3 and codes2.tolist() == [rc3] * S, f"ms {ms}: all-equal call counts: codes {rc2} {codes2.tolist()} vs {rc3}"
        assert np.array_equal(out2, out3), f"ms {ms}: all-equal call counts differ from process_recordings_host in rows {np.nonzero((out2 != out3).any(axis=1))[0].tolist()}"
        for s in range(S):
            assert np.array_equal(b2.digest(s), b3.digest(s)), f"ms {ms}: all-equal call counts: state of stream {s} differs from process_recordings_host"
        for batch in (b, b2, b3):
            batch.close()


def test_cli_batch_of_recordings_of_different_lengths(tmp_path):
    """aecm_run --batch over three WAV pairs of different lengths writes the files three single-pair runs write, and reports
    the frames really processed."""
    import re
    import wave
    from webrtc_aecm_amd import build
    build.build()

    def write(path, x):
        with wave.open(str(path), "wb") as w:
            w.setnchannels(1)
            w.setsampwidth(2)
            w.setframerate(16000)
            w.writeframes(np.asarray(x, dtype="<i2").tobytes())
    sizes = (160000 + 57, 16000, 48000 + 3)
    for k, n in enumerate(sizes):
        far, near = synth_pair(40 + k, n // 64 + 1, 16000, "mixed")
        write(tmp_path / f"f{k}.wav", far[:n])
        write(tmp_path / f"n{k}.wav", near[:n])
    single = []
    for k in range(3):
        r = subprocess.run([str(build.CLI), str(tmp_path / f"f{k}.wav"), str(tmp_path / f"n{k}.wav")], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        single.append((tmp_path / f"n{k}_out.wav").read_bytes())
        (tmp_path / f"n{k}_out.wav").unlink()
    (tmp_path / "pairs.txt").write_text("".join(f"{tmp_path}/f{k}.wav {tmp_path}/n{k}.wav\n" for k in range(3)))
    r = subprocess.run([str(build.CLI), "--batch", str(tmp_path / "pairs.txt")], capture_output=True, text=True)
    assert r.returncode == 0 and "time interval" in r.stdout, r.stdout + r.stderr
    for k in range(3):
        assert (tmp_path / f"n{k}_out.wav").read_bytes() == single[k], k
    m = re.search(r"device 0: 3 recordings at 16000 Hz, (\d+) frames of 64 samples processed", r.stdout)
    assert m, r.stdout
    assert int(m.group(1)) == sum(n // 160 * 160 // 64 for n in sizes)       # the recordings' own samples, not 3 x the longest


def test_committed_ragged_golden_is_reproduced():
    """tests/golden/ragged_16k.npz (tools/gen_golden.py ragged_: lengths, seeds, per-stream output hashes and digests from the
    unmodified reference) on the device, in the forced queue form and with one wavefront per stream -- runs where the
    reference does not exist."""
    g = np.load(GOLDEN / "ragged_16k.npz")
    fs, T, lens, seeds = int(g["fs"]), int(g["n_blocks"]), g["lens"].astype(np.int32), g["seeds"].tolist()
    S = lens.size
    far, near = synth_streams(seeds, T, fs)
    for chunk in (8, 0):
        b = aecm.AecmBatch(S, fs)
        for s in range(S):
            b.set_config(int(g["cng"][s]), int(g["echo_mode"][s]), s, 1)
        b.set_launch_chunking(chunk, 0)
        assert b.describe_ragged_launch(lens)["form"] == (2 if chunk else 0)
        out = _run_device(b, far, near, lens, T)
        for s in range(S):
            n = int(lens[s]) * 64
            assert hashlib.sha256(out[s][:n].tobytes()).hexdigest() == str(g["sha256"][s]), (chunk, s)
            assert (out[s][n:] == SENTINEL).all(), (chunk, s)
            assert np.array_equal(b.digest(s), g["digests"][s]), (chunk, s)
        b.close()
