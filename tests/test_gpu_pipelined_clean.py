"""Pipelined launches for batches with a clean near-end input on the device (WebRtcAecmBatch_SetCleanPipelining): every carried
shape at sizes from one stream to more than a thousand, bit-exact (outputs and 24-word state digests) against the CPU checker,
the clean input's carried-over block across launches of every kind, and no result depending on the switch."""
import numpy as np
import pytest

import test_gpu_ragged as R
import webrtc_aecm_amd as aecm
from helpers import synth_streams
from oracle import pyoracle
from webrtc_aecm_amd.synth import synth_clean, synth_pair

pytestmark = pytest.mark.gpu
CLEAN_BIT = 0x2000
# the shapes the clean kernel is carried in: the policy's wishes that force each, DescribeLaunch's shape bits (without 0x2000), waves
SHAPES = {
    "sixteen waves (42240)": (dict(pipe_tail_waves=2, pipe_front_waves=4, pipe_raw=0, pipe_delay_waves=2, pipe_gain_waves=4), 0x1a02, 16),
    "twelve waves (4220)": (dict(pipe_tail_waves=2, pipe_front_waves=2, pipe_raw=0, pipe_delay_waves=4, pipe_gain_waves=0), 0x802, 12),
    "eight waves (220)": (dict(pipe_tail_waves=2, pipe_front_waves=2, pipe_raw=0, pipe_delay_waves=0, pipe_gain_waves=0), 0x002, 8),
    "six waves (20)": (dict(pipe_tail_waves=0, pipe_front_waves=2, pipe_raw=0, pipe_delay_waves=0, pipe_gain_waves=0), 0x000, 6),
}


def _clean_of(far, near):
    """A clean input per stream: even streams the stock 3/4 of the near end, odd ones a much quieter mix with a Q domain of its own."""
    clean = synth_clean(near)
    odd = (near[1::2].astype(np.int32) // 7 + np.roll(far[1::2], 5, axis=1).astype(np.int32) // 19).astype(np.int16)
    clean[1::2] = odd
    return clean


def _run(b, far, near, clean, T, in_place=False):
    """WebRtcAecmBatch_ProcessBlocks on device tensors (clean may be None); in_place: out_dev = near_clean_dev."""
    import torch
    dev = torch.device("cuda", 0)
    tf, tn = torch.from_numpy(far).to(dev), torch.from_numpy(near).to(dev)
    tc = torch.from_numpy(clean).to(dev) if clean is not None else None
    out = tc if in_place else torch.full_like(tn, R.SENTINEL)
    torch.cuda.synchronize()
    b.process_device(tf.data_ptr(), tn.data_ptr(), out.data_ptr(), far.shape[1], 64, T, tc.data_ptr() if tc is not None else None)
    b.synchronize()
    return out.cpu().numpy()


def _check_all(b, out, T, exp, fs, cfgs, streams=None):
    R._check(b, out, np.full(out.shape[0], T, dtype=np.int32), exp, fs, cfgs, streams)


@pytest.mark.parametrize("fs", [16000, 8000])
@pytest.mark.parametrize("S", [1, 2, 3, 5, 37, 300, 1030])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_every_carried_clean_shape(shape, S, fs):
    wishes, bits, waves = SHAPES[shape]
    T = 60 if S > 100 else 90
    far, near = synth_streams(list(range(5200, 5200 + S)), T, fs)
    clean = _clean_of(far, near)
    b = aecm.AecmBatch(S, fs)
    cfgs = R._configure(b, S)
    b.set_launch_policy(pipelined_min_streams=1, pipelined_min_blocks=1, **wishes)
    assert b.describe_launch(T, clean=True)[0] != 3                      # the default: off
    b.set_clean_pipelining(True)
    assert b.describe_launch(T, clean=True) == (3, bits | CLEAN_BIT)
    out = _run(b, far, near, clean, T)
    lens = np.full(S, T, dtype=np.int32)
    _check_all(b, out, T, R._expected(pyoracle.OracleStream, fs, cfgs, far, near, lens, clean), fs, cfgs)
    b.close()


@pytest.mark.parametrize("shape", [None, *SHAPES])
def test_state_across_launches_of_every_kind(shape):
    """One batch: a clean pipelined launch, a launch without a clean input (pipelined; c_old must come through untouched), a clean
    launch with the switch off (one wavefront per stream), a clean pipelined launch again -- after each, outputs and digests equal
    the oracle run over the same sequence."""
    S, fs = 300, 16000
    lens = (37, 11, 23, 40)
    T = sum(lens)
    far, near = synth_streams(list(range(6400, 6400 + S)), T, fs)
    clean = _clean_of(far, near)
    b = aecm.AecmBatch(S, fs)
    cfgs = R._configure(b, S)
    if shape is not None:
        b.set_launch_policy(pipelined_min_streams=1, pipelined_min_blocks=1, **SHAPES[shape][0])
    oracles = [pyoracle.OracleStream(fs, *cfg) for cfg in cfgs]
    at = 0
    for n, with_clean, switch, form in zip(lens, (True, False, True, True), (True, True, False, True), (3, 3, 0, 3)):
        b.set_clean_pipelining(switch)
        d = b.describe_launch(n, clean=with_clean)
        assert d[0] == form and bool(d[1] & CLEAN_BIT) == (with_clean and switch), (at, d)
        sl = slice(at * 64, (at + n) * 64)
        c = np.ascontiguousarray(clean[:, sl]) if with_clean else None
        out = _run(b, np.ascontiguousarray(far[:, sl]), np.ascontiguousarray(near[:, sl]), c, n)
        for s, o in enumerate(oracles):
            if with_clean:
                exp = np.concatenate([o.process_block_clean(far[s][k * 64:(k + 1) * 64], near[s][k * 64:(k + 1) * 64], clean[s][k * 64:(k + 1) * 64])
                                      for k in range(at, at + n)])
            else:
                exp = o.process(far[s][sl], near[s][sl])
            assert np.array_equal(out[s], exp), f"launch at block {at}: output of stream {s} differs"
            assert np.array_equal(b.digest(s), o.digest()), f"launch at block {at}: state digest of stream {s} differs"
        at += n
    b.close()


def _form_independence(S, with_reference):
    T, fs, K = 512, 16000, 32
    rs = np.random.RandomState(S)
    pairs = [synth_pair(1900 + k, T, fs) for k in range(K)]
    idx = np.arange(S) % K
    far = np.stack([p[0] for p in pairs])[idx]
    near = np.stack([p[1] for p in pairs])[idx]
    clean = _clean_of(far, near)
    sample = sorted({0, 1, S - 1, S - 2, *rs.randint(0, S, size=40).tolist()})[:24]
    lens = np.full(S, T, dtype=np.int32)
    digests, outs = [], []
    for on in (True, False):
        b = aecm.AecmBatch(S, fs)
        cfgs = R._configure(b, S)
        b.set_clean_pipelining(on)
        form, detail = b.describe_launch(T, clean=True)
        assert (form == 3 and detail & CLEAN_BIT) if on else form == 0, (on, form, detail)
        out = _run(b, far, near, clean, T)
        if on:
            cls = pyoracle.RefCoreStream if with_reference else pyoracle.OracleStream
            _check_all(b, out, T, R._expected(cls, fs, cfgs, far, near, lens, clean, streams=sample), fs, cfgs, sample)
        digests.append(np.stack([b.digest(s) for s in range(S)]))
        outs.append(out)
        b.close()
    bad = np.nonzero((digests[0] != digests[1]).any(axis=1))[0]
    assert bad.size == 0, f"state depends on the launch form in streams {bad[:8].tolist()}"
    assert np.array_equal(outs[0], outs[1])


@pytest.mark.parametrize("S", [1024, 2560, 4096])
def test_form_independence_under_the_shipped_policy(S):
    """512 blocks, the shipped policy (sixteen, eight and six waves at these sizes on 256 CUs): switch on against switch off -- all
    outputs and all state digests equal; a sample of 24 streams against the oracle."""
    _form_independence(S, False)


@R._needs_ref
def test_form_independence_sample_against_the_reference():
    _form_independence(1024, True)


def test_default_off_and_the_safe_variant():
    """With the switch off a clean launch is described and run as before the switch existed; a batch on the safe variant is never
    pipelined with the switch on, and its results equal the oracle's."""
    S, T, fs = 300, 60, 16000
    far, near = synth_streams(list(range(8100, 8100 + S)), T, fs)
    clean = _clean_of(far, near)
    lens = np.full(S, T, dtype=np.int32)
    b = aecm.AecmBatch(S, fs)
    cfgs = R._configure(b, S)
    exp = R._expected(pyoracle.OracleStream, fs, cfgs, far, near, lens, clean)
    assert b.describe_launch(T, clean=True) == (0, 0) and b.describe_launch(T)[0] == 3
    _check_all(b, _run(b, far, near, clean, T), T, exp, fs, cfgs)
    b.set_clean_pipelining(True)
    assert b.describe_launch(T, clean=True)[0] == 3
    b.set_clean_pipelining(False)
    assert b.describe_launch(T, clean=True) == (0, 0)
    b.close()
    b = aecm.AecmBatch(S, fs, variant=aecm.KERNEL_SAFE)
    R._configure(b, S)
    b.set_clean_pipelining(True)
    assert b.describe_launch(T, clean=True) == (0, 0)
    _check_all(b, _run(b, far, near, clean, T), T, exp, fs, cfgs)
    b.close()


@pytest.mark.parametrize("shape", [None, "six waves (20)"])
def test_output_in_place_of_the_clean_input(shape):
    """out_dev = near_clean_dev: the one-wavefront-per-stream form gives the oracle's answer in this arrangement (checked first),
    and so does the pipelined one -- no clean row is read after an output row of the launch has been written."""
    S, T, fs = 300, 60, 16000
    far, near = synth_streams(list(range(8700, 8700 + S)), T, fs)
    clean = _clean_of(far, near)
    lens = np.full(S, T, dtype=np.int32)
    exp = None
    for on in (False, True):
        b = aecm.AecmBatch(S, fs)
        cfgs = R._configure(b, S)
        if shape is not None:
            b.set_launch_policy(pipelined_min_streams=1, pipelined_min_blocks=1, **SHAPES[shape][0])
        b.set_clean_pipelining(on)
        assert b.describe_launch(T, clean=True)[0] == (3 if on else 0)
        if exp is None:
            exp = R._expected(pyoracle.OracleStream, fs, cfgs, far, near, lens, clean)
        _check_all(b, _run(b, far, near, clean.copy(), T, in_place=True), T, exp, fs, cfgs)
        b.close()


def test_recordings_with_the_switch_on_equal_the_switch_off():
    fs, frame, n, S = 16000, 160, 60, 40
    far, near = synth_streams(list(range(330, 330 + S)), n * frame // 64 + 1, fs)
    far, near = np.ascontiguousarray(far[:, :n * frame]), np.ascontiguousarray(near[:, :n * frame])
    clean = _clean_of(far, near)
    res = []
    for on in (False, True):
        b = aecm.AecmBatch(S, fs, 1, 3)
        b.set_clean_pipelining(on)
        assert b.describe_launch(n * frame // 64, clean=True)[0] == (3 if on else 0)
        rc, out = b.process_recordings_host(far, near, frame, 40, clean)
        res.append((rc, out, np.stack([b.digest(s) for s in range(S)])))
        b.close()
    assert res[0][0] == res[1][0]
    assert np.array_equal(res[0][1], res[1][1]) and np.array_equal(res[0][2], res[1][2])
