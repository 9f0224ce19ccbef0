"""The lean block loop (aecm_wave.h: AECM_LEAN_BLOCK) on the GPU: 64 streams x 320 blocks, both rates, the signal mix of
tests/test_lean_block.py (bench signal, double talk, silence, hostile inputs), through process_device in the chunk-queue form --
the kernel family that takes the lean forms, forced onto this small batch by launch policy -- and once as one wavefront per
stream (a family that keeps the parent's forms).  Outputs and the 24-word state digest against the oracle, bit for bit."""
import numpy as np
import pytest

import webrtc_aecm_amd as aecm
from helpers import describe_digest_diff
from oracle import pyoracle
from test_lean_block import bench_pair

pytestmark = pytest.mark.gpu
S, T = 64, 320


def _mix(fs):
    """[S] (cng, echo_mode), far [S, T * 64], near."""
    rs = np.random.RandomState(18 + fs)
    n = T * 64
    far, near, cfg = np.empty((S, n), np.int16), np.empty((S, n), np.int16), []
    level = lambda: np.repeat(rs.choice([0, 1, 40, 3000, 32767], size=T), 64).astype(np.int64)
    for s in range(S):
        kind = s % 8
        cfg.append((1, 1) if kind < 5 else (0 if s % 16 == 7 else 1, s % 5))
        if kind < 3:
            far[s], near[s] = bench_pair(100 + s, T)
        elif kind == 3:
            far[s], near[s] = bench_pair(100 + s, T, "double_talk")
        elif kind == 4:
            far[s], near[s] = bench_pair(100 + s, T, "silent")
        elif kind == 5:                       # full scale; runs of -32768
            far[s] = np.where(rs.randint(0, 2, n) == 1, 32767, -32768)
            near[s] = rs.randint(-32768, 32768, n)
            near[s][(np.arange(n) // 640) % 2 == 0] = -32768
        elif kind == 6:                       # level steps, block by block
            far[s] = (rs.randint(-32768, 32768, size=n).astype(np.int64) * level()) >> 15
            near[s] = (rs.randint(-32768, 32768, size=n).astype(np.int64) * level()) >> 15
        else:                                 # loud far end, silent near end / both silent
            far[s] = rs.randint(-32768, 32768, n) if s % 16 == 7 else 0
            near[s] = 0
    return cfg, far, near


@pytest.fixture(scope="module", params=[16000, 8000])
def case(request):
    fs = request.param
    cfg, far, near = _mix(fs)
    exp = []
    for s in range(S):
        o = pyoracle.OracleStream(fs, *cfg[s])
        exp.append((o.process(far[s], near[s]), o.digest()))
    return fs, cfg, far, near, exp


def _run(case, form, **policy):
    import torch
    fs, cfg, far, near, exp = case
    b = aecm.AecmBatch(S, fs)
    for s in range(S):
        b.set_config(cfg[s][0], cfg[s][1], s, 1)
    b.set_launch_policy(**policy)
    got_form = b.describe_launch(T)[0]
    assert got_form in form, (got_form, form)
    dfar, dnear = torch.from_numpy(far).cuda(), torch.from_numpy(near).cuda()
    dout = torch.zeros_like(dnear)
    torch.cuda.synchronize()
    b.process_device(dfar.data_ptr(), dnear.data_ptr(), dout.data_ptr(), T * 64, 64, T)
    b.synchronize()
    out = dout.cpu().numpy()
    for s in range(S):
        assert np.array_equal(out[s], exp[s][0]), (fs, s, int(np.nonzero(out[s] != exp[s][0])[0][0]) // 64)
        assert np.array_equal(b.digest(s), exp[s][1]), (fs, s, describe_digest_diff(b.digest(s), exp[s][1]))
    b.close()


def test_chunk_queue_with_the_lean_forms_equals_the_oracle(case):
    # chunks of 32 blocks: ten hand-overs of every stream's state between waves
    _run(case, (2,), queue_min_streams=0, queue_chunk_blocks=32, queue_chunk_explicit=1, pipelined_min_streams=0)


def test_one_wavefront_per_stream_equals_the_oracle(case):
    _run(case, (0, 1), queue_min_streams=-1, pipelined_min_streams=S + 1)      # a batch below pipelined_min_streams never runs pipelined
