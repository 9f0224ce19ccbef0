"""The second set of lean forms of the block loop (aecm_wave.h: AECM_LEAN_BLOCK bits 16..128) on the GPU: 64 streams x 320 blocks,
both rates, the signal mix of tests/test_gpu_lean_block.py with every eighth stream's echo path re-initialised (to 0, to negative
entries, to a mixture: ch_adapt32 0 and negative, which the NLMS norms special-case).  Through the two kernels that take the
lean forms -- the chunk queue forced by policy with chunks of 32 blocks (ten hand-overs per stream, the start-up blocks inside)
and the same batch as a ragged launch with lengths spread over 80..320 (the ragged twin) -- and once as one wavefront per
stream, a family that keeps the parent's forms.  Outputs and the 24-word state digest against the oracle, bit for bit; the
oracle runs each stream once for the whole module and the ragged test reads the state it had at the stream's own length."""
import numpy as np
import pytest

import webrtc_aecm_amd as aecm
from helpers import describe_digest_diff
from oracle import pyoracle
from test_gpu_lean_block import S, T, _mix

pytestmark = pytest.mark.gpu
SENTINEL = 0x5A5A
LENS = (80 + (np.arange(S) * 53) % 241).astype(np.int32)          # 80 .. 320, every stream another length
LENS[5], LENS[9] = T, 80


def _paths():
    """stream -> echo path (int16[65]) for the streams that get one."""
    rs = np.random.RandomState(222)
    paths = {}
    for s in range(0, S, 8):
        kind = (s // 8) % 3
        paths[s] = (np.zeros(65, np.int16), np.full(65, -9000, np.int16),
                    rs.choice([0, 0, -1, -32768, -12000, 5, 20000], size=65).astype(np.int16))[kind]
    return paths


@pytest.fixture(scope="module", params=[16000, 8000])
def case(request):
    fs = request.param
    cfg, far, near = _mix(fs)
    paths = _paths()
    full, part = [], []
    for s in range(S):
        o = pyoracle.OracleStream(fs, *cfg[s])
        if s in paths:
            o.init_echo_path(paths[s])
        n = int(LENS[s]) * 64
        head = o.process(far[s][:n], near[s][:n])
        part.append((head, o.digest()))
        tail = o.process(far[s][n:], near[s][n:]) if n < T * 64 else np.zeros(0, np.int16)
        full.append((np.concatenate([head, tail]), o.digest()))
    return fs, cfg, far, near, paths, full, part


def _batch(case, **policy):
    fs, cfg, far, near, paths, full, part = case
    b = aecm.AecmBatch(S, fs)
    for s in range(S):
        b.set_config(cfg[s][0], cfg[s][1], s, 1)
    for s, p in paths.items():
        b.init_echo_path(s, p)
    b.set_launch_policy(**policy)
    return b


def _run(case, form, **policy):
    import torch
    fs, cfg, far, near, paths, full, part = case
    b = _batch(case, **policy)
    got_form = b.describe_launch(T)[0]
    assert got_form in form, (got_form, form)
    dfar, dnear = torch.from_numpy(far).cuda(), torch.from_numpy(near).cuda()
    dout = torch.zeros_like(dnear)
    torch.cuda.synchronize()
    b.process_device(dfar.data_ptr(), dnear.data_ptr(), dout.data_ptr(), T * 64, 64, T)
    b.synchronize()
    out = dout.cpu().numpy()
    for s in range(S):
        assert np.array_equal(out[s], full[s][0]), (fs, s, int(np.nonzero(out[s] != full[s][0])[0][0]) // 64)
        assert np.array_equal(b.digest(s), full[s][1]), (fs, s, describe_digest_diff(b.digest(s), full[s][1]))
    b.close()


def test_chunk_queue_with_both_sets_of_lean_forms_equals_the_oracle(case):
    _run(case, (2,), queue_min_streams=0, queue_chunk_blocks=32, queue_chunk_explicit=1, pipelined_min_streams=0)


def test_ragged_chunk_queue_with_both_sets_of_lean_forms_equals_the_oracle(case):
    import torch
    fs, cfg, far, near, paths, full, part = case
    b = _batch(case, queue_min_streams=0, queue_chunk_blocks=32, queue_chunk_explicit=1, pipelined_min_streams=0)
    d = b.describe_ragged_launch(LENS)
    assert (d["form"], d["chunk_blocks"]) == (2, 32), d
    dfar, dnear = torch.from_numpy(far).cuda(), torch.from_numpy(near).cuda()
    dout = torch.full_like(dnear, SENTINEL)
    torch.cuda.synchronize()
    b.process_ragged_device(dfar.data_ptr(), dnear.data_ptr(), dout.data_ptr(), T * 64, 64, T, LENS)
    b.synchronize()
    out = dout.cpu().numpy()
    for s in range(S):
        n = int(LENS[s]) * 64
        assert np.array_equal(out[s][:n], part[s][0]), (fs, s, int(LENS[s]), int(np.nonzero(out[s][:n] != part[s][0])[0][0]) // 64)
        assert (out[s][n:] == SENTINEL).all(), (fs, s, "blocks beyond the stream's length were written")
        assert np.array_equal(b.digest(s), part[s][1]), (fs, s, describe_digest_diff(b.digest(s), part[s][1]))
    b.close()


def test_one_wavefront_per_stream_equals_the_oracle(case):
    _run(case, (0, 1), queue_min_streams=-1, pipelined_min_streams=S + 1)      # a batch below pipelined_min_streams never runs pipelined
