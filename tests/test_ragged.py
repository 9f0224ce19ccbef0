"""Ragged batches (one length per stream) as far as they can be shown without a GPU: the plan a ragged chunk-queue launch runs
by, the launch rule, the prefix property of the recording schedule that ragged recordings rest on, ragged recordings on the
lane simulator, and the C ABI's new symbols and argument errors.  The device side is tests/test_gpu_ragged.py."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import ragged_sim
import simlib
import webrtc_aecm_amd as aecm
from helpers import golden_files
from oracle import pyoracle
from webrtc_aecm_amd import ffi
from webrtc_aecm_amd.synth import synth_clean, synth_pair

ROOT = Path(__file__).resolve().parent.parent
RAGGED_SYMBOLS = ["WebRtcAecmBatch_ProcessBlocksRagged", "WebRtcAecmBatch_ProcessBlocksRaggedHost", "WebRtcAecmBatch_ProcessRecordingsRagged",
                  "WebRtcAecmBatch_ProcessRecordingsRaggedHost", "WebRtcAecmBatch_DescribeRaggedLaunch", "WebRtcAecmBatch_RaggedPlan"]


def _length_vectors():
    rs = np.random.RandomState(5)
    return [("random", rs.randint(0, 201, size=300)),
            ("many zeros", np.where(rs.rand(500) < 0.3, 0, rs.randint(1, 1000, size=500))),
            ("all equal", np.full(97, 640)),
            ("one outlier", np.r_[np.full(255, 20), 1280]),
            ("not multiples of any chunk", rs.randint(1, 130, size=64) * 3 + 1),
            ("one stream", np.array([5])),
            ("one live stream", np.r_[np.zeros(9, dtype=np.int64), 7]),
            ("all zero", np.zeros(12, dtype=np.int64))]


@pytest.mark.parametrize("chunk", [8, 32, 128])
def test_plan_holds_every_chunk_of_every_stream_once_in_claim_order(chunk):
    """Every (chunk, stream) pair with c x chunk < len[s] appears exactly once; the items are chunk-major; (c, s) comes after
    (c - 1, s) -- what the kernel's no-deadlock argument needs --; items == sum of ceil(len / chunk); longest streams first."""
    for name, lens in _length_vectors():
        lens = np.asarray(lens, dtype=np.int64)
        order, first_item = aecm.ragged_plan(lens, chunk)
        n_chunks = -(-int(lens.max()) // chunk)
        assert first_item.size == n_chunks + 1 and first_item[0] == 0, name
        assert sorted(order.tolist()) == list(range(lens.size)), name                       # a permutation of the streams
        sorted_lens = lens[order]
        assert (np.diff(sorted_lens) <= 0).all(), name                                      # longest first ...
        assert all(order[i] < order[i + 1] for i in range(lens.size - 1) if sorted_lens[i] == sorted_lens[i + 1]), name      # ... and stable
        number = {}                                                                         # (chunk, stream) -> item number
        for c in range(n_chunks):
            live = int(first_item[c + 1] - first_item[c])
            assert live == int((lens > c * chunk).sum()), (name, c)
            for r in range(live):
                key = (c, int(order[r]))
                assert key not in number, (name, key)
                number[key] = int(first_item[c]) + r
        want = {(c, s) for s in range(lens.size) for c in range(-(-int(lens[s]) // chunk))}
        assert set(number) == want, name
        assert sorted(number.values()) == list(range(len(want))), name                      # the item numbers are 0 .. items - 1, no gaps
        assert all(number[(c, s)] > number[(c - 1, s)] for (c, s) in number if c > 0), name
        by_number = sorted(number, key=number.get)
        assert [c for c, _ in by_number] == sorted(c for c, _ in by_number), name           # chunk-major
        assert int(first_item[-1]) == int(np.sum(-(-lens // chunk))), name


def test_ragged_launch_rule_without_a_device():
    """All-equal lengths describe exactly the equal-length launch; unequal ones take the chunk queue when enough streams are
    live and the longest has two chunks, else one wavefront per stream; never the pipelined form; the work is the sum."""
    for cus in (256, 64):
        for S, T, clean in ((8192, 512, False), (65536, 1280, False), (1024, 300, False), (5000, 300, True), (7, 40, False), (cus * 28 + 1, 255, False)):
            d = aecm.describe_ragged_launch(np.full(S, T), cus, clean)
            want = aecm.describe_launch_detail(S, T, cus, clean)
            assert {k: d[k] for k in want} == want, (cus, S, T, clean, d)
            assert d["sum_blocks"] == S * T and d["max_blocks"] == T
            assert d["items"] == (S * -(-T // d["chunk_blocks"]) if d["form"] == 2 else 0)
    rs = np.random.RandomState(1)
    lens = rs.randint(128, 513, size=8192)
    lens[0] = 512
    d = aecm.describe_ragged_launch(lens, 256)
    assert (d["form"], d["chunk_blocks"], d["workgroups"]) == (2, 128, 1792), d
    assert d["items"] == int(np.sum(-(-lens // 128))) and d["sum_blocks"] == int(lens.sum()) and d["max_blocks"] == 512
    # between the pipelined form's limit and the chip's resident waves the default chunk is quartered, as for equal lengths
    d = aecm.describe_ragged_launch(lens[:5000], 256)
    assert (d["form"], d["chunk_blocks"]) == (2, 32) and d["items"] == int(np.sum(-(-lens[:5000] // 32)))
    # few live streams: the threshold counts the streams that have blocks to run, and a ragged launch is never pipelined
    few = np.zeros(65536, dtype=np.int64)
    few[:100] = rs.randint(1, 1281, size=100)
    assert aecm.describe_ragged_launch(few, 256)["form"] == 1
    assert aecm.describe_ragged_launch(lens[:1024], 256)["form"] == 0
    # the longest stream shorter than two chunks: one wavefront per stream
    assert aecm.describe_ragged_launch(rs.randint(0, 256, size=8192), 256)["form"] == 1
    # a policy of the caller's: the queue from the first stream, chunks of 8
    p = aecm.default_launch_policy(256)
    p.queue_chunk_blocks, p.queue_chunk_explicit, p.queue_min_streams = 8, 1, 0
    small = rs.randint(0, 201, size=37)
    small[3] = 200
    d = aecm.describe_ragged_launch(small, policy=p)
    assert (d["form"], d["chunk_blocks"], d["items"]) == (2, 8, int(np.sum(-(-small // 8)))), d
    assert aecm.describe_ragged_launch(np.zeros(5, dtype=np.int64), 256)["max_blocks"] == 0


def test_new_symbols_are_declared_exported_and_refuse_bad_arguments():
    lib = aecm.load()
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "aecm_batch.h").read_text(), flags=re.S)
    for name in RAGGED_SYMBOLS:
        assert name in ffi.BATCH_SYMBOLS and hasattr(lib, name) and re.search(r"\b%s\s*\(" % name, header), name
    z = np.zeros(64, dtype=np.int16)
    lens = np.zeros(4, dtype=np.int32)
    codes = np.zeros(4, dtype=np.int32)
    p = z.ctypes.data
    # NULL handle first, as the neighbouring functions do
    assert lib.WebRtcAecmBatch_ProcessBlocksRagged(None, p, p, None, p, 64, 64, 1, lens.ctypes.data) == -1
    assert lib.WebRtcAecmBatch_ProcessBlocksRaggedHost(None, p, p, None, p, 64, 64, 1, lens.ctypes.data) == -1
    assert lib.WebRtcAecmBatch_ProcessRecordingsRagged(None, p, p, None, p, 160, 160, 1, lens.ctypes.data, 40, codes.ctypes.data) == -1
    assert lib.WebRtcAecmBatch_ProcessRecordingsRaggedHost(None, p, p, None, p, 160, 160, 1, lens.ctypes.data, 40, None) == -1
    # the planning calls need no device
    d = ffi.AecmLaunchDescription()
    describe = lib.WebRtcAecmBatch_DescribeRaggedLaunch
    assert describe(None, 256, 4, lens.ctypes.data, 0, None, None, None, None) == ffi.AECM_NULL_POINTER_ERROR
    assert describe(None, 256, 4, None, 0, C.byref(d), None, None, None) == ffi.AECM_NULL_POINTER_ERROR
    assert describe(None, 256, 0, lens.ctypes.data, 0, C.byref(d), None, None, None) == ffi.AECM_BAD_PARAMETER_ERROR
    assert describe(None, 0, 4, lens.ctypes.data, 0, C.byref(d), None, None, None) == ffi.AECM_BAD_PARAMETER_ERROR
    assert describe(None, 256, 4, lens.ctypes.data, 0, C.byref(d), None, None, None) == 0
    bad = np.array([3, -1, 2, 2], dtype=np.int32)
    assert describe(None, 256, 4, bad.ctypes.data, 0, C.byref(d), None, None, None) == ffi.AECM_BAD_PARAMETER_ERROR
    q = aecm.default_launch_policy(256)
    q.struct_size = 8
    assert describe(C.byref(q), 0, 4, lens.ctypes.data, 0, C.byref(d), None, None, None) == ffi.AECM_BAD_PARAMETER_ERROR
    with pytest.raises(aecm.AecmError):
        aecm.ragged_plan(bad, 8)
    with pytest.raises(aecm.AecmError):
        aecm.ragged_plan(lens, 0)
    order = np.zeros(4, dtype=np.int32)
    first = np.zeros(1, dtype=np.int32)
    n = C.c_int32(0)
    long_one = np.array([100, 1, 1, 1], dtype=np.int32)
    assert lib.WebRtcAecmBatch_RaggedPlan(4, long_one.ctypes.data, 8, order.ctypes.data, first.ctypes.data, 1, C.byref(n)) == ffi.AECM_BAD_PARAMETER_ERROR
    assert lib.WebRtcAecmBatch_RaggedPlan(4, long_one.ctypes.data, 8, None, first.ctypes.data, 1, C.byref(n)) == ffi.AECM_NULL_POINTER_ERROR


@pytest.mark.parametrize("fs,frame", [(16000, 160), (8000, 80), (16000, 80), (8000, 160)])
@pytest.mark.parametrize("ms", [0, 40, 500])
def test_schedule_of_k_calls_is_a_prefix_of_the_schedule_of_more_calls(fs, frame, ms):
    """The session machinery is causal: shown, not assumed -- for every k the schedule of k calls equals the first
    blocks_after_call[k - 1] blocks and k x frame output entries of the schedule of 60 calls, and so do the return codes."""
    n = 60
    full = ragged_sim.schedule(fs, frame, n, ms)
    assert full["blocks_after_call"].size == n and full["blocks_after_call"][-1] == full["n_blocks"]
    assert (np.diff(full["blocks_after_call"]) >= 0).all()
    for k in range(1, n + 1):
        part = ragged_sim.schedule(fs, frame, k, ms)
        nb = int(full["blocks_after_call"][k - 1])
        assert part["n_blocks"] == nb, k
        assert np.array_equal(part["far_map"], full["far_map"][:nb * 64]), k
        assert np.array_equal(part["near_map"], full["near_map"][:nb * 64]), k
        assert np.array_equal(part["out_map"], full["out_map"][:k * frame]), k
        assert part["out_map"].max(initial=-1) < max(nb * 64, 1), k                        # a call's output never needs a later block
        assert np.array_equal(part["blocks_after_call"], full["blocks_after_call"][:k]), k
        assert np.array_equal(part["code_after_call"], full["code_after_call"][:k]), k
        assert part["code"] == full["code_after_call"][k - 1], k
    first_nonzero = [c for c in full["code_after_call"] if c != 0]
    assert full["code"] == (first_nonzero[0] if first_nonzero else 0)


def test_ragged_recordings_on_the_lane_simulator():
    """The ragged twin of sim_recordings (tests/sim/sim_ragged.cpp: the engine's procedure -- common schedule, each stream its
    first blocks_after_call[calls - 1] blocks, output assembled up to calls x frame, zeros behind) against single sessions
    that made exactly that many calls: the unmodified reference where it is built, the committed golden recordings otherwise
    (a prefix of a recording is a recording)."""
    for f in golden_files("session_"):
        g = np.load(f)
        fs, frame, ms, cng, em = int(g["fs"]), int(g["frame"]), int(g["ms"]), int(g["cng"]), int(g["echo_mode"])
        with_clean = "clean" in g.files and int(g["clean"]) != 0
        far, near = synth_pair(int(g["seed"]), int(g["n_blocks"]), fs, "mixed")
        n_calls = min(far.size // frame, 120)
        n = n_calls * frame
        calls = np.array([0, 1, 7, 33, n_calls // 2, n_calls], dtype=np.int32)
        fars, nears = np.tile(far[:n], (calls.size, 1)), np.tile(near[:n], (calls.size, 1))
        cleans = synth_clean(nears) if with_clean else None
        rc, out, codes = ragged_sim.recordings_ragged(fars, nears, fs, frame, cng, em, ms, calls, cleans)
        for s, k in enumerate(calls.tolist()):
            if pyoracle.have_reference():
                r = pyoracle.RefSession(fs, cng, em)
                exp = near[:k * frame].copy()
                got_codes = []
                for i in range(k):
                    sl = slice(i * frame, (i + 1) * frame)
                    assert r.buffer_farend(far[sl]) == 0
                    code, exp[sl] = r.process(near[sl], None if cleans is None else cleans[s][sl], ms)
                    got_codes.append(code)
                want_code = next((c for c in got_codes if c != 0), 0)
            else:
                exp = g["out"][:k * frame]
                want_code = int(g["codes"].max()) if k > 0 else 0
            assert np.array_equal(out[s][:k * frame], exp), (f.name, k)
            assert not out[s][k * frame:].any(), (f.name, k)
            assert codes[s] == want_code, (f.name, k, codes[s])
        assert rc == next((c for c in codes.tolist() if c != 0), 0)
        # all-equal call counts: the equal-length form's result
        full = np.full(calls.size, n_calls, dtype=np.int32)
        rc2, out2, _ = ragged_sim.recordings_ragged(fars, nears, fs, frame, cng, em, ms, full, cleans)
        rc3, out3 = simlib.sim_recordings(fars, nears, fs, frame, cng, em, ms, cleans)
        assert rc2 == rc3 and np.array_equal(out2, out3), f.name
