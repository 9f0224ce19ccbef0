"""Pipelined launches for ragged batches the chip holds at once, as far as they can be shown without a GPU: the C ABI's new
symbols and argument errors, the properties of the host plan (which stream sits in which slot of which workgroup on which
compute unit), the launch rule with the batch's opt-in, and one workgroup of four streams of four different lengths through
the kernel's role split on the lane simulator.  The device side is tests/test_gpu_ragged_pipelined.py."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import simlib
import webrtc_aecm_amd as aecm
from oracle import pyoracle
from webrtc_aecm_amd import ffi
from webrtc_aecm_amd.synth import synth_pair

ROOT = Path(__file__).resolve().parent.parent
NEW_SYMBOLS = ["WebRtcAecmBatch_SetRaggedPipelining", "WebRtcAecmBatch_DescribeRaggedLaunchEx", "WebRtcAecmBatch_RaggedPipePlan",
               "WebRtcAecmBatch_DescribeRaggedLaunchOf"]
UNBALANCED_SHAPES = {0x000, 0x002, 0x402, 0x602, 0x802, 0x1a02}      # keys 20, 220, 221, 241, 4220, 42240 as DescribeLaunch's shape bits


def test_new_symbols_are_declared_exported_and_refuse_bad_arguments():
    lib = aecm.load()
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "aecm_batch.h").read_text(), flags=re.S)
    for name in NEW_SYMBOLS:
        assert name in ffi.BATCH_SYMBOLS and hasattr(lib, name) and re.search(r"\b%s\s*\(" % name, header), name
    assert lib.WebRtcAecmBatch_SetRaggedPipelining(None, 1) == ffi.AECM_BAD_PARAMETER_ERROR
    lens = np.array([5, 0, 9, 9], dtype=np.int32)
    d = ffi.AecmLaunchDescription()
    assert lib.WebRtcAecmBatch_DescribeRaggedLaunchOf(None, lens.ctypes.data, 0, C.byref(d), None, None, None) == -1
    describe = lib.WebRtcAecmBatch_DescribeRaggedLaunchEx
    assert describe(None, 256, 4, lens.ctypes.data, 0, 1, None, None, None, None) == ffi.AECM_NULL_POINTER_ERROR
    assert describe(None, 256, 4, None, 0, 1, C.byref(d), None, None, None) == ffi.AECM_NULL_POINTER_ERROR
    assert describe(None, 256, 0, lens.ctypes.data, 0, 1, C.byref(d), None, None, None) == ffi.AECM_BAD_PARAMETER_ERROR
    assert describe(None, 0, 4, lens.ctypes.data, 0, 1, C.byref(d), None, None, None) == ffi.AECM_BAD_PARAMETER_ERROR
    assert describe(None, 256, 4, lens.ctypes.data, 0, 1, C.byref(d), None, None, None) == 0 and d.form == 3
    bad = np.array([3, -1, 2, 2], dtype=np.int32)
    assert describe(None, 256, 4, bad.ctypes.data, 0, 1, C.byref(d), None, None, None) == ffi.AECM_BAD_PARAMETER_ERROR
    q = aecm.default_launch_policy(256)
    q.struct_size = 8
    assert describe(C.byref(q), 0, 4, lens.ctypes.data, 0, 1, C.byref(d), None, None, None) == ffi.AECM_BAD_PARAMETER_ERROR
    plan = lib.WebRtcAecmBatch_RaggedPipePlan
    slots = np.zeros(16, dtype=np.int32)
    n = C.c_int32(0)
    assert plan(None, 256, 4, lens.ctypes.data, None, 16, C.byref(n)) == ffi.AECM_NULL_POINTER_ERROR
    assert plan(None, 256, 4, None, slots.ctypes.data, 16, C.byref(n)) == ffi.AECM_NULL_POINTER_ERROR
    assert plan(None, 256, 4, lens.ctypes.data, slots.ctypes.data, 16, None) == ffi.AECM_NULL_POINTER_ERROR
    assert plan(None, 0, 4, lens.ctypes.data, slots.ctypes.data, 16, C.byref(n)) == ffi.AECM_BAD_PARAMETER_ERROR
    assert plan(None, 256, 0, lens.ctypes.data, slots.ctypes.data, 16, C.byref(n)) == ffi.AECM_BAD_PARAMETER_ERROR
    assert plan(None, 256, 4, bad.ctypes.data, slots.ctypes.data, 16, C.byref(n)) == ffi.AECM_BAD_PARAMETER_ERROR
    assert plan(None, 256, 4, lens.ctypes.data, slots.ctypes.data, 2, C.byref(n)) == ffi.AECM_BAD_PARAMETER_ERROR       # too small a capacity
    assert plan(C.byref(q), 0, 4, lens.ctypes.data, slots.ctypes.data, 16, C.byref(n)) == ffi.AECM_BAD_PARAMETER_ERROR
    zeros = np.zeros(4, dtype=np.int32)
    assert plan(None, 256, 4, zeros.ctypes.data, slots.ctypes.data, 16, C.byref(n)) == ffi.AECM_BAD_PARAMETER_ERROR     # nothing to plan
    assert plan(None, 256, 4, lens.ctypes.data, slots.ctypes.data, 16, C.byref(n)) == 0 and 1 <= n.value <= 3
    with pytest.raises(aecm.AecmError):
        aecm.ragged_pipe_plan(np.full(5000, 7), 256)                      # more live streams than the pipelined form holds


def _length_vectors():
    rs = np.random.RandomState(11)
    out = [("random", rs.randint(0, 201, size=300)),
           ("random, not a multiple of anything", rs.randint(1, 2049, size=1031)),
           ("random, full", rs.randint(512, 2049, size=4096)),
           ("constant but one", np.r_[np.full(999, 640), 641]),
           ("one outlier", np.r_[np.full(255, 20), 1280]),
           ("1 % outliers of 8x", np.where(rs.rand(2048) < 0.01, 2048, 256)),
           ("many zeros", np.where(rs.rand(3000) < 0.6, 0, rs.randint(1, 1000, size=3000))),
           ("100 live of 65 536", np.r_[rs.randint(1, 1281, size=100), np.zeros(65436, dtype=np.int64)]),
           ("two streams", np.array([5, 9])),
           ("one live stream", np.r_[np.zeros(9, dtype=np.int64), 7])]
    return [(name, np.asarray(v, dtype=np.int64)) for name, v in out]


@pytest.mark.parametrize("cus", [256, 64])
def test_plan_properties(cus):
    """Every live stream exactly once, zero-length streams never, at most four per workgroup, the slot rule (longest in slot 0,
    then 2, 1, 3; 1 / 2 / 3 streams in slots 0 / 0, 2 / 0, 1, 2), no more workgroups than the shape holds, lock-step partners
    consecutive in the unit's length order, the longest-processing-time-first bound, and the description's evenness."""
    for name, lens in _length_vectors():
        live = np.nonzero(lens > 0)[0]
        if live.size > 16 * cus:
            with pytest.raises(aecm.AecmError):
                aecm.ragged_pipe_plan(lens, cus)
            continue
        slots = aecm.ragged_pipe_plan(lens, cus)
        n_wg = slots.shape[0]
        placed = slots[slots >= 0]
        assert sorted(placed.tolist()) == live.tolist(), name                               # every live stream once, no other
        assert (slots >= -1).all() and (slots < lens.size).all(), name
        assert (slots[-1] >= 0).any(), name                                                 # the plan ends at the last workgroup that holds a stream
        pattern = {0: (), 1: (0,), 2: (0, 2), 3: (0, 1, 2), 4: (0, 1, 2, 3)}
        for w in range(n_wg):
            used = tuple(np.nonzero(slots[w] >= 0)[0].tolist())
            assert used == pattern[len(used)], (name, w, slots[w])
            by_rank = [slots[w][k] for k in (0, 2, 1, 3) if slots[w][k] >= 0]                # slot 0 the longest, then 2, then 1, then 3
            assert all(lens[a] >= lens[b] for a, b in zip(by_rank, by_rank[1:])), (name, w, slots[w])
        # the description of the same launch
        p = aecm.default_launch_policy(cus)
        d = aecm.describe_ragged_launch(lens, policy=p, ragged_pipelining=True)
        if live.size >= 2 and lens.max() >= 3 and lens.min() != lens.max():
            assert d["form"] == 3 and d["shape"] in UNBALANCED_SHAPES, (name, d)
            assert d["workgroups"] == n_wg <= d["workgroups_per_cu"] * cus, (name, d, n_wg)
        per_cu = max(d["workgroups_per_cu"], 1) if d["form"] == 3 else 4
        # workgroups i, i + cus, ... share a compute unit
        used_cus = min(cus, n_wg)
        load = np.zeros(used_cus, dtype=np.int64)
        count = np.zeros(used_cus, dtype=np.int64)
        for w in range(n_wg):
            s = slots[w][slots[w] >= 0]
            load[w % cus] += lens[s].sum()
            count[w % cus] += s.size
        for c in range(used_cus):                                                           # within a unit: consecutive runs of its length order
            seq = [lens[s] for w in range(c, n_wg, cus) for s in (slots[w][k] for k in (0, 2, 1, 3)) if s >= 0]
            assert all(a >= b for a, b in zip(seq, seq[1:])), (name, c, seq)
            sizes = [int((slots[w] >= 0).sum()) for w in range(c, n_wg, cus)]
            assert max(sizes) - min(s for s in sizes if s > 0) <= 1 or min(sizes) == 0, (name, c, sizes)
        total = int(lens.sum())
        # LPT: the last stream the fullest unit got went to the unit with the fewest blocks at that moment, which held at most the
        # mean -- so fullest <= mean + longest, PROVIDED no unit with fewer blocks was passed over for want of a free slot.  No
        # unit was ever full (every one ends with a free slot under the shape's capacity) is a sufficient condition for that.
        if d["form"] == 3:
            capacity = 4 * np.array([len(range(c, d["workgroups_per_cu"] * cus, cus)) for c in range(used_cus)])
            all_units = min(cus, d["workgroups_per_cu"] * cus)
            if (count < capacity[:used_cus]).all():
                assert load.max() <= total / all_units + lens.max(), (name, load.max(), total / all_units, lens.max())
            want = int((1000 * total // used_cus) // max(int(load.max()), 1))
            assert d["cu_load_evenness_x1000"] == want, (name, d, want)
            assert d["sum_blocks"] == total and d["max_blocks"] == int(lens.max()) and d["items"] == 0


def test_launch_rule_without_a_device():
    """Switch off: DescribeRaggedLaunchEx is DescribeRaggedLaunch on every case of tests/test_ragged.py's rule test.  Switch on:
    a launch the chip holds at once is pipelined in an unbalanced shape -- by its LIVE streams -- unless it has a clean input,
    runs the safe variant (a batch's setting: on the device), is too short, too large, or the queue takes it."""
    rs = np.random.RandomState(1)
    lens = rs.randint(128, 513, size=8192)
    lens[0] = 512
    few = np.zeros(65536, dtype=np.int64)
    few[:100] = rs.randint(1, 1281, size=100)
    short = rs.randint(0, 256, size=8192)
    p = aecm.default_launch_policy(256)
    p.queue_chunk_blocks, p.queue_chunk_explicit, p.queue_min_streams = 8, 1, 0
    small = rs.randint(0, 201, size=37)
    small[3] = 200
    cases = [(np.full(S, T), cus, clean, None) for cus in (256, 64)
             for S, T, clean in ((8192, 512, False), (65536, 1280, False), (1024, 300, False), (5000, 300, True), (7, 40, False), (cus * 28 + 1, 255, False))]
    cases += [(lens, 256, False, None), (lens[:5000], 256, False, None), (few, 256, False, None), (lens[:1024], 256, False, None),
              (short, 256, False, None), (small, 0, False, p), (np.zeros(5, dtype=np.int64), 256, False, None)]
    for v, cus, clean, pol in cases:
        off = aecm.describe_ragged_launch(v, cus, clean, policy=pol, ragged_pipelining=False)
        assert off == aecm.describe_ragged_launch(v, cus, clean, policy=pol), (v.size, cus, clean)
        lib, d = aecm.load(), ffi.AecmLaunchDescription()
        arr = np.ascontiguousarray(v, dtype=np.int32)
        items, total, longest = C.c_int64(0), C.c_int64(0), C.c_int32(0)
        assert lib.WebRtcAecmBatch_DescribeRaggedLaunchEx(C.byref(pol) if pol is not None else None, cus, arr.size, arr.ctypes.data, 1 if clean else 0, 0,
                                                          C.byref(d), C.byref(items), C.byref(total), C.byref(longest)) == 0
        assert dict(d.as_dict(), items=items.value, sum_blocks=total.value, max_blocks=longest.value) == off, (v.size, cus, clean)
    # on: pipelined
    d = aecm.describe_ragged_launch(lens[:1024], 256, ragged_pipelining=True)
    assert d["form"] == 3 and d["shape"] in UNBALANCED_SHAPES and d["shape"] == aecm.describe_launch_detail(1024, 512, 256)["shape"], d
    assert d["chunk_blocks"] == 0 and d["waves_per_workgroup"] == 16 and d["workgroups_per_cu"] == 2
    d = aecm.describe_ragged_launch(few, 256, ragged_pipelining=True)
    assert d["form"] == 3 and d["shape"] in UNBALANCED_SHAPES and d["workgroups"] <= 100, d
    # a size whose equal-length launch is balanced takes the plain six-wave shape
    assert aecm.describe_launch_detail(4096, 512, 256)["shape"] & 0x100
    d = aecm.describe_ragged_launch(lens[:4096], 256, ragged_pipelining=True)
    assert (d["form"], d["shape"], d["waves_per_workgroup"]) == (3, 0, 6), d
    # on, and still not pipelined
    assert aecm.describe_ragged_launch(lens[:1024], 256, clean=True, ragged_pipelining=True)["form"] == 0                 # a clean input
    tiny = np.where(np.arange(1024) % 2 == 0, 2, 1)
    assert aecm.describe_ragged_launch(tiny, 256, ragged_pipelining=True)["form"] == 0                                    # the longest: two blocks
    assert aecm.describe_ragged_launch(tiny + 1, 256, ragged_pipelining=True)["form"] == 3
    assert aecm.describe_ragged_launch(lens[:4097], 256, ragged_pipelining=True) == aecm.describe_ragged_launch(lens[:4097], 256)      # more live than pipelined_max_streams
    assert aecm.describe_ragged_launch(lens[:4097], 256)["form"] == 2
    q = aecm.default_launch_policy(256)
    q.queue_chunk_blocks = 0                                                                                               # no queue at all: above the pipelined form's limit one wavefront per stream
    d = aecm.describe_ragged_launch(lens[:5000], policy=q, ragged_pipelining=True)
    assert d["form"] in (0, 1) and d == aecm.describe_ragged_launch(lens[:5000], policy=q), d
    d = aecm.describe_ragged_launch(small, policy=p, ragged_pipelining=True)                                             # a lowered queue_min_streams: the queue
    assert (d["form"], d["chunk_blocks"]) == (2, 8), d
    q = aecm.default_launch_policy(256)
    q.pipelined_min_streams = 2000
    assert aecm.describe_ragged_launch(lens[:1024], policy=q, ragged_pipelining=True)["form"] == 0                         # fewer live than pipelined_min_streams
    # all-equal lengths: exactly the equal-length launch
    for S, T in ((1024, 300), (4096, 512), (8192, 512), (7, 40)):
        want = aecm.describe_launch_detail(S, T, 256)
        d = aecm.describe_ragged_launch(np.full(S, T), 256, ragged_pipelining=True)
        assert {k: d[k] for k in want} == want, (S, T, d)


@pytest.mark.parametrize("fs", [16000, 8000])
@pytest.mark.parametrize("deep", [True, False], ids=["sixteen-wave roles", "six-wave roles"])
def test_one_workgroup_of_four_lengths_on_the_lane_simulator(deep, fs):
    """Four slots, lengths 0, 1, 23 and 57 (and permutations of them over the slots): outputs and 24-word digests equal
    OracleStream run to each stream's own length, samples behind a stream's end keep the sentinel, no input row at or beyond a
    stream's length is loaded, an empty slot touches nothing, and every role executes the workgroup's step count."""
    T, sentinel = 57, 0x5A5A
    pairs = [synth_pair(70 + k, T, fs) for k in range(4)]
    far, near = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    for lens in ([57, 0, 1, 23], [1, 57, 23, 0], [23, 1, 0, 57], [0, 0, 5, 0]):
        for order in (0, 1):
            wg = simlib.RoleWorkgroup(fs, [(1, 3)] * 4)
            steps, out = wg.launch(far, near, None, deep, order, lens, sentinel)
            digests, counts = wg.digests(), wg.counts
            assert steps == max(lens) + (4 if deep else 1)
            for k, n in enumerate(lens):
                o = pyoracle.OracleStream(fs, 1, 3)
                exp = o.process(far[k][:n * 64], near[k][:n * 64]) if n else np.zeros(0, np.int16)
                assert np.array_equal(out[k][:n * 64], exp), (lens, order, k)
                assert (out[k][n * 64:] == sentinel).all(), (lens, order, k)
                assert np.array_equal(digests[k], o.digest()), (lens, order, k)
                assert counts[k].tolist() == [n, n, n], (lens, order, k, counts[k])
