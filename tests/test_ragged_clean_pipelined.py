"""Pipelined launches for ragged batches with a clean near-end input (WebRtcAecmBatch_SetRaggedCleanPipelining), as far as they
can be shown without a GPU: the C ABI's new symbols and argument errors, the launch rule with the batch's third switch as an
argument, the four ragged clean instantiations in the device assembly with their register bounds, and the hostile clean inputs,
four to a workgroup of four different lengths, through the kernel's role split and its packed hand-over on the lane simulator.
The device side -- and the safe variant, which is a batch's setting -- is tests/test_gpu_ragged_clean_pipelined.py."""
import ctypes as C
import itertools
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import simlib
import webrtc_aecm_amd as aecm
from helpers import adversarial_clean_cases, describe_digest_diff, process_clean
from oracle import pyoracle
from test_ragged_pipelined import _length_vectors
from webrtc_aecm_amd import ffi

ROOT = Path(__file__).resolve().parent.parent
NEW_SYMBOLS = ["WebRtcAecmBatch_SetRaggedCleanPipelining", "WebRtcAecmBatch_DescribeRaggedLaunchEx2"]
CLEAN_BIT = 0x2000
# the shapes that are both ragged and clean shapes: DescribeLaunch's shape bits -> (waves per workgroup, the kernel's <tail, front, delay, gain>)
SHAPES = {0x000: (6, (0, 2, 0, 0)), 0x002: (8, (2, 2, 0, 0)), 0x802: (12, (2, 2, 4, 0)), 0x1a02: (16, (2, 4, 2, 4))}


def _describe_ex2(lens, cus, clean, ragged, ragged_clean, policy=None):
    """WebRtcAecmBatch_DescribeRaggedLaunchEx2 itself (ffi.describe_ragged_launch only calls it with the new argument on)."""
    arr = np.ascontiguousarray(lens, dtype=np.int32)
    d = ffi.AecmLaunchDescription()
    items, total, longest = C.c_int64(0), C.c_int64(0), C.c_int32(0)
    rc = aecm.load().WebRtcAecmBatch_DescribeRaggedLaunchEx2(C.byref(policy) if policy is not None else None, cus, arr.size, arr.ctypes.data,
                                                             1 if clean else 0, 1 if ragged else 0, 1 if ragged_clean else 0, C.byref(d),
                                                             C.byref(items), C.byref(total), C.byref(longest))
    assert rc == 0, rc
    return dict(d.as_dict(), items=items.value, sum_blocks=total.value, max_blocks=longest.value)


def test_new_symbols_are_declared_exported_and_refuse_bad_arguments():
    lib = aecm.load()
    header_text = (ROOT / "include" / "aecm_batch.h").read_text()
    header = re.sub(r"/\*.*?\*/", "", header_text, flags=re.S)
    for name in NEW_SYMBOLS:
        assert name in ffi.BATCH_SYMBOLS and hasattr(lib, name) and re.search(r"\b%s\s*\(" % name, header), name
    assert "do not combine" not in re.sub(r"\s+\*?\s*", " ", header_text)
    assert hasattr(aecm.AecmBatch, "set_ragged_clean_pipelining")
    assert lib.WebRtcAecmBatch_SetRaggedCleanPipelining(None, 1) == ffi.AECM_BAD_PARAMETER_ERROR
    assert lib.WebRtcAecmBatch_SetRaggedCleanPipelining(None, 0) == ffi.AECM_BAD_PARAMETER_ERROR
    lens = np.array([5, 0, 9, 9], dtype=np.int32)
    d = ffi.AecmLaunchDescription()
    describe = lib.WebRtcAecmBatch_DescribeRaggedLaunchEx2
    assert describe(None, 256, 4, lens.ctypes.data, 1, 0, 1, None, None, None, None) == ffi.AECM_NULL_POINTER_ERROR
    assert describe(None, 256, 4, None, 1, 0, 1, C.byref(d), None, None, None) == ffi.AECM_NULL_POINTER_ERROR
    assert describe(None, 256, 0, lens.ctypes.data, 1, 0, 1, C.byref(d), None, None, None) == ffi.AECM_BAD_PARAMETER_ERROR
    assert describe(None, 0, 4, lens.ctypes.data, 1, 0, 1, C.byref(d), None, None, None) == ffi.AECM_BAD_PARAMETER_ERROR
    bad = np.array([3, -1, 2, 2], dtype=np.int32)
    assert describe(None, 256, 4, bad.ctypes.data, 1, 0, 1, C.byref(d), None, None, None) == ffi.AECM_BAD_PARAMETER_ERROR
    q = aecm.default_launch_policy(256)
    q.struct_size = 8
    assert describe(C.byref(q), 0, 4, lens.ctypes.data, 1, 0, 1, C.byref(d), None, None, None) == ffi.AECM_BAD_PARAMETER_ERROR
    assert describe(None, 256, 4, lens.ctypes.data, 1, 0, 1, C.byref(d), None, None, None) == 0 and d.form == 3 and d.shape & CLEAN_BIT
    assert describe(None, 256, 4, lens.ctypes.data, 1, 1, 0, C.byref(d), None, None, None) == 0 and d.form == 0 and d.shape == 0
    # the module-level call: the keyword comes last and is off by default
    assert aecm.describe_ragged_launch(lens, 256, True, None, True)["form"] == 0
    assert aecm.describe_ragged_launch(lens, 256, True, ragged_clean_pipelining=True)["form"] == 3


@pytest.mark.parametrize("cus", [64, 256, 304])
def test_launch_rule_without_a_device(cus):
    """New argument 0: DescribeRaggedLaunchEx2 is DescribeRaggedLaunchEx, with and without a clean input and whatever the second
    switch says.  New argument 1: a ragged launch with a clean input whose LIVE streams the chip holds at once is form 3 in one of
    the four shapes with bit 0x2000, its workgroups those of the plan; a launch without a clean input is what it was; too few
    live streams, too short, too many live streams (the queue, or one wavefront per stream without a queue) are not form 3; all
    lengths equal is the equal-length launch under ITS rule."""
    vectors = _length_vectors()
    for (name, v), clean, ragged in itertools.product(vectors, (False, True), (False, True)):
        want = aecm.describe_ragged_launch(v, cus, clean, ragged_pipelining=ragged)
        assert _describe_ex2(v, cus, clean, ragged, False) == want, (name, clean, ragged)
        on = _describe_ex2(v, cus, clean, ragged, True)
        if not clean:
            assert on == want, (name, ragged)                            # without a clean input the switch changes nothing
            continue
        assert want["form"] != 3, (name, want)                            # the other two switches never pipeline such a launch
        live, longest = int((v > 0).sum()), int(v.max())
        if live < 2 or live > 16 * cus or longest < 3:
            assert on == want, (name, on, want)
            continue
        assert on["form"] == 3 and on["chunk_blocks"] == 0 and on["shape"] & CLEAN_BIT, (name, on)
        bits = on["shape"] & ~CLEAN_BIT
        n_wg = -(-live // 4)
        assert bits == (0x1a02 if n_wg <= 2 * cus else 0x002 if n_wg <= 3 * cus else 0x000), (name, on)
        assert on["waves_per_workgroup"] == SHAPES[bits][0] and on["workgroups_per_cu"] == {0x1a02: 2, 0x002: 3, 0x000: 4}[bits], (name, on)
        assert n_wg <= on["workgroups"] <= min(live, on["workgroups_per_cu"] * cus), (name, on)
        assert (on["items"], on["sum_blocks"], on["max_blocks"]) == (0, int(v.sum()), longest), (name, on)
        assert 0 < on["cu_load_evenness_x1000"] <= 1000, (name, on)
        # the plan, and with it the grid and the evenness, is the one of the same shape without a clean input
        p = aecm.default_launch_policy(cus)
        tail, front, delay, gain = SHAPES[bits][1]
        p.pipe_tail_waves, p.pipe_front_waves, p.pipe_raw, p.pipe_delay_waves, p.pipe_gain_waves = tail, front, 0, delay, gain
        same = aecm.describe_ragged_launch(v, policy=p, ragged_pipelining=True)
        assert same["shape"] == bits and {k: x for k, x in on.items() if k != "shape"} == {k: x for k, x in same.items() if k != "shape"}, (name, on, same)
        assert aecm.describe_ragged_launch(v, cus, True, ragged_pipelining=ragged, ragged_clean_pipelining=True) == on, name
    # every combination of wishes lands on a carried shape, never on a launch error
    rs = np.random.RandomState(cus)
    sizes = [np.array([5, 9]), np.r_[0, rs.randint(1, 41, size=36)], rs.randint(1, 513, size=6 * cus + 1), rs.randint(1, 129, size=12 * cus),
             np.r_[rs.randint(1, 2049, size=16 * cus), np.zeros(50, dtype=np.int64)]]
    for tail, front, raw, delay, gain in itertools.product((-1, 0, 2), (-1, 2, 4), (-1, 0, 1), (-1, 0, 2, 4), (-1, 0, 4)):
        p = aecm.default_launch_policy(cus)
        p.pipelined_min_streams, p.pipelined_min_blocks = 1, 1
        p.pipe_tail_waves, p.pipe_front_waves, p.pipe_raw, p.pipe_delay_waves, p.pipe_gain_waves = tail, front, raw, delay, gain
        for v in sizes:
            d = aecm.describe_ragged_launch(v, policy=p, clean=True, ragged_clean_pipelining=True)
            live = int((v > 0).sum())
            assert d["form"] == 3 and d["shape"] in {0x2000, 0x2002, 0x2802, 0x3a02}, (tail, front, raw, delay, gain, v.size, d)
            assert d["waves_per_workgroup"] == SHAPES[d["shape"] & ~CLEAN_BIT][0], (tail, front, raw, delay, gain, v.size, d)
            assert -(-live // 4) <= d["workgroups"] <= live, (tail, front, raw, delay, gain, v.size, d)
            assert aecm.describe_ragged_launch(v, policy=p, clean=True, ragged_pipelining=True)["form"] != 3
    # switch on, and still not form 3
    lens = rs.randint(128, 513, size=16 * cus + 1)
    lens[0] = 512
    inside = lens[:4 * cus]
    assert aecm.describe_ragged_launch(inside, cus, True, ragged_clean_pipelining=True)["form"] == 3
    q = aecm.default_launch_policy(cus)
    q.pipelined_min_streams = 4 * cus + 1                                   # fewer live streams than pipelined_min_streams
    assert aecm.describe_ragged_launch(inside, policy=q, clean=True, ragged_clean_pipelining=True) == aecm.describe_ragged_launch(inside, policy=q, clean=True)
    q.pipelined_min_streams = 4 * cus - 9
    with_zeros = inside.copy()
    with_zeros[10:20] = 0                                                   # (by the LIVE streams, not the batch's size)
    assert aecm.describe_ragged_launch(inside, policy=q, clean=True, ragged_clean_pipelining=True)["form"] == 3
    assert aecm.describe_ragged_launch(with_zeros, policy=q, clean=True, ragged_clean_pipelining=True)["form"] == 0
    tiny = np.where(np.arange(4 * cus) % 2 == 0, 2, 1)                      # the longest below pipelined_min_blocks
    assert aecm.describe_ragged_launch(tiny, cus, True, ragged_clean_pipelining=True)["form"] == 0
    assert aecm.describe_ragged_launch(tiny + 1, cus, True, ragged_clean_pipelining=True)["form"] == 3
    d = aecm.describe_ragged_launch(lens, cus, True, ragged_clean_pipelining=True)        # more live streams than the limit: the queue
    assert d["form"] == 2 and d == aecm.describe_ragged_launch(lens, cus, True), d
    q = aecm.default_launch_policy(cus)
    q.queue_chunk_blocks = 0                                                # ... or, without a queue, one wavefront per stream
    d = aecm.describe_ragged_launch(lens, policy=q, clean=True, ragged_clean_pipelining=True)
    assert d["form"] in (0, 1) and d == aecm.describe_ragged_launch(lens, policy=q, clean=True), d
    q = aecm.default_launch_policy(cus)
    q.queue_chunk_blocks, q.queue_chunk_explicit, q.queue_min_streams = 8, 1, 0      # a lowered queue threshold: the queue takes the launch
    d = aecm.describe_ragged_launch(inside, policy=q, clean=True, ragged_clean_pipelining=True)
    assert (d["form"], d["chunk_blocks"]) == (2, 8), d
    # all lengths equal: the equal-length launch, by SetCleanPipelining's rule and not by this switch
    for S, T in ((4 * cus, 300), (16 * cus, 512), (32 * cus, 512), (7, 40)):
        want = aecm.describe_launch_detail(S, T, cus, True)
        d = aecm.describe_ragged_launch(np.full(S, T), cus, True, ragged_pipelining=True, ragged_clean_pipelining=True)
        assert want["form"] != 3 and {k: d[k] for k in want} == want, (S, T, d)
    assert C.sizeof(ffi.AecmLaunchPolicy) == 76


def test_the_four_ragged_clean_instantiations_in_the_device_assembly(tmp_path):
    """Present, within the register bounds their residency needs (72 VGPRs for seven waves per SIMD; the sixteen-wave shape, two
    workgroups per CU = eight waves per SIMD: 64 VGPRs and 80 SGPRs), no scratch, workgroup barriers only."""
    from webrtc_aecm_amd import build
    src = "aecm_block_kernels.hip"
    flags = [f for f in build.HIPCC_FLAGS if f not in ("-shared", "-fPIC")]
    out = tmp_path / (src + ".s")
    subprocess.check_call([build._hipcc(), *flags, *build.SOURCE_FLAGS.get(src, []), "-S", "--cuda-device-only", f"-I{build.CSRC}",
                           str(build.CSRC / src), "-o", str(out)], stderr=subprocess.DEVNULL)
    text = out.read_text()
    sgpr_counts = {}
    for block in re.split(r"\n\s*- \.agpr_count:", text)[1:]:
        sgpr_counts[re.search(r"\.name:\s+(\S+)", block).group(1)] = int(re.search(r"\.sgpr_count:\s+(\d+)", block).group(1))
    found = re.findall(r"^(_ZN4aecm42aecm_process_pipelined_ragged_clean_kernelI\w+):", text, re.M)
    assert len(set(found)) == 4, found
    for bits, (waves, (tail, front, delay, gain)) in SHAPES.items():
        m = re.search(r"^(_ZN4aecm42aecm_process_pipelined_ragged_clean_kernelILi%dELb0ELb0ELi%dELi%dELi%dEEE\w*):.*\n" % (tail, front, delay, gain),
                      text, re.M)
        assert m, f"ragged clean pipelined kernel of shape {bits:#x} not found in the device assembly"
        body = text[m.end():]
        body = body[:body.index(".end_amdhsa_kernel")]
        vgprs = int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", body).group(1))
        sgprs = max(int(re.search(r"\.amdhsa_next_free_sgpr (\d+)", body).group(1)), sgpr_counts[m.group(1)])
        lds = int(re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", body).group(1))
        print(f"shape {bits:#x}: {vgprs} VGPRs, {sgprs} SGPRs, {lds} bytes of static LDS")
        assert not re.search(r"^\s*scratch_(load|store)", body, re.M), bits
        assert vgprs <= 72, (bits, vgprs)
        if waves == 16:
            assert vgprs <= 64 and sgprs <= 80, (bits, vgprs, sgprs)
        assert len(re.findall(r"^\s*s_barrier", body, re.M)) >= 4 and not re.search(r"^\s*s_sleep", body, re.M), bits


@pytest.mark.parametrize("fs", [16000, 8000])
@pytest.mark.parametrize("order", [0, 1], ids=["consumers first", "producers first"])
@pytest.mark.parametrize("deep", [True, False], ids=["sixteen-wave roles", "six-wave roles"])
def test_hostile_clean_inputs_in_four_lengths_on_the_lane_simulator(deep, order, fs):
    """The 20 cases of helpers.adversarial_clean_cases at this rate, four to a workgroup, as slots of lengths 0, 1, 23 and 57 and
    then -- continuing -- of 57, 23, 0 and 1: outputs up to each slot's own length, the sentinel behind it, no hand-over slot,
    output block or input row beyond it, and 24-word digests after each launch (c_old of a slot that ended before its workgroup
    did included) equal OracleStream.process_block_clean.  (The workgroup starts from the default echo path.)"""
    L, sentinel = 57, 0x5A5A
    cases = [c for c in adversarial_clean_cases(2 * L) if c["fs"] == fs]
    assert len(cases) == 20
    for g in range(0, 20, 4):
        grp = cases[g:g + 4]
        cfgs = [(c["cng"], c["echo_mode"]) for c in grp]
        wg = simlib.RoleWorkgroup(fs, cfgs)
        oracles = [pyoracle.OracleStream(fs, *cfg) for cfg in cfgs]
        at = [0, 0, 0, 0]
        for lens in ((0, 1, 23, 57), (57, 23, 0, 1)):
            f, n, c = (np.stack([grp[k][x][at[k] * 64:(at[k] + L) * 64] for k in range(4)]) for x in ("far", "near", "clean"))
            steps, out = wg.launch(f, n, c, deep, order, lens, sentinel)
            assert steps == max(lens) + (4 if deep else 1)
            digests = wg.digests()
            for k, o in enumerate(oracles):
                what = (g + k, grp[k]["kind"], grp[k]["base"], lens)
                exp = process_clean(o, f[k], n[k], c[k], 0, lens[k])
                bad = np.nonzero((out[k][:lens[k] * 64] != exp).reshape(-1, 64).any(axis=1))[0]
                assert bad.size == 0, (*what, int(bad[0]))
                assert (out[k][lens[k] * 64:] == sentinel).all(), what
                assert np.array_equal(digests[k], o.digest()), (*what, describe_digest_diff(digests[k], o.digest()))
                assert wg.counts[k].tolist() == [lens[k]] * 3, (*what, wg.counts[k])
                at[k] += lens[k]
