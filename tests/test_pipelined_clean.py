"""Pipelined launches for batches with a clean near-end input (WebRtcAecmBatch_SetCleanPipelining), as far as they can be shown
without a GPU: the C ABI's new symbols, the launch rule with the batch's opt-in as an argument, the four clean instantiations in
the device assembly with their register bounds, and one workgroup of four streams through the kernel's role split and its packed
hand-over on the lane simulator -- clean, then no clean, then clean again.  The device side is tests/test_gpu_pipelined_clean.py."""
import ctypes as C
import itertools
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import simlib
import webrtc_aecm_amd as aecm
from helpers import adversarial_clean_cases, describe_digest_diff, process_clean, stream_config
from oracle import pyoracle
from webrtc_aecm_amd import ffi
from webrtc_aecm_amd.synth import synth_clean, synth_pair

ROOT = Path(__file__).resolve().parent.parent
NEW_SYMBOLS = ["WebRtcAecmBatch_SetCleanPipelining", "WebRtcAecmBatch_DescribeLaunchDetailEx"]
CLEAN_BIT = 0x2000
# the shapes the clean kernel is carried in: DescribeLaunch's shape bits -> (waves per workgroup, the kernel's <tail, front, delay, gain>)
CLEAN_SHAPES = {0x000: (6, (0, 2, 0, 0)), 0x002: (8, (2, 2, 0, 0)), 0x802: (12, (2, 2, 4, 0)), 0x1a02: (16, (2, 4, 2, 4))}


def test_new_symbols_are_declared_exported_and_refuse_bad_arguments():
    lib = aecm.load()
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "aecm_batch.h").read_text(), flags=re.S)
    for name in NEW_SYMBOLS:
        assert name in ffi.BATCH_SYMBOLS and hasattr(lib, name) and re.search(r"\b%s\s*\(" % name, header), name
    assert lib.WebRtcAecmBatch_SetCleanPipelining(None, 1) == ffi.AECM_BAD_PARAMETER_ERROR
    assert lib.WebRtcAecmBatch_SetCleanPipelining(None, 0) == ffi.AECM_BAD_PARAMETER_ERROR
    d = ffi.AecmLaunchDescription()
    describe = lib.WebRtcAecmBatch_DescribeLaunchDetailEx
    assert describe(None, 256, 1024, 300, 1, 1, None) == ffi.AECM_NULL_POINTER_ERROR
    assert describe(None, 0, 1024, 300, 1, 1, C.byref(d)) == ffi.AECM_BAD_PARAMETER_ERROR
    assert describe(None, 256, 0, 300, 1, 1, C.byref(d)) == ffi.AECM_BAD_PARAMETER_ERROR
    assert describe(None, 256, 1024, 0, 1, 1, C.byref(d)) == ffi.AECM_BAD_PARAMETER_ERROR
    q = aecm.default_launch_policy(256)
    q.struct_size = 8
    assert describe(C.byref(q), 0, 1024, 300, 1, 1, C.byref(d)) == ffi.AECM_BAD_PARAMETER_ERROR
    assert describe(None, 256, 1024, 300, 1, 1, C.byref(d)) == 0 and d.form == 3 and d.shape & CLEAN_BIT
    assert describe(None, 256, 1024, 300, 1, 0, C.byref(d)) == 0 and d.form == 0 and d.shape == 0


@pytest.mark.parametrize("cus", [256, 304, 64])
def test_launch_rule_without_a_device(cus):
    """Switch off: DescribeLaunchDetailEx is DescribeLaunchDetail.  Switch on: a launch with a clean input that the chip holds at
    once is pipelined in the shape its size gives (sixteen waves up to two workgroups of four per CU, eight up to three, six
    above), with bit 0x2000; below three blocks one wavefront per stream; above pipelined_max_streams the chunk queue; a launch
    without a clean input is what it was; and whatever the pipe_* wishes say, the shape is one the clean kernel is carried in."""
    sizes = [1, 2, 5, 37, 4 * cus, 4 * cus + 1, 8 * cus - 3, 8 * cus, 8 * cus + 1, 12 * cus, 12 * cus + 1, 16 * cus - 1, 16 * cus, 16 * cus + 1,
             28 * cus + 1, 65536]
    for S, T, clean in itertools.product(sizes, (1, 2, 3, 40, 512, 2048), (False, True)):
        assert aecm.describe_launch_detail(S, T, cus, clean, clean_pipelining=False) == aecm.describe_launch_detail(S, T, cus, clean), (S, T, clean)
        lib, d = aecm.load(), ffi.AecmLaunchDescription()
        assert lib.WebRtcAecmBatch_DescribeLaunchDetailEx(None, cus, S, T, 1 if clean else 0, 0, C.byref(d)) == 0
        assert d.as_dict() == aecm.describe_launch_detail(S, T, cus, clean), (S, T, clean)
        # without a clean input the switch changes nothing
        assert aecm.describe_launch_detail(S, T, cus, False, clean_pipelining=True) == aecm.describe_launch_detail(S, T, cus, False), (S, T)
        off = aecm.describe_launch_detail(S, T, cus, True)
        assert off["form"] != 3, (S, T, off)                              # the default: a clean input is never pipelined
        on = aecm.describe_launch_detail(S, T, cus, True, clean_pipelining=True)
        n_wg = -(-S // 4)
        if S < 2 or S > 16 * cus or T < 3:
            assert on == off, (S, T, on, off)
            if S > 16 * cus and T >= 512:
                assert on["form"] == 2, (S, T, on)
            if T < 3 and S <= 16 * cus:
                assert on["form"] == 0, (S, T, on)
            continue
        bits = 0x1a02 if n_wg <= 2 * cus else 0x002 if n_wg <= 3 * cus else 0x000
        assert (on["form"], on["shape"], on["chunk_blocks"]) == (3, bits | CLEAN_BIT, 0), (S, T, on)
        assert on["waves_per_workgroup"] == CLEAN_SHAPES[bits][0], (S, T, on)
        assert on["workgroups_per_cu"] == {0x1a02: 2, 0x002: 3, 0x000: 4}[bits], (S, T, on)
        assert n_wg <= on["workgroups"] <= min(S, on["workgroups_per_cu"] * cus), (S, T, on)
        # the grid and its quantisation are those of the same shape without a clean input
        p = aecm.default_launch_policy(cus)
        tail, front, delay, gain = CLEAN_SHAPES[bits][1]
        p.pipe_tail_waves, p.pipe_front_waves, p.pipe_raw, p.pipe_delay_waves, p.pipe_gain_waves = tail, front, 0, delay, gain
        same = aecm.describe_launch_detail(S, T, policy=p)
        assert same["shape"] == bits and {k: v for k, v in on.items() if k != "shape"} == {k: v for k, v in same.items() if k != "shape"}, (S, T, on, same)
    # every combination of wishes lands on a carried shape
    for tail, front, raw, delay, gain in itertools.product((-1, 0, 2), (-1, 2, 4), (-1, 0, 1), (-1, 0, 2, 4), (-1, 0, 4)):
        p = aecm.default_launch_policy(cus)
        p.pipelined_min_streams, p.pipelined_min_blocks = 1, 1
        p.pipe_tail_waves, p.pipe_front_waves, p.pipe_raw, p.pipe_delay_waves, p.pipe_gain_waves = tail, front, raw, delay, gain
        for S, T in ((1, 1), (3, 40), (4 * cus, 40), (6 * cus + 1, 512), (10 * cus, 2048), (12 * cus, 128), (13 * cus, 40), (16 * cus, 2048)):
            d = aecm.describe_launch_detail(S, T, policy=p, clean=True, clean_pipelining=True)
            assert d["form"] == 3 and d["shape"] & CLEAN_BIT, (tail, front, raw, delay, gain, S, T, d)
            bits = d["shape"] & ~CLEAN_BIT
            assert bits in CLEAN_SHAPES and d["waves_per_workgroup"] == CLEAN_SHAPES[bits][0], (tail, front, raw, delay, gain, S, T, d)
            assert -(-S // 4) <= d["workgroups"] <= max(S, 1) and d["workgroups"] <= d["workgroups_per_cu"] * cus, (tail, front, raw, delay, gain, S, T, d)
            assert aecm.describe_launch_detail(S, T, policy=p, clean=True)["form"] != 3
    # the policy struct is what it was: the switch is the batch's, not the policy's
    assert C.sizeof(ffi.AecmLaunchPolicy) == 19 * 4


def test_the_four_clean_instantiations_in_the_device_assembly(tmp_path):
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
    found = re.findall(r"^(_ZN4aecm35aecm_process_pipelined_clean_kernelI\w+):", text, re.M)
    assert len(set(found)) == 4, found
    for bits, (waves, (tail, front, delay, gain)) in CLEAN_SHAPES.items():
        m = re.search(r"^(_ZN4aecm35aecm_process_pipelined_clean_kernelILi%dELb0ELb0ELi%dELi%dELi%dEEE\w*):.*\n" % (tail, front, delay, gain), text, re.M)
        assert m, f"clean pipelined kernel of shape {bits:#x} not found in the device assembly"
        body = text[m.end():]
        body = body[:body.index(".end_amdhsa_kernel")]
        vgprs = int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", body).group(1))
        sgprs = max(int(re.search(r"\.amdhsa_next_free_sgpr (\d+)", body).group(1)), sgpr_counts[m.group(1)])
        print(f"shape {bits:#x}: {vgprs} VGPRs, {sgprs} SGPRs")
        assert not re.search(r"^\s*scratch_(load|store)", body, re.M), bits
        assert vgprs <= 72, (bits, vgprs)
        if waves == 16:
            assert vgprs <= 64 and sgprs <= 80, (bits, vgprs, sgprs)
        assert len(re.findall(r"^\s*s_barrier", body, re.M)) >= 4 and not re.search(r"^\s*s_sleep", body, re.M), bits


def _clean_of(near, k, far):
    """A clean input per stream: the stock 3/4 of the near end, or a much quieter mix with a Q domain of its own."""
    if k % 2 == 0:
        return synth_clean(near)
    return (near.astype(np.int32) // 7 + np.roll(far, 5).astype(np.int32) // 19).astype(np.int16)


@pytest.mark.parametrize("fs", [16000, 8000])
@pytest.mark.parametrize("order", [0, 1], ids=["consumers first", "producers first"])
@pytest.mark.parametrize("deep", [True, False], ids=["sixteen-wave roles", "six-wave roles"])
def test_one_workgroup_with_a_clean_input_on_the_lane_simulator(deep, order, fs):
    """Four streams of mixed configurations through three launches on one workgroup -- 44 blocks with a clean input, 9 without
    (c_old must survive them untouched), 41 with one again (whose first block's window starts with the clean samples the FIRST
    launch ended on): outputs block for block and 24-word digests after every launch equal OracleStream's."""
    lens = (44, 9, 41)
    T = sum(lens)
    cfgs = [stream_config(s) for s in (0, 3, 6, 9)]
    pairs = [synth_pair(210 + k, T, fs) for k in range(4)]
    far, near = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    clean = np.stack([_clean_of(near[k], k, far[k]) for k in range(4)])
    wg = simlib.RoleWorkgroup(fs, cfgs)
    oracles = [pyoracle.OracleStream(fs, *cfg) for cfg in cfgs]
    at = 0
    for n, with_clean in zip(lens, (True, False, True)):
        sl = slice(at * 64, (at + n) * 64)
        steps, out = wg.launch(far[:, sl], near[:, sl], clean[:, sl] if with_clean else None, deep, order)
        assert steps == n + (4 if deep else 1)
        digests = wg.digests()
        for k, o in enumerate(oracles):
            for b in range(at, at + n):
                blk = slice(b * 64, (b + 1) * 64)
                exp = o.process_block_clean(far[k][blk], near[k][blk], clean[k][blk]) if with_clean else o.process(far[k][blk], near[k][blk])
                assert np.array_equal(out[k][(b - at) * 64:(b - at + 1) * 64], exp), (deep, order, fs, k, b)
            assert np.array_equal(digests[k], o.digest()), (deep, order, fs, k, at)
        at += n


@pytest.mark.parametrize("fs", [16000, 8000])
@pytest.mark.parametrize("order", [0, 1], ids=["consumers first", "producers first"])
@pytest.mark.parametrize("deep", [True, False], ids=["sixteen-wave roles", "six-wave roles"])
def test_hostile_clean_inputs_on_the_lane_simulator(deep, order, fs):
    """The 20 cases of helpers.adversarial_clean_cases at this rate, four to a workgroup, through launches of 70 blocks with the
    clean input, 9 without and 81 with it again: the clean spectrum shares the hand-over's words with the far and near
    magnitudes (pack_clean_hand_over), so a clean input that is no scaled copy of the near end is what can tell a packing
    error from a correct one.  Outputs block for block and 24-word digests after every launch equal OracleStream's.  (The
    workgroup starts from the default echo path: a case's own path is not loaded here.)"""
    lens = (70, 9, 81)
    cases = [c for c in adversarial_clean_cases(sum(lens)) if c["fs"] == fs]
    assert len(cases) == 20
    for g in range(0, 20, 4):
        grp = cases[g:g + 4]
        cfgs = [(c["cng"], c["echo_mode"]) for c in grp]
        far, near, clean = (np.stack([c[k] for c in grp]) for k in ("far", "near", "clean"))
        wg = simlib.RoleWorkgroup(fs, cfgs)
        oracles = [pyoracle.OracleStream(fs, *cfg) for cfg in cfgs]
        at = 0
        for n, with_clean in zip(lens, (True, False, True)):
            sl = slice(at * 64, (at + n) * 64)
            steps, out = wg.launch(far[:, sl], near[:, sl], clean[:, sl] if with_clean else None, deep, order)
            assert steps == n + (4 if deep else 1)
            digests = wg.digests()
            for k, o in enumerate(oracles):
                exp = process_clean(o, far[k], near[k], clean[k], at, at + n) if with_clean else o.process(far[k][sl], near[k][sl])
                bad = np.nonzero((out[k] != exp).reshape(-1, 64).any(axis=1))[0]
                assert bad.size == 0, (g + k, grp[k]["kind"], grp[k]["base"], at + int(bad[0]))
                assert np.array_equal(digests[k], o.digest()), (g + k, grp[k]["kind"], grp[k]["base"], at, describe_digest_diff(digests[k], o.digest()))
            at += n


@pytest.mark.parametrize("fs", [16000, 8000])
@pytest.mark.parametrize("order", [0, 1], ids=["consumers first", "producers first"])
@pytest.mark.parametrize("deep", [True, False], ids=["sixteen-wave roles", "six-wave roles"])
def test_four_lengths_with_a_clean_input_on_the_lane_simulator(deep, order, fs):
    """Both conditions of the simulator's role split at once: four slots of lengths 0, 1, 23 and 57 AND a clean input (one that
    is no scaled copy of the near end), in two launches that continue each other, the lengths dealt to other slots in the
    second.  NO KERNEL HAS THIS FORM YET -- a ragged launch with a clean input is not pipelined -- so this pins down what such a
    kernel's role split has to compute: outputs up to each stream's own length, the sentinel behind it, and 24-word digests
    after each launch (c_old of a stream that ended before the workgroup did included) equal OracleStream.process_block_clean."""
    L, sentinel = 57, 0x5A5A
    cfgs = [stream_config(s) for s in (0, 3, 6, 9)]
    pairs = [synth_pair(310 + k, 2 * L, fs) for k in range(4)]
    far, near = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    clean = np.stack([_clean_of(near[k], 1, far[k]) for k in range(4)])
    wg = simlib.RoleWorkgroup(fs, cfgs)
    oracles = [pyoracle.OracleStream(fs, *cfg) for cfg in cfgs]
    at = [0, 0, 0, 0]
    for lens in ((0, 1, 23, 57), (57, 23, 0, 1)):
        f, n, c = (np.stack([x[k][at[k] * 64:(at[k] + L) * 64] for k in range(4)]) for x in (far, near, clean))
        steps, out = wg.launch(f, n, c, deep, order, lens, sentinel)
        assert steps == max(lens) + (4 if deep else 1)
        digests = wg.digests()
        for k, o in enumerate(oracles):
            for b in range(lens[k]):
                blk = slice(b * 64, (b + 1) * 64)
                assert np.array_equal(out[k][blk], o.process_block_clean(f[k][blk], n[k][blk], c[k][blk])), (lens, k, b)
            assert (out[k][lens[k] * 64:] == sentinel).all(), (lens, k)
            assert np.array_equal(digests[k], o.digest()), (lens, k, describe_digest_diff(digests[k], o.digest()))
            assert wg.counts[k].tolist() == [lens[k]] * 3, (lens, k, wg.counts[k])
            at[k] += lens[k]
