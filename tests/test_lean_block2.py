"""The second set of lean forms of the block loop (aecm_wave.h: AECM_LEAN_BLOCK bits 16, 32, 64, 128) on the lane simulator.

The kernel source is built with the policy default on and the switch at 15 (the new bits off: the first set alone), 255 (all on)
and 15 plus each new bit alone; every build must equal OracleStream -- and RefCoreStream where the reference library has been
built -- in output samples and in the 24-word state digest on: 4 streams x 1 100 blocks of the bench signal, a double-talk and a
silent stream, the 8 kHz rate, full scale, runs of -32768, level steps, the adversarial cases of tests/test_lean_block.py (random
echo paths), and echo paths re-initialised to 0 and to negative entries (ch_adapt32 0 and negative, which the NLMS norms special-case).

The new forms are identities for every operand; none adds or removes a data-dependent branch.  What they do have is operands at
which a shortened norm takes its special case, and those are counted (AECM_LEAN_COUNT slots 4, 5 and 7): each must occur and not occur
on these inputs.  Bits 32 (delay estimator keys) and 128 (comfort noise: shifts and adds for two products) have no such operand.

What runs here is host code: bit 16's NormU32 is the restated definition of the instruction (aecm_ops.h: norm_u32_v counts leading
zeros with -1 for 0 and takes the maximum with 0), not the inline v_ffbh_u32, and mul24_insn is the range-checked mul24, not the
intrinsic.  The device forms of those two are covered by tests/test_gpu_lean_block2.py only."""
import ctypes as C
import subprocess
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np
import pytest

import simlib
from helpers import describe_digest_diff
from oracle import pyoracle
from test_lean_block import _signal_cases, bench_pair

_i16p = np.ctypeslib.ndpointer(dtype=np.int16, flags="C_CONTIGUOUS")
_u32p = np.ctypeslib.ndpointer(dtype=np.uint32, flags="C_CONTIGUOUS")
_i64p = np.ctypeslib.ndpointer(dtype=np.int64, flags="C_CONTIGUOUS")
_SOURCES = [simlib.ROOT / "tests" / "sim" / "sim_lib.cpp", simlib.ROOT / "tests" / "sim" / "sim_lean2.cpp", simlib.CSRC / "aecm_host_state.cpp"]
FIRST_SET = 15
NEW_BITS = {16: "NLMS norms", 32: "delay estimator keys", 64: "Wiener gain / NLP norms", 128: "comfort-noise tracking step and amplitude"}
MASKS = [FIRST_SET, FIRST_SET | sum(NEW_BITS)] + [FIRST_SET | b for b in NEW_BITS]
# slot -> (the bit that counts it, what is counted per call of the bin update)
SPECIAL_OPERANDS = {4: (16, "NLMS: an adaptive channel entry is 0 (NormU32's zero case)"),
                    5: (16, "NLMS: a channel-times-far product is 0 (NormU32's zero case)"),
                    7: (64, "Wiener gain: an echo filter entry is 0 (the sign-bit count's -1)")}
_libs = {}


def _lib(mask):
    """tests/_build/libaecm_sim_lean2_<mask>.so: BlockEngine<SimWave, .> with the items of `mask`, with counters."""
    if mask in _libs:
        return _libs[mask]
    so = simlib.SIM_SO.parent / f"libaecm_sim_lean2_{mask}.so"
    deps = _SOURCES + [simlib.ROOT / "tests" / "sim" / "wave_sim.h", simlib.CSRC / "aecm_wave.h", simlib.CSRC / "aecm_ops.h", simlib.CSRC / "aecm_state.h"]
    if not so.exists() or any(so.stat().st_mtime < d.stat().st_mtime for d in deps):
        so.parent.mkdir(parents=True, exist_ok=True)
        obj_dir = so.parent / f".obj_lean2_{mask}"
        obj_dir.mkdir(exist_ok=True)
        flags = ["-O2", "-std=c++17", "-fwrapv", "-fPIC", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", f"-I{simlib.CSRC}",
                 f"-I{simlib.ROOT / 'tests' / 'sim'}", "-DAECM_LEAN_POLICY_DEFAULT=1", f"-DAECM_LEAN_BLOCK={mask}", "-DAECM_LEAN_COUNTERS"]

        def compile_one(src):
            obj = obj_dir / (Path(src).name + ".o")
            subprocess.check_call(["g++", *flags, "-c", str(src), "-o", str(obj)])
            return str(obj)
        with ThreadPoolExecutor(max_workers=len(_SOURCES)) as ex:
            objs = list(ex.map(compile_one, _SOURCES))
        subprocess.check_call(["g++", "-shared", *objs, "-o", str(so)])
    l = C.CDLL(str(so))
    l.sim_create.restype = C.c_void_p
    l.sim_create.argtypes = [C.c_int, C.c_int, C.c_int]
    l.sim_free.argtypes = [C.c_void_p]
    l.sim_set_echo_path.argtypes = [C.c_void_p, _i16p]
    l.sim_process.argtypes = [C.c_void_p, _i16p, _i16p, C.c_void_p, _i16p, C.c_int]
    l.sim_digest.argtypes = [C.c_void_p, _u32p]
    l.sim_lean_counters.argtypes = [_i64p, C.c_int]
    assert l.sim_lean_mask() == mask
    _libs[mask] = l
    return l


def _counters(l, reset=False):
    c = np.zeros((8, 2), dtype=np.int64)
    l.sim_lean_counters(c.reshape(-1), 1 if reset else 0)
    return c


def _run(l, fs, cng, em, far, near, path, launches):
    h = l.sim_create(fs, cng, em)
    assert h
    try:
        if path is not None:
            l.sim_set_echo_path(h, np.ascontiguousarray(path, dtype=np.int16))
        far, near = np.ascontiguousarray(far, dtype=np.int16), np.ascontiguousarray(near, dtype=np.int16)
        out = np.empty_like(near)
        n = near.size // 64
        step = -(-n // launches)
        for b in range(0, n, step):            # several launches: the state goes through store_state / load_state in between
            e = min(n, b + step)
            l.sim_process(h, far[b * 64:e * 64], near[b * 64:e * 64], None, out[b * 64:e * 64], e - b)
        d = np.zeros(24, dtype=np.uint32)
        l.sim_digest(h, d)
        return out, d
    finally:
        l.sim_free(h)


def _cases():
    """(name, fs, cng, echo_mode, far, near, echo path): the cases of tests/test_lean_block.py and the re-initialised echo paths."""
    cases = list(_signal_cases())
    rs = np.random.RandomState(22)
    mixed = rs.choice([0, 0, -1, -32768, -12000, 5, 20000], size=65).astype(np.int16)
    for name, path, seed in (("path_zero", np.zeros(65, np.int16), 7), ("path_negative", np.full(65, -9000, np.int16), 8),
                             ("path_mixed", mixed, 9)):
        for fs in (16000, 8000):
            cases.append((f"{name}_{fs}", fs, 1, 1 if fs == 16000 else 3, *bench_pair(seed, 300, "double_talk" if seed == 8 else "recipe"), path))
    return cases


@pytest.fixture(scope="module")
def expected():
    with_ref = pyoracle.have_reference()
    res = {}
    for name, fs, cng, em, far, near, path in _cases():
        o = pyoracle.OracleStream(fs, cng, em)
        if path is not None:
            o.init_echo_path(path)
        res[name] = (o.process(far, near), o.digest())
        if with_ref:
            r = pyoracle.RefCoreStream(fs, cng, em)
            if path is not None:
                r.init_echo_path(path)
            assert np.array_equal(r.process(far, near), res[name][0]), name
            assert np.array_equal(r.digest(), res[name][1]), (name, describe_digest_diff(r.digest(), res[name][1]))
    return res


@pytest.mark.parametrize("mask", MASKS)
def test_every_subset_of_the_new_bits_equals_the_oracle(mask, expected):
    l = _lib(mask)
    _counters(l, reset=True)
    for i, (name, fs, cng, em, far, near, path) in enumerate(_cases()):
        out, digest = _run(l, fs, cng, em, far, near, path, launches=1 + i % 3)
        exp_out, exp_digest = expected[name]
        assert np.array_equal(out, exp_out), (mask, name, int(np.nonzero(out != exp_out)[0][0]) // 64)
        assert np.array_equal(digest, exp_digest), (mask, name, describe_digest_diff(exp_digest, digest))
    c = _counters(l)
    for slot, (bit, what) in SPECIAL_OPERANDS.items():
        if mask & bit:
            assert c[slot, 0] > 0 and c[slot, 1] > 0, f"slot {slot} ({what}) went one way only: absent {c[slot, 0]}, present {c[slot, 1]}"
        else:
            assert not c[slot].any(), f"slot {slot} counted in a build without bit {bit}"


def test_the_shipped_switch_has_every_item_on():
    from webrtc_aecm_amd import build as B
    text = (B.CSRC / "aecm_wave.h").read_text()
    assert f"#define AECM_LEAN_BLOCK {FIRST_SET | sum(NEW_BITS)}\n" in text
