"""TEST INFRASTRUCTURE: build + bind tests/_build/libaecm_inject.so -- tests/sim/sim_inject.cpp, the product's block DSP on the lane
simulator started from a caller's state image, with the claims of aecm_ops.h (as_i16 / as_nonneg / mul24 / shift counts) checked
and reported instead of aborting.  A library of its own: it defines the aecm_*_violation hooks itself, so it is never linked with
tests/_build/libaecm_sim.so."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

import simlib

SRC = simlib.ROOT / "tests" / "sim" / "sim_inject.cpp"
MAIN = simlib.ROOT / "tests" / "sim" / "inject_main.cpp"
SO = simlib.ROOT / "tests" / "_build" / "libaecm_inject.so"
SAN_EXE = simlib.ROOT / "tests" / "_build" / "inject_main_san"
_DEPS = [SRC, SRC.parent / "wave_sim.h", simlib.CSRC / "aecm_wave.h", simlib.CSRC / "aecm_ops.h", simlib.CSRC / "aecm_state.h",
         simlib.CSRC / "aecm_state_check.h", simlib.CSRC / "aecm_tables.h"]
_FLAGS = ["-std=c++17", "-fwrapv", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", f"-I{simlib.CSRC}", f"-I{simlib.ROOT / 'tests' / 'sim'}"]
KINDS = {0: None, 1: "mul24", 2: "as_i16", 3: "shift count", 4: "as_nonneg"}
VEC_WORDS, SCAL_WORDS, HIST_WORDS = 12 * 64, 64, 100 * 64
_lib = None


def _stale(target, deps):
    return not target.exists() or any(target.stat().st_mtime < d.stat().st_mtime for d in deps)


def build():
    if not _stale(SO, _DEPS):
        return
    SO.parent.mkdir(parents=True, exist_ok=True)
    tmp = SO.with_suffix(f".{os.getpid()}.tmp")
    subprocess.check_call(["g++", "-O2", "-fPIC", *_FLAGS, "-shared", str(SRC), "-o", str(tmp)])
    os.replace(tmp, SO)


def build_sanitized_program():
    """tests/sim/inject_main.cpp + sim_inject.cpp as a program of its own under AddressSanitizer and UndefinedBehaviorSanitizer."""
    if _stale(SAN_EXE, _DEPS + [MAIN]):
        SAN_EXE.parent.mkdir(parents=True, exist_ok=True)
        tmp = SAN_EXE.with_suffix(f".{os.getpid()}.tmp")
        subprocess.check_call(["g++", *simlib.SAN_FLAGS, *_FLAGS, str(MAIN), str(SRC), "-o", str(tmp)])
        os.replace(tmp, SAN_EXE)
    return SAN_EXE


def lib():
    global _lib
    if _lib is None:
        build()
        l = C.CDLL(str(SO))
        vp = C.c_void_p
        l.sim_inject_run.argtypes = [vp, vp, vp, vp, vp, vp, C.c_int, vp, vp]
        l.sim_inject_run_many.argtypes = [C.c_int, vp, vp, vp, vp, vp, vp, vp, vp, C.c_int, vp, vp, vp]
        l.sim_inject_validate.restype = C.c_char_p
        l.sim_inject_validate.argtypes = [vp, vp, C.c_int]
        _lib = l
    return _lib


def validate(vec, scal, fs):
    """The product's verdict (aecm_state_check.h: StateImageDefect): None = admitted, else the defect's name."""
    vec = np.ascontiguousarray(vec, dtype=np.uint32)
    scal = np.ascontiguousarray(scal, dtype=np.int32)
    assert vec.size == VEC_WORDS and scal.size == SCAL_WORDS
    r = lib().sim_inject_validate(vec.ctypes.data, scal.ctypes.data, int(fs))
    return None if r is None else r.decode()


def run(vec, scal, hist, far, near, clean=None):
    """One launch of far.size // 64 blocks on the image, which is updated in place (the three arrays must be contiguous and of the
    image's types).  Returns (kind or None, out)."""
    for a, t, n in ((vec, np.uint32, VEC_WORDS), (scal, np.int32, SCAL_WORDS), (hist, np.uint16, HIST_WORDS)):
        assert a.dtype == t and a.size == n and a.flags.c_contiguous and a.flags.writeable
    far, near = np.ascontiguousarray(far, dtype=np.int16), np.ascontiguousarray(near, dtype=np.int16)
    if clean is not None:
        clean = np.ascontiguousarray(clean, dtype=np.int16)
    out = np.zeros_like(near)
    value = np.zeros(1, np.int32)
    kind = lib().sim_inject_run(vec.ctypes.data, scal.ctypes.data, hist.ctypes.data, far.ctypes.data, near.ctypes.data,
                                None if clean is None else clean.ctypes.data, far.size // 64, out.ctypes.data, value.ctypes.data)
    return (None if kind == 0 else f"{KINDS[kind]} ({int(value[0])})"), out


def run_many(vec, scal, hist, far, near, clean, has_clean, lens):
    """n states ([n, ...] arrays, updated in place) through launches of lens blocks each, audio rows [n, sum(lens) * 64].
    Returns (kinds int32[n] -- 0 = no claim violated --, values int32[n], out)."""
    n = vec.shape[0]
    lens = np.ascontiguousarray(lens, dtype=np.int32)
    total = int(lens.sum())
    for a, t, w in ((vec, np.uint32, VEC_WORDS), (scal, np.int32, SCAL_WORDS), (hist, np.uint16, HIST_WORDS)):
        assert a.dtype == t and a.shape == (n, w) and a.flags.c_contiguous and a.flags.writeable
    for a in (far, near, clean):
        assert a.dtype == np.int16 and a.shape == (n, total * 64) and a.flags.c_contiguous
    has_clean = np.ascontiguousarray(has_clean, dtype=np.uint8)
    assert has_clean.shape == (n,)
    out = np.zeros_like(near)
    kinds, values = np.zeros(n, np.int32), np.zeros(n, np.int32)
    lib().sim_inject_run_many(n, vec.ctypes.data, scal.ctypes.data, hist.ctypes.data, far.ctypes.data, near.ctypes.data, clean.ctypes.data,
                              has_clean.ctypes.data, lens.ctypes.data, lens.size, out.ctypes.data, kinds.ctypes.data, values.ctypes.data)
    return kinds, values, out
