"""TEST INFRASTRUCTURE: build + bind tests/_build/libaecm_ops.so -- tests/sim/sim_ops.cpp, the HOST branch of every entry of
webrtc_aecm_amd/csrc/aecm_ops_table.inc (the definitions the lane simulator runs), one tuple at a time.  A library of its own:
it defines the aecm_*_violation hooks itself, so it is never linked with tests/_build/libaecm_sim.so."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

import simlib

SRC = simlib.ROOT / "tests" / "sim" / "sim_ops.cpp"
TABLE = simlib.CSRC / "aecm_ops_table.inc"
SO = simlib.ROOT / "tests" / "_build" / "libaecm_ops.so"
_DEPS = [SRC, TABLE, SRC.parent / "wave_sim.h", simlib.CSRC / "aecm_wave.h", simlib.CSRC / "aecm_ops.h", simlib.CSRC / "aecm_state.h",
         simlib.CSRC / "aecm_tables.h"]
_lib = None


def build():
    if SO.exists() and all(SO.stat().st_mtime >= d.stat().st_mtime for d in _DEPS):
        return
    SO.parent.mkdir(parents=True, exist_ok=True)
    flags = ["-O2", "-std=c++17", "-fwrapv", "-fPIC", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", f"-I{simlib.CSRC}",
             f"-I{simlib.ROOT / 'tests' / 'sim'}"]
    tmp = SO.with_suffix(f".{os.getpid()}.tmp")
    subprocess.check_call(["g++", *flags, "-shared", str(SRC), "-o", str(tmp)])
    os.replace(tmp, SO)


def lib():
    global _lib
    if _lib is None:
        build()
        l = C.CDLL(str(SO))
        vp = C.c_void_p
        l.sim_ops_name.restype = C.c_char_p
        l.sim_ops_name.argtypes = [C.c_int]
        l.sim_ops_arity.argtypes = [C.c_int]
        l.sim_ops_eval.argtypes = [C.c_int, vp, vp, vp, vp, vp, C.c_int]
        _lib = l
    return _lib


def names():
    l = lib()
    return [l.sim_ops_name(k).decode() for k in range(l.sim_ops_count())]


def arity(op: int) -> int:
    return lib().sim_ops_arity(op)


def evaluate(op, a, b=None, c=None):
    """(out, flags): entry `op` (an id or a name) on the int32 tuples; flags[i] = 1 where a range check of the header fired
    (out[i] is then 0)."""
    if isinstance(op, str):
        op = names().index(op)
    a = np.ascontiguousarray(a, dtype=np.int32)
    ops = [a] + [None if x is None else np.ascontiguousarray(x, dtype=np.int32) for x in (b, c)]
    assert all(x is None or x.shape == a.shape for x in ops)
    out = np.zeros(a.size, dtype=np.int32)
    flags = np.zeros(a.size, dtype=np.int32)
    rc = lib().sim_ops_eval(op, *[None if x is None else x.ctypes.data for x in ops], out.ctypes.data, flags.ctypes.data, a.size)
    assert rc >= 0, f"no op {op}"
    assert rc == int(flags.sum())
    return out, flags
