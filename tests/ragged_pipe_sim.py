"""TEST INFRASTRUCTURE: tests/_build/libaecm_sim_ragged_pipe.so -- tests/sim/sim_ragged_pipe.cpp on top of the lane-simulator
library (tests/simlib.py): one workgroup of the ragged pipelined kernel, four slots with a length each."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

import simlib

SRC = simlib.ROOT / "tests" / "sim" / "sim_ragged_pipe.cpp"
SO = simlib.SIM_SO.parent / ("libaecm_sim_ragged_pipe_san.so" if simlib.SANITIZE else "libaecm_sim_ragged_pipe.so")
_lib = None


def build():
    simlib.build()
    deps = [SRC, simlib.SIM_SO, simlib.CSRC / "aecm_wave.h", simlib.CSRC / "aecm_host_state.h", simlib.ROOT / "tests" / "sim" / "wave_sim.h"]
    if SO.exists() and all(SO.stat().st_mtime >= d.stat().st_mtime for d in deps):
        return
    flags = [*(simlib.SAN_FLAGS if simlib.SANITIZE else ["-O2"]), "-std=c++17", "-fwrapv", "-fPIC", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
             f"-I{simlib.CSRC}", f"-I{simlib.ROOT / 'tests' / 'sim'}"]
    tmp = SO.with_suffix(f".{os.getpid()}.tmp")
    subprocess.check_call(["g++", *flags, "-shared", str(SRC), "-o", str(tmp), f"-L{simlib.SIM_SO.parent}", f"-l:{simlib.SIM_SO.name}",
                           "-Wl,-rpath,$ORIGIN"])
    os.replace(tmp, SO)


def lib():
    global _lib
    if _lib is None:
        build()
        simlib.lib()
        l = C.CDLL(str(SO))
        vp = C.c_void_p
        l.sim_ragged_pipe_workgroup.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_int64, vp, vp, vp, vp, vp]
        _lib = l
    return _lib


def workgroup(far, near, lens, fs=16000, cng=1, echo_mode=3, deep=True, order=0, sentinel=0x5A5A):
    """One workgroup of four slots (far, near: [4][samples]; lens: blocks per slot, 0 = empty) through the role split of the
    sixteen-wave (deep) or the six-wave shape.  Returns (steps, out -- `sentinel` where nothing was written --, digests[4][24],
    counts[4][3] = hand-over slots written, output blocks written, input rows loaded)."""
    far = np.ascontiguousarray(far, dtype=np.int16)
    near = np.ascontiguousarray(near, dtype=np.int16)
    lens = np.ascontiguousarray(lens, dtype=np.int32)
    assert far.shape == near.shape and far.shape[0] == 4 and lens.size == 4
    out = np.full_like(near, sentinel)
    digests = np.zeros((4, 24), dtype=np.uint32)
    counts = np.zeros((4, 3), dtype=np.int64)
    steps = lib().sim_ragged_pipe_workgroup(fs, cng, echo_mode, 1 if deep else 0, order, lens.ctypes.data, far.shape[1], far.ctypes.data,
                                            near.ctypes.data, out.ctypes.data, digests.ctypes.data, counts.ctypes.data)
    assert steps >= 0, steps
    return steps, out, digests, counts
