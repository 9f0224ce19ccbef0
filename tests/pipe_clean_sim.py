"""TEST INFRASTRUCTURE: tests/_build/libaecm_sim_pipe_clean.so -- tests/sim/sim_pipe_clean.cpp on top of the lane-simulator
library (tests/simlib.py): one workgroup of the pipelined kernel for launches with a clean near-end input, four streams whose
state lives on from launch to launch."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

import simlib

SRC = simlib.ROOT / "tests" / "sim" / "sim_pipe_clean.cpp"
SO = simlib.SIM_SO.parent / ("libaecm_sim_pipe_clean_san.so" if simlib.SANITIZE else "libaecm_sim_pipe_clean.so")
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
        l.sim_pipe_clean_create.restype = vp
        l.sim_pipe_clean_create.argtypes = [C.c_int, vp, vp]
        l.sim_pipe_clean_free.argtypes = [vp]
        l.sim_pipe_clean_launch.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int64, vp, vp, vp, vp]
        l.sim_pipe_clean_digests.argtypes = [vp, vp]
        _lib = l
    return _lib


class Workgroup:
    """Four streams (configs: four (cng_mode, echo_mode) pairs) through launches of the role split of the sixteen-wave (deep) or
    the six-wave shape."""

    def __init__(self, fs, configs):
        self.lib = lib()
        cng = np.array([c[0] for c in configs], dtype=np.int32)
        em = np.array([c[1] for c in configs], dtype=np.int32)
        assert cng.size == 4
        self.h = self.lib.sim_pipe_clean_create(fs, cng.ctypes.data, em.ctypes.data)
        if not self.h:
            raise ValueError("bad parameters")

    def launch(self, far, near, clean=None, deep=True, order=0):
        """far / near / clean: [4][n_blocks * 64]; clean None = a launch without a clean input.  Returns (steps, out)."""
        far = np.ascontiguousarray(far, dtype=np.int16)
        near = np.ascontiguousarray(near, dtype=np.int16)
        assert far.shape == near.shape and far.shape[0] == 4 and far.shape[1] % 64 == 0
        cptr = None
        if clean is not None:
            clean = np.ascontiguousarray(clean, dtype=np.int16)
            assert clean.shape == near.shape
            cptr = clean.ctypes.data
        out = np.full_like(near, 0x5A5A)
        steps = self.lib.sim_pipe_clean_launch(self.h, 1 if deep else 0, order, far.shape[1] // 64, far.shape[1], far.ctypes.data, near.ctypes.data,
                                               cptr, out.ctypes.data)
        assert steps >= 0, steps
        return steps, out

    def digests(self):
        d = np.zeros((4, 24), dtype=np.uint32)
        self.lib.sim_pipe_clean_digests(self.h, d.ctypes.data)
        return d

    def __del__(self):
        try:
            self.lib.sim_pipe_clean_free(self.h)
        except Exception:
            pass
