"""TEST INFRASTRUCTURE: tests/_build/libaecm_sim_trace.so -- tests/sim/sim_trace.cpp on top of the lane-simulator library
(tests/simlib.py): BlockEngine::run_stream_traced, the block loop of the traced kernels, on the CPU."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

import simlib
from webrtc_aecm_amd.ffi import BLOCK_TRACE_DTYPE

SRC = simlib.ROOT / "tests" / "sim" / "sim_trace.cpp"
SO = simlib.SIM_SO.parent / ("libaecm_sim_trace_san.so" if simlib.SANITIZE else "libaecm_sim_trace.so")
_lib = None


def build():
    simlib.build()
    deps = [SRC, simlib.SIM_SO, SRC.parent / "wave_sim.h", SRC.parent / "sim_stream.h", simlib.CSRC / "aecm_wave.h", simlib.CSRC / "aecm_state.h",
            simlib.CSRC / "aecm_ops.h"]
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
        l.sim_trace_launch.restype = C.c_int64
        l.sim_trace_launch.argtypes = [vp, C.c_int, vp, C.c_int, C.c_int, vp, vp, vp, vp, C.c_int64, C.c_int64, vp, C.c_int64, C.c_int64]
        _lib = l
    return _lib


def traced_launch(streams, far, near, clean=None, lens=None, chunk_blocks=0, trace=None, trace_strides=None, out=None):
    """One traced launch of simlib.SimStream objects (their state lives on): far / near(/ clean) [S, T*64] int16, stream s runs
    lens[s] blocks (None: all T).  trace: a BLOCK_TRACE_DTYPE array the records go to by trace_strides = (stream, block) in records
    (None: a fresh stream-major [S, T] array, filled with 0xA5 bytes).  Returns (out -- 0x5A5A where nothing was written --,
    trace, records written)."""
    far = np.ascontiguousarray(far, dtype=np.int16)
    near = np.ascontiguousarray(near, dtype=np.int16)
    S, T = far.shape[0], far.shape[1] // 64
    assert far.shape == near.shape and len(streams) == S
    cptr = None
    if clean is not None:
        clean = np.ascontiguousarray(clean, dtype=np.int16)
        assert clean.shape == near.shape
        cptr = clean.ctypes.data
    lptr = None
    if lens is not None:
        lens = np.ascontiguousarray(lens, dtype=np.int32)
        assert lens.shape == (S,) and lens.min() >= 0 and lens.max() <= T
        lptr = lens.ctypes.data
    if trace is None:
        trace = np.frombuffer(np.full(S * T * BLOCK_TRACE_DTYPE.itemsize, 0xA5, np.uint8).tobytes(), dtype=BLOCK_TRACE_DTYPE).copy().reshape(S, T)
        trace_strides = (T, 1)
    assert trace.dtype == BLOCK_TRACE_DTYPE and trace.flags.c_contiguous
    need = (S - 1) * trace_strides[0] + (T - 1) * trace_strides[1] + 1
    assert min(trace_strides) > 0 and need <= trace.size, "the records of this launch do not fit the trace array"
    if out is None:
        out = np.full_like(near, 0x5A5A)
    handles = (C.c_void_p * S)(*[s.h for s in streams])
    n = lib().sim_trace_launch(handles, S, lptr, T, chunk_blocks, far.ctypes.data, near.ctypes.data, cptr, out.ctypes.data, far.shape[1], 64,
                               trace.ctypes.data, trace_strides[0], trace_strides[1])
    return out, trace, n
