"""TEST INFRASTRUCTURE: tests/_build/libaecm_sim_ragged.so -- tests/sim/sim_ragged.cpp on top of the lane-simulator library
(tests/simlib.py): the recording schedule as arrays and the ragged twin of sim_recordings."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

import simlib

SRC = simlib.ROOT / "tests" / "sim" / "sim_ragged.cpp"
SO = simlib.SIM_SO.parent / ("libaecm_sim_ragged_san.so" if simlib.SANITIZE else "libaecm_sim_ragged.so")
_lib = None


def build():
    simlib.build()
    deps = [SRC, simlib.SIM_SO, simlib.CSRC / "aecm_engine.h", simlib.CSRC / "aecm_session_flow.h", simlib.CSRC / "aecm_kernels.h"]
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
        l.sim_schedule.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp, C.POINTER(C.c_int32)]
        l.sim_recordings_ragged.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp]
        _lib = l
    return _lib


def schedule(fs, frame, n_calls, ms):
    """aecm::BuildRecordingSchedule as a dict of arrays (aecm_session_flow.h: RecordingSchedule) + `code`."""
    cap = n_calls * frame // 64 + 8
    far_map, near_map = np.zeros(cap * 64, np.int32), np.zeros(cap * 64, np.int32)
    out_map = np.zeros(n_calls * frame, np.int32)
    after, codes = np.zeros(n_calls, np.int32), np.zeros(n_calls, np.int32)
    code = C.c_int32(0)
    nb = lib().sim_schedule(fs, frame, n_calls, ms, cap, far_map.ctypes.data, near_map.ctypes.data, out_map.ctypes.data, after.ctypes.data,
                            codes.ctypes.data, C.byref(code))
    assert nb >= 0
    return dict(n_blocks=nb, far_map=far_map[:nb * 64], near_map=near_map[:nb * 64], out_map=out_map, blocks_after_call=after,
                code_after_call=codes, code=code.value)


def recordings_ragged(far, near, fs, frame, cng, echo_mode, ms, calls, clean=None):
    """(code, out, codes) like AecmBatch.process_recordings_ragged_host, on the simulator."""
    far = np.ascontiguousarray(far, dtype=np.int16)
    near = np.ascontiguousarray(near, dtype=np.int16)
    calls = np.ascontiguousarray(calls, dtype=np.int32)
    cptr = None
    if clean is not None:
        clean = np.ascontiguousarray(clean, dtype=np.int16)
        cptr = clean.ctypes.data
    out = near.copy()
    codes = np.zeros(far.shape[0], dtype=np.int32)
    rc = lib().sim_recordings_ragged(far.shape[0], far.shape[1], fs, frame, cng, echo_mode, ms, far.ctypes.data, near.ctypes.data, cptr,
                                     calls.ctypes.data, out.ctypes.data, codes.ctypes.data)
    assert rc >= 0
    return rc, out, codes
