"""TEST INFRASTRUCTURE: tests/_build/libaecm_sim_sparse.so -- tests/sim/sim_sparse.cpp: sessions that sit out ticks
(AECM_SESSION_IDLE) on sample tags, the live list of a tick, and the wrapper state's lag word.  Header-only on the product's
side (webrtc_aecm_amd/csrc/aecm_flow_plan.h, aecm_session_flow.h): it needs nothing of the lane simulator."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

import simlib

SRC = simlib.ROOT / "tests" / "sim" / "sim_sparse.cpp"
SO = simlib.SIM_SO.parent / ("libaecm_sim_sparse_san.so" if simlib.SANITIZE else "libaecm_sim_sparse.so")
_lib = None


def build():
    deps = [SRC, simlib.CSRC / "aecm_flow_plan.h", simlib.CSRC / "aecm_flow_clean.h", simlib.CSRC / "aecm_tick_plan.h", simlib.CSRC / "aecm_session_flow.h", simlib.CSRC / "aecm_ops.h"]
    if SO.exists() and all(SO.stat().st_mtime >= d.stat().st_mtime for d in deps):
        return
    SO.parent.mkdir(parents=True, exist_ok=True)
    flags = [*(simlib.SAN_FLAGS if simlib.SANITIZE else ["-O2"]), "-std=c++17", "-fwrapv", "-fPIC", f"-I{simlib.CSRC}"]
    tmp = SO.with_suffix(f".{os.getpid()}.tmp")
    subprocess.check_call(["g++", *flags, "-shared", str(SRC), "-o", str(tmp)])
    os.replace(tmp, SO)


def lib():
    global _lib
    if _lib is None:
        build()
        l = C.CDLL(str(SO))
        l.sim_sparse_fuzz.restype = C.c_int64
        l.sim_sparse_fuzz.argtypes = [C.c_uint64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_void_p]
        l.sim_sparse_lag_defect.argtypes = [C.c_int32]
        l.sim_sparse_lag_after.restype = C.c_int32
        l.sim_sparse_lag_after.argtypes = [C.c_int64, C.c_int]
        l.sim_sparse_move_check.argtypes = [C.c_int, C.c_uint32, C.c_uint32, C.c_int]
        l.sim_live_list.restype = C.c_int32
        l.sim_live_list.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
        _lib = l
    return _lib


DETAIL = ("what", "blocks", "idle_ticks", "longest_stretch", "resyncs", "moved_samples", "dense_ticks", "nobody_ticks", "idle_in_startup",
          "idle_after_startup", "idle_two_block")


def fuzz(seed, fs, n_ticks, pattern, idle_percent, start_pos=0):
    """(first differing tick or -1, {detail})."""
    detail = np.zeros(len(DETAIL), dtype=np.int64)
    tick = lib().sim_sparse_fuzz(seed, fs, n_ticks, pattern, idle_percent, start_pos, detail.ctypes.data)
    return tick, dict(zip(DETAIL, detail.tolist()))


def live_list(flags):
    """(live count, list[S] with untouched entries 0xffffffff) as host + planning kernel build it."""
    flags = np.ascontiguousarray(flags, dtype=np.uint8)
    out = np.full(len(flags), 0xffffffff, dtype=np.uint32)
    n = lib().sim_live_list(flags.ctypes.data, len(flags), out.ctypes.data)
    return n, out
