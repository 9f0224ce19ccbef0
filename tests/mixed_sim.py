"""TEST INFRASTRUCTURE: tests/_build/libaecm_sim_mixed.so -- tests/sim/sim_mixed.cpp: an object of sessions of both sampling
rates and both call sizes (WebRtcAecmSessions_InitRates, AECM_SESSION_HALF_CALL) on sample tags, its launch routing and the
host's argument check of a tick's flags.  Header-only on the product's side (webrtc_aecm_amd/csrc/aecm_flow_plan.h,
aecm_session_flow.h), like tests/sparse_sim.py.  standalone(): the same source as a program with its own main, which is the
only form that is ever built with sanitizers."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

import simlib

SRC = simlib.ROOT / "tests" / "sim" / "sim_mixed.cpp"
SO = simlib.SIM_SO.parent / "libaecm_sim_mixed.so"
DEPS = [SRC, simlib.CSRC / "aecm_flow_plan.h", simlib.CSRC / "aecm_flow_clean.h", simlib.CSRC / "aecm_tick_plan.h", simlib.CSRC / "aecm_session_flow.h", simlib.CSRC / "aecm_ops.h"]
_lib = None


def _fresh(target):
    return target.exists() and all(target.stat().st_mtime >= d.stat().st_mtime for d in DEPS)


def build():
    if _fresh(SO):
        return
    SO.parent.mkdir(parents=True, exist_ok=True)
    flags = ["-O2", "-std=c++17", "-fwrapv", "-fPIC", f"-I{simlib.CSRC}"]
    tmp = SO.with_suffix(f".{os.getpid()}.tmp")
    subprocess.check_call(["g++", *flags, "-shared", str(SRC), "-o", str(tmp)])
    os.replace(tmp, SO)


def standalone(sanitize=True):
    """The simulator as a program of its own (its main runs FUZZ_PLAN and the routing check), by default with
    AddressSanitizer and UBSan: nothing is loaded into python.  Returns the path."""
    exe = SO.parent / ("sim_mixed_main_san" if sanitize else "sim_mixed_main")
    if not _fresh(exe):
        exe.parent.mkdir(parents=True, exist_ok=True)
        flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitize else ["-O2"]
        tmp = exe.with_suffix(f".{os.getpid()}.tmp")
        subprocess.check_call(["g++", *flags, "-std=c++17", "-fwrapv", "-DSIM_MIXED_MAIN", f"-I{simlib.CSRC}", str(SRC), "-o", str(tmp)])
        os.replace(tmp, exe)
    return exe


def lib():
    global _lib
    if _lib is None:
        build()
        l = C.CDLL(str(SO))
        l.sim_mixed_fuzz.restype = C.c_int64
        l.sim_mixed_fuzz.argtypes = [C.c_uint64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_void_p]
        l.sim_mixed_route_uniform.restype = C.c_int64
        l.sim_mixed_route_uniform.argtypes = [C.c_uint64, C.c_int, C.c_int]
        l.sim_mixed_route.restype = None
        l.sim_mixed_route.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
        l.sim_mixed_check_flags.argtypes = [C.c_void_p, C.c_int32, C.c_int, C.c_void_p]
        _lib = l
    return _lib


DETAIL = ("what", "session", "blocks", "half_calls", "resyncs", "moved_samples", "mixed_ticks", "sparse_ticks", "dense_ticks", "nobody_ticks",
          "idle", "bursts", "split_calls", "full_calls_8k", "half_calls_16k", "warnings", "max_lag")
UNIFORM, MIXED_RATES, UNIFORM_WITH_HALF = 1, 0, 2
# The fuzz plan (the stand-alone main of sim_mixed.cpp runs the same): seeds [first, first + count) per mode.  Within a mode, seed k
# takes start position (k // 4) % 3 -- the seed's low bits choose the object's rate and the clean input, so every mode meets
# every start with every such combination.
FUZZ_PLAN = ((MIXED_RATES, 0, 24), (UNIFORM_WITH_HALF, 24, 12), (UNIFORM, 36, 12))


def fuzz(seed, n_sessions, n_ticks, rates_mode, idle_percent, start_pos=0):
    """(first tick that differed or -1, {detail})."""
    assert lib().sim_mixed_detail_words() == len(DETAIL)
    detail = np.zeros(len(DETAIL), dtype=np.int64)
    tick = lib().sim_mixed_fuzz(seed, n_sessions, n_ticks, rates_mode, idle_percent, start_pos, detail.ctypes.data)
    return tick, dict(zip(DETAIL, detail.tolist()))


class Router:
    """FlowRouteTickMixed with the object's lag bookkeeping kept between calls."""

    def __init__(self, n_sessions):
        self.S = n_sessions
        self.state = np.zeros(2, dtype=np.int32)

    def tick(self, live, n, half_calls=False, other_rates=False, force_sparse=False):
        out = np.zeros(6, dtype=np.int32)
        lib().sim_mixed_route(self.state.ctypes.data, live, self.S, n, int(force_sparse), int(half_calls), int(other_rates), out.ctypes.data)
        return dict(zip(("launch", "sparse_plan", "sparse_tick", "deferred_lag", "mixed_plan", "may_lag"), out.tolist()))


def check_flags(flags, n):
    """(0 accepted / 1 AECM_BAD_PARAMETER_ERROR, live, OR of the calling sessions' bytes, the bases agree with FlowLiveBlockBases)."""
    flags = np.ascontiguousarray(flags, dtype=np.uint8)
    res = np.zeros(3, dtype=np.int32)
    rc = lib().sim_mixed_check_flags(flags.ctypes.data, len(flags), n, res.ctypes.data)
    return rc, int(res[0]), int(res[1]), bool(res[2])
