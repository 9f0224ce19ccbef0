"""TEST INFRASTRUCTURE: tests/_build/libaecm_sim_calls.so -- tests/sim/sim_calls.cpp: ticks of K call pairs
(WebRtcAecmSessions_TickCalls) on sample tags against SessionFlow<T> called K times and against the device model of ordinary
ticks (tests/sim/sim_sparse.cpp) ticked K times.  Header-only on the product's side, like sparse_sim.py."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

import simlib

SRC = simlib.ROOT / "tests" / "sim" / "sim_calls.cpp"
SO = simlib.SIM_SO.parent / ("libaecm_sim_calls_san.so" if simlib.SANITIZE else "libaecm_sim_calls.so")
_lib = None


def build():
    deps = [SRC, SRC.parent / "sim_sparse.cpp", simlib.CSRC / "aecm_flow_plan.h", simlib.CSRC / "aecm_flow_clean.h", simlib.CSRC / "aecm_tick_plan.h", simlib.CSRC / "aecm_session_flow.h", simlib.CSRC / "aecm_ops.h"]
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
        l.sim_calls_fuzz.restype = C.c_int64
        l.sim_calls_fuzz.argtypes = [C.c_uint64, C.c_int, C.c_int, C.c_uint32, C.c_void_p]
        l.sim_calls_spill_recipe.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
        l.sim_calls_lag_after.restype = C.c_int32
        l.sim_calls_lag_after.argtypes = [C.c_int64, C.c_int, C.c_int, C.c_void_p]
        _lib = l
    return _lib


DETAIL = ("what", "blocks", "calls_ticks", "nondirect_later", "spill_later", "startup_end_later", "stuffing_later", "no_block_calls", "idle_ticks",
          "longest_idle_samples", "nobody_ticks", "resyncs", "field", "ordinary_ticks", "bursts")


def fuzz(seed, fs, n_ticks, start_pos=0):
    """(first differing tick or -1, {detail})."""
    detail = np.zeros(len(DETAIL), dtype=np.int64)
    tick = lib().sim_calls_fuzz(seed, fs, n_ticks, start_pos, detail.ctypes.data)
    return tick, dict(zip(DETAIL, detail.tolist()))


def spill_recipe(fs, pre_ticks, calls, max_ticks=60):
    """{tick, call, row, calls_before} of the first replay-row spill of the recipe (sim_calls.cpp: sim_calls_spill_recipe), or None."""
    res = np.zeros(4, dtype=np.int32)
    if lib().sim_calls_spill_recipe(fs, pre_ticks, calls, max_ticks, res.ctypes.data) != 0:
        return None
    return dict(zip(("tick", "call", "row", "calls_before"), res.tolist()))


def lag_after(ticks, calls, n):
    """(lag after `ticks` idle K-call ticks, lag after the same samples as idle ordinary ticks)."""
    single = C.c_int32(0)
    return lib().sim_calls_lag_after(ticks, calls, n, C.byref(single)), single.value
