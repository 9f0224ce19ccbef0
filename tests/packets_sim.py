"""TEST INFRASTRUCTURE: tests/_build/libaecm_sim_packets.so -- tests/sim/sim_packets.cpp: packet ticks
(WebRtcAecmSessions_TickPackets) of an object of sessions of both rates on sample tags, against one SessionFlow<T> per session
called K times and against the device model of ordinary mixed ticks (tests/sim/sim_mixed.cpp) ticked K times on re-laid rows.
Header-only on the product's side.  A plain shared library; standalone(): the same source as a program with its own main, the only
form that is ever built with sanitizers."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

import simlib

SRC = simlib.ROOT / "tests" / "sim" / "sim_packets.cpp"
SO = simlib.SIM_SO.parent / "libaecm_sim_packets.so"
DEPS = [SRC, SRC.parent / "sim_mixed.cpp", simlib.CSRC / "aecm_flow_plan.h", simlib.CSRC / "aecm_flow_clean.h", simlib.CSRC / "aecm_tick_plan.h", simlib.CSRC / "aecm_session_flow.h", simlib.CSRC / "aecm_ops.h"]
_lib = None


def _fresh(target):
    return target.exists() and all(target.stat().st_mtime >= d.stat().st_mtime for d in DEPS)


def build():
    if _fresh(SO):
        return
    SO.parent.mkdir(parents=True, exist_ok=True)
    tmp = SO.with_suffix(f".{os.getpid()}.tmp")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fwrapv", "-fPIC", "-DAECM_SIM_PACKETS_NO_MAIN", f"-I{simlib.CSRC}", "-shared", str(SRC), "-o", str(tmp)])
    os.replace(tmp, SO)


def standalone(out_dir):
    """The simulator as a program of its own with AddressSanitizer and UBSan (nothing is loaded into python).  Returns the path."""
    exe = out_dir / "sim_packets_san"
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-std=c++17", "-fwrapv",
                           f"-I{simlib.CSRC}", str(SRC), "-o", str(exe)])
    return exe


def lib():
    global _lib
    if _lib is None:
        build()
        l = C.CDLL(str(SO))
        l.sim_packets_fuzz.restype = C.c_int64
        l.sim_packets_fuzz.argtypes = [C.c_uint64, C.c_int, C.c_int, C.c_int, C.c_void_p]
        l.sim_packets_lag_after.restype = C.c_int32
        l.sim_packets_lag_after.argtypes = [C.c_int64, C.c_int]
        l.sim_packets_spill_recipe.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
        _lib = l
    return _lib


DETAIL = ("what", "session", "field", "blocks", "packet_ticks", "calls_shaped_ticks", "ordinary_ticks", "bursts", "nobody_ticks", "longest_idle_samples",
          "half_spill_later", "startup_end_later", "resync_after_idle", "half_and_full", "half_packets", "nondirect_later", "no_block_calls",
          "full_8k_packets")
MIXED_RATES, UNIFORM = 0, 1


def fuzz(seed, n_sessions, n_ticks, rates_mode):
    """(first tick that differed or -1, {detail})."""
    assert lib().sim_packets_detail_words() == len(DETAIL)
    detail = np.zeros(len(DETAIL), dtype=np.int64)
    tick = lib().sim_packets_fuzz(seed, n_sessions, n_ticks, rates_mode, detail.ctypes.data)
    return tick, dict(zip(DETAIL, detail.tolist()))


def lag_after(ticks, calls):
    return lib().sim_packets_lag_after(ticks, calls)


def spill_recipe(fs, pre_ticks, calls, max_ticks=60):
    """{tick, call, row} of the first replay-row spill of the recipe (sim_packets.cpp: sim_packets_spill_recipe), or None."""
    res = np.zeros(3, dtype=np.int32)
    if lib().sim_packets_spill_recipe(fs, pre_ticks, calls, max_ticks, res.ctypes.data) != 0:
        return None
    return dict(zip(("tick", "call", "row"), res.tolist()))
