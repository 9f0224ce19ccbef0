"""TEST INFRASTRUCTURE: tests/_build/libaecm_sim_split.so -- tests/sim/sim_split.cpp: the two live lists of a tick with
AECM_SESSION_NO_CLEAN sessions (host half + the planning kernel's half, lane by lane) and the per-session clean history as
the host's tick planner (aecm_tick_plan.h) applies it.  Header-only on the product's side (webrtc_aecm_amd/csrc/aecm_tick_plan.h, aecm_flow_clean.h, aecm_flow_plan.h),
like tests/mixed_sim.py.  standalone(): the same source as a program with its own main, the only form ever built with sanitizers."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

import simlib

SRC = simlib.ROOT / "tests" / "sim" / "sim_split.cpp"
SO = simlib.SIM_SO.parent / "libaecm_sim_split.so"
DEPS = [SRC, simlib.CSRC / "aecm_tick_plan.h", simlib.CSRC / "aecm_flow_clean.h", simlib.CSRC / "aecm_flow_plan.h"]
ACCEPTED, BAD_PARAMETER, UNSUPPORTED = 0, 1, 2
_lib = None


def _fresh(target):
    return target.exists() and all(target.stat().st_mtime >= d.stat().st_mtime for d in DEPS)


def build():
    if _fresh(SO):
        return
    SO.parent.mkdir(parents=True, exist_ok=True)
    tmp = SO.with_suffix(f".{os.getpid()}.tmp")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fwrapv", "-fPIC", f"-I{simlib.CSRC}", "-shared", str(SRC), "-o", str(tmp)])
    os.replace(tmp, SO)


def standalone(sanitize=True):
    """The simulator as a program of its own (its main runs the self check), by default with AddressSanitizer and UBSan: nothing is
    loaded into python.  Returns the path."""
    exe = SO.parent / ("sim_split_main_san" if sanitize else "sim_split_main")
    if not _fresh(exe):
        exe.parent.mkdir(parents=True, exist_ok=True)
        flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitize else ["-O2"]
        tmp = exe.with_suffix(f".{os.getpid()}.tmp")
        subprocess.check_call(["g++", *flags, "-std=c++17", "-fwrapv", "-DSIM_SPLIT_MAIN", f"-I{simlib.CSRC}", str(SRC), "-o", str(tmp)])
        os.replace(tmp, exe)
    return exe


def lib():
    global _lib
    if _lib is None:
        build()
        l = C.CDLL(str(SO))
        l.sim_split_lists.restype = None
        l.sim_split_lists.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
        l.sim_split_list_entries.argtypes = [C.c_int32]
        l.sim_split_object_new.restype = C.c_void_p
        l.sim_split_object_new.argtypes = [C.c_int32]
        l.sim_split_object_free.restype = None
        l.sim_split_object_free.argtypes = [C.c_void_p]
        l.sim_split_object_init.restype = None
        l.sim_split_object_init.argtypes = [C.c_void_p]
        l.sim_split_object_tick.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]
        l.sim_split_object_reset_session.restype = None
        l.sim_split_object_reset_session.argtypes = [C.c_void_p, C.c_int32]
        l.sim_split_object_state.restype = None
        l.sim_split_object_state.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        _lib = l
    return _lib


def lists(flags):
    """(the device list as the planning kernel leaves it -- 0xffffffff where nothing was stored --, clean count, plain count, start of the
    plain list, stores the kernel's guard dropped)."""
    flags = np.ascontiguousarray(flags, dtype=np.uint8)
    out = np.full(lib().sim_split_list_entries(len(flags)), 0xffffffff, dtype=np.uint32)
    res = np.zeros(4, dtype=np.int32)
    lib().sim_split_lists(flags.ctypes.data, len(flags), out.ctypes.data, res.ctypes.data)
    return out, int(res[0]), int(res[1]), int(res[2]), int(res[3])


class Object:
    """An object of S sessions as the host keeps it, ticked by the host's planner."""

    def __init__(self, n_sessions):
        self.S = n_sessions
        self.h = lib().sim_split_object_new(n_sessions)

    def __del__(self):
        if getattr(self, "h", None):
            lib().sim_split_object_free(self.h)
            self.h = None

    def init(self):
        lib().sim_split_object_init(self.h)

    def tick(self, flags=None, clean=True, calls=1, n=160):
        """(verdict, {split launches, kernels with a clean input, checked})."""
        route = np.zeros(3, dtype=np.int32)
        f = None if flags is None else np.ascontiguousarray(flags, dtype=np.uint8)
        assert f is None or len(f) == self.S
        rc = lib().sim_split_object_tick(self.h, None if f is None else f.ctypes.data, int(clean), calls, n, route.ctypes.data)
        return rc, dict(zip(("split", "clean_kernels", "checked"), (bool(v) for v in route)))

    def init_session(self, session):
        lib().sim_split_object_reset_session(self.h, session)

    def state(self):
        """(modes[S], position, split_used): everything a caller could observe."""
        modes = np.zeros(self.S, dtype=np.uint8)
        rest = np.zeros(2, dtype=np.int64)
        lib().sim_split_object_state(self.h, modes.ctypes.data, rest.ctypes.data)
        return modes, int(rest[0]), bool(rest[1])
