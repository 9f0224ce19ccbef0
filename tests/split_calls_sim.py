"""TEST INFRASTRUCTURE: tests/_build/libaecm_sim_split_calls.so -- tests/sim/sim_split_calls.cpp: K-call and packet ticks with a
clean near-end input per session (WebRtcAecmSessions_SetSplitCallTicks) on sample tags -- whole objects through the host's planner
with the switch on, the two-list planning texts lane by lane and the loop body once per list, against one SessionFlow per session and
against a twin object of K ordinary split ticks -- and the host's planner with the switch and a call trace, for a table of plans.
Header-only on the product's side, like tests/packets_sim.py.  standalone(): the same source as a program with its own main, the only
form ever built with sanitizers."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

import simlib

SIM = simlib.ROOT / "tests" / "sim"
SRC = SIM / "sim_split_calls.cpp"
SO = simlib.SIM_SO.parent / "libaecm_sim_split_calls.so"
DEPS = [SRC, SIM / "sim_packets.cpp", SIM / "sim_mixed.cpp"] + [simlib.CSRC / h for h in (
    "aecm_tick_plan.h", "aecm_flow_clean.h", "aecm_flow_plan.h", "aecm_session_flow.h", "aecm_ops.h")]
UNSPECIFIED, UNSUPPORTED, UNINITIALIZED, NULL_POINTER, BAD_PARAMETER = 12000, 12001, 12002, 12003, 12004
NO_FAREND, SPLIT_CALLS, IDLE, HALF_CALL, NO_CLEAN = 1, 2, 4, 8, 16
PLAN_FIELDS = ("family", "live", "span", "k_calls", "mixed_plan", "split_tick", "clean_plane", "clean_count", "plain_count", "sparse_tick", "half_calls",
               "checked")
DETAIL = ("what", "session", "field", "blocks", "split_calls_ticks", "split_packet_ticks", "all_clean_ticks", "all_plain_ticks", "ordinary_split", "nobody",
          "clean_mult4", "clean_other", "reinit", "half_plain", "startup_plain_calls", "bursts")
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
    """The simulator as a program of its own (its main runs whole objects of 6 .. 300 sessions and the switch), by default with
    AddressSanitizer and UBSan: nothing sanitized is loaded into python.  Returns the path."""
    exe = SO.parent / ("sim_split_calls_main_san" if sanitize else "sim_split_calls_main")
    if not _fresh(exe):
        exe.parent.mkdir(parents=True, exist_ok=True)
        flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitize else ["-O2"]
        tmp = exe.with_suffix(f".{os.getpid()}.tmp")
        subprocess.check_call(["g++", *flags, "-std=c++17", "-fwrapv", "-DSIM_SPLIT_CALLS_MAIN", f"-I{simlib.CSRC}", str(SRC), "-o", str(tmp)])
        os.replace(tmp, exe)
    return exe


def lib():
    global _lib
    if _lib is None:
        build()
        l = C.CDLL(str(SO))
        l.sim_split_calls_fuzz.restype = C.c_int64
        l.sim_split_calls_fuzz.argtypes = [C.c_uint64, C.c_int, C.c_int, C.c_int, C.c_void_p]
        l.sim_split_calls_family_name.restype = C.c_char_p
        l.sim_split_calls_family_name.argtypes = [C.c_int32]
        l.sim_split_calls_object_new.restype = C.c_void_p
        l.sim_split_calls_object_new.argtypes = [C.c_int32, C.c_int32]
        for name in ("free", "init"):
            getattr(l, f"sim_split_calls_object_{name}").restype = None
            getattr(l, f"sim_split_calls_object_{name}").argtypes = [C.c_void_p]
        l.sim_split_calls_object_init_session.restype = None
        l.sim_split_calls_object_init_session.argtypes = [C.c_void_p, C.c_int32, C.c_int32]
        l.sim_split_calls_object_switch.restype = None
        l.sim_split_calls_object_switch.argtypes = [C.c_void_p, C.c_int32]
        for name in ("get_switch",):
            getattr(l, f"sim_split_calls_object_{name}").argtypes = [C.c_void_p]
        for name in ("call_trace", "session_trace"):
            getattr(l, f"sim_split_calls_object_{name}").argtypes = [C.c_void_p, C.c_int32]
        l.sim_split_calls_object_tick.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        l.sim_split_calls_object_state.restype = None
        l.sim_split_calls_object_state.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        _lib = l
    return _lib


def fuzz(seed, n_sessions, n_ticks, rates_mode=0):
    """(-1 or the tick that failed, the details by name)."""
    detail = np.zeros(lib().sim_split_calls_detail_words(), dtype=np.int64)
    assert len(detail) == len(DETAIL)
    tick = lib().sim_split_calls_fuzz(seed, n_sessions, n_ticks, rates_mode, detail.ctypes.data)
    return int(tick), dict(zip(DETAIL, (int(v) for v in detail)))


class Object:
    """The host state of an object of S sessions, ticked by the host's planner; the switch and the traces as the product sets them."""

    def __init__(self, n_sessions, fs=16000, rates=None, switch=False):
        self.S = n_sessions
        self.h = lib().sim_split_calls_object_new(n_sessions, fs)
        for s, r in enumerate(rates or []):
            self.init_session(s, r)
        self.switch(switch)

    def __del__(self):
        if getattr(self, "h", None):
            lib().sim_split_calls_object_free(self.h)
            self.h = None

    def init(self):
        lib().sim_split_calls_object_init(self.h)

    def init_session(self, session, fs=16000):
        lib().sim_split_calls_object_init_session(self.h, session, fs)

    def switch(self, on):
        lib().sim_split_calls_object_switch(self.h, int(on))

    def switched(self):
        return bool(lib().sim_split_calls_object_get_switch(self.h))

    def call_trace(self, on):
        return bool(lib().sim_split_calls_object_call_trace(self.h, int(on)))

    def session_trace(self, on):
        return bool(lib().sim_split_calls_object_session_trace(self.h, int(on)))

    def tick(self, flags=None, n=160, calls=1, packets=False, clean=True, fast=True):
        """(code, the plan's fields by name -- of an accepted tick, which is committed)."""
        f = None if flags is None else np.ascontiguousarray(flags, dtype=np.uint8)
        assert f is None or len(f) == self.S
        args = np.array([n, calls, packets, clean, fast], dtype=np.int32)
        out = np.zeros(len(PLAN_FIELDS), dtype=np.int32)
        rc = lib().sim_split_calls_object_tick(self.h, None if f is None else f.ctypes.data, args.ctypes.data, out.ctypes.data)
        plan = dict(zip(PLAN_FIELDS, (int(v) for v in out)))
        plan["family"] = lib().sim_split_calls_family_name(plan["family"]).decode() if rc == 0 else ""
        return rc, plan

    def state(self):
        """Everything a tick can move: {modes[S], near_pos, split_used, call_trace_calls, deferred_lag}."""
        modes = np.zeros(self.S, dtype=np.uint8)
        rest = np.zeros(4, dtype=np.int64)
        lib().sim_split_calls_object_state(self.h, modes.ctypes.data, rest.ctypes.data)
        return dict(modes=modes.tolist(), near_pos=int(rest[0]), split_used=bool(rest[1]), call_trace_calls=int(rest[2]), deferred_lag=int(rest[3]))
