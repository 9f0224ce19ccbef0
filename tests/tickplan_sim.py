"""TEST INFRASTRUCTURE: tests/_build/libaecm_sim_tickplan.so -- tests/sim/sim_tickplan.cpp: the host's tick planner
(webrtc_aecm_amd/csrc/aecm_tick_plan.h) ticked without a device, and the random run of it against the one restatement from the
primitives.  standalone(): the same source as a program with its own main, the only form ever built with sanitizers.

COINCIDING: the table of ticks that trip two adjacent checks of a tick at once, with the code SessionBatch::Tick has always returned
for them (the earlier check's) -- shared by tests/test_tick_plan.py and tests/test_gpu_tick_refusals.py."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

import simlib

SRC = simlib.ROOT / "tests" / "sim" / "sim_tickplan.cpp"
SO = simlib.SIM_SO.parent / "libaecm_sim_tickplan.so"
DEPS = [SRC, simlib.CSRC / "aecm_tick_plan.h", simlib.CSRC / "aecm_flow_clean.h", simlib.CSRC / "aecm_flow_plan.h"]
UNSPECIFIED, UNSUPPORTED, UNINITIALIZED, NULL_POINTER, BAD_PARAMETER, WARNING = 12000, 12001, 12002, 12003, 12004, 12100
NO_FAREND, SPLIT_CALLS, IDLE, HALF_CALL, NO_CLEAN = 1, 2, 4, 8, 16
PLAN_FIELDS = ("family", "live", "span", "sparse_plan", "sparse_tick", "deferred_lag", "mixed_plan", "need_slot", "zero_out", "clean_plane",
               "split_tick", "clean_count", "plain_count", "half_calls", "checked")
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
    """The simulator as a program of its own (its main runs the random ticks at every size), by default with AddressSanitizer and
    UBSan: nothing sanitized is loaded into python.  Returns the path."""
    exe = SO.parent / ("sim_tickplan_main_san" if sanitize else "sim_tickplan_main")
    if not _fresh(exe):
        exe.parent.mkdir(parents=True, exist_ok=True)
        flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitize else ["-O2"]
        tmp = exe.with_suffix(f".{os.getpid()}.tmp")
        subprocess.check_call(["g++", *flags, "-std=c++17", "-fwrapv", "-DSIM_TICKPLAN_MAIN", f"-I{simlib.CSRC}", str(SRC), "-o", str(tmp)])
        os.replace(tmp, exe)
    return exe


def lib():
    global _lib
    if _lib is None:
        build()
        l = C.CDLL(str(SO))
        l.tickplan_family_name.restype = C.c_char_p
        l.tickplan_family_name.argtypes = [C.c_int32]
        l.tickplan_new.restype = C.c_void_p
        l.tickplan_new.argtypes = [C.c_int32, C.c_int32]
        l.tickplan_free.restype = None
        l.tickplan_free.argtypes = [C.c_void_p]
        l.tickplan_init_session.restype = None
        l.tickplan_init_session.argtypes = [C.c_void_p, C.c_int32, C.c_int32]
        l.tickplan_force_sparse.restype = None
        l.tickplan_force_sparse.argtypes = [C.c_void_p, C.c_int32]
        l.tickplan_split_call_ticks.restype = None
        l.tickplan_split_call_ticks.argtypes = [C.c_void_p, C.c_int32]
        l.tickplan_attach_trace.argtypes = [C.c_void_p, C.c_int32, C.c_int32]
        l.tickplan_trace_counts.restype = None
        l.tickplan_trace_counts.argtypes = [C.c_void_p, C.c_void_p]
        l.tickplan_tick.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        l.tickplan_state.restype = None
        l.tickplan_state.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        l.tickplan_codes.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p]
        l.tickplan_fuzz.restype = C.c_int64
        l.tickplan_fuzz.argtypes = [C.c_uint64, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p]
        _lib = l
    return _lib


def families():
    """The kernel families' names in the order of their numbers (aecm_tick_plan.h: TickFamily)."""
    return [lib().tickplan_family_name(f).decode() for f in range(lib().tickplan_families())]


class Object:
    """The host state of an object of S sessions (fs = 0: created, never initialised)."""

    def __init__(self, n_sessions, fs=16000, rates=None, force_sparse=False):
        self.S = n_sessions
        self.h = lib().tickplan_new(n_sessions, fs)
        for s, r in enumerate(rates or []):
            self.init_session(s, r)
        lib().tickplan_force_sparse(self.h, int(force_sparse))

    def __del__(self):
        if getattr(self, "h", None):
            lib().tickplan_free(self.h)
            self.h = None

    def init_session(self, session, fs):
        lib().tickplan_init_session(self.h, session, fs)

    def force_sparse(self, on=True):
        lib().tickplan_force_sparse(self.h, int(on))

    def split_call_ticks(self, on=True):
        """WebRtcAecmSessions_SetSplitCallTicks."""
        lib().tickplan_split_call_ticks(self.h, int(on))

    def attach_trace(self, which, on=True):
        """which: "session" / "call".  False where the planner refuses (the other trace is attached)."""
        return bool(lib().tickplan_attach_trace(self.h, int(which == "call"), int(on)))

    def trace_counts(self):
        """(ticks the session trace has counted, call slots the call trace has)."""
        c = np.zeros(2, dtype=np.int64)
        lib().tickplan_trace_counts(self.h, c.ctypes.data)
        return int(c[0]), int(c[1])

    def tick(self, flags=None, all_flags=0, n=160, calls=1, stride=None, packets=False, clean=False, host=False, ms_per_session=False, far=True,
             near_out=True, poisoned=False, fast=True, commit=True):
        """(code, the plan's fields by name); an accepted tick is committed."""
        f = None if flags is None else np.ascontiguousarray(flags, dtype=np.uint8)
        assert f is None or len(f) == self.S
        args = np.array([all_flags, n, calls, n * calls if stride is None else stride, packets, clean, host, ms_per_session, far, near_out, poisoned,
                         fast, commit], dtype=np.int64)
        out = np.zeros(len(PLAN_FIELDS), dtype=np.int32)
        rc = lib().tickplan_tick(self.h, None if f is None else f.ctypes.data, args.ctypes.data, out.ctypes.data)
        plan = dict(zip(PLAN_FIELDS, (int(v) for v in out)))
        plan["family"] = families()[plan["family"]]
        return rc, plan

    def state(self):
        """{near_pos, deferred_lag, may_lag, split_used, other_rates, modes[S]}: everything a tick can move."""
        rest = np.zeros(5, dtype=np.int64)
        modes = np.zeros(self.S, dtype=np.uint8)
        lib().tickplan_state(self.h, rest.ctypes.data, modes.ctypes.data)
        return dict(near_pos=int(rest[0]), deferred_lag=int(rest[1]), may_lag=bool(rest[2]), split_used=bool(rest[3]), other_rates=int(rest[4]),
                    modes=modes.tolist())


def codes(ms, flags, n_sessions):
    """(first code, codes[S]) of a tick's msInSndCardBuf: ms one int for everybody or S values."""
    out = np.full(n_sessions, -1, dtype=np.int32)
    f = None if flags is None else np.ascontiguousarray(flags, dtype=np.uint8)
    per = None if np.ndim(ms) == 0 else np.ascontiguousarray(ms, dtype=np.int16)
    rc = lib().tickplan_codes(None if per is None else per.ctypes.data, 0 if per is not None else int(ms), None if f is None else f.ctypes.data,
                              n_sessions, out.ctypes.data)
    return rc, out.tolist()


def fuzz(seed, n_sessions, ticks):
    """(-1 or the tick that failed, what failed, {family or 'refused': ticks seen})."""
    what = C.c_int32(0)
    seen = np.zeros(len(families()) + 1, dtype=np.int64)
    at = lib().tickplan_fuzz(seed, n_sessions, ticks, C.byref(what), seen.ctypes.data)
    return at, what.value, dict(zip(families() + ["refused"], seen.tolist()))


def pattern(n_sessions, *first):
    """Flag bytes for S sessions: `first` for sessions 0, 1, ..., repeated over the rest."""
    return [first[s % len(first)] for s in range(n_sessions)]


# (name, object: rates pattern or None + "uninit", the tick as Object.tick's keywords with flags as a pattern, the code).  The checks in
# the order SessionBatch::Tick makes them: near / out null; far null while somebody buffers; not initialised; n; calls; stride; poisoned;
# safe variant; K calls in an object of two rates; [the device: events]; flags that need 160 samples or exclude each other; K-call flags;
# the clean history (unsupported before refused).  Every row trips two neighbours; the earlier one names the code.  gpu: the row can
# be made through the C ABI without harming the object (no poison, no variant switch).
COINCIDING = [
    dict(name="near null + far null while everybody buffers", tick=dict(near_out=False, far=False), code=NULL_POINTER, gpu=True),
    dict(name="far null while somebody buffers + bad n", tick=dict(far=False, flags=(NO_FAREND, 0), n=81), code=NULL_POINTER, gpu=True),
    dict(name="far null, one byte for all + not initialised", uninit=True, tick=dict(far=False), code=NULL_POINTER, gpu=False),
    dict(name="far null, flags array (not read before Init) + not initialised", uninit=True, tick=dict(far=False, flags=(0,)), code=UNINITIALIZED, gpu=False),
    dict(name="not initialised + bad n", uninit=True, tick=dict(n=81), code=UNINITIALIZED, gpu=False),
    dict(name="bad n + calls out of range", tick=dict(n=81, calls=0), code=BAD_PARAMETER, gpu=True),
    dict(name="calls out of range + short stride", tick=dict(calls=7, stride=160), code=BAD_PARAMETER, gpu=True),
    dict(name="short stride + poisoned", tick=dict(stride=159, poisoned=True), code=BAD_PARAMETER, gpu=False),
    dict(name="poisoned + safe variant", tick=dict(poisoned=True, fast=False), code=UNSPECIFIED, gpu=False),
    dict(name="safe variant + K calls at two rates", rates=(16000, 8000), tick=dict(fast=False, calls=2), code=UNSUPPORTED, gpu=False),
    dict(name="K calls at two rates + split calls in 80 samples", rates=(16000, 8000), tick=dict(calls=2, n=80, flags=(SPLIT_CALLS, 0)), code=UNSUPPORTED, gpu=True),
    dict(name="half call in 80 samples + half call in a K-call tick", tick=dict(calls=2, n=80, flags=(HALF_CALL, 0)), code=BAD_PARAMETER, gpu=True),
    dict(name="half and split together + split calls in a K-call tick", tick=dict(calls=2, flags=(HALF_CALL | SPLIT_CALLS, 0)), code=BAD_PARAMETER, gpu=True),
    dict(name="split calls in a K-call tick + K calls with callers of both kinds", tick=dict(calls=2, clean=True, flags=(SPLIT_CALLS, NO_CLEAN)), code=BAD_PARAMETER, gpu=True),
    dict(name="K calls with callers of both kinds + a changed kind", after_split=True, tick=dict(calls=2, clean=True, flags=(NO_CLEAN, 0)), code=UNSUPPORTED, gpu=True),
    dict(name="a changed kind (one check behind the K-call flags)", after_split=True, tick=dict(clean=True, flags=(NO_CLEAN, 0)), code=BAD_PARAMETER, gpu=True),
]
# after_split: the object has accepted this tick first (a clean plane; sessions 1, 3, ... without theirs)
SPLIT_FIRST = dict(clean=True, flags=(0, NO_CLEAN))
