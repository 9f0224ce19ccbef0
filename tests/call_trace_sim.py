"""TEST INFRASTRUCTURE: tests/_build/libaecm_sim_call_trace.so -- tests/sim/sim_call_trace.cpp on top of the lane-simulator library
(tests/simlib.py): the CPU double of the call trace (include/aecm_batch.h: WebRtcAecmSessions_SetCallTrace).  The planning kernels'
text with the call trace's sink and the K-call loop's record hook run on the host, next to the per-tick session trace of ticks of one
call pair, on one object: the host's tick planner with both switches, wrapper words, plans and the core state of every session."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

import simlib
from webrtc_aecm_amd.ffi import SESSION_TRACE_DTYPE

SRC = simlib.ROOT / "tests" / "sim" / "sim_call_trace.cpp"
SO = simlib.SIM_SO.parent / ("libaecm_sim_call_trace_san.so" if simlib.SANITIZE else "libaecm_sim_call_trace.so")
NO_FAREND, SPLIT_CALLS, IDLE, HALF_CALL = 1, 2, 4, 8
UNSUPPORTED, BAD_PARAMETER = 12001, 12004
PER_TICK, PER_CALL = 1, 2
FILL = 0xA5
_lib = None


def build():
    simlib.build()
    csrc = simlib.CSRC
    deps = [SRC, simlib.SIM_SO, SRC.parent / "wave_sim.h", SRC.parent / "sim_stream.h", csrc / "aecm_wave.h", csrc / "aecm_state.h", csrc / "aecm_ops.h",
            csrc / "aecm_session_trace.h", csrc / "aecm_tick_plan.h", csrc / "aecm_flow_plan.h", csrc / "aecm_flow_clean.h", csrc / "aecm_flow_plan_lane.inc",
            csrc / "aecm_kernels.h"]
    if SO.exists() and all(SO.stat().st_mtime >= d.stat().st_mtime for d in deps):
        return
    flags = [*(simlib.SAN_FLAGS if simlib.SANITIZE else ["-O2"]), "-std=c++17", "-fwrapv", "-fPIC", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
             f"-I{csrc}", f"-I{simlib.ROOT / 'tests' / 'sim'}"]
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
        l.ctsim_new.restype = vp
        l.ctsim_new.argtypes = [C.c_int, C.c_int, vp]
        l.ctsim_free.restype = None
        l.ctsim_free.argtypes = [vp]
        l.ctsim_attach.argtypes = [vp, C.c_int, vp, C.c_int64, C.c_int64, C.c_int32]
        l.ctsim_count.restype = C.c_int64
        l.ctsim_count.argtypes = [vp, C.c_int]
        l.ctsim_near_pos.restype = C.c_int64
        l.ctsim_near_pos.argtypes = [vp]
        l.ctsim_blocks_run.restype = C.c_int64
        l.ctsim_blocks_run.argtypes = [vp, C.c_int]
        l.ctsim_digest.restype = None
        l.ctsim_digest.argtypes = [vp, C.c_int, vp]
        l.ctsim_flow.restype = None
        l.ctsim_flow.argtypes = [vp, C.c_int, vp]
        l.ctsim_tick.argtypes = [vp, vp, C.c_int, vp, C.c_int, C.c_int, C.c_int, vp, vp, vp, C.c_int64, vp, vp]
        _lib = l
    return _lib


def trace_buffer(records):
    """`records` SESSION_TRACE_DTYPE records of FILL bytes."""
    return np.frombuffer(np.full(records * SESSION_TRACE_DTYPE.itemsize, FILL, np.uint8).tobytes(), dtype=SESSION_TRACE_DTYPE).copy()


class SimSessions:
    """S sessions of an object at fs, session s at rates[s]; far / near: every session's streams of 64-sample blocks
    [S, blocks * 64] int16 (a session's blocks take them in order, whatever the form of the tick)."""

    def __init__(self, far, near, fs=16000, rates=None):
        self.far = np.ascontiguousarray(far, dtype=np.int16)
        self.near = np.ascontiguousarray(near, dtype=np.int16)
        assert self.far.shape == self.near.shape and self.far.shape[1] % 64 == 0
        self.S, self.stream_blocks = self.far.shape[0], self.far.shape[1] // 64
        self.out = np.full_like(self.near, 0x5A5A)
        self.rates = np.full(self.S, fs, dtype=np.int32) if rates is None else np.ascontiguousarray(rates, dtype=np.int32)
        self.h = lib().ctsim_new(self.S, fs, self.rates.ctypes.data)
        self.trace = None

    def __del__(self):
        if getattr(self, "h", None):
            lib().ctsim_free(self.h)
            self.h = None

    def attach(self, kind, trace, session_stride, slot_stride, ring, byte_offset=0):
        """trace: a SESSION_TRACE_DTYPE array (kept alive here), or None to detach `kind`.  Returns the code."""
        if trace is None:
            return lib().ctsim_attach(self.h, kind, None, 0, 0, 0)
        rc = lib().ctsim_attach(self.h, kind, trace.ctypes.data + byte_offset, session_stride, slot_stride, ring)
        if rc == 0:
            self.trace = trace
        return rc

    def count(self, kind):
        return int(lib().ctsim_count(self.h, kind))

    @property
    def near_pos(self):
        return int(lib().ctsim_near_pos(self.h))

    def blocks_run(self):
        return np.array([lib().ctsim_blocks_run(self.h, s) for s in range(self.S)], dtype=np.int64)

    def digest(self, s):
        d = np.zeros(24, dtype=np.uint32)
        lib().ctsim_digest(self.h, s, d.ctypes.data)
        return d

    def flow(self, s):
        w = np.zeros(lib().ctsim_flow_words(), dtype=np.int32)
        lib().ctsim_flow(self.h, s, w.ctypes.data)
        return w

    def tick(self, ms, flags=None, all_flags=0, n=160, calls=1, packets=False):
        """(code, family number or -1, blocks [S, calls]: n_blocks per call, -1 for a session that sat out)."""
        ms = np.ascontiguousarray(np.broadcast_to(ms, (self.S,)), dtype=np.int16)
        f = None if flags is None else np.ascontiguousarray(flags, dtype=np.uint8)
        assert f is None or f.shape == (self.S,)
        blocks = np.full((self.S, max(calls, 1)), -1, dtype=np.int32)
        fam = C.c_int32(-2)
        rc = lib().ctsim_tick(self.h, None if f is None else f.ctypes.data, all_flags, ms.ctypes.data, n, calls, int(packets), self.far.ctypes.data,
                              self.near.ctypes.data, self.out.ctypes.data, self.stream_blocks, blocks.ctypes.data, C.byref(fam))
        assert rc != -2, "the sessions' block streams are too short for this run"
        return rc, fam.value, blocks
