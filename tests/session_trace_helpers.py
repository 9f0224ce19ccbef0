"""TEST INFRASTRUCTURE shared by tests/test_session_trace.py and tests/test_gpu_session_trace.py.

The yardstick of the session trace (include/aecm_batch.h: AecmSessionTrace).  The reference publishes no session state, so the
expected record is the header's own contract: every wrapper field is the value ExportSession shows directly after that tick, `core`
is AecmBlockTrace of the core blob of that same snapshot, `blocks` the advance of F_BLK_POS over the tick / 64.  A TWIN object that
makes the same calls without a trace is exported after every tick (export_sessions: the parent's code, held to the reference by the
existing suites); expected_records() turns those snapshots into SESSION_TRACE_DTYPE records -- wrapper words at snapshot offset
16 192, the core blob at offset 32 through import_state + digest on a one-stream AecmBatch and trace_helpers.records_of_digests.

Also: the binding of tests/sim/sim_session_trace.cpp (the host compile of aecm_session_trace.h and of the planner's trace rules) and a
Python restatement of the record's wrapper half from the header's table."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

import simlib
from webrtc_aecm_amd.ffi import SESSION_TRACE_DTYPE

SRC = simlib.ROOT / "tests" / "sim" / "sim_session_trace.cpp"
SO = simlib.SIM_SO.parent / "libaecm_sim_session_trace.so"
DEPS = [SRC, simlib.CSRC / "aecm_session_trace.h", simlib.CSRC / "aecm_tick_plan.h", simlib.CSRC / "aecm_flow_clean.h", simlib.CSRC / "aecm_flow_plan.h"]
UNSUPPORTED, BAD_PARAMETER = 12001, 12004
NO_FAREND, SPLIT_CALLS, IDLE, HALF_CALL, NO_CLEAN = 1, 2, 4, 8, 16
SNAPSHOT_BYTES, STATE_AT, FLOW_AT, FLOW_WORDS = 34304, 32, 16192, 32
# include/aecm_batch.h: AecmSessionTrace -- (field, offset, the wrapper word it is read from or None)
LAYOUT = (("tick", 0, None), ("blocks", 4, None), ("samp_khz", 6, None), ("ms_in_snd_card_buf", 8, "F_MS"), ("known_delay", 10, "F_KNOWN_DELAY"),
          ("filt_delay", 12, "F_FILT_DELAY"), ("buf_size_start", 14, "F_BUF_SIZE_START"), ("ec_startup", 16, "F_EC_STARTUP"),
          ("check_buff_size", 18, "F_CHECK_BUFF_SIZE"), ("delay_change", 20, "F_DELAY_CHANGE"), ("last_delay_diff", 22, "F_LAST_DELAY_DIFF"),
          ("far_buffered", 24, None), ("time_for_delay_change", 28, "F_TIME_FOR_DELAY_CHANGE"), ("core", 32, None))
# aecm_flow_plan.h: FlowField, in the order of the enum (what tests/test_gpu_flow_corpus.py compares field by field)
FLOW_FIELDS = ("F_BUF_SIZE_START", "F_KNOWN_DELAY", "F_COUNTER", "F_SUM", "F_FIRST_VAL", "F_CHECK_BUF_SIZE_CTR", "F_MS", "F_FILT_DELAY",
               "F_TIME_FOR_DELAY_CHANGE", "F_EC_STARTUP", "F_CHECK_BUFF_SIZE", "F_DELAY_CHANGE", "F_LAST_DELAY_DIFF", "F_FAR_RP", "F_FAR_WP", "F_FRM_POS",
               "F_BLK_POS")
F = {name: i for i, name in enumerate(FLOW_FIELDS)}
_lib = None


def build():
    if SO.exists() and all(SO.stat().st_mtime >= d.stat().st_mtime for d in DEPS):
        return
    SO.parent.mkdir(parents=True, exist_ok=True)
    tmp = SO.with_suffix(f".{os.getpid()}.tmp")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fwrapv", "-fPIC", f"-I{simlib.CSRC}", "-shared", str(SRC), "-o", str(tmp)])
    os.replace(tmp, SO)


def lib():
    global _lib
    if _lib is None:
        build()
        l = C.CDLL(str(SO))
        l.strace_header_words.restype = None
        l.strace_header_words.argtypes = [C.c_void_p, C.c_uint32, C.c_int, C.c_int, C.c_void_p]
        l.strace_field.argtypes = [C.c_char_p]
        l.strace_object_new.restype = C.c_void_p
        l.strace_object_new.argtypes = [C.c_int, C.c_int]
        l.strace_object_free.restype = None
        l.strace_object_free.argtypes = [C.c_void_p]
        l.strace_object_attach.restype = None
        l.strace_object_attach.argtypes = [C.c_void_p, C.c_int]
        l.strace_object_ticks.restype = C.c_int64
        l.strace_object_ticks.argtypes = [C.c_void_p]
        l.strace_object_near_pos.restype = C.c_int64
        l.strace_object_near_pos.argtypes = [C.c_void_p]
        l.strace_object_tick.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
        _lib = l
    return _lib


def sim_header_words(flow, tick, blocks, khz):
    """SessionTraceHeaderWords of the host compile: flow = 32 int32 wrapper words -> the record's first eight words."""
    flow = np.ascontiguousarray(flow, dtype=np.int32)
    assert flow.shape == (FLOW_WORDS,)
    out = np.zeros(8, dtype=np.uint32)
    lib().strace_header_words(flow.ctypes.data, tick & 0xffffffff, blocks, khz, out.ctypes.data)
    return out


def header_record(flow, tick, blocks, khz):
    """The same eight words from the header's table alone, as one SESSION_TRACE_DTYPE record (core: zeros)."""
    flow = np.asarray(flow, dtype=np.int64)
    r = np.zeros((), dtype=SESSION_TRACE_DTYPE)
    r["tick"] = tick & 0xffffffff
    r["blocks"] = np.int64(blocks).astype(np.int16)
    r["samp_khz"] = khz
    for name, _, word in LAYOUT:
        if word is not None:
            r[name] = flow[F[word]].astype(SESSION_TRACE_DTYPE[name])               # (the 16-bit fields: the low half of the word)
    r["far_buffered"] = ((flow[F["F_FAR_WP"]] - flow[F["F_FAR_RP"]]) & 0xffffffff).astype(np.uint32).view(np.int32)
    return r


class PlanObject:
    """aecm_tick_plan.h: TickObject of S sessions at 16 kHz, with the session trace's switch."""

    def __init__(self, n_sessions, fs=16000):
        self.S, self.h = n_sessions, lib().strace_object_new(n_sessions, fs)

    def __del__(self):
        if getattr(self, "h", None):
            lib().strace_object_free(self.h)
            self.h = None

    def attach(self, on=True):
        lib().strace_object_attach(self.h, int(on))

    @property
    def ticks(self):
        return int(lib().strace_object_ticks(self.h))

    @property
    def near_pos(self):
        return int(lib().strace_object_near_pos(self.h))

    def tick(self, flags=None, all_flags=0, n=160, calls=1, packets=False, clean=False):
        """(code, family number or -1 when refused)."""
        f = None if flags is None else np.ascontiguousarray(flags, dtype=np.uint8)
        assert f is None or f.shape == (self.S,)
        fam = C.c_int32(-2)
        rc = lib().strace_object_tick(self.h, None if f is None else f.ctypes.data, all_flags, n, calls, int(packets), int(clean), C.byref(fam))
        return rc, fam.value


# ---- the yardstick -----------------------------------------------------------------------------------------------------------
def wrapper_words(blob, sessions):
    """[S, 32] int32: the wrapper words of export_sessions()'s snapshots."""
    snaps = np.frombuffer(blob, dtype=np.int32).reshape(sessions, SNAPSHOT_BYTES // 4)
    return snaps[:, FLOW_AT // 4:FLOW_AT // 4 + FLOW_WORDS]


class CoreDigests:
    """Core blob of a session snapshot -> its 24-word digest, by import_state + digest on a one-stream AecmBatch (any rate)."""

    def __init__(self):
        import webrtc_aecm_amd as aecm
        self.batch = aecm.AecmBatch(1, 16000)
        self.size = aecm.load().WebRtcAecmBatch_state_size_bytes()
        self.cache = {}

    def __call__(self, snapshot):
        core = bytes(snapshot[STATE_AT:STATE_AT + self.size])
        if core not in self.cache:
            self.batch.import_state(0, core)
            self.cache[core] = self.batch.digest(0).copy()
        return self.cache[core]

    def close(self):
        self.batch.close()


def expected_records(start_blob, blobs, called, rates):
    """start_blob: export_sessions() of the twin before its first tick; blobs[t]: after tick t (None where nothing was exported: a
    tick nobody made); called [T, S] bool: who made a call in tick t; rates [S].  Returns records [S, T] of SESSION_TRACE_DTYPE;
    entries of sessions that did not call are zeros (no record is written for them)."""
    import trace_helpers as th
    called = np.asarray(called, dtype=bool)
    T, S = called.shape
    rec = np.zeros((S, T), dtype=SESSION_TRACE_DTYPE)
    digests = CoreDigests()
    prev = wrapper_words(start_blob, S)[:, F["F_BLK_POS"]].astype(np.int64)
    for t in range(T):
        if blobs[t] is None:
            assert not called[t].any()
            continue
        words = wrapper_words(blobs[t], S)
        raw = np.frombuffer(blobs[t], dtype=np.uint8).reshape(S, SNAPSHOT_BYTES)
        blk = words[:, F["F_BLK_POS"]].astype(np.int64)
        advance = (blk - prev) & 0xffffffff
        assert (advance % 64 == 0).all() and (advance[~called[t]] == 0).all()
        for s in np.flatnonzero(called[t]):
            r = header_record(words[s], t, int(advance[s]) // 64, int(rates[s]) // 1000)
            r["core"] = th.records_of_digests(digests(raw[s]))
            rec[s, t] = r
        prev = blk
    digests.close()
    return rec


def flat_fields():
    """(name or (\"core\", name)) of every field of the record."""
    return [n for n in SESSION_TRACE_DTYPE.names if n != "core"] + [("core", n) for n in SESSION_TRACE_DTYPE["core"].names]


def field(rec, name):
    return rec[name] if isinstance(name, str) else rec[name[0]][name[1]]


def first_record_difference(got, want, mask=None):
    """got, want: [S, T] records; mask [S, T]: where to compare (None: everywhere).  None, or a sentence naming the session, the
    tick and the field of the first difference."""
    for name in flat_fields():
        g, w = field(got, name), field(want, name)
        bad = g != w if mask is None else (g != w) & mask
        if bad.any():
            s, t = (int(x) for x in np.argwhere(bad)[0])
            label = name if isinstance(name, str) else ".".join(name)
            return f"session {s}, tick {t}, field {label}: traced {g[s, t].item()} != expected {w[s, t].item()}"
    return None


def assert_track_is_alive(rec, mask=None):
    """What the issue demands of the TWIN's track before anything is compared with it: a trace of constants cannot pass."""
    m = np.ones(rec.shape, dtype=bool) if mask is None else mask
    values = lambda name: set(field(rec, name)[m].tolist())
    assert {0, 1} <= values("ec_startup"), values("ec_startup")
    assert {0, 2, 3} <= values("blocks"), values("blocks")
    assert len(values(("core", "startup_state"))) >= 2 and len(values(("core", "vad"))) >= 2
    changes = sum(len(set(rec["known_delay"][s][m[s]].tolist())) >= 2 for s in range(rec.shape[0]))
    assert changes >= 2, f"known_delay changes in {changes} sessions only"
    assert len(values("far_buffered")) >= 3, values("far_buffered")
