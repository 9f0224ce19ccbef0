"""The session trace without a device (include/aecm_batch.h: AecmSessionTrace, WebRtcAecmSessions_SetSessionTrace): the size and
the layout of the record, the one text of its wrapper half (webrtc_aecm_amd/csrc/aecm_session_trace.h, compiled for the host by
tests/sim/sim_session_trace.cpp) against a Python restatement of the header's table, and the trace's rules on the tick planner
(aecm_tick_plan.h): a refused tick does not count, a tick nobody makes does, ticks of several calls are refused only while a trace is
attached.  The device side is tests/test_gpu_session_trace.py."""
import re

import numpy as np

import session_trace_helpers as sh
import webrtc_aecm_amd as aecm
from helpers import GOLDEN
from webrtc_aecm_amd import ffi

ROOT = GOLDEN.parent.parent


def test_record_size_and_symbols():
    lib = aecm.load()
    assert aecm.session_trace_size_bytes() == 64 == ffi.SESSION_TRACE_DTYPE.itemsize
    header = (ROOT / "include" / "aecm_batch.h").read_text()
    for name in ("WebRtcAecmSessions_session_trace_size_bytes", "WebRtcAecmSessions_SetSessionTrace", "WebRtcAecmSessions_GetSessionTraceTicks"):
        assert name in ffi.SESSIONS_SYMBOLS and hasattr(lib, name) and re.search(r"\b%s\s*\(" % name, header), name
    for name in ("set_session_trace", "clear_session_trace", "session_trace_ticks"):
        assert callable(getattr(aecm.AecmSessions, name))


def test_dtype_offsets_are_the_headers_table():
    """The offsets in the comments of AecmSessionTrace, field by field, and the nested block trace at 32."""
    header = (ROOT / "include" / "aecm_batch.h").read_text()
    body = header[header.index("typedef struct AecmSessionTrace {"):header.index("} AecmSessionTrace;")]
    table = [(m.group(2), int(m.group(3))) for m in re.finditer(r"^\s*(\w+)\s+(\w+);\s*/\*\s*(\d+)\s", body, re.M)]
    assert table == [(n, o) for n, o, _ in sh.LAYOUT], table
    dt = ffi.SESSION_TRACE_DTYPE
    assert [(n, dt.fields[n][1]) for n in dt.names] == table
    assert dt["core"] == ffi.BLOCK_TRACE_DTYPE and dt["tick"] == np.dtype("<u4")
    assert all(dt[n] == np.dtype("<i2") for n, o, _ in sh.LAYOUT if 4 <= o < 24) and dt["far_buffered"] == dt["time_for_delay_change"] == np.dtype("<i4")
    assert sh.lib().strace_words() == 16 and sh.lib().strace_header_words_count() == 8
    # the wrapper words the record reads: the enum's own numbers, from the host compile
    for name in ("F_MS", "F_KNOWN_DELAY", "F_FILT_DELAY", "F_BUF_SIZE_START", "F_EC_STARTUP", "F_CHECK_BUFF_SIZE", "F_DELAY_CHANGE", "F_LAST_DELAY_DIFF",
                 "F_FAR_WP", "F_FAR_RP", "F_TIME_FOR_DELAY_CHANGE"):
        assert sh.lib().strace_field(name.encode()) == sh.F[name], name
    assert sh.lib().strace_field(b"F_BLK_POS") == -1


def _check(flow, tick, blocks, khz):
    words = sh.sim_header_words(flow, tick, blocks, khz)
    want = np.frombuffer(sh.header_record(flow, tick, blocks, khz).tobytes(), dtype=np.uint32)[:8]
    assert np.array_equal(words, want), (flow.tolist(), tick, blocks, khz, words.tolist(), want.tolist())
    return words


def test_header_words_equal_the_restatement():
    """Seeded random wrapper states, then the edges: every 16-bit field at both extremes, the jitter buffer's fill across the 2^32
    wrap of its two counters and at 0 and 4 000, the tick counter at its ends."""
    rs = np.random.RandomState(31)
    for _ in range(500):
        flow = rs.randint(-(1 << 31), (1 << 31) - 1, sh.FLOW_WORDS, dtype=np.int64).astype(np.int32)
        _check(flow, int(rs.randint(0, 1 << 32, dtype=np.int64)), int(rs.randint(0, 4)), 8 if rs.rand() < 0.5 else 16)
    shorts = [w for _, o, w in sh.LAYOUT if w is not None and o < 24]
    assert len(shorts) == 8
    for word in shorts:
        for v in (-32768, 32767, -1, 0, 1):
            flow = np.zeros(sh.FLOW_WORDS, dtype=np.int32)
            flow[sh.F[word]] = v
            w = _check(flow, 7, 2, 16)
            rec = np.frombuffer(w.tobytes() + bytes(32), dtype=ffi.SESSION_TRACE_DTYPE)[0]
            name = next(n for n, _, x in sh.LAYOUT if x == word)
            assert rec[name] == v and sum(int(rec[n]) != 0 for n, o, x in sh.LAYOUT if x is not None and n != name) == 0
    for v in (-(1 << 31), (1 << 31) - 1):
        flow = np.zeros(sh.FLOW_WORDS, dtype=np.int32)
        flow[sh.F["F_TIME_FOR_DELAY_CHANGE"]] = v
        assert _check(flow, 0, 0, 8)[7] == (v & 0xffffffff)
    for rp, fill in ((0, 0), (0, 4000), (0xffffff00, 4000), (0xfffffff0, 16), (0x7fffffc0, 160), (0xffffffff, 1), (12345, 0)):
        flow = np.zeros(sh.FLOW_WORDS, dtype=np.int32)
        flow[sh.F["F_FAR_RP"]] = np.uint32(rp).view(np.int32)
        flow[sh.F["F_FAR_WP"]] = np.uint32((rp + fill) & 0xffffffff).view(np.int32)
        assert _check(flow, 1, 3, 16)[6] == fill
    for tick in (0, 1, 0x7fffffff, 0x80000000, 0xffffffff):
        w = _check(np.zeros(sh.FLOW_WORDS, dtype=np.int32), tick, 3, 8)
        assert w[0] == tick and w[1] == (3 | 8 << 16)


def test_planner_counts_accepted_ticks_only():
    """The count moves in Commit: accepted ticks count, the tick nobody makes included; refused ticks -- a bad size, flags that
    exclude each other, several calls while attached -- change neither the count nor the position."""
    S = 5
    o = sh.PlanObject(S)
    assert o.ticks == 0
    assert o.tick()[0] == 0 and o.ticks == 0 and o.near_pos == 160                 # nothing attached: nothing counts
    o.attach()
    assert o.ticks == 0
    assert o.tick()[0] == 0 and o.ticks == 1
    idle = np.full(S, sh.IDLE, dtype=np.uint8)
    pos = o.near_pos
    rc, family = o.tick(flags=idle)
    assert rc == 0 and family == 0 and o.ticks == 2 and o.near_pos == pos + 160     # nobody calls: family `nothing`, and it counts
    pos = o.near_pos
    assert o.tick(n=81)[0] == sh.BAD_PARAMETER and o.ticks == 2 and o.near_pos == pos
    both = np.full(S, sh.HALF_CALL | sh.SPLIT_CALLS, dtype=np.uint8)
    assert o.tick(flags=both)[0] == sh.BAD_PARAMETER and o.ticks == 2 and o.near_pos == pos
    some = np.array([0, sh.IDLE, sh.NO_FAREND, sh.SPLIT_CALLS, sh.IDLE], dtype=np.uint8)
    assert o.tick(flags=some)[0] == 0 and o.ticks == 3
    o.attach()                                                                      # attaching again starts at 0
    assert o.ticks == 0
    o.attach(False)
    assert o.tick()[0] == 0 and o.ticks == 0


def test_several_calls_are_refused_only_while_attached():
    S = 4
    o = sh.PlanObject(S)
    for packets in (False, True):
        assert o.tick(calls=2, packets=packets)[0] == 0
    o.attach()
    pos = o.near_pos
    for packets in (False, True):
        for calls in (2, 3, 6):
            assert o.tick(calls=calls, packets=packets)[0] == sh.UNSUPPORTED
            assert o.tick(calls=calls, packets=packets, n=80)[0] == sh.UNSUPPORTED
    assert o.ticks == 0 and o.near_pos == pos
    assert o.tick(calls=7)[0] == sh.BAD_PARAMETER                                   # the earlier check names the code
    for packets in (False, True):
        assert o.tick(calls=1, packets=packets)[0] == 0                             # one call pair: the ordinary tick, traced
    assert o.ticks == 2
    o.attach(False)
    assert o.tick(calls=2)[0] == 0 and o.tick(calls=3, packets=True)[0] == 0 and o.ticks == 0
