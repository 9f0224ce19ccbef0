"""The call trace on the device (include/aecm_batch.h: WebRtcAecmSessions_SetCallTrace; aecm_call_trace_plan_kernels.hip,
aecm_call_trace_kernels.hip): one record per session and call pair from K-call and packet ticks.  The yardstick of every record is
tests/session_trace_helpers.py's: an untraced twin object driven by K ORDINARY ticks and exported after every call pair
(expected_records).  Outputs, codes and final snapshots are compared with the twin too.  Every trace buffer is pre-filled with 0xA5
and has guard records on both sides; guards, idle sessions' slots and records outside the ring must keep the fill.  The CPU side is
tests/test_call_trace.py."""
import functools
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import session_trace_helpers as sh
import test_gpu_session_trace as st
import webrtc_aecm_amd as aecm
from helpers import GOLDEN
from webrtc_aecm_amd import ffi

pytestmark = pytest.mark.gpu
REC = ffi.SESSION_TRACE_DTYPE
FILL, SENTINEL, GUARD = st.FILL, st.SENTINEL, 2
NO_FAREND, IDLE, HALF_CALL, NO_CLEAN, SPLIT_CALLS = sh.NO_FAREND, sh.IDLE, sh.HALF_CALL, sh.NO_CLEAN, sh.SPLIT_CALLS


def _k_tick(sb, api, packets, f, d, c, n, K, ms, fl):
    """One tick of K call pairs on rows [S, K n] through `api` (device / host / async); (code, out with SENTINEL where unwritten)."""
    import torch
    if api == "host":
        rc, out, _ = (sb.tick_packets_host if packets else sb.tick_calls_host)(f, d, K, ms, clean=c, flags=fl)
        return rc, out
    tf, tn = torch.from_numpy(f).cuda(), torch.from_numpy(d).cuda()
    tc = torch.from_numpy(c).cuda() if c is not None else None
    out = torch.full_like(tn, SENTINEL)
    torch.cuda.synchronize()
    fn = sb.tick_packets_device if packets else sb.tick_calls_device
    args = (tf.data_ptr(), tn.data_ptr(), out.data_ptr(), K * n, n, K, ms)
    cp = tc.data_ptr() if tc is not None else None
    if api == "async":
        done = torch.cuda.Event()
        done.record()
        rc, _ = fn(*args, clean_ptr=cp, flags=fl, asynchronous=True, done_event=done.cuda_event)
        done.synchronize()                       # the records are visible where out is
    else:
        rc, _ = fn(*args, clean_ptr=cp, flags=fl)
        assert sb.synchronize() == 0
    return rc, out.cpu().numpy()


def _rows(src, cur, own, S, width):
    r = np.full((S, width), 77, dtype=np.int16)
    for s in np.flatnonzero(own):
        r[s, :own[s]] = src[s, cur[s]:cur[s] + own[s]]
    return r


def _run(rates, n, K, ms, flags=None, clean=False, packets=False, api="device", seed0=700, ring=None, strides=None, setup=None, pertick=False,
         words_every_tick=False):
    """T ticks of K call pairs (ms [T, S], flags [T, S] or None) on an object with a call trace; the same calls as T K ordinary ticks
    on an untraced twin, exported after every one (and, pertick, on a second twin under SetSessionTrace with the same geometry).
    Asserts outputs, codes, the count and the final snapshots.  Returns dict(raw [records + 2 GUARD, 64] uint8, rec expected [S, T K],
    called [T K, S], final: the final snapshots, pertick_raw)."""
    ms = np.asarray(ms, dtype=np.int16)
    T, S = ms.shape
    C_ = T * K
    flags = None if flags is None else np.asarray(flags, dtype=np.uint8)
    far, near, cl = st._signals(tuple(rates), C_ * n, seed0)
    objs = [st._object(rates) for _ in range(3 if pertick else 2)]
    traced, twin = objs[0], objs[1]
    for sb in objs:
        if setup:
            setup(sb)
    ring = C_ if ring is None else ring
    strides = (ring, 1) if strides is None else strides
    records = (S - 1) * strides[0] + (ring - 1) * strides[1] + 1
    buf, ptr = st._trace_buffer(records, GUARD)
    assert traced.set_call_trace(ptr, strides[0], strides[1], ring) == 0 and traced.call_trace_calls() == 0
    if pertick:
        buf2, ptr2 = st._trace_buffer(records, GUARD)
        assert objs[2].set_session_trace(ptr2, strides[0], strides[1], ring) == 0
    rc, start = twin.export_sessions()
    assert rc == 0
    cur = np.zeros(S, dtype=np.int64)
    blobs, called = [], np.zeros((C_, S), dtype=bool)
    for t in range(T):
        fl = None if flags is None else flags[t]
        own = st._own(fl, n, S)                                   # per CALL: 0 idle, 80 with a half call, else n
        f, d, c = (_rows(x, cur, K * own, S, K * n) for x in (far, near, cl))
        rc, out = _k_tick(traced, api, packets, f, d, c if clean else None, n, K, np.ascontiguousarray(ms[t]), fl)
        assert traced.call_trace_calls() == (t + 1) * K
        codes = []
        for k in range(K):
            f1, d1, c1 = (_rows(x, cur + k * own, own, S, n) for x in (far, near, cl))
            for sb in objs[1:]:
                rc1, o1 = st._tick(sb, "flags", f1, d1, c1 if clean else None, n, np.ascontiguousarray(ms[t]), fl)
                if sb is twin:
                    codes.append(rc1)
                    for s in np.flatnonzero(own):
                        assert np.array_equal(out[s, k * own[s]:(k + 1) * own[s]], o1[s, :own[s]]), ("output", t, k, s)
            rc1, blob = twin.export_sessions()
            assert rc1 == 0
            blobs.append(blob)
            called[t * K + k] = own > 0
        assert rc == max(codes), ("code of tick", t, rc, codes)
        if api != "host":
            for s in range(S):
                assert (out[s, K * own[s]:] == SENTINEL).all(), ("written past the session's samples", t, s)
        cur += K * own
        if words_every_tick:                                      # the traced planners against the untraced ones, every session
            rc1, mine = traced.export_sessions()
            assert np.array_equal(sh.wrapper_words(mine, S), sh.wrapper_words(blobs[-1], S)), ("wrapper words after tick", t)
    final = traced.export_sessions()
    assert final == twin.export_sessions(), "final snapshots"
    raw = buf.cpu().numpy().reshape(-1, REC.itemsize)
    pertick_raw = buf2.cpu().numpy().reshape(-1, REC.itemsize) if pertick else None
    for sb in objs:
        sb.close()
    assert (raw[:GUARD] == FILL).all() and (raw[GUARD + records:] == FILL).all(), "a guard record was written"
    return dict(raw=raw, rec=sh.expected_records(start, blobs, called, rates), called=called, final=final[1], pertick_raw=pertick_raw, records=records)


def _records(r, S, C_):
    """[S, C] records of a session-major ring of C calls (every call in its own slot)."""
    return r["raw"][GUARD:GUARD + S * C_].reshape(-1).view(REC).reshape(S, C_)


def _assert_idle_slots_keep_the_fill(r, S, C_):
    raw = r["raw"][GUARD:GUARD + S * C_].reshape(S, C_, REC.itemsize)
    assert (raw[~r["called"].T] == FILL).all(), "a slot of a session that sat out was written"


# ---- 1. K-call records -------------------------------------------------------------------------------------------------------
# 216 calls, as the dense session-trace test and for its reason: the core's start-up state first changes at its 512th block
K3_S, K3_K, K3_T = st.DENSE_S, 3, st.DENSE_T // 3


@functools.lru_cache(maxsize=None)
def _k3_run():
    ms = st._dense_ms()[::3]                                       # per-session msInSndCardBuf as in DENSE_MS; the last session's steps
    assert ms.shape == (K3_T, K3_S)
    return _run([16000] * K3_S, 160, K3_K, ms, pertick=True)


def test_k_call_every_record_and_the_per_tick_trace():
    """Nine 16 kHz sessions (two full workgroups and one wavefront), K = 3 x 72 ticks: every record equals the yardstick, and the
    buffer is byte for byte the buffer of a twin under SetSessionTrace that makes the 216 calls as ordinary ticks."""
    r = _k3_run()
    C_ = K3_K * K3_T
    sh.assert_track_is_alive(r["rec"])
    got = _records(r, K3_S, C_)
    assert (got["tick"] == np.arange(C_, dtype=np.uint32)).all() and (got["samp_khz"] == 16).all()
    st._assert_records(got, r["rec"], np.ones((K3_S, C_), dtype=bool), "K-call tick")
    assert np.array_equal(r["raw"], r["pertick_raw"]), "the buffer differs from the per-tick trace's"


@pytest.mark.parametrize("K", [2, 6])
def test_k_call_8khz(K):
    """8 kHz, calls of 80 samples, K = 2 and 6, a quarter of the sessions idle per tick, ticks without a far end."""
    S, T = 6, 36 // K
    rs = np.random.RandomState(K)
    flags = np.where(rs.rand(T, S) < 0.25, IDLE, 0).astype(np.uint8)
    flags[rs.rand(T, S) < 0.1] |= NO_FAREND
    flags[:, 0] = 0
    flags[T // 2] = IDLE                                           # one tick nobody makes: it writes nothing and counts
    ms = np.broadcast_to(np.array([40, 60, 100, 20, 200, 300], dtype=np.int16), (T, S))
    r = _run([8000] * S, 80, K, ms, flags=flags, seed0=720)
    got = _records(r, S, T * K)
    live = r["called"].T
    assert {0, 1} <= set(r["rec"]["ec_startup"][live].tolist()) and {0, 1, 2} <= set(r["rec"]["blocks"][live].tolist())
    assert (got["samp_khz"][live] == 8).all()
    st._assert_records(got, r["rec"], live, f"8 kHz, K = {K}")
    _assert_idle_slots_keep_the_fill(r, S, T * K)


# ---- 2. packet records -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("clean", [False, True], ids=["plain", "clean"])
@pytest.mark.parametrize("K", [2, 3])
def test_packet_records(K, clean):
    """Both rates in one object, half of the sessions on half calls (packed rows), with and without a clean input."""
    S, T = 8, 36 // K
    rates = [16000 if s % 3 else 8000 for s in range(S)]
    flags = np.zeros((T, S), dtype=np.uint8)
    flags[:, [0, 1, 3, 6]] = HALF_CALL                            # the three 8 kHz sessions (10 ms calls of 80 samples) and a 16 kHz one
    flags[2:, 3] |= NO_FAREND
    flags[T // 2, 4] = IDLE
    flags[T // 2 + 1, 5] = IDLE
    ms = np.broadcast_to(np.array([40, 60, 100, 150, 200, 300, 20, 80], dtype=np.int16), (T, S))
    r = _run(rates, 160, K, ms, flags=flags, clean=clean, packets=True, seed0=740)
    got = _records(r, S, T * K)
    live = r["called"].T
    assert (got["samp_khz"][live] == np.broadcast_to((np.array(rates) // 1000)[:, None], live.shape)[live]).all()
    assert {0, 1} <= set(r["rec"]["ec_startup"][live].tolist()) and {0, 1, 2, 3} <= set(r["rec"]["blocks"][live].tolist())
    st._assert_records(got, r["rec"], live, f"packet tick, K = {K}, clean = {clean}")
    _assert_idle_slots_keep_the_fill(r, S, T * K)


# ---- 3. planner boundaries and divergence ------------------------------------------------------------------------------------
def test_planner_boundaries_and_divergent_neighbours():
    """300 sessions -- the planning kernels run 256 lanes per workgroup, wavefronts end at 64, 128, 192, 256 --, 12 ticks of K = 3,
    neighbours in different phases: fresh, past start-up (snapshots of the nine-session run), without a far end, and about a quarter
    idle, changing per tick.  Records against the yardstick; after every tick every session's wrapper words against the untraced
    planners'."""
    S, T, K = 300, 12, 3
    snaps = np.frombuffer(_k3_run()["final"], dtype=np.uint8).reshape(K3_S, -1)
    veterans = np.arange(1, S, 4)

    def setup(sb):
        assert sb.import_sessions(veterans, np.ascontiguousarray(snaps[np.arange(veterans.size) % K3_S])) == 0

    rs = np.random.RandomState(9)
    flags = np.where(rs.rand(T, S) < 0.25, IDLE, 0).astype(np.uint8)
    flags[:, 2::4] |= np.where(flags[:, 2::4] & IDLE, 0, NO_FAREND).astype(np.uint8)
    for edge in (63, 64, 127, 128, 191, 192, 255, 256, 299):        # the lanes at the wavefront and workgroup boundaries call in tick 0 ...
        flags[0, edge] &= ~np.uint8(IDLE)
        flags[1, edge] = IDLE if edge % 2 else flags[1, edge]       # ... and every other one of them sits tick 1 out
    ms = np.broadcast_to((40 + 20 * (np.arange(S) % 13)).astype(np.int16), (T, S))
    r = _run([16000] * S, 160, K, ms, flags=flags, seed0=760, setup=setup, words_every_tick=True)
    got = _records(r, S, T * K)
    live = r["called"].T
    assert 0.15 < 1 - live.mean() < 0.35 and {0, 1} <= set(r["rec"]["ec_startup"][live].tolist())
    assert (r["rec"]["ec_startup"][veterans][live[veterans]] == 0).all() and r["rec"]["blocks"][live].max() >= 2
    st._assert_records(got, r["rec"], live, "300 sessions")
    _assert_idle_slots_keep_the_fill(r, S, T * K)


# ---- 4. rings ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,ring,call_major", [(3, 1, False), (6, 4, True), (2, 5, True)])
def test_rings(K, ring, call_major):
    """ring_calls == 1 keeps the latest call's record; a ring shorter than the tick (6 calls into 4 slots) leaves what in-order writing
    leaves; a ring that is no multiple of K wraps inside a tick; call-major strides.  Nothing outside the ring's records is written."""
    S, T = 5, 24 // K                                              # (24 calls: past the start-up phase, blocks run)
    C_ = T * K
    ms = np.broadcast_to(np.array([40, 60, 100, 150, 200], dtype=np.int16), (T, S))
    flags = np.zeros((T, S), dtype=np.uint8)
    flags[T - 1, 2] = IDLE                                         # session 2 sits the last tick out: its slots keep the calls before
    r = _run([16000] * S, 160, K, ms, flags=flags, seed0=780, ring=ring, strides=(1, S) if call_major else (ring, 1))
    rec = r["raw"][GUARD:GUARD + r["records"]].reshape(-1).view(REC)
    for s in range(S):
        last = {}
        for j in range(C_):
            if r["called"][j, s]:
                last[j % ring] = j
        assert len(last) == ring
        for slot, j in last.items():
            at = s + slot * S if call_major else s * ring + slot
            assert rec[at]["tick"] == j, (s, slot, int(rec[at]["tick"]), j)
            st._assert_records(rec[at:at + 1].reshape(1, 1), r["rec"][s:s + 1, j:j + 1], None, f"session {s}, slot {slot} (call {j})")
    assert rec["blocks"].max() >= 2 and (rec["ec_startup"] == 0).all()      # (the ring's records are of calls past the start-up phase)


# ---- 5. entry points and mixing ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("api", ["host", "async"])
@pytest.mark.parametrize("packets", [False, True], ids=["calls", "packets"])
def test_host_and_async_forms(api, packets):
    S, K, T = 5, 3, 8
    rates = [16000, 8000, 16000, 16000, 8000] if packets else [16000] * S
    flags = np.zeros((T, S), dtype=np.uint8)
    flags[3, 2] = IDLE
    flags[4:, 1] = NO_FAREND
    if packets:
        flags[:, 3] |= HALF_CALL
    ms = np.broadcast_to(np.array([40, 60, 100, 150, 200], dtype=np.int16), (T, S))
    r = _run(rates, 160, K, ms, flags=flags, packets=packets, api=api, seed0=800)
    got = _records(r, S, T * K)
    live = r["called"].T
    assert {0, 1} <= set(r["rec"]["ec_startup"][live].tolist())
    st._assert_records(got, r["rec"], live, f"{api}, packets = {packets}")
    _assert_idle_slots_keep_the_fill(r, S, T * K)


def test_one_call_ticks_process_bursts_and_k_call_ticks_on_one_object():
    """calls == 1 ticks (plain, split calls, TickCalls with calls = 1), Process, BufferFarend (writes nothing, counts nothing) and
    K-call ticks interleaved: the slot numbering stays continuous, every record is the yardstick's; detaching leaves the buffer and
    changes no output."""
    import torch
    S, n = 5, 160
    far, near, _ = st._signals((16000,) * S, 40 * n, 820)
    traced, twin = st._object([16000] * S), st._object([16000] * S)
    ms = np.array([40, 60, 100, 150, 200], dtype=np.int16)
    split = np.array([0, SPLIT_CALLS, 0, SPLIT_CALLS, 0], dtype=np.uint8)
    some = np.array([0, IDLE, NO_FAREND, 0, IDLE], dtype=np.uint8)
    ops = [("tick", None), ("calls", 3, None), ("burst", 2), ("process",), ("calls", 2, some), ("tick", split), ("calls1", None), ("calls", 6, None),
           ("tick", some), ("calls", 3, None), ("process",), ("calls", 2, None), ("calls", 3, None)]
    C_ = sum(op[1] if op[0] == "calls" else 0 if op[0] == "burst" else 1 for op in ops)
    buf, ptr = st._trace_buffer(S * C_, GUARD)
    assert traced.set_call_trace(ptr, C_, 1, C_) == 0
    rc, start = twin.export_sessions()
    cur, blobs, called, slot = 0, [], [], 0

    def ordinary(sb, fl, pos, api="flags"):
        return st._tick(sb, api, far[:, pos:pos + n].copy(), near[:, pos:pos + n].copy(), None, n, ms, fl)

    for op in ops:
        if op[0] == "burst":
            tf = torch.from_numpy(far[:, cur:cur + op[1] * n].copy()).cuda()
            for sb in (traced, twin):
                assert sb.buffer_farend_device(tf.data_ptr(), op[1] * n, n, op[1]) == 0 and sb.synchronize() == 0
            cur += op[1] * n
            assert traced.call_trace_calls() == slot
            continue
        if op[0] == "process":
            tn = torch.from_numpy(near[:, cur:cur + n].copy()).cuda()
            outs = []
            for sb in (traced, twin):
                out = torch.full_like(tn, SENTINEL)
                assert sb.process_device(tn.data_ptr(), out.data_ptr(), n, n, ms_per_session=ms) == 0 and sb.synchronize() == 0
                outs.append(out.cpu().numpy())
            assert np.array_equal(outs[0], outs[1])
            cur, k, fl = cur + n, 1, None
            blobs.append(twin.export_sessions()[1])
        elif op[0] in ("tick", "calls1"):
            fl = op[1]
            a, b = ordinary(traced, fl, cur, "calls1" if op[0] == "calls1" else "flags"), ordinary(twin, fl, cur)
            live = np.ones(S, bool) if fl is None else (fl & IDLE) == 0
            assert a[0] == b[0] and np.array_equal(a[1][live], b[1][live])
            cur, k = cur + n, 1
            blobs.append(twin.export_sessions()[1])
        else:
            k, fl = op[1], op[2]
            rc, out = _k_tick(traced, "device", False, far[:, cur:cur + k * n].copy(), near[:, cur:cur + k * n].copy(), None, n, k, ms, fl)
            assert rc == 0
            live = np.ones(S, bool) if fl is None else (fl & IDLE) == 0
            for c in range(k):
                rc1, o1 = ordinary(twin, fl, cur + c * n)
                assert np.array_equal(out[live, c * n:(c + 1) * n], o1[live])
                blobs.append(twin.export_sessions()[1])
            cur += k * n
        for _ in range(k):
            called.append(np.ones(S, bool) if fl is None else (fl & IDLE) == 0)
        slot += k
        assert traced.call_trace_calls() == slot
    assert slot == C_
    called = np.array(called)
    want = sh.expected_records(start, blobs, called, [16000] * S)
    raw = buf.cpu().numpy().reshape(-1, REC.itemsize)
    got = raw[GUARD:GUARD + S * C_].reshape(-1).view(REC).reshape(S, C_)
    assert (got["tick"][called.T] == np.broadcast_to(np.arange(C_, dtype=np.uint32), (S, C_))[called.T]).all()
    st._assert_records(got, want, called.T, "mixed entry points")
    assert (raw[:GUARD] == FILL).all() and (raw[-GUARD:] == FILL).all()
    assert (raw[GUARD:GUARD + S * C_].reshape(S, C_, -1)[~called.T] == FILL).all()
    # detach: the same calls run, the buffer stays, the count is gone
    assert traced.clear_call_trace() == 0 and traced.call_trace_calls() == 0
    rc, out = _k_tick(traced, "device", False, far[:, cur:cur + 2 * n].copy(), near[:, cur:cur + 2 * n].copy(), None, n, 2, ms, None)
    for c in range(2):
        assert np.array_equal(out[:, c * n:(c + 1) * n], ordinary(twin, None, cur + c * n)[1])
    assert np.array_equal(buf.cpu().numpy().reshape(-1, REC.itemsize), raw) and traced.call_trace_calls() == 0
    assert traced.export_sessions() == twin.export_sessions()
    traced.close(), twin.close()


# ---- 6. refusals -------------------------------------------------------------------------------------------------------------
def test_refusals():
    """Every refusal against a twin that did not take the refused call: device state and trace bytes byte-equal, the count unmoved;
    the codes are those an object without a trace gives for the same call."""
    import torch
    S, n = 6, 160
    far, near, cl = st._signals((16000,) * S, 8 * n, 840)
    traced, twin, plain = (st._object([16000] * S) for _ in range(3))
    buf, ptr = st._trace_buffer(S * 4, GUARD)
    other, optr = st._trace_buffer(S * 4, GUARD)
    bad = ffi.AECM_BAD_PARAMETER_ERROR

    def bad_arguments():
        assert traced.lib.WebRtcAecmSessions_SetCallTrace(None, ptr, 4, 1, 4) == bad
        assert traced.set_call_trace(ptr + 2, 4, 1, 4) == bad
        assert traced.set_call_trace(ptr, 0, 1, 4) == bad and traced.set_call_trace(ptr, -1, 1, 4) == bad
        assert traced.set_call_trace(ptr, 4, 0, 4) == bad and traced.set_call_trace(ptr, 4, -2, 4) == bad
        assert traced.set_call_trace(ptr, 4, 1, 0) == bad and traced.set_call_trace(ptr, 4, 1, -3) == bad

    def k_tick(sb, k, calls, packets=False, fl=None, clean=False, width=None):
        width = 2 * n if width is None else width
        rows = [torch.from_numpy(x[:, k * n:k * n + width].copy()).cuda() for x in (far, near, cl)]
        out = torch.full_like(rows[1], SENTINEL)
        fn = sb.tick_packets_device if packets else sb.tick_calls_device
        rc, _ = fn(rows[0].data_ptr(), rows[1].data_ptr(), out.data_ptr(), width, n, calls, 40, clean_ptr=rows[2].data_ptr() if clean else None, flags=fl)
        assert sb.synchronize() == 0
        return rc, out.cpu().numpy()

    bad_arguments()
    assert traced.call_trace_calls() == 0
    assert traced.set_call_trace(ptr, 4, 1, 4) == 0
    for sb in (traced, twin, plain):
        assert k_tick(sb, 0, 2)[0] == 0
    assert traced.call_trace_calls() == 2
    bad_arguments()                                               # ... and the attached trace stays attached, its count too
    assert traced.call_trace_calls() == 2
    # the other kind while this one is attached; NULL of the other kind detaches nothing; the session trace's count answers for itself
    assert traced.set_session_trace(optr, 4, 1, 4) == bad and traced.clear_session_trace() == 0
    assert traced.call_trace_calls() == 2 and traced.session_trace_ticks() == 0
    before, raw_before = traced.export_sessions(), buf.cpu().numpy().copy()
    assert before == twin.export_sessions()
    no_clean = np.array([NO_CLEAN, 0, 0, 0, 0, 0], dtype=np.uint8)
    refused = [dict(calls=7), dict(calls=0), dict(calls=2, width=n), dict(calls=2, fl=np.full(S, SPLIT_CALLS, np.uint8)),
               dict(calls=2, fl=np.full(S, HALF_CALL, np.uint8)), dict(calls=2, packets=True, fl=np.full(S, SPLIT_CALLS, np.uint8)),
               dict(calls=2, fl=no_clean, clean=True), dict(calls=2, packets=True, fl=no_clean, clean=True)]
    for kw in refused:
        rc, out = k_tick(traced, 2, **kw)
        want, _ = k_tick(plain, 2, **kw)
        assert rc == want != 0, (kw, rc, want)
        assert (out == SENTINEL).all() and traced.call_trace_calls() == 2
        assert traced.export_sessions() == before and np.array_equal(buf.cpu().numpy(), raw_before), kw
    for sb in (traced, plain):                                    # the safe kernel variant
        assert sb.lib.WebRtcAecmSessions_SetKernelVariant(sb.h, ffi.KERNEL_SAFE) == 0
    for calls in (1, 2):
        rc, out = k_tick(traced, 2, calls)
        assert rc == k_tick(plain, 2, calls)[0] == ffi.AECM_UNSUPPORTED_FUNCTION_ERROR and (out == SENTINEL).all()
    for sb in (traced, plain):
        assert sb.lib.WebRtcAecmSessions_SetKernelVariant(sb.h, ffi.KERNEL_FAST) == 0
    assert traced.call_trace_calls() == 2 and traced.export_sessions() == before and np.array_equal(buf.cpu().numpy(), raw_before)
    # the sessions are as the twin's: the next accepted tick gives the twin's output, and its records land in slots 2 and 3
    a, b = k_tick(traced, 2, 2), k_tick(twin, 2, 2)
    assert a[0] == b[0] == 0 and np.array_equal(a[1], b[1]) and traced.call_trace_calls() == 4
    assert traced.export_sessions() == twin.export_sessions()
    got = buf.cpu().numpy().reshape(-1, REC.itemsize)[GUARD:GUARD + S * 4].reshape(-1).view(REC).reshape(S, 4)
    assert (got["tick"] == np.arange(4, dtype=np.uint32)).all()
    # a session trace attached: the call trace is refused, and the per-tick mode refuses what it refused
    assert traced.clear_call_trace() == 0 and traced.set_session_trace(optr, 4, 1, 4) == 0
    assert traced.set_call_trace(ptr, 4, 1, 4) == bad and traced.clear_call_trace() == 0
    assert k_tick(traced, 4, 2)[0] == ffi.AECM_UNSUPPORTED_FUNCTION_ERROR and traced.session_trace_ticks() == 0
    assert (other.cpu().numpy() == FILL).all()
    for sb in (traced, twin, plain):
        sb.close()


# ---- 7. the audit build ------------------------------------------------------------------------------------------------------
def test_checked_build_counts_nothing(tmp_path):
    """The K-call run and a packet run on the audit build (-DAECM_CHECKED), in a child process: the records are the yardstick's, the
    counters stay 0 0."""
    from webrtc_aecm_amd import build
    assert build.LIB_CHECKED.exists()
    script = tmp_path / "audit_call_trace.py"
    script.write_text(textwrap.dedent("""
        import webrtc_aecm_amd as aecm
        import test_gpu_call_trace as T
        assert aecm.check_counters(0, reset=True) is not None
        T.test_k_call_every_record_and_the_per_tick_trace()
        T.test_packet_records(2, True)
        c = aecm.check_counters(0)
        print("AUDIT", int(c[0]), int(c[1]))
    """))
    env = dict(os.environ, AECM_LIB_PATH=str(build.LIB_CHECKED),
               PYTHONPATH=os.pathsep.join([str(GOLDEN.parent.parent), str(GOLDEN.parent), os.environ.get("PYTHONPATH", "")]))
    r = subprocess.run([sys.executable, str(script)], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("AUDIT")]
    assert line and line[-1].split()[1:] == ["0", "0"], r.stdout[-500:]
