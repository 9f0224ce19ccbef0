"""The session trace on the device (include/aecm_batch.h: WebRtcAecmSessions_SetSessionTrace; aecm_tick_trace_kernels.hip): every
record of every traced tick launch -- dense, live list, both split-clean forms -- against the yardstick of
tests/session_trace_helpers.py (a twin object without a trace, exported after every tick), with outputs, codes and the final
snapshots equal to the twin's; idle sessions, flags, both rates, the ring and its layouts, bursts, TickAsync, the refusals, detaching
and the audit build.  The buffer is pre-filled with 0xA5.  The CPU side is tests/test_session_trace.py."""
import functools
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import session_trace_helpers as sh
import webrtc_aecm_amd as aecm
from helpers import GOLDEN
from oracle import pyoracle
from webrtc_aecm_amd import ffi
from webrtc_aecm_amd.synth import synth_clean, synth_pair

pytestmark = pytest.mark.gpu
REC = ffi.SESSION_TRACE_DTYPE
FILL = 0xA5
SENTINEL = 0x5A5A
NO_FAREND, SPLIT_CALLS, IDLE, HALF_CALL, NO_CLEAN = sh.NO_FAREND, sh.SPLIT_CALLS, sh.IDLE, sh.HALF_CALL, sh.NO_CLEAN


@functools.lru_cache(maxsize=None)
def _signals(rates, samples, seed0):
    """(far, near, clean) [S, samples]: session s from seed seed0 + s at its own rate; read-only, shared."""
    pairs = [synth_pair(seed0 + s, (samples + 63) // 64, fs) for s, fs in enumerate(rates)]
    far, near = np.stack([p[0][:samples] for p in pairs]), np.stack([p[1][:samples] for p in pairs])
    clean = synth_clean(near)
    for a in (far, near, clean):
        a.flags.writeable = False
    return far, near, clean


def _object(rates):
    rates = list(rates)
    return aecm.AecmSessions(len(rates), rates[0], 1, 3, rates=None if len(set(rates)) == 1 else rates)


def _trace_buffer(records, guard=0):
    """(tensor of (records + 2 guard) records of 0xA5, pointer of record `guard`)."""
    import torch
    t = torch.full(((records + 2 * guard) * REC.itemsize,), FILL, dtype=torch.uint8, device="cuda")
    return t, t.data_ptr() + guard * REC.itemsize


def _own(flags_t, n, S):
    """Samples of its rows every session consumes in a tick of n: 0 idle, 80 with a half call, else n."""
    fl = np.zeros(S, dtype=np.uint8) if flags_t is None else flags_t
    return np.where(fl & IDLE, 0, np.where(fl & HALF_CALL, 80, n)).astype(np.int64)


def _tick(sb, api, f, d, c, n, ms, fl):
    """One tick of [S, n] rows through `api`; returns (code, out [S, n] with SENTINEL where nothing was written)."""
    import torch
    if api == "host":
        rc, out, _ = sb.tick_host_per_session(f, d, ms, clean=c, flags=fl)
        return rc, out
    tf, tn = torch.from_numpy(f).cuda(), torch.from_numpy(d).cuda()
    tc = torch.from_numpy(c).cuda() if c is not None else None
    out = torch.full_like(tn, SENTINEL)
    torch.cuda.synchronize()
    cp = tc.data_ptr() if tc is not None else None
    args = (tf.data_ptr(), tn.data_ptr(), out.data_ptr(), n, n)
    if api == "per_session":
        rc = sb.tick_device_per_session(*args, ms, clean_ptr=cp)
    elif api == "flags":
        rc, _ = sb.tick_device_flags(*args, ms, np.zeros(len(ms), np.uint8) if fl is None else fl, clean_ptr=cp)
    elif api == "scalar":
        assert fl is None and len(set(ms.tolist())) == 1
        rc = sb.tick_device(*args, int(ms[0]), clean_ptr=cp)
    elif api == "async":
        done = torch.cuda.Event()
        done.record()
        rc = sb.tick_async(*args, clean_ptr=cp, ms_per_session=ms, flags=fl, done_event=done.cuda_event)
        done.synchronize()                       # the records are visible where out is
    elif api == "calls1":
        rc, _ = sb.tick_calls_device(*args, 1, ms, clean_ptr=cp, flags=fl)
    elif api == "packets1":
        rc, _ = sb.tick_packets_device(*args, 1, ms, clean_ptr=cp, flags=fl)
    else:
        raise ValueError(api)
    if api != "async":
        assert sb.synchronize() == 0
    return rc, out.cpu().numpy()


def _run(rates, n, ms, flags=None, clean=False, api="per_session", seed0=500, ring=None, strides=None, guard=0, setup=None, attach=True):
    """The schedule (ms [T, S], flags [T, S] or None) on a traced object and on its twin.  Asserts that outputs, codes and the final
    snapshots are the twin's.  Returns dict(trace raw uint8 [records + 2 guard, 64], rec expected [S, T], called [T, S], out [S, T n],
    ticks, signals)."""
    ms = np.asarray(ms, dtype=np.int16)
    T, S = ms.shape
    flags = None if flags is None else np.asarray(flags, dtype=np.uint8)
    far, near, cl = _signals(tuple(rates), T * n, seed0)
    traced, twin = _object(rates), _object(rates)
    for sb in (traced, twin):
        if setup:
            setup(sb)
    ring = T if ring is None else ring
    strides = (ring, 1) if strides is None else strides
    records = (S - 1) * strides[0] + (ring - 1) * strides[1] + 1
    buf, ptr = _trace_buffer(records, guard)
    if attach:
        assert traced.set_session_trace(ptr, strides[0], strides[1], ring) == 0
    rc, start = twin.export_sessions()
    assert rc == 0
    cur = np.zeros(S, dtype=np.int64)
    out = np.zeros((S, T * n), dtype=np.int16)
    blobs, called = [], np.zeros((T, S), dtype=bool)
    for t in range(T):
        fl = None if flags is None else flags[t]
        own = _own(fl, n, S)
        f, d, c = (np.full((S, n), 77, dtype=np.int16) for _ in range(3))
        for s in np.flatnonzero(own):
            f[s, :own[s]], d[s, :own[s]], c[s, :own[s]] = far[s, cur[s]:cur[s] + own[s]], near[s, cur[s]:cur[s] + own[s]], cl[s, cur[s]:cur[s] + own[s]]
        res = [_tick(sb, api, f, d, c if clean else None, n, ms[t], fl) for sb in (traced, twin)]
        assert res[0][0] == res[1][0], ("codes of tick", t, res[0][0], res[1][0])
        assert np.array_equal(res[0][1], res[1][1]), ("output of tick", t)
        for s in np.flatnonzero(own):
            out[s, cur[s]:cur[s] + own[s]] = res[0][1][s, :own[s]]
        cur += own
        called[t] = own > 0
        rc, blob = twin.export_sessions()
        assert rc == 0
        blobs.append(blob)
    ticks = traced.session_trace_ticks() if attach else 0
    assert traced.export_sessions() == twin.export_sessions(), "final snapshots"
    raw = buf.cpu().numpy().reshape(-1, REC.itemsize)
    traced.close(), twin.close()
    return dict(raw=raw, rec=sh.expected_records(start, blobs, called, rates), called=called, out=out, ticks=ticks, far=far, near=near, clean=cl,
                strides=strides, ring=ring, guard=guard)


def _records(r, S, T):
    """[S, T] records of a session-major ring of T ticks (every tick in its own slot)."""
    assert r["strides"] == (T, 1) and r["ring"] == T and r["guard"] == 0
    return r["raw"].reshape(-1).view(REC).reshape(S, T)


def _assert_records(got, want, mask, what):
    diff = sh.first_record_difference(got, want, mask)
    assert diff is None, f"{what}: {diff}"


def _steps(T, lo, hi, first, last):
    a = np.full(T, lo, dtype=np.int16)
    a[first:last] = hi
    return a


# ---- 1. the dense kernel ---------------------------------------------------------------------------------------------------
# 216 ticks, not 48: the core's start-up state first changes at its 512th block, 2.5 blocks per tick (the twin's track must be alive)
DENSE_S, DENSE_T = 9, 216
# (delay compensation keeps the estimated delay under 96 samples wherever the jitter buffer can hold msInSndCardBuf's worth of far end:
# knownDelay moves only for the sessions whose msInSndCardBuf exceeds its 4 000 samples -- 300, 400 and 500 ms at 16 kHz)
DENSE_MS = (40, 60, 100, 150, 200, 300, 400, 500)


def _dense_ms():
    ms = np.stack([np.full(DENSE_T, v, dtype=np.int16) for v in DENSE_MS] + [_steps(DENSE_T, 40, 120, 10, 80)], axis=1)      # the last: 40 -> 120 -> 40
    assert ms.shape == (DENSE_T, DENSE_S)
    return ms


@functools.lru_cache(maxsize=None)
def _dense_run():
    return _run([16000] * DENSE_S, 160, _dense_ms())


def test_dense_every_record_and_the_reference():
    """Nine 16 kHz sessions (two full workgroups and one wave), per-session msInSndCardBuf, ticks of 160 samples, session-major ring
    of one slot per tick: every record equals the yardstick; outputs equal the twin's and, for three sessions, the reference's."""
    r = _dense_run()
    everybody = np.ones((DENSE_S, DENSE_T), dtype=bool)
    sh.assert_track_is_alive(r["rec"])
    assert r["ticks"] == DENSE_T and r["called"].all()
    got = _records(r, DENSE_S, DENSE_T)
    assert (got["tick"] == np.arange(DENSE_T, dtype=np.uint32)).all() and (got["samp_khz"] == 16).all()
    _assert_records(got, r["rec"], everybody, "dense tick")
    ms = _dense_ms()
    for s in (0, 4, 8):
        if pyoracle.have_reference():
            ref = pyoracle.RefSession(16000, 1, 3)
        else:
            ref = aecm.Aecm()
            assert ref.init(16000) == 0 and ref.set_config(1, 3) == 0
        for t in range(DENSE_T):
            sl = slice(t * 160, (t + 1) * 160)
            assert ref.buffer_farend(r["far"][s, sl]) == 0
            rc, o = ref.process(r["near"][s, sl], ms=int(ms[t, s]))
            assert rc == 0 and np.array_equal(o, r["out"][s, sl]), ("the reference's output", s, t)


# ---- 2. a clean input ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fs,n,T", [(16000, 160, 24), (8000, 80, 40)], ids=["16000-160", "8000-80"])
def test_clean_input(fs, n, T):
    S = 5
    ms = np.stack([np.full(T, v, dtype=np.int16) for v in (40, 100, 200, 20, 300)], axis=1)
    r = _run([fs] * S, n, ms, clean=True, seed0=520)
    got = _records(r, S, T)
    assert {0, 1} <= set(r["rec"]["ec_startup"].ravel().tolist()) and (got["samp_khz"] == fs // 1000).all()
    _assert_records(got, r["rec"], np.ones((S, T), dtype=bool), "clean input")


# ---- 3. idle sessions: the live list ---------------------------------------------------------------------------------------
IDLE_S, IDLE_T, NOBODY_AT = 13, 33, 20


@functools.lru_cache(maxsize=None)
def _idle_schedule():
    rs = np.random.RandomState(3)
    flags = np.where(rs.rand(IDLE_T, IDLE_S) < 0.3, IDLE, 0).astype(np.uint8)
    flags[NOBODY_AT] = IDLE                                       # one tick nobody makes
    flags[0] = 0                                                   # (and one everybody makes)
    ms = np.broadcast_to(np.array([40, 60, 100, 150, 200, 300, 20, 80, 120, 250, 30, 500, 70], dtype=np.int16), (IDLE_T, IDLE_S))
    return flags, ms


@functools.lru_cache(maxsize=None)
def _idle_run():
    flags, ms = _idle_schedule()
    return _run([16000] * IDLE_S, 160, ms, flags=flags, api="flags", seed0=540)


def test_idle_sessions_keep_their_slots():
    """13 sessions, 30 % idle per tick, 32 ticks and one nobody makes: the records of the sessions that call are right, an idle
    session's slot of that tick is still 0xA5, and the count holds every accepted tick."""
    flags, _ = _idle_schedule()
    r = _idle_run()
    assert r["ticks"] == IDLE_T and not r["called"][NOBODY_AT].any() and 0.15 < 1 - r["called"].mean() < 0.45
    got = _records(r, IDLE_S, IDLE_T)
    live = r["called"].T
    assert (got["tick"][live] == np.broadcast_to(np.arange(IDLE_T, dtype=np.uint32), (IDLE_S, IDLE_T))[live]).all()
    _assert_records(got, r["rec"], live, "tick with idle sessions")
    raw = r["raw"].reshape(IDLE_S, IDLE_T, REC.itemsize)
    assert (raw[~live] == FILL).all(), "an idle session's slot was written"
    assert {0, 2, 3} <= set(r["rec"]["blocks"][live].tolist())


# ---- 4. flags and rates: the mixed planner ---------------------------------------------------------------------------------
def test_flags_and_both_rates():
    """An InitRates object of both rates, per-session HALF_CALL, NO_FAREND and SPLIT_CALLS at random: samp_khz shows 8 and 16, a
    split tick has ONE record, taken after its second call."""
    S, T = 10, 40
    rates = [16000 if s % 3 else 8000 for s in range(S)]
    rs = np.random.RandomState(4)
    choices = np.array([0, NO_FAREND, SPLIT_CALLS, HALF_CALL, HALF_CALL | NO_FAREND, SPLIT_CALLS | NO_FAREND, 0, 0], dtype=np.uint8)
    flags = choices[rs.randint(0, choices.size, (T, S))]
    flags[:8] &= ~np.uint8(NO_FAREND)                            # (a start-up phase that ends)
    ms = np.broadcast_to(np.array([40, 60, 100, 150, 200, 300, 20, 80, 120, 250], dtype=np.int16), (T, S))
    r = _run(rates, 160, ms, flags=flags, api="flags", seed0=560)
    got = _records(r, S, T)
    assert r["ticks"] == T and r["called"].all()
    assert set(got["samp_khz"].ravel().tolist()) == {8, 16} and (got["samp_khz"] == (np.array(rates) // 1000)[:, None]).all()
    assert {0, 1} <= set(r["rec"]["ec_startup"].ravel().tolist()) and {0, 1, 2, 3} <= set(r["rec"]["blocks"].ravel().tolist())
    _assert_records(got, r["rec"], np.ones((S, T), dtype=bool), "flags and rates")


# ---- 5. sessions without a clean input among others: both split-clean forms -------------------------------------------------
@pytest.mark.parametrize("two_launches", [False, True], ids=["fused", "one launch per list"])
def test_split_clean(two_launches):
    S, T = 7, 24
    flags = np.broadcast_to(np.array([NO_CLEAN if s % 2 else 0 for s in range(S)], dtype=np.uint8), (T, S)).copy()
    flags[5:, 2] |= IDLE                                           # (a list shorter than its neighbours')
    ms = np.broadcast_to(np.array([40, 60, 100, 150, 200, 300, 20], dtype=np.int16), (T, S))
    r = _run([16000] * S, 160, ms, flags=flags, clean=True, api="flags", seed0=580, setup=lambda sb: sb.split_clean_two_launches(two_launches))
    got = _records(r, S, T)
    live = r["called"].T
    assert r["ticks"] == T and {0, 1} <= set(r["rec"]["ec_startup"][live].tolist())
    _assert_records(got, r["rec"], live, f"split clean tick, two_launches={two_launches}")
    assert (r["raw"].reshape(S, T, REC.itemsize)[~live] == FILL).all()


# ---- 6. the ring and its layouts -------------------------------------------------------------------------------------------
def test_ring_and_tick_major_layout():
    """ring_ticks = 4 over 10 ticks, tick-major strides (1, S): slot j % 4 holds tick j of the last four, by its tick field, and
    nothing outside the ring's records is written."""
    S, T, R, G = 6, 10, 4, 3
    ms = np.broadcast_to(np.array([40, 60, 100, 150, 200, 300], dtype=np.int16), (T, S))
    r = _run([16000] * S, 160, ms, seed0=600, ring=R, strides=(1, S), guard=G)
    raw = r["raw"]
    assert raw.shape[0] == R * S + 2 * G and (raw[:G] == FILL).all() and (raw[G + R * S:] == FILL).all()
    ring = raw[G:G + R * S].reshape(-1).view(REC).reshape(R, S)
    for j in range(T - R, T):
        assert (ring[j % R]["tick"] == j).all(), (j, ring[j % R]["tick"])
        _assert_records(ring[j % R][:, None], r["rec"][:, j][:, None], None, f"slot {j % R} (tick {j})")
    assert r["ticks"] == T


# ---- 7. bursts, Process, TickAsync, the other entry points -----------------------------------------------------------------
def test_burst_writes_nothing_process_writes_one():
    import torch
    S, n = 5, 160
    far, near, _ = _signals((16000,) * S, 4 * n, 620)
    traced, twin = _object([16000] * S), _object([16000] * S)
    buf, ptr = _trace_buffer(S)
    assert traced.set_session_trace(ptr, 1, 1, 1) == 0
    tf = torch.from_numpy(far.copy()).cuda()
    tn = torch.from_numpy(near[:, :n].copy()).cuda()
    rc, start = twin.export_sessions()
    outs = []
    for sb in (traced, twin):
        assert sb.buffer_farend_device(tf.data_ptr(), 4 * n, n, 2) == 0
        assert sb.synchronize() == 0
        if sb is traced:
            assert (buf.cpu().numpy() == FILL).all() and sb.session_trace_ticks() == 0, "a burst wrote a record"
        out = torch.full_like(tn, SENTINEL)
        assert sb.process_device(tn.data_ptr(), out.data_ptr(), n, n, ms=50) == 0
        assert sb.synchronize() == 0
        outs.append(out.cpu().numpy())
    assert np.array_equal(outs[0], outs[1]) and traced.session_trace_ticks() == 1
    rc, blob = twin.export_sessions()
    want = sh.expected_records(start, [blob], np.ones((1, S), dtype=bool), [16000] * S)
    got = buf.cpu().numpy().view(REC).reshape(S, 1)
    assert (got["far_buffered"] == 2 * n).all() and (got["ms_in_snd_card_buf"] == 60).all()
    _assert_records(got, want, None, "Process behind a burst")
    assert traced.export_sessions() == twin.export_sessions()
    traced.close(), twin.close()


@pytest.mark.parametrize("api", ["async", "host", "scalar", "calls1", "packets1"])
def test_other_entry_points(api):
    """TickAsync (records visible behind done_hip_event), the host form, the one-ms tick, and TickCalls / TickPackets with calls = 1."""
    S, T = 5, 12
    ms = np.full((T, S), 60, dtype=np.int16) if api == "scalar" else np.broadcast_to(np.array([40, 60, 100, 150, 200], dtype=np.int16), (T, S))
    flags = None
    if api in ("async", "host"):
        flags = np.zeros((T, S), dtype=np.uint8)
        flags[3:, 1] = NO_FAREND
        flags[6, 2] = IDLE
    r = _run([16000] * S, 160, ms, flags=flags, api=api, seed0=640)
    got = _records(r, S, T)
    assert r["ticks"] == T and {0, 1} <= set(r["rec"]["ec_startup"][r["called"].T].tolist())
    _assert_records(got, r["rec"], r["called"].T, api)


# ---- 8. refusals -----------------------------------------------------------------------------------------------------------
def test_refusals():
    import torch
    S, n = 6, 160
    far, near, _ = _signals((16000,) * S, 6 * n, 660)
    traced, twin = _object([16000] * S), _object([16000] * S)
    buf, ptr = _trace_buffer(S + 1)
    bad = ffi.AECM_BAD_PARAMETER_ERROR
    lib = traced.lib

    def bad_arguments():
        assert lib.WebRtcAecmSessions_SetSessionTrace(None, ptr, 1, 1, 1) == bad
        assert traced.set_session_trace(ptr + 2, 1, 1, 1) == bad
        assert traced.set_session_trace(ptr, 0, 1, 1) == bad and traced.set_session_trace(ptr, -1, 1, 1) == bad
        assert traced.set_session_trace(ptr, 1, 0, 1) == bad
        assert traced.set_session_trace(ptr, 1, 1, 0) == bad and traced.set_session_trace(ptr, 1, 1, -3) == bad

    def one_tick(k, calls=1, packets=False):
        tf, tn = torch.from_numpy(far[:, k * n:(k + 2) * n].copy()).cuda(), torch.from_numpy(near[:, k * n:(k + 2) * n].copy()).cuda()
        res = []
        for sb in (traced, twin):
            out = torch.full_like(tn, SENTINEL)
            fn = sb.tick_packets_device if packets else sb.tick_calls_device
            rc, _ = fn(tf.data_ptr(), tn.data_ptr(), out.data_ptr(), 2 * n, n, calls, 40)
            assert sb.synchronize() == 0
            res.append((rc, out.cpu().numpy()))
        return res

    bad_arguments()
    assert traced.session_trace_ticks() == 0
    res = one_tick(0)                                             # nothing is attached: nothing is written
    assert res[0][0] == 0 and np.array_equal(res[0][1], res[1][1]) and (buf.cpu().numpy() == FILL).all()
    assert traced.set_session_trace(ptr, 1, 1, 1) == 0
    res = one_tick(1)
    assert res[0][0] == 0 and traced.session_trace_ticks() == 1
    bad_arguments()                                               # ... and the attached trace stays attached, its count too
    assert traced.session_trace_ticks() == 1
    before, raw_before = traced.export_sessions(), buf.cpu().numpy().copy()
    assert before == twin.export_sessions()
    for packets in (False, True):
        tf, tn = torch.from_numpy(far[:, 2 * n:4 * n].copy()).cuda(), torch.from_numpy(near[:, 2 * n:4 * n].copy()).cuda()
        out = torch.full_like(tn, SENTINEL)
        fn = traced.tick_packets_device if packets else traced.tick_calls_device
        rc, _ = fn(tf.data_ptr(), tn.data_ptr(), out.data_ptr(), 2 * n, n, 2, 40)
        assert rc == ffi.AECM_UNSUPPORTED_FUNCTION_ERROR and traced.synchronize() == 0
        assert (out.cpu().numpy() == SENTINEL).all() and traced.session_trace_ticks() == 1
        assert traced.export_sessions() == before and np.array_equal(buf.cpu().numpy(), raw_before)
    assert traced.clear_session_trace() == 0 and traced.session_trace_ticks() == 0
    for packets in (False, True):                                 # the same calls run once the trace is gone
        res = one_tick(2 if not packets else 4, calls=2, packets=packets)
        assert res[0][0] == 0 and np.array_equal(res[0][1], res[1][1]) and not (res[0][1] == SENTINEL).all()
    assert traced.export_sessions() == twin.export_sessions() and np.array_equal(buf.cpu().numpy(), raw_before)
    traced.close(), twin.close()


# ---- 9. detaching ----------------------------------------------------------------------------------------------------------
def test_detach_leaves_the_buffer_and_changes_no_output():
    """Ticks behind clear_session_trace() leave the buffer untouched; an attach -- detach cycle in the middle of a run changes no
    output: the whole run equals a run that never had a trace."""
    S, T, n = 5, 16, 160
    ms = np.broadcast_to(np.array([40, 60, 100, 150, 200], dtype=np.int16), (T, S))
    plain = _run([16000] * S, n, ms, seed0=680, attach=False)
    assert (plain["raw"] == FILL).all()
    far, near, _ = plain["far"], plain["near"], None
    sb = _object([16000] * S)
    buf, ptr = _trace_buffer(S * 4)
    out = np.zeros_like(plain["out"])
    snap = None
    for t in range(T):
        if t == 4:
            assert sb.set_session_trace(ptr, 4, 1, 4) == 0
        if t == 10:
            assert sb.session_trace_ticks() == 6 and sb.clear_session_trace() == 0
            snap = buf.cpu().numpy().copy()
            assert (snap.view(REC).reshape(S, 4)["tick"] == np.array([4, 5, 2, 3], dtype=np.uint32)).all()
        rc, o = _tick(sb, "per_session", far[:, t * n:(t + 1) * n].copy(), near[:, t * n:(t + 1) * n].copy(), None, n, np.ascontiguousarray(ms[t]), None)
        assert rc == 0
        out[:, t * n:(t + 1) * n] = o
    assert np.array_equal(buf.cpu().numpy(), snap), "a tick behind clear_session_trace() wrote a record"
    assert np.array_equal(out, plain["out"])
    want = plain["rec"]
    got = snap.view(REC).reshape(S, 4)
    for j, tick in ((0, 8), (1, 9), (2, 6), (3, 7)):              # the records of ticks 8, 9, 6, 7 of the run = ticks 4, 5, 2, 3 of the trace
        w = want[:, tick].copy()
        w["tick"] = tick - 4
        _assert_records(got[:, j][:, None], w[:, None], None, f"slot {j}")
    sb.close()


# ---- 10. the audit build ---------------------------------------------------------------------------------------------------
def test_checked_build_counts_nothing(tmp_path):
    """Tests 1 and 3 on the audit build (-DAECM_CHECKED), in a child process: the records are the yardstick's, the counters stay 0 0."""
    from webrtc_aecm_amd import build
    assert build.LIB_CHECKED.exists()
    script = tmp_path / "audit_session_trace.py"
    script.write_text(textwrap.dedent("""
        import webrtc_aecm_amd as aecm
        import test_gpu_session_trace as T
        assert aecm.check_counters(0, reset=True) is not None
        T.test_dense_every_record_and_the_reference()
        T.test_idle_sessions_keep_their_slots()
        c = aecm.check_counters(0)
        print("AUDIT", int(c[0]), int(c[1]))
    """))
    env = dict(os.environ, AECM_LIB_PATH=str(build.LIB_CHECKED),
               PYTHONPATH=os.pathsep.join([str(GOLDEN.parent.parent), str(GOLDEN.parent), os.environ.get("PYTHONPATH", "")]))
    r = subprocess.run([sys.executable, str(script)], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("AUDIT")]
    assert line and line[-1].split()[1:] == ["0", "0"], r.stdout[-500:]
