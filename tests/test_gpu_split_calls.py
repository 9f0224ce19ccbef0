"""K-call and packet ticks with a clean near-end input per session on the GPU (WebRtcAecmSessions_SetSplitCallTicks): a tick of K call
pairs that carries a clean plane, in which the sessions flagged AECM_SESSION_NO_CLEAN get nearendClean = NULL in all K of their
WebRtcAecm_Process calls and every other session its clean row.

The reference of every run but the twins' is one WebRtcAecm_* instance per session (the unmodified reference where oracle/_ref exists,
the project's single-session ABI otherwise), a flagged session's never handed a clean pointer (split_calls_helpers.WithoutClean).  The
flagged sessions' clean rows hold junk in all K pieces.  Every output sample, every code, the echo paths and the modes must be equal.
No exclusions.  Without the feature every test here stops at set_split_call_ticks."""
import os
import subprocess
import sys
import textwrap
from pathlib import Path

import numpy as np
import pytest

import calls_helpers as ch
import mixed_helpers as mh
import packets_helpers as ph
import sparse_helpers as sh
import split_calls_helpers as sch
import split_helpers as sph
import webrtc_aecm_amd as aecm

pytestmark = pytest.mark.gpu

IDLE, NO_FAREND, NO_CLEAN, HALF = sph.IDLE, sph.NO_FAREND, sph.NO_CLEAN, sph.HALF_CALL
BAD, UNSUPPORTED = aecm.ffi.AECM_BAD_PARAMETER_ERROR, aecm.ffi.AECM_UNSUPPORTED_FUNCTION_ERROR
S11, NEVER11 = sph.S11, sph.NEVER11
TESTS = Path(__file__).resolve().parent
_runs = {}


def modes_of(sb):
    got = [sb.get_session_clean_mode(s) for s in range(sb.num_streams)]
    assert all(rc == 0 for rc, _ in got)
    return [m for _, m in got]


def kinds_modes(S, never):
    return [sph.NEVER if s in set(never) else sph.ALWAYS for s in range(S)]


def check(out, codes, sb, exp, what):
    exp_out, exp_codes, exp_paths = exp
    assert np.array_equal(codes, exp_codes), (what, np.argwhere(codes != exp_codes)[:3].tolist())
    bad = np.argwhere(out != exp_out)
    assert bad.size == 0, (what, "first difference: session, sample", bad[0].tolist(), "differing sessions", sorted(set(bad[:, 0].tolist())))
    for s in range(out.shape[0]):
        rc, path = sb.get_echo_path(s)
        assert rc == 0 and np.array_equal(path, exp_paths[s]), (what, "echo path of session", s)


# ---- 1. the uniform object --------------------------------------------------------------------------------------------------------
def uniform_case(fs, n, K):
    """11 sessions, about 30 packets of K calls: pattern, signals and the reference's results, computed once per case and shared."""
    key = (fs, n, K)
    if key not in _runs:
        T = 30 if K < 6 else 16
        flags, ms = sch.kinds_pattern(9900 + K + n, S11, T, NEVER11)
        far, near, clean = sh.signals(9900 + K, S11, T * K * n, fs, with_clean=True)
        ops = ch.calls_ops(K, n, flags, ms)
        refs = sch.reference_sessions(sch.make_reference(), [fs] * S11, NEVER11)
        out, codes, _ = ch.run_reference(None, ops, ch.Feed(far, near, clean), sessions=refs)
        paths = np.stack([r.get_echo_path()[1] for r in refs])
        for a in (out, codes, paths):
            a.setflags(write=False)
        _runs[key] = (flags, ms, ops, far, near, sph.object_clean(clean, NEVER11), (out, codes, paths))
    return _runs[key]


@pytest.mark.parametrize("form", ["device", "host", "async"])
@pytest.mark.parametrize("fs,n,K", [(16000, 160, 2), (16000, 160, 3), (16000, 160, 6), (8000, 80, 3)])
def test_uniform_object(fs, n, K, form):
    """Sessions 0, 2, .. 10 without a clean input, 1, 3, .. 9 with: 30 % idle (idle bytes carrying the bit at random), NO_FAREND
    underruns, per-session msInSndCardBuf with out-of-range values, junk in all K pieces of the flagged sessions' clean rows; TickCalls,
    TickCallsHost and TickCallsAsync.  Halfway every session moves into a second object by ExportSessions / ImportSessions and continues
    there.  Every session leaves its start-up phase; the clean list is a multiple of four in some ticks and not in others."""
    flags, ms, ops, far, near, clean_obj, ref = uniform_case(fs, n, K)
    calling = (flags & IDLE) == 0
    lc = (calling & ((flags & NO_CLEAN) == 0)).sum(axis=1)
    lp = (calling & ((flags & NO_CLEAN) != 0)).sum(axis=1)
    both = (lc > 0) & (lp > 0)
    assert (lc[both] % 4 != 0).any() and (lc[both] % 4 == 0).any() and both.sum() > len(ops) * 3 // 4
    assert (((flags & NO_CLEAN) != 0) & ~calling)[:, [s for s in range(S11) if s not in NEVER11]].any()      # idle bytes of "always" sessions with the bit
    assert (ms[calling] == 700).any()
    cut = len(ops) // 2
    feed = ch.Feed(far, near, clean_obj)
    a = sch.switched_object(S11, fs)
    out0, codes0 = ch.run_object(a, ops[:cut], feed, form=form)
    assert modes_of(a) == kinds_modes(S11, NEVER11)
    rc, snaps = a.export_sessions()
    assert rc == 0
    b = sch.switched_object(S11, fs)
    warm = np.zeros((S11, n), dtype=np.int16)
    for _ in range(3):                                   # (an age of its own, and a clean ring of its own)
        assert b.tick_host_per_session(warm, warm, np.full(S11, 40, np.int16), clean=warm)[0] == 0
    assert b.import_sessions(None, snaps) == 0 and modes_of(b) == [sph.NONE] * S11
    out1, codes1 = ch.run_object(b, ops[cut:], feed, form=form)
    out, codes = np.concatenate([out0, out1], axis=1), np.concatenate([codes0, codes1])
    check(out, codes, b, ref, (fs, n, K, form))
    assert modes_of(b) == kinds_modes(S11, NEVER11)
    # every session has left its start-up phase: its last packet is not the copy of its (clean or noisy) near end
    for s in range(S11):
        t = int(np.flatnonzero(calling[:, s])[-1])
        seen = int(calling[:t, s].sum()) * K * n
        src = near if s in NEVER11 else clean_obj
        assert not np.array_equal(out[s, t * K * n:(t + 1) * K * n], src[s, seen:seen + K * n]), s
    # ... and a flagged session's first one IS the copy of its noisy near end
    s = NEVER11[1]
    t = int(np.flatnonzero(calling[:, s])[0])
    assert np.array_equal(out[s, t * K * n:t * K * n + n], near[s, :n])
    a.close(), b.close()


# ---- 2. packet ticks on the mixed-rate object -----------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["device", "host", "async"])
@pytest.mark.parametrize("K", [2, 3])
def test_packet_ticks_on_the_mixed_rate_object(K, form):
    """The 9 sessions of mixed_helpers (both rates; 8 kHz sessions and sometimes a 16 kHz one on half calls, packed rows), sessions
    1, 3, 5, 8 without a clean input: the packet planning lane at per-session rates with two lists, and the packet body per list.
    Against the instances and against a twin of K ordinary split ticks flagged HALF_CALL on re-laid rows."""
    key = ("mixed", K)
    if key not in _runs:
        T = 36 // K + 14
        flags, ms = ph.golden_pattern(K, 9950 + K)
        reps = -(-T // flags.shape[0])
        flags, ms = np.tile(flags, (reps, 1))[:T].copy(), np.tile(ms, (reps, 1))[:T].copy()
        flags[:, list(sph.NEVER9)] |= NO_CLEAN
        far, near, clean = mh.signals(9950 + K, mh.RATES, T * K * 160, with_clean=True)
        ops = ph.packets_ops(K, 160, flags, ms)
        refs = sch.reference_sessions(sch.make_reference(), mh.RATES, sph.NEVER9)
        out, codes, _ = ph.run_reference(None, mh.RATES, ops, ph.Feed(far, near, clean), sessions=refs)
        paths = np.stack([r.get_echo_path()[1] for r in refs])
        clean_obj = sph.object_clean(clean, sph.NEVER9)
        twin = aecm.AecmSessions(mh.S9, mh.OBJECT_FS, 1, 3, rates=mh.RATES)
        tout, tcodes = ph.run_object(twin, ops, ph.Feed(far, near, clean_obj), as_single_ticks=True)
        assert np.array_equal(tout, out) and np.array_equal(tcodes, codes), "the twin itself"
        rc, tsnaps = twin.export_sessions()
        assert rc == 0
        twin.close()
        _runs[key] = (flags, ops, far, near, clean_obj, (out, codes, paths), tsnaps)
    flags, ops, far, near, clean_obj, ref, tsnaps = _runs[key]
    calling = (flags & IDLE) == 0
    assert (calling & ((flags & (HALF | NO_CLEAN)) == (HALF | NO_CLEAN))).any() and (calling & ((flags & (HALF | NO_CLEAN)) == HALF)).any()
    sb = sch.switched_object(mh.S9, mh.OBJECT_FS, rates=mh.RATES)
    out, codes = ph.run_object(sb, ops, ph.Feed(far, near, clean_obj), form=form)
    check(out, codes, sb, ref, ("mixed", K, form))
    assert modes_of(sb) == kinds_modes(mh.S9, sph.NEVER9)
    rc, snaps = sb.export_sessions()
    assert rc == 0
    size = len(snaps) // mh.S9
    for s in range(mh.S9):
        assert sh.snapshot_state(snaps[s * size:(s + 1) * size]) == sh.snapshot_state(tsnaps[s * size:(s + 1) * size]), ("state of session", s)
    sb.close()


# ---- 3. 300 sessions: two planning workgroups ---------------------------------------------------------------------------------
def test_300_sessions_across_a_planning_workgroup():
    """300 sessions, K = 2, 20 packets of 160-sample calls.  The first wavefront is all of one kind.  Packet 0: only flagged sessions
    call -- the K-call tick without a clean plane: the object still has no clean ring (the snapshot header says so).  Packet 10: those
    sit out, nobody who calls is flagged: the K-call tick with a clean input.  Before packet 13 session 130 is initialised anew and
    switches kind."""
    S, T, n, K, SW, T_SW = 300, 20, 160, 2, 130, 13
    never = np.zeros(S, dtype=bool)
    never[:70] = True
    never[70:256:3] = True
    never[256::2] = True
    never[SW] = False
    rng = np.random.default_rng(9960)
    flags = np.zeros((T, S), dtype=np.uint8)
    flags[:, never] = NO_CLEAN
    flags |= (rng.random((T, S)) < 0.1).astype(np.uint8) * NO_FAREND
    flags[rng.random((T, S)) < 0.2] |= IDLE
    flags[0, ~never] = IDLE
    flags[0, never] &= ~np.uint8(IDLE)
    flags[10, never] |= IDLE
    flags[10, ~never] &= ~np.uint8(IDLE)
    flags[T_SW:, SW] |= NO_CLEAN
    flags[T_SW, SW] &= ~np.uint8(IDLE)
    ms = (40 + (np.arange(S) % 40)[None, :] + rng.integers(-3, 4, (T, S))).astype(np.int16)
    base = sh.signals(9960, 20, T * K * n, 16000, with_clean=True)
    pick = np.arange(S) % 20
    far, near, clean = (a[pick] for a in base)
    near = (near + (np.arange(S)[:, None] // 20)).astype(np.int16)          # (fifteen sessions share a far end; their near ends differ)
    make = sch.make_reference()
    never_after = never.copy()
    never_after[SW] = True
    refs = sch.reference_sessions(make, [16000] * S, np.flatnonzero(never))
    sb = sch.switched_object(S, 16000)
    ops = ch.calls_ops(K, n, flags, ms)
    feed, rfeed = ch.Feed(far, near, None), ch.Feed(far, near, clean)
    for t0, t1 in ((0, 1), (1, T_SW), (T_SW, T)):
        if t0 == T_SW:
            assert sb.init_session(SW) == 0 and sb.set_config_session(SW, 1, 3) == 0 and sb.get_session_clean_mode(SW) == (0, sph.NONE)
            refs[SW] = sch.WithoutClean(make(16000))
            feed.cur[SW] = rfeed.cur[SW] = 0
        kinds = never_after if t0 >= T_SW else never
        feed.clean = sph.object_clean(clean, np.flatnonzero(kinds))
        out, codes = ch.run_object(sb, ops[t0:t1], feed, form="device")
        eout, ecodes, _ = ch.run_reference(None, ops[t0:t1], rfeed, sessions=refs)
        check(out, codes, sb, (eout, ecodes, [r.get_echo_path()[1] for r in refs]), (t0, t1))
        if t0 == 0:
            rc, snap = sb.export_session(0)
            assert rc == 0 and int(np.frombuffer(snap[12:16], dtype=np.uint32)[0]) == 0        # has_clean: no clean ring was made
            assert modes_of(sb) == [sph.NEVER if k else sph.NONE for k in never]
    assert modes_of(sb) == [sph.NEVER if k else sph.ALWAYS for k in never_after]
    sb.close()


# ---- 4. interchangeable with ordinary split ticks -----------------------------------------------------------------------------
def test_interchangeable_with_ordinary_split_ticks():
    """Twin objects of 257 sessions, no reference: K = 2, 3, 6 in turn, ordinary ticks, BufferFarend + Process and a tick of another K
    in between; one twin makes every K-call tick as such, the other as K ordinary split ticks on the same rows.  Outputs and the
    snapshots of all sessions are byte for byte equal after every packet."""
    S, fs, n = 257, 16000, 160
    rng = np.random.default_rng(9970)
    never = np.flatnonzero(rng.random(S) < 0.45)
    kinds = np.zeros(S, dtype=np.uint8)
    kinds[never] = NO_CLEAN
    plan = [("calls", 2), ("tick", 1), ("calls", 3), ("burst", 2), ("calls", 6), ("calls", 4), ("calls", 2), ("tick", 1), ("calls", 3), ("calls", 6), ("burst", 1),
            ("calls", 5), ("calls", 2), ("calls", 3), ("calls", 6)]
    ops = []
    for kind, k in plan:
        fl = kinds | (rng.random(S) < 0.25).astype(np.uint8) * IDLE | (rng.random(S) < 0.1).astype(np.uint8) * NO_FAREND
        ms = (40 + (np.arange(S) % 50) + rng.integers(-5, 6, S)).astype(np.int16)
        ops.append(dict(kind="calls", K=k, n=n, flags=fl, ms=ms) if kind == "calls" else dict(kind="burst", B=k, n=n, ms=ms) if kind == "burst"
                   else dict(kind="tick", n=n, flags=fl, ms=ms))
    total = sum(ch.span_of(op) for op in ops)
    base = sh.signals(9970, 16, total, fs, with_clean=True)
    pick = np.arange(S) % 16
    far, near = base[0][pick], (base[1][pick] + np.arange(S)[:, None] // 16).astype(np.int16)
    clean = sph.object_clean(base[2][pick], never)
    farx = sh.signals(9971, 16, 4000, fs)[0][pick]
    assert farx.shape[1] >= sum(op["B"] * n for op in ops if op["kind"] == "burst")
    a, b = sch.switched_object(S, fs), aecm.AecmSessions(S, fs, 1, 3)
    fa, fb = ch.Feed(far, near, clean, farx), ch.Feed(far, near, clean, farx)
    # (a burst op's Process hands everybody the clean plane: after a split tick that is refused -- the burst goes in front of an ordinary tick)
    for i, op in enumerate(ops):
        if op["kind"] == "burst":
            fx = fa.burst_rows(op["B"] * n)
            fb.burst_rows(op["B"] * n)
            assert a.buffer_farend_host(fx, n, op["B"]) == 0 and b.buffer_farend_host(fx, n, op["B"]) == 0
            op = dict(kind="tick", n=n, flags=kinds | NO_FAREND, ms=op["ms"])
        oa, ca = ch.run_object(a, [op], fa, form="device" if i % 2 else "host")
        ob, cb = ch.run_object(b, [op], fb, as_single_ticks=True)
        assert np.array_equal(oa, ob) and np.array_equal(ca, cb), (i, op["kind"])
        ra, rb = a.export_sessions(), b.export_sessions()
        assert ra[0] == 0 and rb[0] == 0 and ra[1] == rb[1], (i, op["kind"])
    assert modes_of(a) == modes_of(b) == kinds_modes(S, never)
    a.close(), b.close()


# ---- 5. K = 6 with a replay-row spill -----------------------------------------------------------------------------------------
def test_replay_row_spill_inside_a_split_tick():
    """flow_corpus' calls6_spill schedule (ordinary ticks, then ticks of six, five and four calls of 80 samples during which farendOld[1]
    is lapped in the far ring and moves to its row in the middle of a tick's calls, then ticks without a far end that replay it), 84
    sessions, every other one flagged, with a clean plane."""
    import flow_corpus as fc
    sch_ = fc.schedule_calls_spill(sessions=84)
    T, S = sch_["flags"].shape
    never = np.arange(1, S, 2)
    flags = sch_["flags"].copy()
    flags[:, never] |= NO_CLEAN
    far, near = fc.signals(sch_)
    clean = (near.astype(np.int32) * 3 // 4).astype(np.int16)
    ops = []
    for t in range(T):
        n, K, kind, _, _ = fc.tick_layout(sch_, t)
        ops.append(dict(kind="calls", K=K, n=n, flags=flags[t], ms=sch_["ms"][t]) if kind else dict(kind="tick", n=n, flags=flags[t], ms=sch_["ms"][t]))
    assert {op["K"] for op in ops if op["kind"] == "calls"} == {2, 4, 5, 6}
    refs = sch.reference_sessions(sch.make_reference(), [16000] * S, never)
    eout, ecodes, _ = ch.run_reference(None, ops, ch.Feed(far, near, clean), sessions=refs)
    sb = sch.switched_object(S, 16000)
    out, codes = ch.run_object(sb, ops, ch.Feed(far, near, sph.object_clean(clean, never)), form="host")
    check(out, codes, sb, (eout, ecodes, [r.get_echo_path()[1] for r in refs]), "calls6_spill")
    sb.close()


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing():
    """Twins take the same accepted K-call split ticks; one also takes, before each, every refused form -- the switch off, a changed
    kind, call-traced, and what TickCalls / TickPackets always refused -- through the sync, async and host entry points.  The refused
    calls leave a sentinel out plane untouched; the twins' outputs and snapshots stay byte for byte equal."""
    import torch
    S, fs, n, K = 11, 16000, 160, 2
    SENT = 0x7b7b
    kinds = np.zeros(S, dtype=np.uint8)
    kinds[list(NEVER11)] = NO_CLEAN
    far, near, clean = sh.signals(9980, S, 8 * K * n, fs, with_clean=True)
    clean = sph.object_clean(clean, NEVER11)
    a, b = sch.switched_object(S, fs), sch.switched_object(S, fs)
    ms = np.full(S, 40, dtype=np.int16)
    W = 3 * n                                                                   # every plane of the refused calls: rows of the longest one that is sized right
    host = {k: np.ascontiguousarray(v[:, :W]) for k, v in (("far", far), ("near", near), ("clean", clean))}
    dev = {k: torch.from_numpy(v).cuda() for k, v in host.items()}
    dout = torch.full((S, W), SENT, dtype=torch.int16, device="cuda")
    hout = np.full((S, W), SENT, dtype=np.int16)
    trace = torch.zeros(S * 4 * 16, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()

    def refused(flags, want, packets=False, calls=K):
        fl = np.ascontiguousarray(flags, dtype=np.uint8)
        codes = np.zeros(S, dtype=np.int32)
        name = "WebRtcAecmSessions_Tick" + ("Packets" if packets else "Calls")
        common = lambda p: [a.h, p("far"), p("near"), p("clean"), None, W, n, calls, 40, ms.ctypes.data, fl.ctypes.data, codes.ctypes.data]
        for form in ("", "Async", "Host"):
            args = common((lambda k: host[k].ctypes.data) if form == "Host" else (lambda k: dev[k].data_ptr()))
            args[4] = hout.ctypes.data if form == "Host" else dout.data_ptr()
            assert getattr(a.lib, name + form)(*args, *((None, None) if form == "Async" else ())) == want, (name + form, want)
        assert a.synchronize() == 0
        assert (hout == SENT).all() and bool((dout == SENT).all()), "a refused call wrote its out plane"

    feeds = [ch.Feed(far, near, clean), ch.Feed(far, near, clean)]
    for t in range(6):
        before = (a.export_sessions(), modes_of(a))
        if t > 0:                                                               # (before any split tick nobody has a kind to change)
            bad = kinds.copy()
            bad[1] = NO_CLEAN
            refused(bad, BAD)                                                   # always + flagged
            bad = kinds.copy()
            bad[0] = 0
            refused(bad, BAD, packets=True)                                     # never + unflagged
        assert a.set_split_call_ticks(False) == 0
        refused(kinds, UNSUPPORTED)
        refused(kinds, UNSUPPORTED, packets=True, calls=3)
        assert a.set_split_call_ticks(True) == 0
        assert a.set_call_trace(trace.data_ptr(), 4, 1, 4) == 0
        refused(kinds, UNSUPPORTED)                                             # call-traced: whatever the switch says
        assert a.call_trace_calls() == 0 and a.clear_call_trace() == 0
        refused(kinds | sph.SPLIT_CALLS, BAD)
        refused(kinds | HALF, BAD)                                              # a half call in TickCalls
        refused(kinds, BAD, calls=7)
        assert a.lib.WebRtcAecmSessions_SetKernelVariant(a.h, aecm.ffi.KERNEL_SAFE) == 0
        refused(kinds, UNSUPPORTED)
        assert a.lib.WebRtcAecmSessions_SetKernelVariant(a.h, aecm.ffi.KERNEL_FAST) == 0
        assert (a.export_sessions(), modes_of(a)) == before
        fl = kinds.copy()
        fl[(t * 3 + 5) % S] |= IDLE
        op = dict(kind="calls", K=K, n=n, flags=fl, ms=ms)
        oa, ca = ch.run_object(a, [op], feeds[0], form="device")
        ob, cb = ch.run_object(b, [op], feeds[1], form="device")
        assert np.array_equal(oa, ob) and np.array_equal(ca, cb) and a.export_sessions() == b.export_sessions(), t
    assert not bool(trace.any())
    # two rates in TickCalls stay refused with the switch on; the packet form of the same tick is accepted
    m = sch.switched_object(mh.S9, mh.OBJECT_FS, rates=mh.RATES)
    z = np.zeros((mh.S9, K * n), dtype=np.int16)
    k9 = np.zeros(mh.S9, dtype=np.uint8)
    k9[list(sph.NEVER9)] = NO_CLEAN
    assert m.tick_calls_host(z, z, K, np.full(mh.S9, 40, np.int16), clean=z, flags=k9)[0] == UNSUPPORTED
    assert m.tick_packets_host(z, z, K, np.full(mh.S9, 40, np.int16), clean=z, flags=k9)[0] == 0
    m.close(), a.close(), b.close()


# ---- 7. the audit build, and the golden run ---------------------------------------------------------------------------------
def test_checked_build_counts_nothing(tmp_path):
    """One uniform run on the audit build (-DAECM_CHECKED), in a child process: the results are the reference's and the counters --
    which include the new tick unit's pair -- stay 0 0."""
    from webrtc_aecm_amd import build
    assert build.LIB_CHECKED.exists()
    script = tmp_path / "audit_split_calls.py"
    script.write_text(textwrap.dedent("""
        import webrtc_aecm_amd as aecm
        import test_gpu_split_calls as T
        assert aecm.check_counters(0, reset=True) is not None
        T.test_uniform_object(16000, 160, 3, "device")
        c = aecm.check_counters(0)
        print("AUDIT", int(c[0]), int(c[1]))
    """))
    env = dict(os.environ, AECM_LIB_PATH=str(build.LIB_CHECKED), PYTHONPATH=os.pathsep.join([str(TESTS.parent), str(TESTS), os.environ.get("PYTHONPATH", "")]))
    r = subprocess.run([sys.executable, str(script)], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("AUDIT")]
    assert line and line[-1].split()[1:] == ["0", "0"], r.stdout[-500:]


@pytest.mark.parametrize("name", sorted(sch.GOLDEN_CASES))
def test_golden_run(name):
    """tests/golden/sesssplitcalls_*.npz: the unmodified reference's outputs, codes and final echo paths of 11 sessions x 48 calls."""
    fs, n, K, seed = sch.GOLDEN_CASES[name]
    g = np.load(sh.GOLDEN_CASES_DIR / f"{name}.npz")
    flags, ms = g["flags"], g["ms"]
    assert int(g["seed"]) == seed and int(g["calls"]) == K and flags.shape == (sch.GOLDEN_CALLS // K, S11)
    far, near, clean = sh.signals(seed, S11, sch.GOLDEN_CALLS * n, fs, with_clean=True)
    for form in ("device", "host"):
        sb = sch.switched_object(S11, fs)
        out, codes = ch.run_object(sb, ch.calls_ops(K, n, flags, ms), ch.Feed(far, near, sph.object_clean(clean, NEVER11)), form=form)
        check(out, codes, sb, (g["out"], g["codes"], g["paths"]), ("golden", form))
        sb.close()
