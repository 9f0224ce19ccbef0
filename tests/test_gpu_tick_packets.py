"""Packet ticks on the GPU (WebRtcAecmSessions_TickPackets / TickPacketsHost / TickPacketsAsync): one tick is one packet of K 10 ms
calls per session, every session at its own rate and its own call size (80 with HALF_CALL in a 160-sample tick), rows packed.

9 sessions at the rates of mixed_helpers (three workgroups of the tick kernel, the last a quarter full), signals from
webrtc_aecm_amd.synth at per-session rates.  The references of every run: one WebRtcAecm_* instance per session at its rate and
sizes (the unmodified reference where oracle/_ref exists, the project's single-session ABI otherwise), and always a twin object that
makes every packet tick as K ordinary ticks flagged HALF_CALL on re-laid rows.  Every output sample, every code, every echo path
and every ExportSessions blob must be equal.  No exclusions."""
import numpy as np
import pytest

import calls_helpers as ch
import mixed_helpers as mh
import packets_helpers as ph
import sparse_helpers as sh
import webrtc_aecm_amd as aecm
from oracle import pyoracle

pytestmark = pytest.mark.gpu

S9 = mh.S9
IDLE, NO_FAREND, SPLIT, HALF = aecm.ffi.SESSION_IDLE, aecm.ffi.SESSION_NO_FAREND, aecm.ffi.SESSION_SPLIT_CALLS, aecm.ffi.SESSION_HALF_CALL
BAD, UNSUPPORTED, WARNING, NULL = 12004, 12001, 12100, 12003


def make_reference(fs):
    if pyoracle.have_reference():
        return pyoracle.RefSession(fs, 1, 3)
    s = aecm.Aecm()
    assert s.init(fs) == 0 and s.set_config(1, 3) == 0
    return s


def new_object(fs, rates):
    return aecm.AecmSessions(len(rates), fs, 1, 3, rates=rates)


def assert_same_objects(sb, twin, what, paths=None):
    for s in range(sb.num_streams):
        rc, path = sb.get_echo_path(s)
        rc2, path2 = twin.get_echo_path(s)
        assert rc == 0 and rc2 == 0 and np.array_equal(path, path2), (what, "echo path", s)
        if paths is not None:
            assert np.array_equal(path, paths[s]), (what, "echo path against the reference", s)
    a, b = sb.export_sessions(), twin.export_sessions()
    assert a[0] == 0 and b[0] == 0
    n = len(a[1]) // sb.num_streams
    for s in range(sb.num_streams):
        assert a[1][s * n:(s + 1) * n] == b[1][s * n:(s + 1) * n], (what, "snapshot of session", s)


def check_schedule(fs, rates, ops, far, near, clean=None, farx=None, forms=("device",), what=None):
    """The schedule on the reference, on the twin (K ordinary ticks per packet tick) and, per form, on an object of its own."""
    exp_out, exp_codes, refs = ph.run_reference(make_reference, rates, ops, ph.Feed(far, near, clean, farx))
    paths = [r.get_echo_path()[1] for r in refs]
    twin = new_object(fs, rates)
    tout, tcodes = ph.run_object(twin, ops, ph.Feed(far, near, clean, farx), as_single_ticks=True)
    assert np.array_equal(tcodes, exp_codes) and np.array_equal(tout, exp_out), (what, "the twin itself")
    for form in forms:
        sb = new_object(fs, rates)
        out, codes = ph.run_object(sb, ops, ph.Feed(far, near, clean, farx), form=form)
        assert np.array_equal(codes, exp_codes), (what, form)
        bad = np.argwhere(out != exp_out)
        assert bad.size == 0, (what, form, "first difference: session, sample", bad[0].tolist())
        assert_same_objects(sb, twin, (what, form), paths)
        sb.close()
    twin.close()


def mixed_flags(seed, T, n, rates, idle_p=0.2):
    """Half calls always for sessions 1, 2, 4, 7, sometimes for session 3 (n = 160 only); underruns; idle sessions; wandering
    per-session msInSndCardBuf with out-of-range values."""
    rng = np.random.default_rng(seed)
    flags = (rng.random((T, S9)) < idle_p).astype(np.uint8) * IDLE | (rng.random((T, S9)) < 0.12).astype(np.uint8) * NO_FAREND
    if n == 160:
        for s in mh.ALWAYS_HALF:
            flags[:, s] |= HALF
        flags[rng.random(T) < 1 / 3, mh.SOMETIMES_HALF] |= HALF
    ms = (40 + 5 * np.arange(S9)[None, :] + rng.integers(-3, 4, (T, S9))).astype(np.int16)
    wild = rng.random((T, S9)) < 0.06
    wild[:T // 3] = False
    ms[wild] = np.where(rng.random(int(wild.sum())) < 0.5, -300, 700).astype(np.int16)
    return flags, ms


@pytest.mark.parametrize("with_clean", [0, 1])
@pytest.mark.parametrize("fs,n", [(16000, 160), (8000, 80)])
@pytest.mark.parametrize("K", [2, 3, 6])
def test_mixed_objects(K, fs, n, with_clean):
    """Both object rates: a 16 kHz object ticking 160 (8 kHz sessions on half calls, session 8 on full 160-sample calls, a 16 kHz
    session on half calls now and then) and an 8 kHz object ticking 80 with 16 kHz sessions; 48 calls per session from Init, so the
    start-up phases end inside packets; idle sessions, underruns, per-session msInSndCardBuf; device, async and host forms."""
    T = 48 // K
    flags, ms = mixed_flags(40 + K + fs, T, n, mh.RATES)
    far, near, clean = mh.signals(1500 + K, mh.RATES, 48 * n, with_clean=bool(with_clean))
    check_schedule(fs, mh.RATES, ph.packets_ops(K, n, flags, ms), far, near, clean, forms=("device", "async", "host"), what=(K, fs, n, with_clean))


def test_at_size():
    """261 sessions: two planning workgroups, the second with 5 lanes; 66 tick workgroups when everybody calls, the last with one
    wave.  Rates alternate by lane, half flags at random per lane, 30 % idle, K = 3, 12 ticks; InitSessionRate on every 7th session
    at tick 6, so that sessions in their start-up phase and running sessions share planning wavefronts.  Against the twin: outputs
    and ExportSessions blobs."""
    import torch
    S, fs, n, K, T = 261, 16000, 160, 3, 12
    rates = np.where(np.arange(S) % 2 == 0, 16000, 8000).astype(np.int32)
    base8, base16 = mh.signals(1700, [8000] * 8, T * K * n), mh.signals(1800, [16000] * 8, T * K * n)
    pick = np.arange(S) % 8
    far = np.where((rates == 8000)[:, None], base8[0][pick], base16[0][pick])
    near = np.where((rates == 8000)[:, None], base8[1][pick], base16[1][pick])
    rng = np.random.default_rng(4)
    flags = (rng.random((T, S)) < 0.3).astype(np.uint8) * IDLE | (rng.random((T, S)) < 0.5).astype(np.uint8) * HALF
    ms = (40 + 10 * (np.arange(S) % 7))[None, :].repeat(T, axis=0).astype(np.int16)
    a, b = new_object(fs, rates), new_object(fs, rates)
    ops = ph.packets_ops(K, n, flags, ms)
    fa, fb = ph.Feed(far, near), ph.Feed(far, near)

    def reinit(t, op, sb):
        if t == 5:                                                             # before tick 6
            for s in range(0, S, 7):
                assert sb.init_session_rate(s, 8000 if s % 14 == 0 else 16000) == 0
    oa, ca = ph.run_object(a, ops, fa, form="async", check=lambda t, op: reinit(t, op, a))
    ob, cb = ph.run_object(b, ops, fb, as_single_ticks=True, check=lambda t, op: reinit(t, op, b))
    assert np.array_equal(ca, cb)
    bad = np.argwhere(oa != ob)
    assert bad.size == 0, ("first difference: session, sample", bad[0].tolist())
    ra, rb = a.export_sessions(), b.export_sessions()
    assert ra[0] == 0 and rb[0] == 0 and ra[1] == rb[1]
    a.close(), b.close()
    torch.cuda.synchronize()


def test_interleaving_and_migration():
    """Packet ticks among ordinary ticks (half and split calls), bursts + Process, other K; mid-run, session by session, export and
    ImportSessionAnyRate into an object of the OTHER own rate (8 kHz, ticking 160 from there on would not do: it continues with
    80-sample packet ticks for everybody -- no half calls there)."""
    fs, rng = 16000, np.random.default_rng(6)
    kinds = [("tick", 160, 0), ("packets", 160, 2), ("burst", 80, 2), ("packets", 160, 6), ("split", 160, 0), ("packets", 160, 3), ("half", 160, 0),
             ("packets", 160, 2), ("burst", 160, 1), ("packets", 160, 5)]
    ops = []
    for rep in range(4):
        for kind, n, k in kinds:
            if rep >= 2:
                n = 80                                                       # behind the migration: the 8 kHz object's tick
            fl = (rng.random(S9) < 0.2).astype(np.uint8) * IDLE | (rng.random(S9) < 0.15).astype(np.uint8) * NO_FAREND
            ms = (40 + 20 * np.arange(S9) + rng.integers(-15, 16, S9)).astype(np.int16)
            if n == 160 and kind in ("packets", "half", "tick"):
                for s in mh.ALWAYS_HALF:
                    fl[s] |= HALF
                if kind == "half" or rng.random() < 0.4:
                    fl[mh.SOMETIMES_HALF] |= HALF
            if kind == "packets":
                ops.append(dict(kind="packets", K=k, n=n, flags=fl, ms=ms))
            elif kind == "burst":
                ops.append(dict(kind="burst", B=k, n=n, ms=ms))
            else:
                if kind == "split" and n == 160:
                    fl[mh.SPLIT] |= SPLIT
                ops.append(dict(kind="tick", n=n, flags=fl, ms=ms))
    total = sum(ph.span_of(op) for op in ops)
    far, near, _ = mh.signals(1900, mh.RATES, total)
    farx = mh.signals(2000, mh.RATES, sum(op["B"] * op["n"] for op in ops if op["kind"] == "burst"))[0]
    exp_out, exp_codes, refs = ph.run_reference(make_reference, mh.RATES, ops, ph.Feed(far, near, None, farx))
    cut = 2 * len(kinds)
    feed, tfeed = ph.Feed(far, near, None, farx), ph.Feed(far, near, None, farx)
    a, ta = new_object(fs, mh.RATES), new_object(fs, mh.RATES)
    out1, codes1 = ph.run_object(a, ops[:cut], feed, form="device")
    tout1, tcodes1 = ph.run_object(ta, ops[:cut], tfeed, as_single_ticks=True)
    assert_same_objects(a, ta, "before the migration")
    b, tb = aecm.AecmSessions(S9, 8000, 1, 3), aecm.AecmSessions(S9, 8000, 1, 3)
    junk = sh.signals(990, S9, 800, 8000)
    for obj in (b, tb):
        for k in range(5):                                                   # the second object has a past of its own
            obj.tick_host_per_session(junk[0][:, k * 80:(k + 1) * 80], junk[1][:, k * 80:(k + 1) * 80], np.full(S9, 40, np.int16))
    for src, dst in ((a, b), (ta, tb)):
        for s in range(S9):
            rc, blob = src.export_session(s)
            assert rc == 0 and dst.import_session_any_rate(s, blob) == 0
            assert dst.get_session_rate(s) == (0, int(mh.RATES[s]))
    out2, codes2 = ph.run_object(b, ops[cut:], feed, form="async")
    tout2, tcodes2 = ph.run_object(tb, ops[cut:], tfeed, as_single_ticks=True)
    out, codes = np.concatenate([out1, out2], axis=1), np.concatenate([codes1, codes2])
    assert np.array_equal(codes, exp_codes) and np.array_equal(np.concatenate([tcodes1, tcodes2]), exp_codes)
    assert np.array_equal(np.concatenate([tout1, tout2], axis=1), exp_out), "the twin itself"
    bad = np.argwhere(out != exp_out)
    assert bad.size == 0, ("first difference: session, sample", bad[0].tolist())
    assert_same_objects(b, tb, "after the migration", [r.get_echo_path()[1] for r in refs])
    for o in (a, ta, b, tb):
        o.close()


def test_k_call_ticks_among_packet_ticks_while_the_object_is_uniform():
    """A uniform 16 kHz object: TickCalls, packet ticks with half calls for some sessions, TickCalls again (its planning launch
    brings the sessions the half calls left behind back in step), ordinary ticks."""
    fs, n, rng = 16000, 160, np.random.default_rng(8)
    rates = np.full(S9, fs, np.int32)
    ops = []
    for rep in range(6):
        for kind, k in (("calls", 2), ("packets", 3), ("calls", 3), ("packets", 2), ("tick", 0)):
            fl = (rng.random(S9) < 0.2).astype(np.uint8) * IDLE | (rng.random(S9) < 0.15).astype(np.uint8) * NO_FAREND
            if kind == "packets":
                fl |= (rng.random(S9) < 0.5).astype(np.uint8) * HALF
            ms = (40 + 10 * np.arange(S9)).astype(np.int16)
            ops.append(dict(kind=kind, K=k, n=n, flags=fl, ms=ms) if k else dict(kind="tick", n=n, flags=fl, ms=ms))
    far, near, clean = mh.signals(2100, rates, sum(ph.span_of(op) for op in ops), with_clean=True)
    check_schedule(fs, rates, ops, far, near, clean, forms=("device",), what="uniform")


def test_replay_row_spill_inside_a_packet_of_half_calls():
    """calls_helpers.SPILL_RECIPE on an 8 kHz session making half calls in a 16 kHz object (tests/test_tick_packets.py confirms on
    the CPU double that a row is spilled at a call c > 0): pre_ticks ordinary full ticks, then more than 98 calls of 80 samples in
    packets of K = 6 half calls, then a 160-sample tick without a far end, which replays from the row."""
    r = ch.SPILL_RECIPE
    K = r["calls"]
    rates = np.array([16000, 8000, 8000, 16000], dtype=np.int32)
    S = len(rates)
    one = lambda v, dt: np.full(S, v, dt)
    half = np.array([0, HALF, HALF, HALF], dtype=np.uint8)
    ops = [dict(kind="tick", n=160, flags=one(0, np.uint8), ms=one(40, np.int16)) for _ in range(r["pre_ticks"])]
    ops += [dict(kind="packets", K=K, n=160, flags=half, ms=one(40, np.int16)) for _ in range(r["k_ticks"])]
    assert r["k_ticks"] * K > 98
    ops += [dict(kind="tick", n=160, flags=one(NO_FAREND, np.uint8), ms=one(40, np.int16))]
    far, near, _ = mh.signals(2200, rates, sum(ph.span_of(op) for op in ops))
    exp_out, exp_codes, refs = ph.run_reference(make_reference, rates, ops, ph.Feed(far, near))
    sb, twin = new_object(16000, rates), new_object(16000, rates)
    out, codes = ph.run_object(sb, ops, ph.Feed(far, near), form="device")
    tout, tcodes = ph.run_object(twin, ops, ph.Feed(far, near), as_single_ticks=True)
    assert np.array_equal(out, exp_out) and np.array_equal(tout, exp_out) and np.array_equal(codes, exp_codes) and np.array_equal(tcodes, exp_codes)
    assert_same_objects(sb, twin, "spill", [x.get_echo_path()[1] for x in refs])
    sb.close(), twin.close()


def test_one_call_is_the_ordinary_tick():
    """calls == 1 equals TickFlags with the same arguments, SPLIT_CALLS and HALF_CALL included, in a mixed object."""
    fs, n, T = 16000, 160, 24
    flags, ms = mh.mixed_pattern(77, T, 0.2)
    far, near, clean = mh.signals(2300, mh.RATES, T * n, with_clean=True)
    a, b = new_object(fs, mh.RATES), new_object(fs, mh.RATES)
    for t in range(T):
        if not ((flags[t] & IDLE) == 0).any() or ((flags[t] & (HALF | SPLIT | IDLE)) == (HALF | SPLIT)).any():
            continue
        sl = slice(t * n, (t + 1) * n)
        ra = a.tick_packets_host(far[:, sl], near[:, sl], 1, ms[t], clean=clean[:, sl], flags=flags[t])
        rb = b.tick_host_per_session(far[:, sl], near[:, sl], ms[t], clean[:, sl], flags=flags[t])
        assert ra[0] == rb[0] and np.array_equal(ra[1], rb[1]) and np.array_equal(ra[2], rb[2]), t
    assert a.export_sessions()[1] == b.export_sessions()[1]
    a.close(), b.close()


def test_a_uniform_object_without_half_calls_makes_k_call_ticks():
    """No calling session flagged HALF_CALL, no session of another rate: TickPackets is TickCalls -- outputs, codes and blobs."""
    fs, n, K, T = 16000, 160, 3, 10
    flags, ms = sh.pattern(92, S9, T, 0.2, n=80, flags_p=0.15, ms_spread=True)
    far, near, clean = sh.signals(2400, S9, T * K * n, fs, with_clean=True)
    a, b = aecm.AecmSessions(S9, fs, 1, 3), aecm.AecmSessions(S9, fs, 1, 3)
    for t in range(T):
        if not ((flags[t] & IDLE) == 0).any():
            continue
        sl = slice(t * K * n, (t + 1) * K * n)
        ra = a.tick_packets_host(far[:, sl], near[:, sl], K, ms[t], clean=clean[:, sl], flags=flags[t])
        rb = b.tick_calls_host(far[:, sl], near[:, sl], K, ms[t], clean=clean[:, sl], flags=flags[t])
        assert ra[0] == rb[0] and np.array_equal(ra[1], rb[1]) and np.array_equal(ra[2], rb[2]), t
    assert a.export_sessions()[1] == b.export_sessions()[1]
    a.close(), b.close()


def test_refusals_change_nothing():
    """Bad `calls`, a short stride, HALF_CALL in a tick of 80, SPLIT_CALLS with calls > 1, the safe kernel variant: the right code,
    and afterwards the run continues exactly as the twin's.  TickCalls on the same mixed object still returns what it returns."""
    import torch
    fs, n, K, T = 16000, 160, 3, 6
    flags, ms = mixed_flags(11, T, n, mh.RATES)
    far, near, _ = mh.signals(2500, mh.RATES, 48 * n)
    ops = ph.packets_ops(K, n, flags, ms)
    sb, twin = new_object(fs, mh.RATES), new_object(fs, mh.RATES)
    feed, tfeed = ph.Feed(far, near), ph.Feed(far, near)
    ph.run_object(sb, ops[:3], feed, form="device")
    ph.run_object(twin, ops[:3], tfeed, as_single_ticks=True)
    f = torch.from_numpy(far[:, :K * n].copy()).cuda()
    d = torch.from_numpy(near[:, :K * n].copy()).cuda()
    o = torch.zeros_like(d)
    msa = np.full(S9, 40, np.int16)
    call = lambda calls, stride=K * n, fl=None, nn=n, fp=f.data_ptr(), dp=d.data_ptr(): sb.tick_packets_device(fp, dp, o.data_ptr(), stride, nn, calls, msa, flags=fl)[0]
    host = lambda calls, fl=None, w=K * n: sb.tick_packets_host(far[:, :w], near[:, :w], calls, msa, flags=fl)[0]
    assert call(0) == BAD and call(7) == BAD and call(-1) == BAD
    assert call(K, stride=K * n - 1) == BAD and call(2, stride=n) == BAD
    assert call(K, nn=100) == BAD
    assert call(K, dp=None) == NULL and call(K, fp=None) == NULL
    fl = np.zeros(S9, np.uint8)
    fl[4] = HALF
    assert call(K, fl=fl, nn=80) == BAD and host(K, fl, w=K * 80) == BAD            # a half call needs a tick of 160
    assert call(1, fl=fl, nn=80, stride=80) == BAD
    fl[4] = SPLIT
    assert call(K, fl=fl) == BAD and host(K, fl) == BAD
    fl[4] = SPLIT | HALF
    assert call(K, fl=fl) == BAD and call(1, fl=fl) == BAD
    assert sb.lib.WebRtcAecmSessions_SetKernelVariant(sb.h, 0) == 0
    assert call(K) == UNSUPPORTED and host(K) == UNSUPPORTED
    assert sb.lib.WebRtcAecmSessions_SetKernelVariant(sb.h, 1) == 0
    # TickCalls keeps its refusals on this very object: another rate, and (in a uniform object) a half call
    assert sb.tick_calls_host(far[:, :2 * n], near[:, :2 * n], 2, msa)[0] == UNSUPPORTED
    uni = aecm.AecmSessions(S9, fs, 1, 3)
    fl[4] = HALF
    assert uni.tick_calls_host(far[:, :2 * n], near[:, :2 * n], 2, msa, flags=fl)[0] == BAD
    assert uni.tick_packets_host(far[:, :2 * n], near[:, :2 * n], 2, msa, flags=fl)[0] == 0
    uni.close()
    # nothing changed: the run goes on as the twin's
    out, codes = ph.run_object(sb, ops[3:], feed, form="device")
    tout, tcodes = ph.run_object(twin, ops[3:], tfeed, as_single_ticks=True)
    assert np.array_equal(out, tout) and np.array_equal(codes, tcodes)
    assert_same_objects(sb, twin, "after the refusals")
    sb.close(), twin.close()


@pytest.mark.parametrize("name", sorted(ph.GOLDEN_CASES))
def test_golden_runs(name):
    """tests/golden/sesspackets_*.npz: the unmodified reference's outputs, codes and final echo paths of 9 sessions x 48 calls,
    through the device form."""
    fs, n, K, seed = ph.GOLDEN_CASES[name]
    g = np.load(mh.GOLDEN_DIR / f"{name}.npz")
    flags, ms = g["flags"], g["ms"]
    assert flags.shape == (ph.GOLDEN_CALLS // K, S9)
    far, near, _ = mh.signals(seed, mh.RATES, ph.GOLDEN_CALLS * n)
    sb = new_object(fs, mh.RATES)
    out, codes = ph.run_object(sb, ph.packets_ops(K, n, flags, ms), ph.Feed(far, near), form="device")
    assert np.array_equal(out, g["out"]) and np.array_equal(codes, g["codes"])
    for s in range(S9):
        assert np.array_equal(sb.get_echo_path(s)[1], g["paths"][s]), s
    sb.close()
