"""A clean near-end input per session (AECM_SESSION_NO_CLEAN) on the GPU: in one tick that carries a clean plane, some sessions'
WebRtcAecm_Process gets its clean row and the others' gets nearendClean = NULL.

The reference of every run is one WebRtcAecm_* instance per session, each call made with or without the clean pointer as the
session's flag byte says: the unmodified reference (oracle.pyoracle.RefSession) where oracle/_ref exists, the project's
single-session ABI where it does not.  Every output sample of every call made, every return code, at the end every echo path, and
the continuation of every session from its snapshot in another object must be equal.  The clean rows of the sessions that take none
hold junk.  No exclusions."""
import numpy as np
import pytest

import mixed_helpers as mh
import split_helpers as sh
import webrtc_aecm_amd as aecm
from test_gpu_mixed_sessions import check_equal, make_reference, run_object

pytestmark = pytest.mark.gpu

BAD = aecm.ffi.AECM_BAD_PARAMETER_ERROR
UNSUPPORTED = aecm.ffi.AECM_UNSUPPORTED_FUNCTION_ERROR
_runs = {}


def modes_of(sb):
    got = [sb.get_session_clean_mode(s) for s in range(sb.num_streams)]
    assert all(rc == 0 for rc, _ in got)
    return [m for _, m in got]


def uniform_case():
    """The uniform run (split_helpers): pattern, signals, the reference's results -- computed once and shared, never modified."""
    if "uniform" not in _runs:
        rates = np.full(sh.S11, 16000, dtype=np.int32)
        flags, ms = sh.uniform_pattern(9700)
        far, near, clean = mh.signals(9700, rates, sh.T_RUN * 160, with_clean=True)
        out, codes, paths, _ = sh.drive_reference(make_reference, rates, flags, ms, 160, far, near, clean)
        for a in (out, codes, paths):
            a.setflags(write=False)
        _runs["uniform"] = (rates, flags, ms, far, near, clean, (out, codes, paths))
    return _runs["uniform"]


def mixed_case():
    """The mixed-rate run: the object, pattern and signals of mixed_helpers' idle run, sessions 1, 3, 5, 8 without a clean input."""
    if "mixed" not in _runs:
        seed, idle_p, _ = mh.GOLDEN_CASES["sessmixed_idle"]
        flags, ms = mh.mixed_pattern(seed, idle_p=idle_p)
        flags = flags.copy()
        flags[:, list(sh.NEVER9)] |= sh.NO_CLEAN
        flags[3, 6] |= sh.NO_CLEAN                       # (an idle byte of an "always" session that carries every bit there is)
        far, near, clean = mh.signals(seed, mh.RATES, mh.T_MIXED * 160, with_clean=True)
        out, codes, paths, _ = sh.drive_reference(make_reference, mh.RATES, flags, ms, 160, far, near, clean)
        for a in (out, codes, paths):
            a.setflags(write=False)
        _runs["mixed"] = (flags, ms, far, near, clean, (out, codes, paths))
    return _runs["mixed"]


def run_with_migration(make_object, flags, ms, far, near, clean_obj, form, T0):
    """Ticks [0, T0) on one object, then every session by its snapshot into a second object of another age, ticks [T0, T) there.
    Returns the outputs and codes of the whole run, the second object, and the modes the first one reported at T0."""
    S = flags.shape[1]
    a = make_object()
    cursors = np.zeros(S, dtype=np.int64)
    out0, codes0 = run_object(a, flags[:T0], ms[:T0], 160, far, near, clean_obj, form=form, cursors=cursors)
    modes = modes_of(a)
    rc, snaps = a.export_sessions()
    assert rc == 0
    b = make_object()
    warm = np.zeros((S, 160), dtype=np.int16)
    for _ in range(3):                                   # (an age of its own, and a clean ring of its own)
        assert b.tick_host_per_session(warm, warm, np.full(S, 40, np.int16), clean=warm)[0] == 0
    assert modes_of(b) == [sh.ALWAYS] * S
    assert b.import_sessions(None, snaps, any_rate=True) == 0
    assert modes_of(b) == [sh.NONE] * S                  # an imported session starts at "none": the caller continues it as it was
    out1, codes1 = run_object(b, flags[T0:], ms[T0:], 160, far, near, clean_obj, form=form, cursors=cursors, t0=T0)
    a.close()
    return np.concatenate([out0, out1], axis=1), np.concatenate([codes0, codes1]), b, modes


@pytest.mark.parametrize("form", ["device", "host", "async"])
def test_split_run(form):
    """11 sessions at 16 kHz, 90 ticks of 160: sessions 0, 2, .. 10 without a clean input, 1, 3, .. 9 with; far-end underruns, one
    session on split calls, 30 % idle ticks (idle bytes carrying the bit at random), per-session msInSndCardBuf with out-of-range
    values; junk in the clean rows of the flagged sessions.  TickFlags, TickFlagsHost and TickAsync each against the reference
    instances; the out rows of idle sessions are not written (host form: zeros), those of flagged sessions are.  At tick 60 every
    session moves into another object by its snapshot and continues there.  On the commit before this flag existed bit 16 was
    ignored, the flagged sessions were processed with their junk rows as a clean input, and this test fails."""
    rates, flags, ms, far, near, clean, ref = uniform_case()
    calling = (flags & sh.IDLE) == 0
    is_never = np.isin(np.arange(sh.S11), sh.NEVER11)[None, :]
    assert np.array_equal(((flags & sh.NO_CLEAN) != 0)[calling], np.broadcast_to(is_never, flags.shape)[calling])
    assert ((flags & sh.NO_CLEAN) != 0)[~calling & ~is_never].any()                  # idle bytes of "always" sessions that carry the bit
    lc = (calling & ((flags & sh.NO_CLEAN) == 0)).sum(axis=1)
    assert (lc % 4 != 0).any() and (lc % 4 == 0).any() and (lc > 4).any()          # the plain list starts behind a gap, and right behind
    out, codes, b, modes = run_with_migration(lambda: aecm.AecmSessions(sh.S11, 16000, 1, 3), flags, ms, far, near, sh.object_clean(clean, sh.NEVER11), form, 60)
    assert modes == sh.expected_modes(flags[:60], sh.S11).tolist() and set(modes) == {sh.ALWAYS, sh.NEVER}
    check_equal(out, codes, b, ref, ("split", form))
    assert modes_of(b) == sh.expected_modes(flags[60:], sh.S11).tolist()
    # the flagged sessions' outputs differ from what a clean input of junk would have given: their start-up copy is the noisy near end
    s = sh.NEVER11[1]
    first = int(np.flatnonzero(calling[:, s])[0])
    assert np.array_equal(out[s, first * 160:first * 160 + 160], near[s, :160])
    b.close()


@pytest.mark.parametrize("form", ["device", "host"])
def test_split_run_on_the_mixed_rate_object(form):
    """The 9 sessions of both rates of mixed_helpers (half calls, a split session, idle ticks, a tick nobody makes), sessions
    1, 3, 5, 8 without a clean input: the planning launch that knows per-session rates and call sizes, with two lists."""
    flags, ms, far, near, clean, ref = mixed_case()
    make = lambda: aecm.AecmSessions(mh.S9, mh.OBJECT_FS, 1, 3, rates=mh.RATES)
    out, codes, b, modes = run_with_migration(make, flags, ms, far, near, sh.object_clean(clean, sh.NEVER9), form, 50)
    assert modes == [sh.NEVER if s in sh.NEVER9 else sh.ALWAYS for s in range(mh.S9)]
    check_equal(out, codes, b, ref, ("split mixed", form))
    assert [b.get_session_rate(s)[1] for s in range(mh.S9)] == mh.RATES.tolist()
    b.close()


def test_300_sessions_across_a_planning_workgroup():
    """300 sessions (two planning workgroups with different counts of either kind), 40 ticks.  Tick 0: only the sessions without a
    clean input call -- everybody who calls is flagged, the tick takes the launches of a tick without a clean input: the object
    still has no clean ring afterwards (a snapshot's header says so).  Tick 20: those sessions sit out, nobody who calls is flagged:
    today's tick.  Before tick 25 session 130 is initialised afresh and switches kind."""
    S, T, n, SW, T_SW = 300, 40, 160, 130, 25
    rates = np.full(S, 16000, dtype=np.int32)
    never = np.zeros(S, dtype=bool)
    never[:70] = True                                     # the first wavefront of the first planning workgroup: one kind only
    never[70:256:3] = True
    never[256::2] = True
    never[SW] = False
    rng = np.random.default_rng(9800)
    flags = np.zeros((T, S), dtype=np.uint8)
    flags[:, never] = sh.NO_CLEAN
    flags |= (rng.random((T, S)) < 0.1).astype(np.uint8) * sh.NO_FAREND
    flags[rng.random((T, S)) < 0.2] |= sh.IDLE
    flags[0, ~never] = sh.IDLE
    flags[0, never] &= ~np.uint8(sh.IDLE)
    flags[20, never] |= sh.IDLE
    flags[20, ~never] &= ~np.uint8(sh.IDLE)
    flags[T_SW:, SW] |= sh.NO_CLEAN
    flags[T_SW, SW] &= ~np.uint8(sh.IDLE)
    ms = (40 + (np.arange(S) % 40)[None, :] + rng.integers(-3, 4, (T, S))).astype(np.int16)
    far, near, clean = mh.signals(9800, rates, T * n, with_clean=True)
    never_after = never.copy()
    never_after[SW] = True
    sb = aecm.AecmSessions(S, 16000, 1, 3)
    refs = [make_reference(16000) for _ in range(S)]
    cursors, rcursors = np.zeros(S, dtype=np.int64), np.zeros(S, dtype=np.int64)
    for t0, t1 in ((0, 1), (1, T_SW), (T_SW, T)):
        if t0 == T_SW:
            assert sb.init_session(SW) == 0 and sb.set_config_session(SW, 1, 3) == 0
            assert sb.get_session_clean_mode(SW) == (0, sh.NONE)
            refs[SW] = make_reference(16000)
            cursors[SW] = rcursors[SW] = 0
        kinds = never_after if t0 >= T_SW else never
        out, codes = run_object(sb, flags[t0:t1], ms[t0:t1], n, far, near, sh.object_clean(clean, np.flatnonzero(kinds)), form="device", cursors=cursors)
        exp = sh.drive_reference(None, rates, flags[t0:t1], ms[t0:t1], n, far, near, clean, sessions=refs, cursors=rcursors)
        check_equal(out, codes, sb, exp[:3], (t0, t1))
        if t0 == 0:
            rc, snap = sb.export_session(0)
            assert rc == 0 and int(np.frombuffer(snap[12:16], dtype=np.uint32)[0]) == 0        # has_clean: no clean ring was made
            assert modes_of(sb) == [sh.NEVER if k else sh.NONE for k in never]
    want = [sh.NEVER if k else sh.ALWAYS for k in never_after]
    assert modes_of(sb) == want
    sb.close()


@pytest.mark.parametrize("two", [True, False])
def test_both_forms_of_the_tick_launch_give_the_same(two):
    """WebRtcAecmSessions_SplitCleanTwoLaunches: the tick launch of a split tick as one launch per list (what large ticks take by
    themselves), and as the fused launch (what a tick this small takes anyway), each forced."""
    rates, flags, ms, far, near, clean, ref = uniform_case()
    sb = aecm.AecmSessions(sh.S11, 16000, 1, 3)
    assert sb.split_clean_two_launches(two) == 0
    out, codes = run_object(sb, flags, ms, 160, far, near, sh.object_clean(clean, sh.NEVER11), form="device")
    check_equal(out, codes, sb, ref, ("two launches", two))
    sb.close()


def test_refusals_change_nothing():
    """always + flagged, never + unflagged (with flags, without, Tick, Process), a tick without a clean input in which an "always"
    session calls: AECM_BAD_PARAMETER_ERROR; a K-call or packet tick with a calling flagged session: AECM_UNSUPPORTED_FUNCTION_ERROR.
    The snapshots of all sessions and their modes are the same bytes before and after, and the next accepted ticks match the
    reference as if the calls had not been made.  The same unflagged tick is accepted by an object that never used the flag."""
    rates, flags, ms, far, near, clean, ref = uniform_case()
    S = sh.S11
    sb = aecm.AecmSessions(S, 16000, 1, 3)
    clean_obj = sh.object_clean(clean, sh.NEVER11)
    cursors = np.zeros(S, dtype=np.int64)
    outs, codes = [], []
    z, z2, m = np.zeros((S, 160), np.int16), np.zeros((S, 320), np.int16), np.full(S, 40, np.int16)
    kinds = np.zeros(S, dtype=np.uint8)
    kinds[list(sh.NEVER11)] = sh.NO_CLEAN
    for t0 in range(0, sh.T_RUN, 30):
        o, c = run_object(sb, flags[t0:t0 + 30], ms[t0:t0 + 30], 160, far, near, clean_obj, form="host", cursors=cursors)
        outs.append(o), codes.append(c)
        before = (sb.export_sessions(), modes_of(sb))
        bad = kinds.copy(); bad[1] = sh.NO_CLEAN                                                  # always + flagged
        assert sb.tick_host_per_session(z, z, m, clean=z, flags=bad)[0] == BAD
        bad = kinds.copy(); bad[0] = 0                                                            # never + unflagged
        assert sb.tick_host_per_session(z, z, m, clean=z, flags=bad)[0] == BAD
        assert sb.tick_host_per_session(z, z, m, clean=z)[0] == BAD and sb.tick_host(z, z, 40, clean=z)[0] == BAD
        assert sb.process_host(z, 40, clean=z)[0] == BAD
        assert sb.tick_host(z, z, 40)[0] == BAD and sb.process_host(z, 40)[0] == BAD              # no clean input: the "always" sessions object
        assert sb.tick_calls_host(z2, z2, 2, m, clean=z2, flags=kinds)[0] == UNSUPPORTED
        assert sb.tick_packets_host(z2, z2, 2, m, clean=z2, flags=kinds)[0] == UNSUPPORTED
        bad = kinds | sh.HALF_CALL | sh.SPLIT_CALLS                                               # the older checks come first
        assert sb.tick_host_per_session(z, z, m, clean=z, flags=bad)[0] == BAD
        assert (sb.export_sessions(), modes_of(sb)) == before
    check_equal(np.concatenate(outs, axis=1), np.concatenate(codes), sb, ref, "after refusals")
    sb.close()
    fresh = aecm.AecmSessions(S, 16000, 1, 3)
    assert fresh.tick_host_per_session(z, z, m, flags=kinds)[0] == 0                              # no clean input: the bit means nothing ...
    assert fresh.tick_host_per_session(z, z, m, clean=z)[0] == 0 and modes_of(fresh) == [sh.BOTH] * S      # ... and the object was never checked
    assert fresh.tick_host_per_session(z, z, m, clean=z, flags=kinds)[0] == BAD                   # its first use is
    fresh.close()
