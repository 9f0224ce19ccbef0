"""TEST INFRASTRUCTURE for a clean near-end input per session (AECM_SESSION_NO_CLEAN; tests/test_gpu_split_clean.py): the kinds and
patterns of the runs, and a driver for one WebRtcAecm_* instance per session that passes every call its session's clean row, or None
where the session's flag byte carries the bit -- on top of tests/mixed_helpers.py, which knows a clean input for everybody or nobody."""
from __future__ import annotations

import numpy as np

import mixed_helpers as mh

NO_FAREND, SPLIT_CALLS, IDLE, HALF_CALL, NO_CLEAN = mh.NO_FAREND, mh.SPLIT_CALLS, mh.IDLE, mh.HALF_CALL, 16
NONE, ALWAYS, NEVER, BOTH = 0, 1, 2, 3
JUNK = 0x5a5a          # what the clean rows of the sessions without a clean input hold

# The uniform run: 11 sessions at 16 kHz, ticks of 160; 6 without a clean input and 5 with, interleaved by id -- with everybody
# calling, the tick kernel's clean workgroups are 1 1/4 full and the plain ones 1 1/2.
S11, T_RUN = 11, 90
NEVER11 = (0, 2, 4, 6, 8, 10)
SPLIT11, SPLIT_FROM = 5, 10          # one session on two call pairs of 80 (from tick 10 on: mixed_helpers.SPLIT_FROM explains)
# The mixed-rate run: the 9 sessions of mixed_helpers; without a clean input: an 8 kHz session on half calls, the 16 kHz session that
# sometimes makes half calls, the split session, the 8 kHz session on full calls.
NEVER9 = (1, 3, 5, 8)


def uniform_pattern(seed, S=S11, T=T_RUN, never=NEVER11, idle_p=0.3):
    """flags[T, S] uint8, ms[T, S] int16: the sessions of `never` carry NO_CLEAN in every tick; far-end underruns at random; 30 % of
    every session's ticks idle (the idle bytes keep their other bits and get NO_CLEAN at random: all of it must be ignored);
    per-session msInSndCardBuf with out-of-range values after the start-up phases."""
    rng = np.random.default_rng(seed)
    flags = np.zeros((T, S), dtype=np.uint8)
    flags[:, list(never)] |= NO_CLEAN
    if S > SPLIT11:
        flags[SPLIT_FROM:, SPLIT11] |= SPLIT_CALLS
    flags |= (rng.random((T, S)) < 0.1).astype(np.uint8) * NO_FAREND
    idle = rng.random((T, S)) < idle_p
    flags[idle] |= IDLE
    flags[idle] ^= (rng.random(int(idle.sum())) < 0.5).astype(np.uint8) * NO_CLEAN
    ms = (40 + 5 * (np.arange(S) % 12)[None, :] + rng.integers(-3, 4, (T, S))).astype(np.int16)
    wild = rng.random((T, S)) < 0.04
    wild[:30] = False
    ms[wild] = np.where(rng.random(int(wild.sum())) < 0.5, -300, 700).astype(np.int16)
    return flags, ms


def object_clean(clean, never):
    """The clean signal as the OBJECT gets it: junk in the rows of the sessions that take none."""
    c = clean.copy()
    c[list(never)] = JUNK
    return c


def drive_reference(make_session, rates, flags, ms, n, far, near, clean, sessions=None, cursors=None):
    """mixed_helpers.drive_reference with the clean pointer per CALL: session s's call in tick t gets its clean row unless
    flags[t, s] carries NO_CLEAN, then None.  Returns out[S, T * n], codes[T, S], paths[S, 65], the instances."""
    T, S = flags.shape
    sessions = [make_session(int(fs)) for fs in rates] if sessions is None else sessions
    out = np.zeros((S, T * n), dtype=np.int16)
    codes = np.zeros((T, S), dtype=np.int32)
    cursors = np.zeros(S, dtype=np.int64) if cursors is None else cursors
    for t in range(T):
        take = mh.consumed(flags[t], n)
        f, d, c = mh.tick_rows(far, near, clean, cursors, take, n)
        for s in np.flatnonzero(take):
            k = int(take[s])
            cs = None if flags[t, s] & NO_CLEAN else c[s, :k]
            codes[t, s], out[s, t * n:t * n + k] = mh.session_call(sessions[s], f[s, :k], d[s, :k], cs, k, int(flags[t, s]) & (NO_FAREND | SPLIT_CALLS), ms[t, s])
        cursors += take
    paths = np.stack([sessions[s].get_echo_path()[1] for s in range(S)])
    return out, codes, paths, sessions


def expected_modes(flags, S):
    """What GetSessionCleanMode says after the ticks of flags[T, S], all with a clean plane, from fresh sessions."""
    modes = np.zeros(S, dtype=np.int64)
    for row in flags:
        calls = (row & IDLE) == 0
        modes[calls & ((row & NO_CLEAN) != 0)] |= NEVER
        modes[calls & ((row & NO_CLEAN) == 0)] |= ALWAYS
    return modes
