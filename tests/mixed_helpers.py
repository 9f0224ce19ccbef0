"""TEST INFRASTRUCTURE for objects of mixed rates and call sizes (WebRtcAecmSessions_InitRates, AECM_SESSION_HALF_CALL): the
recipe of the mixed run (tools/gen_golden.py: sessmixed_*; tests/test_gpu_mixed_sessions.py), per-session signals at per-session
rates, the rows of a tick in which sessions consume 80 or 160 samples, and a driver for one WebRtcAecm_* instance per session,
each initialised at its session's rate and called with its session's sizes."""
from __future__ import annotations

from pathlib import Path

import numpy as np

from webrtc_aecm_amd.synth import synth_clean, synth_pair

NO_FAREND, SPLIT_CALLS, IDLE, HALF_CALL = 1, 2, 4, 8
GOLDEN_DIR = Path(__file__).resolve().parent / "golden"

# The mixed run: 9 sessions (three workgroups of the tick kernel, the last a quarter full), the object's rate 16 000, ticks of 160.
S9 = 9
OBJECT_FS = 16000
RATES = np.array([16000, 8000, 8000, 16000, 8000, 16000, 16000, 8000, 8000], dtype=np.int32)
ALWAYS_HALF = (1, 2, 4, 7)          # 8 kHz: 10 ms = 80 samples
SOMETIMES_HALF = 3                  # 16 kHz, a half call on a random third of its ticks
SPLIT = 5                           # 16 kHz, two call pairs of 80
SPLIT_FROM = 10                     # ... from this tick on: a 16 kHz instance that only ever gets 80-sample calls never leaves its
                                    # start-up phase (nBlocks10ms = 1 / 2 = 0, echo_control_mobile.cc:282-283, 320, 330)
T_MIXED = 90
GOLDEN_CASES = {"sessmixed_plain": (9300, 0.0, False), "sessmixed_idle": (9400, 0.3, True)}      # name: (seed, idle probability, bursts)


def mixed_pattern(seed, T=T_MIXED, idle_p=0.0):
    """flags[T, 9] uint8, ms[T, 9] int16 of the mixed run.  Session 8 (8 kHz) makes full 160-sample calls, sessions 0 and 6 (16 kHz)
    too; far-end underruns at random; per-session msInSndCardBuf around 40 + 5 s, out-of-range values after the start-up phases."""
    rng = np.random.default_rng(seed)
    flags = np.zeros((T, S9), dtype=np.uint8)
    for s in ALWAYS_HALF:
        flags[:, s] |= HALF_CALL
    flags[rng.random(T) < 1 / 3, SOMETIMES_HALF] |= HALF_CALL
    flags[SPLIT_FROM:, SPLIT] |= SPLIT_CALLS
    flags |= (rng.random((T, S9)) < 0.1).astype(np.uint8) * NO_FAREND
    if idle_p:
        idle = rng.random((T, S9)) < idle_p
        flags[idle] |= IDLE                             # (an idle session keeps its other bits: they must be ignored)
        flags[7, :] |= IDLE                             # a tick nobody makes
        flags[3, 6] = IDLE | HALF_CALL | SPLIT_CALLS    # refused in a session that calls, nothing in one that does not
    ms = (40 + 5 * np.arange(S9)[None, :] + rng.integers(-3, 4, (T, S9))).astype(np.int16)
    wild = rng.random((T, S9)) < 0.04
    wild[:30] = False
    ms[wild] = np.where(rng.random(int(wild.sum())) < 0.5, -300, 700).astype(np.int16)
    return flags, ms


def burst_pattern(seed, T=T_MIXED):
    """calls[T, 9] uint8: WebRtcAecm_BufferFarend calls of 80 samples session s makes before tick t (mostly none)."""
    rng = np.random.default_rng(seed + 1)
    calls = np.zeros((T, S9), dtype=np.uint8)
    ticks = rng.random(T) < 0.15
    calls[ticks] = rng.integers(0, 4, (int(ticks.sum()), S9)).astype(np.uint8)
    return calls


def signals(seed0, rates, samples, with_clean=False):
    """far[S, samples], near[S, samples] (, clean) int16: session s is synth_pair(seed0 + s, ..., rates[s], "mixed")."""
    nb = samples // 64 + 1
    pairs = [synth_pair(seed0 + s, nb, int(fs), "mixed") for s, fs in enumerate(rates)]
    far = np.stack([p[0][:samples] for p in pairs])
    near = np.stack([p[1][:samples] for p in pairs])
    return far, near, (synth_clean(near) if with_clean else None)


def consumed(flags_t, n):
    """Samples each session's calls consume in a tick of n: 0 idle, 80 a half call, else n."""
    c = np.full(len(flags_t), n, dtype=np.int64)
    c[(flags_t & HALF_CALL) != 0] = 80
    c[(flags_t & IDLE) != 0] = 0
    return c


def tick_rows(far, near, clean, cursors, take, n):
    """The [S, n] rows of one tick: session s's next take[s] samples (its own cursor) at the start of its rows; the rest of a
    row -- an idle session's whole row, the second half of a half-call session's -- holds junk that must never influence anything."""
    S = far.shape[0]
    f = np.full((S, n), 12345, dtype=np.int16)
    d = np.full((S, n), -12345, dtype=np.int16)
    c = None if clean is None else np.full((S, n), 4321, dtype=np.int16)
    for s in range(S):
        k = int(take[s])
        sl = slice(cursors[s], cursors[s] + k)
        f[s, :k], d[s, :k] = far[s, sl], near[s, sl]
        if c is not None:
            c[s, :k] = clean[s, sl]
    return f, d, c


def session_call(sess, f, d, c, n, flag, ms):
    """One tick of ONE session on a WebRtcAecm_* instance: BufferFarend unless NO_FAREND, Process, on n samples; two call pairs of
    n / 2 with SPLIT_CALLS.  Returns (first non-zero code, out[n])."""
    out = np.empty(n, dtype=np.int16)
    code = 0
    calls = 2 if (flag & SPLIT_CALLS) and n == 160 else 1
    ln = n // calls
    for k in range(calls):
        sl = slice(k * ln, (k + 1) * ln)
        if not (flag & NO_FAREND):
            assert sess.buffer_farend(f[sl]) == 0
        rc, o = sess.process(d[sl], None if c is None else c[sl], int(ms))
        out[sl] = o
        code = code or rc
    return code, out


def drive_reference(make_session, rates, flags, ms, n, far, near, clean=None, bursts=None, burst_far=None, sessions=None, cursors=None):
    """Every session on an instance of its own (make_session(fs)), at its own rate, called with its own sizes; an idle tick = no call.
    bursts[T, S] / burst_far[S, T, 3 * 80]: far-end calls of 80 samples before a tick.  Returns out[S, T * n] (zeros where a session
    made no call: an idle tick, the second half of a half call's row), codes[T, S], final echo paths[S, 65], the instances, and
    active_from[S]: the first tick in which a session's output was not the start-up phase's copy of its (clean) near end (T: never)."""
    T, S = flags.shape
    sessions = [make_session(int(fs)) for fs in rates] if sessions is None else sessions
    out = np.zeros((S, T * n), dtype=np.int16)
    codes = np.zeros((T, S), dtype=np.int32)
    cursors = np.zeros(S, dtype=np.int64) if cursors is None else cursors
    active_from = np.full(S, T, dtype=np.int64)
    for t in range(T):
        if bursts is not None:
            for s in range(S):
                for k in range(int(bursts[t, s])):
                    assert sessions[s].buffer_farend(burst_far[s, t, 80 * k:80 * k + 80]) == 0
        take = consumed(flags[t], n)
        f, d, c = tick_rows(far, near, clean, cursors, take, n)
        for s in np.flatnonzero(take):
            k = int(take[s])
            codes[t, s], out[s, t * n:t * n + k] = session_call(sessions[s], f[s, :k], d[s, :k], None if c is None else c[s, :k], k,
                                                                 int(flags[t, s]) & (NO_FAREND | SPLIT_CALLS), ms[t, s])
            if active_from[s] == T and not np.array_equal(out[s, t * n:t * n + k], (d if c is None else c)[s, :k]):
                active_from[s] = t
        cursors += take
    paths = np.stack([sessions[s].get_echo_path()[1] for s in range(S)])
    return out, codes, paths, sessions, active_from


def burst_signals(seed, T=T_MIXED):
    """burst_far[S, T, 240] int16: the far-end samples of the bursts (their own signal: a burst's frames come on top of the ticks')."""
    rng = np.random.default_rng(seed + 2)
    return rng.integers(-8000, 8000, (S9, T, 240)).astype(np.int16)
