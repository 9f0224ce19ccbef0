"""TEST INFRASTRUCTURE: the block corpus (tests/block_corpus.py) as sessions -- one session per case with the case's configuration
and echo path (sessions have no control(): a case's control settings do not apply), driven for the whole length of the case
with helpers.call_pattern delays and underruns, as schedules for packets_helpers.run_reference / run_object: ordinary ticks,
ticks of K calls, packet ticks of a mixed-rate object (the 8 kHz sessions make half calls) and sparse ticks with idle stretches.
A session whose case has ended is idle for the rest of the run; what a K-call schedule leaves of a case (fewer than K calls)
is made with ordinary ticks at the end.  tools/gen_golden.py records the ordinary-tick run of each rate on the unmodified
reference (tests/golden/sesscorpus_*.npz)."""
from __future__ import annotations

import hashlib

import numpy as np

import packets_helpers as ph
from block_corpus import corpus_cases
from helpers import call_pattern

NO_FAREND, IDLE, HALF_CALL = ph.NO_FAREND, ph.IDLE, ph.HALF_CALL
LONG = 1200
GOLDEN_CASES = {"sesscorpus_fs16000": 16000, "sesscorpus_fs8000": 8000}
GOLDEN_TAIL = 3200                              # samples of every session's output kept in a fixture


def session_cases(fs=None, long_cases=True):
    """The corpus cases without a clean input (an object's ticks carry a clean row for every session or for none)."""
    return [c for c in corpus_cases(fs=fs, clean=False) if long_cases or c["n_blocks"] <= LONG]


def plan(cases, object_fs, K=1, kind="tick", idle_stretches=False, seed=0):
    """(ops, far[S, L], near[S, L], rates[S]) of a run of `cases` as the sessions of an object at object_fs.  A tick is n = 10 ms of
    the object's rate wide; a session at the lower rate makes half calls.  kind: "tick" (K = 1), "calls" or "packets"."""
    S = len(cases)
    n = object_fs // 100
    rates = np.array([c["fs"] for c in cases], dtype=np.int32)
    n_s = rates // 100
    assert (n_s <= n).all() and (kind != "calls" or (n_s == n).all())
    calls = np.array([c["n_blocks"] * 64 // k for c, k in zip(cases, n_s)], dtype=np.int64)
    pats = [call_pattern(seed + 10 * k, int(calls[k]) + 1) for k in range(S)]
    rng = np.random.default_rng(seed)
    made, stretch, ops = np.zeros(S, dtype=np.int64), np.zeros(S, dtype=np.int64), []
    half = np.where(n_s < n, HALF_CALL, 0).astype(np.uint8)

    def op_of(k_calls, what):
        ready = calls - made >= k_calls
        if idle_stretches:
            start = ready & (stretch == 0) & (rng.random(S) < 0.03)
            stretch[start] = rng.integers(1, 40, S)[start]
        live = ready & (stretch == 0)
        np.subtract(stretch, 1, out=stretch, where=stretch > 0)
        if not live.any() and idle_stretches:
            return True
        flags = half.copy()
        flags[~live] |= IDLE
        ms = np.full(S, 40, dtype=np.int16)
        for s in np.flatnonzero(live):
            ms[s] = pats[s][0][made[s]]
            if not pats[s][1][made[s]]:
                flags[s] |= NO_FAREND
        ops.append(dict(kind=what, K=k_calls, n=n, flags=flags, ms=ms))
        made[live] += k_calls
        return True
    while (calls - made >= K).any():
        op_of(K, kind)
    while (calls - made >= 1).any():
        op_of(1, "tick")
    assert (made == calls).all()
    L = int((calls * n_s).max()) + 6 * n
    far, near = np.zeros((S, L), dtype=np.int16), np.zeros((S, L), dtype=np.int16)
    for k, c in enumerate(cases):
        far[k, :c["far"].size], near[k, :c["near"].size] = c["far"], c["near"]
    return ops, far, near, rates


def configure_session(sess, c):
    """A WebRtcAecm_* instance (RefSession / webrtc_aecm_amd.Aecm) already initialised at the case's rate."""
    assert sess.set_config(c["cng"], c["echo_mode"]) == 0
    if c["path"] is not None:
        assert sess.init_echo_path(c["path"]) == 0
    return sess


def configure_object(sb, cases):
    for k, c in enumerate(cases):
        assert sb.set_config_session(k, c["cng"], c["echo_mode"]) == 0
        if c["path"] is not None:
            assert sb.init_echo_path(k, c["path"]) == 0
    return sb


def summary(cases, out, codes, paths):
    """What a fixture keeps of an ordinary-tick run: the last GOLDEN_TAIL samples of every session's own output (a session's calls
    are the first ones of the run), a SHA-256 of the whole output, the (tick, session, code) triples of the non-zero codes and the
    final echo paths."""
    t, s = np.nonzero(codes)
    ends = [c["n_blocks"] * 64 // (c["fs"] // 100) * (c["fs"] // 100) for c in cases]
    return dict(tail=np.stack([out[k, e - GOLDEN_TAIL:e] for k, e in enumerate(ends)]), sha256=hashlib.sha256(np.ascontiguousarray(out).tobytes()).hexdigest(),
                codes=np.stack([t, s, codes[t, s]], axis=1).astype(np.int32), paths=np.asarray(paths, dtype=np.int16))
