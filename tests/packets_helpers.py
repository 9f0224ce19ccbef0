"""TEST INFRASTRUCTURE for packet ticks (WebRtcAecmSessions_TickPackets): schedules of packet ticks, ordinary ticks (half and split
calls included), K-call ticks and far-end bursts with a Process on objects that hold sessions of both rates, executed
  - on an AecmSessions object (packet ticks as such: device, async or host form),
  - on a twin object that makes every packet tick as K ordinary ticks flagged HALF_CALL on re-laid rows (ordinary tick c gets
    row[c * n_s .. c * n_s + n_s) at the start of an n-sample row, junk behind it),
  - on one WebRtcAecm_* instance per session, initialised at the session's rate and called with the session's sizes;
and the recipe of the golden runs sesspackets_* (tools/gen_golden.py)."""
from __future__ import annotations

import numpy as np

import mixed_helpers as mh

NO_FAREND, SPLIT_CALLS, IDLE, HALF_CALL = mh.NO_FAREND, mh.SPLIT_CALLS, mh.IDLE, mh.HALF_CALL
SENTINEL = 0x7b7b
JUNK_FAR, JUNK_NEAR, JUNK_CLEAN = 12345, -12345, 4321

# tools/gen_golden.py: sesspackets_* -- the 9 sessions and RATES of mixed_helpers, 48 calls each, ticks of 160 in a 16 kHz object.
GOLDEN_CASES = {"sesspackets_fs16000_f160_k2": (16000, 160, 2, 9500), "sesspackets_fs16000_f160_k3": (16000, 160, 3, 9600)}
GOLDEN_CALLS = 48


def golden_pattern(K, seed):
    """flags[T, 9] uint8, ms[T, 9] int16 of a golden run, T = 48 / K packet ticks: half calls always on sessions 1, 2, 4, 7 (8 kHz),
    on a random third of session 3's ticks (16 kHz); session 8 (8 kHz) on full calls; 20 % idle, 10 % underruns, per-session
    msInSndCardBuf around 40 + 5 s with out-of-range values behind the start-up phases."""
    T = GOLDEN_CALLS // K
    rng = np.random.default_rng(seed)
    flags = np.zeros((T, mh.S9), dtype=np.uint8)
    for s in mh.ALWAYS_HALF:
        flags[:, s] |= HALF_CALL
    flags[rng.random(T) < 1 / 3, mh.SOMETIMES_HALF] |= HALF_CALL
    flags |= (rng.random((T, mh.S9)) < 0.1).astype(np.uint8) * NO_FAREND
    flags[rng.random((T, mh.S9)) < 0.2] |= IDLE
    ms = (40 + 5 * np.arange(mh.S9)[None, :] + rng.integers(-3, 4, (T, mh.S9))).astype(np.int16)
    wild = rng.random((T, mh.S9)) < 0.08
    wild[:T // 3] = False
    ms[wild] = np.where(rng.random(int(wild.sum())) < 0.5, -300, 700).astype(np.int16)
    return flags, ms


def packets_ops(K, n, flags, ms):
    return [dict(kind="packets", K=K, n=n, flags=flags[t], ms=ms[t]) for t in range(flags.shape[0])]


def span_of(op):
    return op["n"] * (op["K"] if op["kind"] in ("packets", "calls") else 1)


def call_sizes(op, S):
    """n_s[S]: the samples of ONE call of each session in this op (0: the session makes none)."""
    flags = op.get("flags", np.zeros(S, np.uint8))
    n_s = np.full(S, op["n"], dtype=np.int64)
    if op["kind"] in ("packets", "tick"):
        n_s[(flags & HALF_CALL) != 0] = 80
    if op["kind"] != "burst":
        n_s[(flags & IDLE) != 0] = 0
    return n_s


class Feed:
    """Every session's next samples, by its own cursor: a session consumes what its calls take, the rest of its rows is junk."""

    def __init__(self, far, near, clean=None, farx=None):
        self.far, self.near, self.clean, self.farx = far, near, clean, farx
        S = far.shape[0]
        self.cur, self.xcur = np.zeros(S, dtype=np.int64), np.zeros(S, dtype=np.int64)

    def rows(self, take, width):
        f, d, c = mh.tick_rows(self.far, self.near, self.clean, self.cur, take, width)
        self.cur = self.cur + take
        return f, d, c

    def burst_rows(self, width):
        S = self.far.shape[0]
        f = np.stack([self.farx[s, self.xcur[s]:self.xcur[s] + width] for s in range(S)])
        self.xcur = self.xcur + width
        return f


def run_reference(make_session, rates, ops, feed, sessions=None):
    """One instance per session (make_session(fs)).  Returns (out[S, total]: zeros where a session made no call, codes[len(ops), S], sessions)."""
    S = feed.far.shape[0]
    sessions = [make_session(int(fs)) for fs in rates] if sessions is None else sessions
    outs, codes = [], np.zeros((len(ops), S), dtype=np.int32)
    for t, op in enumerate(ops):
        span, n_s = span_of(op), call_sizes(op, S)
        K = op["K"] if op["kind"] in ("packets", "calls") else 1
        flags = op.get("flags", np.zeros(S, np.uint8))
        fx = feed.burst_rows(op["B"] * op["n"]) if op["kind"] == "burst" else None
        f, d, c = feed.rows(K * n_s, span)
        o = np.zeros((S, span), dtype=np.int16)
        for s in np.flatnonzero(n_s):
            sess, ms, k = sessions[s], int(op["ms"][s]), int(n_s[s])
            if op["kind"] == "burst":
                for b in range(op["B"]):
                    assert sess.buffer_farend(fx[s, b * k:(b + 1) * k]) == 0
                codes[t, s], o[s] = sess.process(d[s], None if c is None else c[s], ms)
                continue
            for q in range(K):
                sl = slice(q * k, (q + 1) * k)
                rc, o[s, sl] = mh.session_call(sess, f[s, sl], d[s, sl], None if c is None else c[s, sl], k,
                                               int(flags[s]) & (NO_FAREND | (SPLIT_CALLS if op["kind"] == "tick" else 0)), ms)
                codes[t, s] = codes[t, s] or rc
        outs.append(o)
    return np.concatenate(outs, axis=1), codes, sessions


def relaid(rows, n_s, q, n, junk):
    """The [S, n] rows of ordinary tick q of a packet tick: session s's samples [q n_s, (q + 1) n_s) first, junk behind them."""
    S = rows.shape[0]
    r = np.full((S, n), junk, dtype=np.int16)
    for s in range(S):
        k = int(n_s[s])
        r[s, :k] = rows[s, q * k:(q + 1) * k]
    return r


def run_object(sb, ops, feed, form="host", as_single_ticks=False, check=None):
    """The schedule on an AecmSessions object.  form (packet ticks only; everything else through the host forms): host
    (TickPacketsHost), device (TickPackets), async (TickPacketsAsync + Synchronize).  as_single_ticks: every packet tick and every
    K-call tick as K ordinary ticks on re-laid rows (the twin).  Device forms: an idle session's out row and a half-call session's
    samples [K * 80, K * n) must keep their sentinel.  Returns (out, codes); out is zero wherever no call delivered a sample."""
    S = feed.far.shape[0]
    outs, codes = [], np.zeros((len(ops), S), dtype=np.int32)
    for t, op in enumerate(ops):
        n, span, n_s = op["n"], span_of(op), call_sizes(op, S)
        K = op["K"] if op["kind"] in ("packets", "calls") else 1
        flags = np.ascontiguousarray(op.get("flags", np.zeros(S, np.uint8)), dtype=np.uint8)
        ms = np.ascontiguousarray(op["ms"], dtype=np.int16)
        fx = feed.burst_rows(op["B"] * n) if op["kind"] == "burst" else None
        f, d, c = feed.rows(K * n_s, span)
        written = np.arange(span)[None, :] < (K * n_s)[:, None]               # [S, span]: the samples the session's calls deliver
        if op["kind"] == "tick":
            rc, o, codes[t] = sb.tick_host_per_session(f, d, ms, c, flags=flags)
        elif op["kind"] == "burst":
            assert sb.buffer_farend_host(fx, n, op["B"]) == 0
            rc, o, codes[t] = sb.process_host(d, clean=c, ms_per_session=ms)
        elif as_single_ticks:
            o, rc = np.zeros((S, span), dtype=np.int16), 0
            for q in range(K):
                r1, oq, c1 = sb.tick_host_per_session(relaid(f, n_s, q, n, JUNK_FAR), relaid(d, n_s, q, n, JUNK_NEAR), ms,
                                                      None if c is None else relaid(c, n_s, q, n, JUNK_CLEAN), flags=flags)
                for s in range(S):
                    k = int(n_s[s])
                    o[s, q * k:(q + 1) * k] = oq[s, :k]
                    assert not oq[s, k:].any(), ("the twin's host form returns zeros behind a call", t, s)
                rc = rc or r1
                codes[t] = np.where(codes[t] != 0, codes[t], c1)
        elif op["kind"] == "calls":
            rc, o, codes[t] = sb.tick_calls_host(f, d, K, ms, clean=c, flags=flags)
        elif form == "host":
            rc, o, codes[t] = sb.tick_packets_host(f, d, K, ms, clean=c, flags=flags)
            assert not o[~written].any(), ("the host form returns zeros where no call delivers", t)
        else:
            import torch
            df, dd = torch.from_numpy(f).cuda(), torch.from_numpy(d).cuda()
            dc = None if c is None else torch.from_numpy(c).cuda()
            do = torch.full((S, span), SENTINEL, dtype=torch.int16, device="cuda")
            torch.cuda.synchronize()
            rc, codes[t] = sb.tick_packets_device(df.data_ptr(), dd.data_ptr(), do.data_ptr(), span, n, K, ms, clean_ptr=None if dc is None else dc.data_ptr(),
                                                  flags=flags, asynchronous=form == "async")
            if form == "async":
                assert sb.synchronize() == 0
            o = do.cpu().numpy()
            assert np.all(o[~written] == SENTINEL), ("an idle row or a half-call session's samples behind its calls were written", t)
            o[~written] = 0
        nz = codes[t][codes[t] != 0]
        assert rc == (int(nz[0]) if nz.size else 0), (t, rc, codes[t])
        assert np.all(codes[t][n_s == 0] == 0)
        if check is not None:
            check(t, op)
        outs.append(o)
    return np.concatenate(outs, axis=1), codes
