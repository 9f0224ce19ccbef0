"""TEST INFRASTRUCTURE for ticks of K call pairs (WebRtcAecmSessions_TickCalls): schedules of K-call ticks, ordinary ticks and
far-end bursts with a Process, executed on an AecmSessions object (K-call ticks as such, or -- the twin -- as K ordinary ticks on
the same rows) and on one WebRtcAecm_* instance per session (the reference); the recipes of the golden runs and of the replay-row
spill inside a K-call tick."""
from __future__ import annotations

import numpy as np

import sparse_helpers as sh

NO_FAREND, SPLIT_CALLS, IDLE = sh.NO_FAREND, sh.SPLIT_CALLS, sh.IDLE
SENTINEL = 0x7b7b

# Replay-row spill inside a K-call tick (tests/sim/sim_calls.cpp: sim_calls_spill_recipe confirms call > 0), 16 kHz, ms 40:
# PRE ordinary ticks of 160 samples (the start-up phase ends, farendOld[1] lives in the far ring), then K_TICKS ticks of K calls
# of 80 samples (only farendOld[0] is refreshed; more than 98 calls: the ring's write position laps farendOld[1], which moves
# to its row), then one 160-sample tick without a far end: it replays farendOld[1] from the row.
SPILL_RECIPE = dict(fs=16000, pre_ticks=12, calls=6, k_ticks=17)

# tools/gen_golden.py: sesscalls_* -- 9 sessions x 48 calls each, the unmodified reference.
GOLDEN_CASES = {"sesscalls_fs16000_f160_k2": (16000, 160, 2, 9300), "sesscalls_fs8000_f80_k3": (8000, 80, 3, 9400)}
GOLDEN_S, GOLDEN_CALLS = 9, 48


def golden_pattern(n, K, seed):
    """flags[T, S], ms[T, S] of a golden run: T = 48 / K ticks, 20 % idle, underruns, per-session msInSndCardBuf with out-of-range values."""
    flags, ms = sh.pattern(seed, GOLDEN_S, GOLDEN_CALLS // K, 0.2, n=80, flags_p=0.15, ms_spread=True)
    return flags, ms


def calls_ops(K, n, flags, ms):
    return [dict(kind="calls", K=K, n=n, flags=flags[t], ms=ms[t]) for t in range(flags.shape[0])]


def per_call(K, flags, ms):
    """The per-tick arrays of T K-call ticks as those of the T * K ordinary ticks they stand for."""
    return np.repeat(flags, K, axis=0), np.repeat(ms, K, axis=0)


class Feed:
    """Every session's next samples: a live session consumes, an idle one gets junk that must not be read."""

    def __init__(self, far, near, clean=None, farx=None):
        self.far, self.near, self.clean, self.farx = far, near, clean, farx
        S = far.shape[0]
        self.cur, self.xcur = np.zeros(S, dtype=np.int64), np.zeros(S, dtype=np.int64)

    def rows(self, live, width):
        f, d, c = sh.tick_rows(self.far, self.near, self.clean, self.cur, live, width)
        self.cur[live] += width
        return f, d, c

    def burst_rows(self, width):
        S = self.far.shape[0]
        f = np.stack([self.farx[s, self.xcur[s]:self.xcur[s] + width] for s in range(S)])
        self.xcur += width
        return f


def span_of(op):
    return op["n"] * (op["K"] if op["kind"] == "calls" else 1)


def run_reference(make_session, ops, feed, sessions=None):
    """One instance per session.  Returns (out[S, total] with an idle session's tick as zeros, codes[len(ops), S], sessions)."""
    S = feed.far.shape[0]
    sessions = [make_session() for _ in range(S)] if sessions is None else sessions
    outs, codes = [], np.zeros((len(ops), S), dtype=np.int32)
    for t, op in enumerate(ops):
        n, span = op["n"], span_of(op)
        flags = op.get("flags", np.zeros(S, np.uint8))
        live = (flags & IDLE) == 0 if op["kind"] != "burst" else np.ones(S, bool)
        fx = feed.burst_rows(op["B"] * n) if op["kind"] == "burst" else None
        f, d, c = feed.rows(live, span)
        o = np.zeros((S, span), dtype=np.int16)
        for s in np.flatnonzero(live):
            sess, ms, cs = sessions[s], int(op["ms"][s]), None if c is None else c[s]
            if op["kind"] == "tick":
                codes[t, s], o[s] = sh.session_call(sess, f[s], d[s], cs, n, int(flags[s]), ms)
            elif op["kind"] == "calls":
                for k in range(op["K"]):
                    sl = slice(k * n, (k + 1) * n)
                    if not (flags[s] & NO_FAREND):
                        assert sess.buffer_farend(f[s, sl]) == 0
                    rc, o[s, sl] = sess.process(d[s, sl], None if cs is None else cs[sl], ms)
                    codes[t, s] = codes[t, s] or rc
            else:
                for b in range(op["B"]):
                    assert sess.buffer_farend(fx[s, b * n:(b + 1) * n]) == 0
                codes[t, s], o[s] = sess.process(d[s], cs, ms)
        outs.append(o)
    return np.concatenate(outs, axis=1), codes, sessions


def run_object(sb, ops, feed, form="host", as_single_ticks=False):
    """The schedule on an AecmSessions object.  form (K-call ticks only; everything else through the host forms): host
    (TickCallsHost), device (TickCalls), async (TickCallsAsync + Synchronize).  as_single_ticks: every K-call tick as K ordinary
    ticks on the same rows (the twin).  Device forms: an idle session's out row must keep its sentinel.  Returns (out, codes)."""
    S = feed.far.shape[0]
    outs, codes = [], np.zeros((len(ops), S), dtype=np.int32)
    for t, op in enumerate(ops):
        n, span = op["n"], span_of(op)
        flags = np.ascontiguousarray(op.get("flags", np.zeros(S, np.uint8)), dtype=np.uint8)
        live = (flags & IDLE) == 0 if op["kind"] != "burst" else np.ones(S, bool)
        ms = np.ascontiguousarray(op["ms"], dtype=np.int16)
        fx = feed.burst_rows(op["B"] * n) if op["kind"] == "burst" else None
        f, d, c = feed.rows(live, span)
        if op["kind"] == "tick":
            rc, o, codes[t] = sb.tick_host_per_session(f, d, ms, c, flags=flags)
        elif op["kind"] == "burst":
            assert sb.buffer_farend_host(fx, n, op["B"]) == 0
            rc, o, codes[t] = sb.process_host(d, clean=c, ms_per_session=ms)
        elif as_single_ticks:
            o, rc = np.zeros((S, span), dtype=np.int16), 0
            for k in range(op["K"]):
                sl = slice(k * n, (k + 1) * n)
                r1, o[:, sl], c1 = sb.tick_host_per_session(f[:, sl], d[:, sl], ms, None if c is None else c[:, sl], flags=flags)
                rc = rc or r1
                codes[t] = np.where(codes[t] != 0, codes[t], c1)
        elif form == "host":
            rc, o, codes[t] = sb.tick_calls_host(f, d, op["K"], ms, clean=c, flags=flags)
            assert np.all(o[~live] == 0), ("idle rows of the host form are zeros", t)
        else:
            import torch
            df, dd = torch.from_numpy(f).cuda(), torch.from_numpy(d).cuda()
            dc = None if c is None else torch.from_numpy(c).cuda()
            do = torch.full((S, span), SENTINEL, dtype=torch.int16, device="cuda")
            torch.cuda.synchronize()
            rc, codes[t] = sb.tick_calls_device(df.data_ptr(), dd.data_ptr(), do.data_ptr(), span, n, op["K"], ms, clean_ptr=None if dc is None else dc.data_ptr(),
                                                flags=flags, asynchronous=form == "async")
            if form == "async":
                assert sb.synchronize() == 0
            o = do.cpu().numpy()
            assert np.all(o[~live] == SENTINEL), ("an idle session's out row was written", t)
            o[~live] = 0
        nz = codes[t][codes[t] != 0]
        assert rc == (int(nz[0]) if nz.size else 0), (t, rc, codes[t])
        assert np.all(codes[t][~live] == 0)
        outs.append(o)
    return np.concatenate(outs, axis=1), codes
