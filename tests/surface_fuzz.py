"""TEST INFRASTRUCTURE: the session API fuzz over the whole tick surface (tests/test_session_surface_fuzz.py on the CPU,
tests/test_gpu_session_surface_fuzz.py on the device).  No product code and no device is touched here.

  generate(case)  a seeded PROGRAM: a list of ops (plain dicts of ints, strings and lists) on two objects, 0 = A and 1 = B -- every
                  tick entry point in its device, Host and Async form, far-end bursts, Process, slot life, migration, the diagnostic
                  switches, a safe-variant window, the two traces, and about one op in eight that the header says is refused (RULES).
                  The generator keeps a Shadow of both objects, so that every op it emits is legal or refused by exactly one named rule.
  Shadow          what include/aecm_batch.h says an object remembers between calls (rates, clean modes, switches, traces, counts) and
                  tick_code(): the header's refusals of a tick restated in the order it gives them.  Nothing is imported from the product.
  Model           Shadow + one reference instance per session slot.  session_calls() restates the header's loops (TickCalls,
                  TickPackets, HALF_CALL, SPLIT_CALLS, NO_FAREND, IDLE, NO_CLEAN): which WebRtcAecm_* calls a session receives from an
                  op, on which samples, with which nearendClean.  rows_of() lays the same samples out as the rows the object is given,
                  with junk wherever the device must not read.

python -m surface_fuzz --case small-16k --until 40 --print      lists a program (run from tests/)."""
from __future__ import annotations

import hashlib
import json
from collections import Counter

import numpy as np

NO_FAREND, SPLIT_CALLS, IDLE, HALF_CALL, NO_CLEAN = 1, 2, 4, 8, 16
FLAG_NAMES = {NO_FAREND: "NO_FAREND", SPLIT_CALLS: "SPLIT_CALLS", IDLE: "IDLE", HALF_CALL: "HALF_CALL", NO_CLEAN: "NO_CLEAN"}
UNSUPPORTED, BAD_PARAMETER, WARNING = 12001, 12004, 12100
NONE, ALWAYS, NEVER = 0, 1, 2                       # a session's clean mode (WebRtcAecmSessions_GetSessionCleanMode) and its kind
MAX_TICK_CALLS = 6
FILL = 0x7b7b                                       # every out buffer before the call
POOL, POOL_SAMPLES, WIDEST = 12, 48000, 40 * 160

# entry point -> its forms.  (TickAsync is the Async form of TickFlags / Tick: its own entry, because it takes flags optionally.)
FORMS = {"Tick": ("device", "host"), "TickPerSession": ("device", "host"), "TickFlags": ("device", "host"), "TickAsync": ("async",),
         "TickCalls": ("device", "host", "async"), "TickPackets": ("device", "host", "async")}
TAKES_FLAGS = {"TickFlags": "always", "TickAsync": "optional", "TickCalls": "optional", "TickPackets": "optional"}

# The cases: the smallest shapes at which the planners and lists can still go wrong.  families: what the host planner twin must name
# over the case (tests/test_session_surface_fuzz.py; an object that holds two rates plans every tick of one call pair as "mixed").  special: where single-slot ops land two times in three.
CASES = {
    "small-16k": dict(seed=4101, S=6, fs=(16000, 16000), rates="uniform", steps=900,
                      families=["calls", "dense", "mixed", "nothing", "packets", "sparse", "split"]),
    "small-8k": dict(seed=4102, S=6, fs=(8000, 8000), rates="uniform", steps=600,
                     families=["calls", "dense", "mixed", "nothing", "packets", "sparse", "split"]),
    "wave-mixed": dict(seed=4103, S=70, fs=(16000, 8000), rates="alternate", steps=520,
                       families=["mixed", "nothing", "packets", "split"]),
    "group-mixed": dict(seed=4104, S=261, fs=(16000, 16000), rates="third", steps=380,
                        families=["mixed", "nothing", "packets", "split"]),
}


def case_rates(case):
    """[rates of A's slots, rates of B's] at the start of the case."""
    c = CASES[case]
    S = c["S"]
    out = []
    for o in range(2):
        fs = c["fs"][o]
        if c["rates"] == "uniform":
            out.append([fs] * S)
        elif c["rates"] == "alternate":
            out.append([16000 if s % 2 == 0 else 8000 for s in range(S)])
        else:
            out.append([8000 if s % 3 == 2 else fs for s in range(S)])
    return out


def special_slots(case):
    S = CASES[case]["S"]
    if S <= 8:
        return []
    return sorted({0, 3, 4, 63, 64, 65, S - 2, S - 1} | ({255, 256} if S > 256 else set()))


# ---- the reference instance that can be cloned ------------------------------------------------------------------------------------
class LoggedRef:
    """A reference session that remembers every call it received, so that a second reference session in the same state can be
    made by replaying them (the reference has no way to copy an instance; migration tests need the copy).  make(fs): a fresh
    instance (split_calls_helpers.make_reference()); without one, the unmodified reference's."""

    def __init__(self, fs, make=None):
        if make is None:
            from oracle import pyoracle
            make = lambda f: pyoracle.RefSession(f, 1, 3)
        self.fs, self.make = fs, make
        self.ref = make(fs)
        self.log = []

    def call(self, name, *args):
        self.log.append((name, args))
        return getattr(self.ref, name)(*args)

    def clone(self):
        c = LoggedRef(self.fs, self.make)
        for name, args in self.log:
            c.call(name, *args)
        return c


# ---- what an object remembers --------------------------------------------------------------------------------------------------
class Obj:
    def __init__(self, S, fs, rates):
        self.S, self.fs, self.rates = S, fs, list(rates)
        self.mode = [NONE] * S                     # GetSessionCleanMode
        self.kind = [NONE] * S                     # what the slot's reference instance has been given in its life (survives migration)
        self.cfg = [(1, 3)] * S
        self.pending = [False] * S                 # far frames of a burst buffered, no Process call since
        self.split_used = False
        self.split_call_ticks = self.force_sparse = self.safe = False
        self.two_launches = -1
        self.trace = None                          # None, "session", "call"
        self.trace_ring, self.trace_layout, self.trace_count = 1, "session-major", 0

    def other_rates(self):
        return sum(r != self.fs for r in self.rates)


def gives(flag, clean):
    return ALWAYS if clean and not flag & NO_CLEAN else NEVER


def flag_of(op, s):
    return 0 if op.get("flags") is None else op["flags"][s]


def callers(op, S):
    if op["kind"] == "process" or op.get("flags") is None:
        return list(range(S))
    return [s for s in range(S) if not op["flags"][s] & IDLE]


def tick_code(ob, op):
    """0, or the code a tick / Process is refused with: the header's rules in the order it checks them (TickCalls: 'the arguments are
    checked in the reference's order ... then', the paragraphs of TickPackets, SetSessionTrace, AECM_SESSION_NO_CLEAN, SetSplitCallTicks)."""
    n, K = op["n"], op.get("K", 1)
    packets = op.get("entry") == "TickPackets"
    if K < 1 or K > MAX_TICK_CALLS:
        return BAD_PARAMETER
    if op["stride"] < n * K:
        return BAD_PARAMETER
    if ob.safe:
        return UNSUPPORTED
    if K > 1 and ob.other_rates() and not packets:
        return UNSUPPORTED
    if K > 1 and ob.trace == "session":
        return UNSUPPORTED
    live = callers(op, ob.S)
    flags = [NO_FAREND if op["kind"] == "process" else flag_of(op, s) for s in live]
    anybits = 0
    for f in flags:
        anybits |= f
    if (anybits & (SPLIT_CALLS | HALF_CALL)) and n != 160:
        return BAD_PARAMETER
    if any(f & SPLIT_CALLS and f & HALF_CALL for f in flags):
        return BAD_PARAMETER
    if K > 1 and anybits & (SPLIT_CALLS if packets else SPLIT_CALLS | HALF_CALL):
        return BAD_PARAMETER
    split = bool(op["clean"]) and op.get("flags") is not None and bool(anybits & NO_CLEAN)
    if split and K > 1 and not (ob.split_call_ticks and ob.trace != "call"):
        return UNSUPPORTED
    if split or ob.split_used:
        for s, f in zip(live, flags):
            if ob.mode[s] not in (NONE, gives(f, op["clean"])):
                return BAD_PARAMETER
    return 0


class Shadow:
    """Both objects of a case as the header describes them; apply(op) is what an op leaves behind."""

    def __init__(self, case):
        c = CASES[case]
        self.case = case
        self.ob = [Obj(c["S"], c["fs"][o], case_rates(case)[o]) for o in range(2)]

    def apply(self, op):
        ob = self.ob[op["obj"]]
        k = op["kind"]
        if op.get("expect", 0) not in (0, WARNING):
            return
        if k in ("tick", "process"):
            live = callers(op, ob.S)
            if ob.trace:
                ob.trace_count += op.get("K", 1) if ob.trace == "call" else 1
            if not live:
                return
            split = bool(op["clean"]) and op.get("flags") is not None and any(flag_of(op, s) & NO_CLEAN for s in live)
            ob.split_used = ob.split_used or split
            for s in live:
                g = gives(flag_of(op, s), op["clean"])
                assert ob.kind[s] in (NONE, g), ("the generator gave a session another kind", op, s)
                ob.kind[s] = g
                ob.mode[s] |= g
                ob.pending[s] = False
        elif k == "burst":
            for s in range(ob.S):
                if burst_calls(op, s):
                    ob.pending[s] = True
        elif k in ("init_session", "init_session_rate"):
            s = op["s"]
            ob.rates[s] = ob.fs if k == "init_session" else op["rate"]
            ob.mode[s] = ob.kind[s] = NONE
            ob.cfg[s] = (1, 3)
            ob.pending[s] = False
        elif k == "set_config":
            ob.cfg[op["s"]] = (op["cng"], op["echo"])
        elif k in ("migrate", "migrate_bulk"):
            dst = self.ob[op["dst"]]
            pairs = [(op["s"], op["j"])] if k == "migrate" else list(zip(op["ss"], op["js"]))
            moved = [(ob.rates[a], ob.kind[a], ob.cfg[a], ob.pending[a]) for a, _ in pairs]
            for (_, j), (rate, kind, cfg, pend) in zip(pairs, moved):
                dst.rates[j], dst.kind[j], dst.cfg[j], dst.pending[j] = rate, kind, cfg, pend
                dst.mode[j] = NONE
        elif k == "force_sparse":
            ob.force_sparse = bool(op["on"])
        elif k == "two_launches":
            ob.two_launches = op["on"]
        elif k == "split_call_ticks":
            ob.split_call_ticks = bool(op["on"])
        elif k == "variant":
            ob.safe = bool(op["safe"])
        elif k == "trace":
            ob.trace, ob.trace_count = op["which"], 0
            ob.trace_ring, ob.trace_layout = op.get("ring", 1), op.get("layout", "session-major")


# ---- the header's loops -----------------------------------------------------------------------------------------------------------
def burst_calls(op, s):
    return op["calls"] if op.get("calls_host") is None else op["calls_host"][s]


def session_calls(op, s):
    """The WebRtcAecm_* call pairs session s receives from a tick / Process op, in order: [(offset into its rows, samples, with a
    WebRtcAecm_BufferFarend, with nearendClean)] -- include/aecm_batch.h: TickFlags' flags, TickCalls, TickPackets, Process."""
    n = op["n"]
    if op["kind"] == "process":
        return [(0, n, False, bool(op["clean"]))]
    f = flag_of(op, s)
    if f & IDLE:
        return []
    far, clean = not f & NO_FAREND, bool(op["clean"]) and not f & NO_CLEAN
    K = op.get("K", 1)
    if f & SPLIT_CALLS:                                     # (K == 1, n == 160: two call pairs of 80, first half then second half)
        return [(0, 80, far, clean), (80, 80, far, clean)]
    n_s = 80 if f & HALF_CALL else n                        # (packed: call c of a half-call session lies at c * 80)
    return [(c * n_s, n_s, far, clean) for c in range(K)]


def consumed(op, s):
    return sum(p[1] for p in session_calls(op, s))


class Audio:
    """POOL recordings (far, near, clean); slot s of object o reads recording (o * S + s) % POOL at its own far and near positions."""

    def __init__(self):
        from webrtc_aecm_amd.synth import synth_clean, synth_pair
        pairs = [synth_pair(7300 + p, POOL_SAMPLES // 64 + 1, 16000 if p % 2 == 0 else 8000, "mixed") for p in range(POOL)]
        self.far = [p[0][:POOL_SAMPLES] for p in pairs]
        self.near = [p[1][:POOL_SAMPLES] for p in pairs]
        self.clean = [synth_clean(a) for a in self.near]

    @staticmethod
    def at(pos):
        return pos % (POOL_SAMPLES - WIDEST)


_audio = None


def audio():
    global _audio
    if _audio is None:
        _audio = Audio()
    return _audio


def row_width(op):
    if op["kind"] == "burst":                                # (a refused burst: rows of six calls, all junk)
        return (op["calls"] if 0 < op["calls"] <= 40 else 6) * op["n"]
    return max(1, op.get("K", 1)) * op["n"]


def rows_of(op, S):
    """The planes an op's call is given: {far, near, clean (or None)} [S, row_width] int16.  A session's samples lie where
    session_calls() says; everything the device must not read -- an idle session's rows, the far row of NO_FAREND, the clean row of
    NO_CLEAN, what a half call leaves unused -- holds the op's junk value (another one in every op and plane)."""
    au, W = audio(), row_width(op)
    j = op["junk"]
    far = np.full((S, W), j, dtype=np.int16)
    if op["kind"] == "burst":
        for s in range(S if "rule" not in op else 0):
            m = burst_calls(op, s) * op["n"]
            p = (op["obj"] * S + s) % POOL
            a = au.at(op["far_at"][s])
            far[s, :m] = au.far[p][a:a + m]
        return dict(far=far, near=None, clean=None)
    near = np.full((S, W), j + 1, dtype=np.int16)
    clean = np.full((S, W), j + 2, dtype=np.int16) if op["clean"] else None
    for s in range(S):
        p = (op["obj"] * S + s) % POOL
        fa, na = au.at(op["far_at"][s]), au.at(op["near_at"][s])
        done = 0
        for off, m, with_far, with_clean in session_calls(op, s):
            if with_far:
                far[s, off:off + m] = au.far[p][fa + done:fa + done + m]
            near[s, off:off + m] = au.near[p][na + done:na + done + m]
            if with_clean:
                clean[s, off:off + m] = au.clean[p][na + done:na + done + m]
            done += m
    return dict(far=far, near=near, clean=clean)


# ---- the model -------------------------------------------------------------------------------------------------------------------
class Model(Shadow):
    """Shadow + the reference instances.  apply(op) -> what the object must answer:
    tick / process: rc, codes[S], out[S, W] (zeros where nothing is written), written[S, W], rows;  get_echo_path: path;  else rc."""

    def __init__(self, case, make=None):
        super().__init__(case)
        if make is None:
            import split_calls_helpers as sch
            make = sch.make_reference()
        self.refs = [[LoggedRef(r, make) for r in ob.rates] for ob in self.ob]
        self.compared = self.working = 0
        self.digest = hashlib.sha256()

    def _ms(self, op, s):
        return op["ms"] if isinstance(op["ms"], int) else op["ms"][s]

    def apply(self, op):
        o, k = op["obj"], op["kind"]
        ob, refs = self.ob[o], self.refs[o]
        exp = dict(rc=op.get("expect", 0))
        refused = exp["rc"] not in (0, WARNING)
        if k in ("tick", "process", "burst"):
            exp["rows"] = rows_of(op, ob.S)
        if refused:
            pass
        elif k in ("tick", "process"):
            rows, W = exp["rows"], row_width(op)
            out, written = np.zeros((ob.S, W), np.int16), np.zeros((ob.S, W), bool)
            codes = np.zeros(ob.S, np.int32)
            for s in range(ob.S):
                for off, m, with_far, with_clean in session_calls(op, s):
                    if with_far:
                        assert refs[s].call("buffer_farend", rows["far"][s, off:off + m].copy()) == 0
                    near = rows["near"][s, off:off + m].copy()
                    clean = rows["clean"][s, off:off + m].copy() if with_clean else None
                    rc, o1 = refs[s].call("process", near, clean, self._ms(op, s))
                    out[s, off:off + m], written[s, off:off + m] = o1, True
                    codes[s] = codes[s] or rc
                    self.compared += 1
                    self.working += int(not np.array_equal(o1, clean if with_clean else near))      # (start-up: the copy of that input)
            nz = codes[codes != 0]
            exp.update(rc=int(nz[0]) if nz.size else 0, codes=codes, out=out, written=written)
            assert exp["rc"] == op.get("expect", 0), ("the reference's code is not the one the generator expected", op["step"], exp["rc"])
            self.digest.update(codes.tobytes() + out.tobytes())
        elif k == "burst":
            for s in range(ob.S):
                for c in range(burst_calls(op, s)):
                    assert refs[s].call("buffer_farend", exp["rows"]["far"][s, c * op["n"]:(c + 1) * op["n"]].copy()) == 0
        elif k in ("init_session", "init_session_rate"):
            rate = ob.fs if k == "init_session" else op["rate"]
            assert refs[op["s"]].call("init", rate) == 0
            refs[op["s"]].log = refs[op["s"]].log[-1:]              # (WebRtcAecm_Init leaves nothing of what came before)
        elif k == "set_config":
            assert refs[op["s"]].call("set_config", op["cng"], op["echo"]) == 0
        elif k == "init_echo_path":
            assert refs[op["s"]].call("init_echo_path", np.array(op["path"], dtype=np.int16)) == 0
        elif k == "get_echo_path":
            rc, exp["path"] = refs[op["s"]].call("get_echo_path")
            assert rc == 0
            self.digest.update(exp["path"].tobytes())
        elif k in ("migrate", "migrate_bulk"):
            pairs = [(op["s"], op["j"])] if k == "migrate" else list(zip(op["ss"], op["js"]))
            clones = [refs[a].clone() for a, _ in pairs]
            for (_, j), c in zip(pairs, clones):
                self.refs[op["dst"]][j] = c
        super().apply(op)
        return exp

    def echo_paths(self, o):
        return np.stack([r.ref.get_echo_path()[1] for r in self.refs[o]])


# ---- the refusals: one table ---------------------------------------------------------------------------------------------------------
# (name, how to build the op from the generator's state -- None where the state does not admit it --, the code the header states).
# Only rules that are refused on the host before any launch.
def _r_calls_range(g, o):
    if g.rs.rand() < 0.3:
        op = g.draw_burst(o)
        op["calls"], op["calls_host"] = int(g.rs.choice([-1, 256])), None
        return op
    op = g.draw_tick(o, entry=g.pick(["TickCalls", "TickPackets"]), K=1)
    op["K"] = int(g.rs.choice([0, 7]))
    op["stride"] = max(1, op["K"]) * op["n"]
    return op


def _r_short_stride(g, o):
    op = g.draw_tick(o)
    op["stride"] = op["n"] * op["K"] - int(g.rs.choice([1, 16, 80]))
    return op


def _flag_a_caller(g, op, bit, clear=0):
    live = [s for s in range(len(op["flags"])) if not op["flags"][s] & IDLE]
    if not live:
        return None
    s = g.pick(live)
    op["flags"][s] = (op["flags"][s] | bit) & ~clear
    return op


def _r_half_80(g, o):
    op = g.draw_tick(o, entry=g.pick(["TickFlags", "TickAsync", "TickCalls", "TickPackets"]), n=80, K=1, flags=True)
    return _flag_a_caller(g, op, HALF_CALL)


def _r_flags_k(g, o):
    ob = g.sh.ob[o]
    if ob.trace == "session":
        return None
    if ob.other_rates() == 0 and g.rs.rand() < 0.7:
        op = g.draw_tick(o, entry="TickCalls", n=160, K=int(g.rs.randint(2, 7)), flags=True)
        return _flag_a_caller(g, op, int(g.rs.choice([HALF_CALL, SPLIT_CALLS])))
    op = g.draw_tick(o, entry="TickPackets", n=160, K=int(g.rs.randint(2, 7)), flags=True)
    return _flag_a_caller(g, op, SPLIT_CALLS, clear=HALF_CALL)


def _r_two_rates(g, o):
    if not g.sh.ob[o].other_rates() or g.sh.ob[o].trace == "session":
        return None
    op = g.draw_tick(o, entry="TickPackets", K=int(g.rs.randint(2, 7)))
    op["entry"] = "TickCalls"
    return op


def _r_kind(g, o):
    ob = g.sh.ob[o]
    if not any(m == ALWAYS for m in ob.mode):
        return None
    op = g.draw_tick(o, entry=g.pick(["TickFlags", "TickAsync", "TickCalls", "TickPackets"]), K=1, flags=True, clean=True)
    s = g.pick([s for s in range(ob.S) if ob.mode[s] == ALWAYS])
    op["flags"][s] = (op["flags"][s] & ~IDLE) | NO_CLEAN
    if op["n"] == 80:
        op["flags"][s] &= ~(HALF_CALL | SPLIT_CALLS)
    if op["flags"][s] & SPLIT_CALLS:
        op["flags"][s] &= ~HALF_CALL
    return op


def _mixed_k(g, o):
    ob = g.sh.ob[o]
    never = [s for s in range(ob.S) if ob.kind[s] in (NONE, NEVER)]
    if not never or ob.trace == "session":
        return None
    op = g.draw_tick(o, entry="TickPackets" if ob.other_rates() or g.rs.rand() < 0.5 else "TickCalls", K=int(g.rs.randint(2, 7)), flags=True, clean=True,
                     clean_only=True)
    s = g.pick(never)
    op["flags"][s] = (op["flags"][s] & ~(IDLE | SPLIT_CALLS | (0 if op["entry"] == "TickPackets" and op["n"] == 160 else HALF_CALL))) | NO_CLEAN
    return op


def _r_mixed_switch_off(g, o):
    ob = g.sh.ob[o]
    return None if ob.split_call_ticks or ob.trace == "call" else _mixed_k(g, o)


def _r_mixed_call_trace(g, o):
    return _mixed_k(g, o) if g.sh.ob[o].trace == "call" else None


def _r_session_trace_k(g, o):
    if g.sh.ob[o].trace != "session":
        return None
    op = g.draw_tick(o, entry="TickPackets", K=1)
    op["K"] = int(g.rs.randint(2, 7))
    op["stride"] = op["K"] * op["n"]
    if op["flags"] is not None:                              # (K call pairs of the flags of a legal tick of one: no SPLIT_CALLS)
        op["flags"] = [f & ~SPLIT_CALLS for f in op["flags"]]
    return op


def _r_safe(g, o):
    return None                                              # (made by the safe-variant window, not drawn on its own)


def _r_init_range(g, o):
    return dict(kind="init_session", obj=o, s=g.sh.ob[o].S)


def _r_config(g, o):
    s = g.slot(o)
    return dict(kind="set_config", obj=o, s=s, cng=g.sh.ob[o].cfg[s][0], echo=7)


def _r_import_rate(g, o):
    ob, dst = g.sh.ob[o], g.sh.ob[1 - o]
    other = [s for s in range(ob.S) if ob.rates[s] != dst.fs]
    if not other or ob.safe or dst.safe:
        return None
    return dict(kind="migrate", obj=o, s=g.pick(other), dst=1 - o, j=g.slot(1 - o), how="plain", sync_before=True)


RULES = [
    ("calls out of range", _r_calls_range, BAD_PARAMETER),
    ("a short stride", _r_short_stride, BAD_PARAMETER),
    ("HALF_CALL with n == 80", _r_half_80, BAD_PARAMETER),
    ("HALF_CALL or SPLIT_CALLS with K > 1", _r_flags_k, BAD_PARAMETER),
    ("K > 1 in TickCalls on an object of two rates", _r_two_rates, UNSUPPORTED),
    ("a tick that would change a session's clean kind", _r_kind, BAD_PARAMETER),
    ("mixed kinds with K > 1, SetSplitCallTicks off", _r_mixed_switch_off, UNSUPPORTED),
    ("mixed kinds with K > 1 under a call trace", _r_mixed_call_trace, UNSUPPORTED),
    ("K > 1 under a session trace", _r_session_trace_k, UNSUPPORTED),
    ("the safe-variant window", _r_safe, UNSUPPORTED),
    ("init_session(S)", _r_init_range, BAD_PARAMETER),
    ("set_config_session(.., 7)", _r_config, BAD_PARAMETER),
    ("a snapshot of the other rate through plain ImportSession", _r_import_rate, BAD_PARAMETER),
]
RULE_NAMES = [r[0] for r in RULES]

# op kinds the coverage conditions count (op["cov"]), with the generator's base weights
KINDS = {
    "Tick": 5, "TickPerSession": 5, "TickFlags": 10, "TickAsync": 9, "TickCalls": 12, "TickPackets": 12,
    "BufferFarend": 2.5, "BufferFarendHost": 2.5, "BufferFarendAsync": 2.5, "Process": 2.5, "ProcessHost": 2.5, "late_near": 1.5,
    "InitSession": 1.5, "InitSessionRate": 1, "set_config_session": 1.5, "init_echo_path": 1.2, "get_echo_path": 1.5,
    "ImportSession": 2, "ImportSessionAnyRate": 1.5, "ImportSessions": 1, "ImportSessionsDevice": 1,
    "ForceSparseTicks": 1, "SplitCleanTwoLaunches": 1, "SetSplitCallTicks": 1.5, "safe_window": 1, "SetSessionTrace": 1.2, "SetCallTrace": 1.2,
    "refused": 22,
}
QUOTA = 5


class Generator:
    def __init__(self, case):
        c = CASES[case]
        self.case, self.c = case, c
        self.rs = np.random.RandomState(c["seed"])
        self.sh = Shadow(case)
        self.S = c["S"]
        self.prog = []
        self.far_pos = [[997 * (o * self.S + s) for s in range(self.S)] for o in range(2)]
        self.near_pos = [[991 * (o * self.S + s) for s in range(self.S)] for o in range(2)]
        self.count, self.rules, self.kcount, self.formcount = Counter(), Counter(), Counter(), Counter()
        self.migrations = self.migrations_pending = 0
        self.special = special_slots(case)
        self.unsynced_export = 0

    # -- small helpers
    def pick(self, seq):
        return seq[int(self.rs.randint(len(seq)))]

    def slot(self, o):
        if self.special and self.rs.rand() < 2 / 3:
            return self.pick(self.special)
        return int(self.rs.randint(self.S))

    def phase1(self):
        return len(self.prog) < 0.3 * self.c["steps"]

    def policy(self, o):
        """What a session that has had no Process call yet is given: in the first 30 % of a program A's sessions a clean input and B's
        none -- the objects stay of one kind, so that the entry points without flags (Tick, TickPerSession, Process) can be made --,
        then either, and migration mixes the objects."""
        return (ALWAYS if o == 0 else NEVER) if self.phase1() else NONE

    def emit(self, op, cov=None):
        op["step"] = len(self.prog)
        ob = self.sh.ob[op["obj"]]
        if op["kind"] in ("tick", "process"):
            op.setdefault("expect", 0)
            code = tick_code(ob, op)
            if "rule" in op:
                op["expect"] = dict((r[0], r[2]) for r in RULES)[op["rule"]]
                assert code == op["expect"], ("a refusal that the restated rules answer otherwise", op, code)
            else:
                assert code == 0, ("the generator made a tick the header refuses", op, code)
                live = callers(op, ob.S)
                bad = [s for s in live if not 0 <= (op["ms"] if isinstance(op["ms"], int) else op["ms"][s]) <= 500]
                op["expect"] = WARNING if bad else 0
        elif "rule" in op:
            op["expect"] = dict((r[0], r[2]) for r in RULES)[op["rule"]]
        if op["kind"] in ("tick", "process", "burst"):
            o = op["obj"]
            op["far_at"], op["near_at"] = list(self.far_pos[o]), list(self.near_pos[o])
            op["junk"] = int(self.rs.randint(-30000, 30000))
            if op.get("expect", 0) in (0, WARNING):
                for s in range(self.S):
                    if op["kind"] == "burst":
                        self.far_pos[o][s] += burst_calls(op, s) * op["n"]
                    else:
                        m = consumed(op, s)
                        self.far_pos[o][s] += m
                        self.near_pos[o][s] += m
        if "rule" in op:
            self.rules[op["rule"]] += 1
            cov = "refused"
        if cov:
            op["cov"] = cov
            self.count[cov] += 1
        if op["kind"] == "tick" and "rule" not in op:
            self.formcount[(op["entry"], op["form"])] += 1
            if op["K"] > 1:
                self.kcount[(op["entry"], op["K"])] += 1
        self.sh.apply(op)
        self.prog.append(op)
        return op

    # -- ticks
    def draw_tick(self, o, entry=None, form=None, n=None, K=None, flags=None, clean=None, clean_only=False, idle=(), nofar=()):
        """A tick the header accepts in the object's present state (not emitted).  flags=True: with a flags array; clean: with / without a
        clean plane; clean_only: a clean plane whose callers all take their row; idle / nofar: sessions that sit out / get no far frame."""
        rs, ob = self.rs, self.sh.ob[o]
        S = ob.S
        ok_clean = all(k in (NONE, ALWAYS) for k in ob.kind)
        ok_plain = all(k in (NONE, NEVER) for k in ob.kind)
        uniform = ok_clean or ok_plain
        if entry is None:
            entry = self.pick(list(FORMS))
        if entry in ("Tick", "TickPerSession") and (not uniform or flags or idle or nofar or clean_only or (clean is True and not ok_clean) or (clean is False and not ok_plain)):
            entry = "TickFlags"
        if form is None or form not in FORMS[entry]:          # (the form this entry point has taken least often)
            form = min(FORMS[entry], key=lambda f: (self.formcount[(entry, f)], rs.rand()))
        n = int(rs.choice([80, 160])) if n is None else n
        forced_k = K is not None
        if K is None:
            K = 1
            if entry in ("TickCalls", "TickPackets") and rs.rand() < 0.9:
                low = [k for k in range(2, 7) if self.kcount[(entry, k)] < 3]
                K = self.pick(low) if low else int(rs.randint(2, 7))
        if K > 1 and ob.trace == "session":
            K = 1
        if K > 1 and entry == "TickCalls" and ob.other_rates():
            if not forced_k and rs.rand() < 0.6:
                K = 1                                        # (TickCalls of one call pair is what an object of two rates takes)
            else:
                entry = "TickPackets"
        with_flags = entry in TAKES_FLAGS and (TAKES_FLAGS[entry] == "always" or bool(flags) or not uniform or bool(idle) or bool(nofar) or clean_only or rs.rand() < 0.85)
        pol = self.policy(o)
        if not with_flags:                                   # everybody calls, nobody is flagged: the object is of one kind
            if clean is None:
                clean = (pol != NEVER if pol else rs.rand() < 0.5) if ok_clean and ok_plain else ok_clean
            if (clean and not ok_clean) or (not clean and not ok_plain):
                with_flags = True
        if with_flags and entry not in TAKES_FLAGS:
            entry, form = "TickFlags", self.pick(["device", "host"])
        fl = None
        if with_flags:
            if clean is None:
                clean = rs.rand() < (0.95 if pol == ALWAYS else 0.5 if pol == NEVER else 0.7)
            split_k = K == 1 or (ob.split_call_ticks and ob.trace != "call")
            if clean and not split_k and not clean_only:
                if rs.rand() < 0.5 or any(ob.kind[s] == ALWAYS for s in nofar):
                    clean_only = True
                else:
                    clean = False
            p_idle = float(rs.choice([0.0, 0.1, 0.3, 0.9], p=[0.25, 0.45, 0.25, 0.05]))
            fl = []
            for s in range(S):
                k = ob.kind[s]
                sit = rs.rand() < p_idle or s in idle
                if s in nofar:
                    sit = False
                if (not clean and k == ALWAYS) or (clean and clean_only and k == NEVER):
                    sit = True
                if sit:
                    fl.append(IDLE | (int(rs.randint(32)) & ~IDLE))         # an idle session's other bits mean nothing
                    continue
                f = 0
                if clean and not clean_only and (k == NEVER or (k == NONE and (pol == NEVER or (pol == NONE and rs.rand() < 0.5)))):
                    f |= NO_CLEAN
                if not clean and rs.rand() < 0.1:
                    f |= NO_CLEAN                                           # (without a clean plane the flag is ignored)
                if rs.rand() < 0.12 or s in nofar:
                    f |= NO_FAREND
                if n == 160:
                    narrow = ob.rates[s] == 8000
                    if K == 1 and rs.rand() < 0.1:
                        f |= SPLIT_CALLS
                    elif (K == 1 or entry == "TickPackets") and rs.rand() < (0.6 if narrow else 0.12):
                        f |= HALF_CALL
                fl.append(f)
        if with_flags or entry == "TickPerSession" or (entry != "Tick" and rs.rand() < 0.5):
            ms = [int(v) for v in 40 + rs.randint(-15, 16, size=S)]
            if rs.rand() < 0.08:
                ms[int(rs.randint(S))] = int(rs.choice([-5, 700]))
        else:
            ms = int(40 + rs.randint(-15, 16)) if rs.rand() > 0.05 else int(rs.choice([-5, 700]))
        return dict(kind="tick", obj=o, entry=entry, form=form, n=n, K=K, clean=bool(clean), ms=ms, flags=fl, stride=n * K)

    def draw_process(self, o):
        ob = self.sh.ob[o]
        ok_clean = all(k in (NONE, ALWAYS) for k in ob.kind)
        ok_plain = all(k in (NONE, NEVER) for k in ob.kind)
        if not (ok_clean or ok_plain):
            return None
        pol = self.policy(o)
        clean = (pol != NEVER if pol else self.rs.rand() < 0.5) if ok_clean and ok_plain else ok_clean
        n = int(self.rs.choice([80, 160]))
        ms = [int(v) for v in 40 + self.rs.randint(-15, 16, size=ob.S)] if self.rs.rand() < 0.5 else int(40 + self.rs.randint(-15, 16))
        return dict(kind="process", obj=o, form="device", n=n, clean=bool(clean), ms=ms, stride=n)

    def draw_burst(self, o, form=None, only=None):
        rs = self.rs
        n = int(rs.choice([80, 160]))
        calls = 40 if rs.rand() < 0.1 else 6
        if only is not None:
            calls, host = 1, [1 if s in only else 0 for s in range(self.S)]
        else:
            host = None if rs.rand() < 0.15 else [int(v) for v in rs.randint(0, calls + 1, size=self.S)]
        return dict(kind="burst", obj=o, form=form or self.pick(["device", "host", "async"]), n=n, calls=calls, calls_host=host, stride=calls * n)

    def emit_async_chain(self, o, first):
        """Up to three Async ops back to back on buffers of their own, then Synchronize -- or, now and then, an ExportSession(s)
        without one: export waits for the ticks enqueued so far."""
        self.emit(first, first.pop("_cov"))
        for _ in range(int(self.rs.randint(0, 3))):
            if self.rs.rand() < 0.3:
                self.emit(self.draw_burst(o, form="async"), "BufferFarendAsync")
            else:
                entry = self.pick(["TickAsync", "TickCalls", "TickPackets"])
                op = self.draw_tick(o, entry=entry, form="async")
                self.emit(op, op["entry"])
        dst = self.sh.ob[1 - o]
        if not self.phase1() and not dst.safe and (self.unsynced_export == 0 or self.rs.rand() < 0.25):
            self.unsynced_export += 1
            self.emit_migration(o, sync_before=False)
        else:
            self.emit(dict(kind="sync", obj=o))

    def emit_tick(self, o, entry):
        op = self.draw_tick(o, entry=entry)
        if op["form"] == "async":
            op["_cov"] = op["entry"]
            self.emit_async_chain(o, op)
        else:
            self.emit(op, op["entry"])

    # -- migration
    def emit_migration(self, o, sync_before=True, bulk=None, anyrate=None):
        rs, ob, dst = self.rs, self.sh.ob[o], self.sh.ob[1 - o]
        pend = [s for s in range(ob.S) if ob.pending[s]]
        if bulk is None:
            s = self.pick(pend) if pend and rs.rand() < 0.45 else self.slot(o)
            need = ob.rates[s] != dst.fs
            how = "anyrate" if need or anyrate or (anyrate is None and rs.rand() < 0.3) else "plain"
            self.migrations += 1
            self.migrations_pending += int(ob.pending[s])
            return self.emit(dict(kind="migrate", obj=o, s=s, dst=1 - o, j=self.slot(1 - o), how=how, sync_before=sync_before),
                             "ImportSessionAnyRate" if how == "anyrate" else "ImportSession")
        count = max(1, min(ob.S, int(ob.S ** rs.rand())))
        ss = [int(v) for v in rs.permutation(ob.S)[:count]]
        if pend and rs.rand() < 0.45 and pend[0] not in ss:
            ss[0] = pend[0]
        js = [int(v) for v in rs.permutation(dst.S)[:count]]
        any_rate = any(ob.rates[s] != dst.fs for s in ss) or rs.rand() < 0.3
        self.migrations += 1
        self.migrations_pending += int(any(ob.pending[s] for s in ss))
        return self.emit(dict(kind="migrate_bulk", obj=o, ss=ss, dst=1 - o, js=js, form=bulk, any_rate=bool(any_rate),
                              sync_before=sync_before), "ImportSessions" if bulk == "host" else "ImportSessionsDevice")

    # -- one step
    def weights(self):
        w = {}
        for k, base in KINDS.items():
            w[k] = base * (8.0 if self.count[k] < QUOTA else 1.0)
            if self.phase1() and k in ("Tick", "TickPerSession", "Process", "ProcessHost") and self.count[k] < QUOTA:
                w[k] *= 4                                    # (they need an object of one kind)
        for entry in ("TickCalls", "TickPackets"):
            if any(self.kcount[(entry, k)] < 3 for k in range(2, 7)):
                w[entry] *= 2
        if self.c["rates"] == "uniform" and any(ob.other_rates() for ob in self.sh.ob):
            w["InitSession"] *= 6                            # (a slot at the other rate is soon recycled: TickCalls needs an object of one rate)
        if self.phase1():                                    # (nothing crosses between the objects while they are kept of one kind)
            for k in ("ImportSession", "ImportSessionAnyRate", "ImportSessions", "ImportSessionsDevice"):
                w[k] = 0
        return w

    def step(self):
        rs = self.rs
        o = int(rs.randint(2))
        ob = self.sh.ob[o]
        w = self.weights()
        names = list(w)
        p = np.array([w[k] for k in names], dtype=np.float64)
        kind = names[int(rs.choice(len(names), p=p / p.sum()))]
        under = [k for k in names if w[k] > 0 and self.count[k] < QUOTA]
        first = [k for k in under if k in ("Tick", "TickPerSession", "Process", "ProcessHost")]
        if first and self.phase1():                          # (while the objects are of one kind: the entry points that need that)
            under = first
        if under and rs.rand() < 0.4:                        # (coverage first: a kind that has not come up five times yet)
            kind = self.pick(under)
        if kind in FORMS:
            self.emit_tick(o, kind)
        elif kind in ("BufferFarend", "BufferFarendHost", "BufferFarendAsync"):
            form = {"BufferFarend": "device", "BufferFarendHost": "host", "BufferFarendAsync": "async"}[kind]
            op = self.draw_burst(o, form=form)
            if form == "async":
                op["_cov"] = kind
                self.emit_async_chain(o, op)
            else:
                self.emit(op, kind)
        elif kind in ("Process", "ProcessHost"):
            op = self.draw_process(o)
            if op is None:                                   # sessions of both kinds: the same calls through TickFlags, everybody NO_FAREND
                op = self.draw_tick(o, entry="TickFlags", K=1, nofar=range(ob.S))
                self.emit(op, "TickFlags")
            else:
                op["form"] = "host" if kind == "ProcessHost" else "device"
                self.emit(op, kind)
        elif kind == "late_near":                            # the far end arrived, the near end is late: burst, IDLE tick, NO_FAREND tick
            late = sorted(set(int(v) for v in rs.randint(0, ob.S, size=max(1, ob.S // 8))))
            self.emit(self.draw_burst(o, form=self.pick(["device", "host"]), only=late), "late_near")
            for part in ("idle", "nofar"):
                entry = self.pick(["TickFlags", "TickAsync", "TickCalls", "TickPackets"])
                want_clean = True if any(ob.kind[s] == ALWAYS for s in late) else None
                op = self.draw_tick(o, entry=entry, K=1, flags=True, clean=want_clean, **{part: late})
                if op["form"] == "async":
                    op["form"] = "device" if entry != "TickAsync" else "async"
                self.emit(op, op["entry"])
                if op["form"] == "async":
                    self.emit(dict(kind="sync", obj=o))
        elif kind == "InitSession":
            other = [s for s in range(ob.S) if ob.rates[s] != ob.fs]
            s = self.pick(other) if other and self.c["rates"] == "uniform" and rs.rand() < 0.8 else self.slot(o)
            self.emit(dict(kind="init_session", obj=o, s=s), kind)
        elif kind == "InitSessionRate":
            self.emit(dict(kind="init_session_rate", obj=o, s=self.slot(o), rate=24000 - ob.fs), kind)
        elif kind == "set_config_session":
            self.emit(dict(kind="set_config", obj=o, s=self.slot(o), cng=int(rs.randint(0, 2)), echo=int(rs.randint(0, 5))), kind)
        elif kind == "init_echo_path":
            self.emit(dict(kind="init_echo_path", obj=o, s=self.slot(o), path=[int(v) for v in rs.randint(0, 6000, size=65)]), kind)
        elif kind == "get_echo_path":
            self.emit(dict(kind="get_echo_path", obj=o, s=self.slot(o)), kind)
        elif kind in ("ImportSession", "ImportSessionAnyRate"):
            self.emit_migration(o, anyrate=kind == "ImportSessionAnyRate")
        elif kind in ("ImportSessions", "ImportSessionsDevice"):
            self.emit_migration(o, bulk="host" if kind == "ImportSessions" else "device")
        elif kind == "ForceSparseTicks":
            self.emit(dict(kind="force_sparse", obj=o, on=int(not ob.force_sparse)), kind)
        elif kind == "SplitCleanTwoLaunches":
            self.emit(dict(kind="two_launches", obj=o, on=int(self.pick([v for v in (-1, 0, 1) if v != ob.two_launches]))), kind)
        elif kind == "SetSplitCallTicks":
            self.emit(dict(kind="split_call_ticks", obj=o, on=int(not ob.split_call_ticks)), kind)
        elif kind == "safe_window":
            self.emit(dict(kind="variant", obj=o, safe=1), kind)
            for _ in range(int(rs.randint(2, 5))):
                if rs.rand() < 0.3:
                    op = self.draw_burst(o, form=self.pick(["device", "host"]))
                    self.emit(op, "BufferFarend" if op["form"] == "device" else "BufferFarendHost")
                else:
                    op = self.draw_process(o) if rs.rand() < 0.15 else None
                    op = op or self.draw_tick(o)
                    op["rule"] = "the safe-variant window"
                    self.emit(op)
            self.emit(dict(kind="variant", obj=o, safe=0))
        elif kind in ("SetSessionTrace", "SetCallTrace"):
            if ob.trace:
                self.emit(dict(kind="trace", obj=o, which=None), None)
            self.emit(dict(kind="trace", obj=o, which="session" if kind == "SetSessionTrace" else "call", ring=int(self.pick([1, 3])),
                           layout=self.pick(["session-major", "tick-major"])), kind)
            for i in range(int(rs.randint(3, 8))):           # its ticks; every few of them the records are compared
                entry = self.pick(list(TAKES_FLAGS) + ["TickPackets"])
                op = self.draw_tick(o, entry=entry)
                if op["form"] == "async":
                    op["form"] = "device" if op["entry"] != "TickAsync" else "async"
                op["records"] = int(i % 2 == 0)
                self.emit(op, op["entry"])
                if op["form"] == "async":
                    self.emit(dict(kind="sync", obj=o))
                if rs.rand() < 0.35:
                    rule = self.next_rule(o, ["K > 1 under a session trace", "mixed kinds with K > 1 under a call trace"])
                    if rule:
                        self.emit(rule)
            if rs.rand() < 0.7:
                self.emit(dict(kind="trace", obj=o, which=None), None)
        else:
            op = self.next_rule(o)
            if op:
                self.emit(op)

    def next_rule(self, o, among=None):
        """The refusal made least often so far that the object's state admits."""
        order = sorted((r for r in RULES if among is None or r[0] in among), key=lambda r: (self.rules[r[0]], self.rs.rand()))
        for name, build, _ in order:
            op = build(self, o)
            if op is not None:
                op["rule"] = name
                if op["kind"] == "tick" and op["form"] == "async":
                    op["form"] = "device" if op["entry"] != "TickAsync" else "async"
                return op
        return None


def generate(case, steps=None):
    """The program of a case (its first `steps` ops)."""
    g = Generator(case)
    total = CASES[case]["steps"]
    while len(g.prog) < total:
        g.step()
    for o in range(2):
        g.emit(dict(kind="sync", obj=o))
    return g.prog if steps is None else g.prog[:steps]


def program_sha256(program):
    return hashlib.sha256(json.dumps(program, sort_keys=True, separators=(",", ":")).encode()).hexdigest()


def run_reference(case, program=None):
    """The whole program on the model alone.  Returns the model (digest: the SHA-256 of every expected code, output and echo path)."""
    program = generate(case) if program is None else program
    m = Model(case)
    for op in program:
        m.apply(op)
    for o in range(2):
        m.digest.update(m.echo_paths(o).tobytes())
    return m


# ---- listing ------------------------------------------------------------------------------------------------------------------------
def flag_names(f):
    return "|".join(name for bit, name in FLAG_NAMES.items() if f & bit) or "0"


def describe(op, session=None):
    """One line per op; with a session, its flag byte and msInSndCardBuf in that op."""
    k, o = op["kind"], "AB"[op["obj"]]
    head = f"{op['step']:5d} {o} "
    tail = f"  -> refused: {op['rule']} ({op['expect']})" if "rule" in op else (f"  -> {op['expect']}" if op.get("expect") else "")
    if k == "tick":
        fl = op["flags"]
        live = len(callers(op, len(op["far_at"])))
        text = (f"{op['entry']}[{op['form']}] n={op['n']} K={op['K']} stride={op['stride']} clean={int(op['clean'])} "
                f"ms={'per session' if isinstance(op['ms'], list) else op['ms']} flags={'none' if fl is None else 'S'} calling={live}")
        if fl is not None and session is None:
            c = Counter()
            for f in fl:
                for bit, name in FLAG_NAMES.items():
                    c[name] += bool(f & bit) and (bit == IDLE or not f & IDLE)
            text += " " + " ".join(f"{name}:{v}" for name, v in c.items() if v)
        if session is not None:
            text += f" | session {session}: flags={flag_names(flag_of(op, session))} ms={op['ms'] if isinstance(op['ms'], int) else op['ms'][session]}"
        if op.get("records"):
            text += " [records]"
    elif k == "process":
        text = f"Process[{op['form']}] n={op['n']} clean={int(op['clean'])} ms={'per session' if isinstance(op['ms'], list) else op['ms']}"
    elif k == "burst":
        ch = op["calls_host"]
        text = f"BufferFarend[{op['form']}] n={op['n']} calls={op['calls']} calls_host={'none' if ch is None else (ch if len(ch) <= 8 else 'S')}"
        if session is not None and ch is not None:
            text += f" | session {session}: {ch[session]} calls"
    elif k == "migrate":
        text = f"ExportSession({op['s']}) -> {'AB'[op['dst']]}.{'ImportSessionAnyRate' if op['how'] == 'anyrate' else 'ImportSession'}({op['j']})" + \
               ("" if op["sync_before"] else " [no Synchronize before]")
    elif k == "migrate_bulk":
        pairs = list(zip(op["ss"], op["js"]))
        text = f"ExportSessions[{op['form']}] x{len(pairs)} -> {'AB'[op['dst']]}.ImportSessions any_rate={int(op['any_rate'])} " + \
               (str(pairs) if len(pairs) <= 6 else f"{pairs[:6]} ...") + ("" if op["sync_before"] else " [no Synchronize before]")
    else:
        text = k + " " + " ".join(f"{a}={v if not isinstance(v, list) else '[..]'}" for a, v in op.items() if a not in ("kind", "obj", "step", "cov", "expect", "rule"))
    return head + text + tail


def touches(op, o, s):
    """Does the op reach session s of object o?"""
    if op["kind"] in ("migrate", "migrate_bulk"):
        src = [op["s"]] if op["kind"] == "migrate" else op["ss"]
        dst = [op["j"]] if op["kind"] == "migrate" else op["js"]
        return (op["obj"] == o and s in src) or (op["dst"] == o and s in dst)
    if op["obj"] != o:
        return False
    return "s" not in op or op["s"] == s


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(description="list the program of a case of the session surface fuzz")
    ap.add_argument("--case", required=True, choices=sorted(CASES))
    ap.add_argument("--until", type=int, default=None, help="the ops before this step")
    ap.add_argument("--session", default=None, help="A3 / B64: only the ops that reach this session, with its flags")
    ap.add_argument("--print", action="store_true", dest="listing")
    a = ap.parse_args(argv)
    prog = generate(a.case, a.until)
    print(f"{a.case}: {len(prog)} ops, sha256 {program_sha256(prog)[:16]}")
    if a.listing:
        o, s = (("AB".index(a.session[0]), int(a.session[1:])) if a.session else (None, None))
        for op in prog:
            if o is None or touches(op, o, s):
                print(describe(op, s if o is not None and op["obj"] == o else None))


if __name__ == "__main__":
    main()
