"""The session API fuzz over the whole tick surface on the GPU (tests/surface_fuzz.py): every case's program on two AecmSessions
objects, compared after EVERY op with one reference instance per session slot (the unmodified reference where oracle/_ref exists, the
project's single-session ABI otherwise) -- every output sample of every row (an idle session's row and the span a half call leaves
unused must still hold the fill in the device forms and be zeros in the Host forms), every code per session and as the return value,
the clean modes, the trace counts, the trace records every few traced ticks, echo paths on get_echo_path ops and of all sessions at
the end.  No exclusions.  A refused op must return the code of its rule, write nothing and leave the clean modes alone; the next
accepted op's comparison shows that nothing else changed.

The reference side of a case takes 0.4 / 0.3 / 1.8 / 3.9 s (small-16k / small-8k / wave-mixed / group-mixed) on the build machine;
every case prints its wall time."""
import os
import subprocess
import sys
import textwrap
import time
from pathlib import Path

import numpy as np
import pytest

import session_trace_helpers as sth
import surface_fuzz as sf
import webrtc_aecm_amd as aecm

pytestmark = pytest.mark.gpu
TESTS = Path(__file__).resolve().parent
FILL = np.int16(sf.FILL)
TICK_NAMES = {("Tick", "device"): "Tick", ("Tick", "host"): "TickHost", ("TickPerSession", "device"): "TickPerSession",
              ("TickPerSession", "host"): "TickPerSessionHost", ("TickFlags", "device"): "TickFlags", ("TickFlags", "host"): "TickFlagsHost",
              ("TickAsync", "async"): "TickAsync", ("TickCalls", "device"): "TickCalls", ("TickCalls", "host"): "TickCallsHost",
              ("TickCalls", "async"): "TickCallsAsync", ("TickPackets", "device"): "TickPackets", ("TickPackets", "host"): "TickPacketsHost",
              ("TickPackets", "async"): "TickPacketsAsync"}
BURST_NAMES = {"device": "BufferFarend", "host": "BufferFarendHost", "async": "BufferFarendAsync"}


class Run:
    def __init__(self, case):
        import torch
        self.torch = torch
        self.case, self.c = case, sf.CASES[case]
        self.prog = sf.generate(case)
        self.model = sf.Model(case)
        rates = sf.case_rates(case)
        self.objs = [aecm.AecmSessions(self.c["S"], self.c["fs"][o], 1, 3, rates=None if self.c["rates"] == "uniform" else rates[o]) for o in range(2)]
        self.pending = [[], []]                    # Async ticks enqueued and not yet compared: (op, expected out, out tensor, its inputs)
        self.trace_buf = [None, None]
        self.keep = []                             # buffers enqueued work may still touch
        self.records_checked = 0

    def close(self):
        for sb in self.objs:
            sb.close()

    # -- messages
    def where(self, op, s=None):
        text = f"case {self.case} (seed {self.c['seed']}), step {op['step']}: {sf.describe(op, s)}"
        if s is not None:
            last = [sf.describe(p, s if p['obj'] == op['obj'] else None) for p in self.prog[:op["step"]] if sf.touches(p, op["obj"], s)][-5:]
            text += "\n  the session's last ops:\n    " + "\n    ".join(last)
        return text

    # -- buffers
    def planes(self, op, rows, W):
        """(far, near, clean, out) as pointers + what keeps them alive; out pre-filled."""
        S = self.c["S"]
        if op["form"] == "host":
            out = np.full((S, W), FILL, dtype=np.int16)
            hold = [rows["far"], rows["near"], rows["clean"], out]
            ptr = lambda a: None if a is None else a.ctypes.data
        else:
            t = self.torch
            hold = [None if a is None else t.from_numpy(a).cuda() for a in (rows["far"], rows["near"], rows["clean"])]
            out = t.full((S, W), int(FILL), dtype=t.int16, device="cuda")
            hold.append(out)
            t.cuda.synchronize()
            ptr = lambda a: None if a is None else a.data_ptr()
        return [ptr(a) for a in hold], hold, out

    @staticmethod
    def host_out(out):
        return out if isinstance(out, np.ndarray) else out.cpu().numpy()

    def compare_out(self, op, exp, out):
        got = self.host_out(out)
        unwritten = np.int16(0) if op["form"] == "host" else FILL
        want = np.where(exp["written"], exp["out"], unwritten)
        if not np.array_equal(got, want):
            s, at = (int(v) for v in np.argwhere(got != want)[0])
            what = "a sample that must not be written was" if not exp["written"][s, at] else "output differs"
            pytest.fail(f"{what}: session {s}, sample {at}: got {int(got[s, at])}, expected {int(want[s, at])}; "
                        f"differing sessions {sorted(set(np.argwhere(got != want)[:, 0].tolist()))[:12]}\n" + self.where(op, s))

    def flush(self, o):
        for op, exp, out, _ in self.pending[o]:
            self.compare_out(op, exp, out)
        self.pending[o] = []

    # -- the ops
    def tick(self, op, exp):
        o, sb, S = op["obj"], self.objs[op["obj"]], self.c["S"]
        is_tick = op["kind"] == "tick"
        W = sf.row_width(op)
        (far, near, clean, outp), hold, out = self.planes(op, exp["rows"], W)
        per = isinstance(op["ms"], list)
        ms = np.array(op["ms"], dtype=np.int16) if per else None
        ms_one = 0 if per else op["ms"]
        fl = None if not is_tick or op["flags"] is None else np.array(op["flags"], dtype=np.uint8)
        codes = np.full(S, -77, dtype=np.int32)
        p = lambda a: None if a is None else a.ctypes.data
        head = [sb.h, far, near, clean, outp, op["stride"], op["n"]]
        refused = exp["rc"] not in (0, sf.WARNING)
        trace = self.model.ob[o].trace                     # (the model has applied the op: an accepted tick leaves the attachment alone)
        with_codes = True
        if not is_tick:
            fn = getattr(sb.lib, "WebRtcAecmSessions_Process" + ("Host" if op["form"] == "host" else ""))
            args = [sb.h, near, clean, outp, op["stride"], op["n"], ms_one, p(ms), p(codes)]
        else:
            fn = getattr(sb.lib, "WebRtcAecmSessions_" + TICK_NAMES[(op["entry"], op["form"])])
            if op["entry"] == "Tick":
                args, with_codes = head + [ms_one], False
            elif op["entry"] == "TickPerSession":
                args = head + [p(ms), p(codes)]
            elif op["entry"] == "TickFlags":
                args = head + [p(ms), p(fl), p(codes)]
            elif op["entry"] == "TickAsync":
                args = head + [ms_one, p(ms), p(fl), p(codes), None, None]
            else:
                args = head + [op["K"], ms_one, p(ms), p(fl), p(codes)] + ([None, None] if op["form"] == "async" else [])
        check_records = bool(op.get("records")) and trace and not refused and op["form"] != "async" and not self.pending[o]
        if check_records:
            before = self.records_before(op)
        rc = fn(*args)
        assert rc == exp["rc"], f"returned {rc}, expected {exp['rc']}\n" + self.where(op)
        if refused:
            if op["form"] == "async":
                assert sb.synchronize() == 0
            got = self.host_out(out)
            assert (got == FILL).all(), "a refused call wrote its out plane\n" + self.where(op, int(np.argwhere(got != FILL)[0][0]))
            return
        if with_codes and not np.array_equal(codes, exp["codes"]):
            s = int(np.flatnonzero(codes != exp["codes"])[0])
            pytest.fail(f"code of session {s}: {int(codes[s])}, expected {int(exp['codes'][s])}\n" + self.where(op, s))
        if op["form"] == "async":
            self.pending[o].append((op, exp, out, hold))
        else:
            self.flush(o)                                  # (a synchronous form waits for everything enqueued before it)
            self.compare_out(op, exp, out)
        if check_records and before is not None:
            self.records_after(op, before)

    def burst(self, op, exp):
        o, sb, S = op["obj"], self.objs[op["obj"]], self.c["S"]
        far = exp["rows"]["far"]
        if op["form"] == "host":
            hold, ptr = far, far.ctypes.data
        else:
            hold = self.torch.from_numpy(far).cuda()
            self.torch.cuda.synchronize()
            ptr = hold.data_ptr()
        ch = None if op["calls_host"] is None else np.array(op["calls_host"], dtype=np.uint8)
        args = [sb.h, ptr, op["stride"], op["n"], op["calls"], None if ch is None else ch.ctypes.data] + ([None, None] if op["form"] == "async" else [])
        rc = getattr(sb.lib, "WebRtcAecmSessions_" + BURST_NAMES[op["form"]])(*args)
        assert rc == exp["rc"], f"returned {rc}, expected {exp['rc']}\n" + self.where(op)
        self.keep.append(hold)
        if op["form"] != "async":
            self.flush(o)

    def sub_sessions(self, op):
        """Up to eight calling sessions whose records are compared: the lanes that matter first."""
        live = sf.callers(op, self.c["S"])
        first = [s for s in sf.special_slots(self.case) if s in live]
        return (first + [s for s in live if s not in first])[:8]

    def records_before(self, op):
        sub = self.sub_sessions(op)
        if not sub:
            return None
        sb = self.objs[op["obj"]]
        rc, blob = sb.export_sessions(sub)
        assert rc == 0
        count = sb.session_trace_ticks() if self.model.ob[op["obj"]].trace == "session" else sb.call_trace_calls()
        return sub, blob, count

    def records_after(self, op, before):
        """The records of the tick's last call slot against the header's contract: every wrapper field is what ExportSession shows
        directly after the tick, `core` the block trace of that snapshot's core state (session_trace_helpers.expected_records); `blocks`
        is the advance over ONE call pair, so it is compared in ticks of one only."""
        sub, blob0, count = before
        o, S, K = op["obj"], self.c["S"], op.get("K", 1)
        ob, sb = self.model.ob[o], self.objs[o]
        rc, blob1 = sb.export_sessions(sub)
        assert rc == 0
        want = sth.expected_records(blob0, [blob1], np.ones((1, len(sub)), dtype=bool), [ob.rates[s] for s in sub])[:, 0]
        slot = count + (K if ob.trace == "call" else 1) - 1
        R = ob.trace_ring
        got_all = self.trace_buf[o].cpu().numpy().view(np.uint8).view(aecm.ffi.SESSION_TRACE_DTYPE)
        for i, s in enumerate(sub):
            got = got_all[s * R + slot % R] if ob.trace_layout == "session-major" else got_all[(slot % R) * S + s]
            for name in sth.flat_fields():
                if name == "blocks" and K > 1:
                    continue
                w = slot if name == "tick" else sth.field(want[i], name)
                g = sth.field(got, name)
                assert g == w, f"{ob.trace} trace, slot {slot}, session {s}, field {name}: traced {g}, expected {w}\n" + self.where(op, s)
        self.records_checked += 1

    def migrate(self, op, exp):
        src, dst = self.objs[op["obj"]], self.objs[op["dst"]]
        if op["sync_before"]:
            assert src.synchronize() == 0
        if op["kind"] == "migrate":
            rc, snap = src.export_session(op["s"])
            assert rc == 0, self.where(op)
            rc = dst.import_session_any_rate(op["j"], snap) if op["how"] == "anyrate" else dst.import_session(op["j"], snap)
        elif op["form"] == "host":
            rc, blob = src.export_sessions(op["ss"])
            assert rc == 0, self.where(op)
            rc = dst.import_sessions(op["js"], blob, any_rate=op["any_rate"])
        else:
            size = src.lib.WebRtcAecmSessions_session_size_bytes()
            buf = self.torch.zeros(len(op["ss"]) * size, dtype=self.torch.uint8, device="cuda")
            self.torch.cuda.synchronize()
            assert src.export_sessions_device(buf.data_ptr(), op["ss"]) == 0, self.where(op)
            rc = dst.import_sessions_device(buf.data_ptr(), op["js"], len(op["js"]), any_rate=op["any_rate"])
            self.keep.append(buf)
        assert rc == exp["rc"], f"import returned {rc}, expected {exp['rc']}\n" + self.where(op)
        self.flush(op["obj"])                              # (export waits for the ticks enqueued so far: their rows are complete now)

    def trace(self, op):
        o, sb, S = op["obj"], self.objs[op["obj"]], self.c["S"]
        before = self.model.ob[o]                          # (already after the op)
        if op["which"] is None:
            assert sb.clear_session_trace() == 0 and sb.clear_call_trace() == 0
            return
        R = op["ring"]
        buf = self.torch.zeros(S * R * 16, dtype=self.torch.int32, device="cuda")
        self.torch.cuda.synchronize()
        self.keep.append(buf)
        self.trace_buf[o] = buf
        strides = (R, 1, R) if op["layout"] == "session-major" else (1, S, R)
        attach = sb.set_session_trace if op["which"] == "session" else sb.set_call_trace
        assert attach(buf.data_ptr(), *strides) == 0, self.where(op)
        assert before.trace == op["which"]

    def step(self, op):
        exp = self.model.apply(op)
        o, k = op["obj"], op["kind"]
        sb = self.objs[o]
        if k in ("tick", "process"):
            self.tick(op, exp)
        elif k == "burst":
            self.burst(op, exp)
        elif k == "sync":
            assert sb.synchronize() == 0
            self.flush(o)
        elif k == "init_session":
            assert sb.init_session(op["s"]) == exp["rc"], self.where(op)
        elif k == "init_session_rate":
            assert sb.init_session_rate(op["s"], op["rate"]) == exp["rc"], self.where(op)
        elif k == "set_config":
            assert sb.set_config_session(op["s"], op["cng"], op["echo"]) == exp["rc"], self.where(op)
        elif k == "init_echo_path":
            assert sb.init_echo_path(op["s"], np.array(op["path"], dtype=np.int16)) == 0, self.where(op)
        elif k == "get_echo_path":
            rc, path = sb.get_echo_path(op["s"])
            assert rc == 0 and np.array_equal(path, exp["path"]), "echo path differs\n" + self.where(op, op["s"])
        elif k in ("migrate", "migrate_bulk"):
            self.migrate(op, exp)
        elif k == "force_sparse":
            assert sb.force_sparse_ticks(bool(op["on"])) == 0
        elif k == "two_launches":
            assert sb.split_clean_two_launches(None if op["on"] < 0 else bool(op["on"])) == 0
        elif k == "split_call_ticks":
            assert sb.set_split_call_ticks(bool(op["on"])) == 0
        elif k == "variant":
            assert sb.lib.WebRtcAecmSessions_SetKernelVariant(sb.h, aecm.ffi.KERNEL_SAFE if op["safe"] else aecm.ffi.KERNEL_FAST) == 0
        elif k == "trace":
            self.trace(op)
        else:
            raise AssertionError(k)
        # what the object says about itself, after every op (a refused one included): the clean modes and the trace counts
        for x in ({o, op["dst"]} if "dst" in op else {o}):
            ob, sx = self.model.ob[x], self.objs[x]
            for s in range(ob.S):
                rc, mode = sx.get_session_clean_mode(s)
                assert rc == 0 and mode == ob.mode[s], f"clean mode of session {s} of {'AB'[x]}: {mode}, expected {ob.mode[s]}\n" + self.where(op, s if x == o else None)
            want = (ob.trace_count if ob.trace == "session" else 0, ob.trace_count if ob.trace == "call" else 0)
            assert (sx.session_trace_ticks(), sx.call_trace_calls()) == want, f"trace counts, expected {want}\n" + self.where(op)

    def run(self):
        for op in self.prog:
            self.step(op)
        for o, sb in enumerate(self.objs):
            assert not self.pending[o]
            paths = self.model.echo_paths(o)
            for s in range(self.c["S"]):
                rc, path = sb.get_echo_path(s)
                assert rc == 0 and np.array_equal(path, paths[s]), f"final echo path of session {s} of {'AB'[o]}\n" + self.where(self.prog[-1], None)
                assert sb.get_session_rate(s) == (0, self.model.ob[o].rates[s])


def run_case(case):
    t0 = time.perf_counter()
    r = Run(case)
    try:
        r.run()
    finally:
        r.close()
    seconds = time.perf_counter() - t0
    print(f"surface fuzz {case}: {len(r.prog)} ops, {r.model.compared} session-calls compared, {r.records_checked} record checks, {seconds:.2f} s")
    assert r.records_checked >= 3
    return seconds


@pytest.mark.parametrize("case", list(sf.CASES))
def test_surface_fuzz(case):
    """The case's whole program; see the module's text.  A failure names the seed, the step, the op with its form, n, K and the flags of
    the first differing session, and that session's last five ops; `python -m surface_fuzz --case .. --until STEP --print` lists the
    program up to there without a device."""
    run_case(case)


def test_checked_build_counts_nothing(tmp_path):
    """small-16k on the audit build (-DAECM_CHECKED), in a child process: the results are the reference's and the counters stay 0 0."""
    from webrtc_aecm_amd import build
    assert build.LIB_CHECKED.exists()
    script = tmp_path / "audit_surface_fuzz.py"
    script.write_text(textwrap.dedent("""
        import webrtc_aecm_amd as aecm
        import test_gpu_session_surface_fuzz as T
        assert aecm.check_counters(0, reset=True) is not None
        T.run_case("small-16k")
        c = aecm.check_counters(0)
        print("AUDIT", int(c[0]), int(c[1]))
    """))
    env = dict(os.environ, AECM_LIB_PATH=str(build.LIB_CHECKED), PYTHONPATH=os.pathsep.join([str(TESTS.parent), str(TESTS), os.environ.get("PYTHONPATH", "")]))
    r = subprocess.run([sys.executable, str(script)], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("AUDIT")]
    assert line and line[-1].split()[1:] == ["0", "0"], r.stdout[-500:]
