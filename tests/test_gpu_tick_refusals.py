"""A refused tick changes nothing, on the GPU: two twin objects take the same accepted ticks -- one of every kernel family, a tick nobody
makes and split ticks among them --, and only one of the twins also takes, before every accepted tick, every refused tick of the
coinciding-defects table (tests/tickplan_sim.py: two adjacent checks tripped at once, the code of the earlier one) through the
synchronous, the asynchronous and the host-pointer entry point.  After every accepted tick the twins' outputs and the snapshots of all
their sessions are byte for byte equal, and their clean modes those of the host's planner ticked alongside (tests/sim/sim_tickplan.cpp),
which also names the family of every accepted tick.  Every refusal is made on the host before any launch: nothing here can fault."""
import numpy as np
import pytest

import tickplan_sim as T
import webrtc_aecm_amd as aecm
from tickplan_sim import HALF_CALL, IDLE, NO_CLEAN, NO_FAREND

pytestmark = pytest.mark.gpu

ROW = 2 * 160                                        # samples per row of the buffers: the longest accepted tick
ALWAYS_EVERY = 5                                     # sessions 2, 7, 12, ...: initialised anew before the split ticks, then "always"


def accepted_ticks(S):
    """(flags pattern or None, n, calls, clean): the K-call ticks go through TickPackets, which in an object of one rate without
    half calls IS the K-call tick."""
    split = [IDLE | NO_CLEAN if s % ALWAYS_EVERY == 4 else 0 if s % ALWAYS_EVERY == 2 else NO_CLEAN for s in range(S)]
    return [
        (None, 160, 1, False),                                           # dense
        (T.pattern(S, 0, IDLE, 0), 80, 1, False),                        # sparse
        (T.pattern(S, IDLE), 160, 1, False),                             # nobody calls
        (None, 160, 1, False),                                           # sparse plan (the deferred lag), dense tick
        (T.pattern(S, HALF_CALL, 0, 0, IDLE), 160, 1, False),            # mixed
        (T.pattern(S, 0, NO_FAREND, IDLE), 80, 2, False),                # calls
        (T.pattern(S, HALF_CALL, 0, IDLE), 160, 2, False),               # packets
        "init",                                                          # sessions 2, 7, ...: WebRtcAecm_Init
        (split, 160, 1, True),                                           # split
        (split, 160, 1, True),                                           # split, after the refusals that need one behind them
    ]


class Twin:
    def __init__(self, S, rates):
        import torch
        self.S, self.torch = S, torch
        self.sb = aecm.AecmSessions(S, 16000, 1, 3, rates=rates)
        self.dev = {k: torch.zeros((S, ROW), dtype=torch.int16, device="cuda") for k in ("far", "near", "clean", "out")}
        self.host = {k: np.zeros((S, ROW), dtype=np.int16) for k in ("far", "near", "clean", "out")}
        self.ms = np.full(S, 40, dtype=np.int16)
        self.codes = np.zeros(S, dtype=np.int32)

    def call(self, form, flags=None, n=160, calls=1, stride=None, clean=False, far=True, near_out=True, packets=False, **_):
        """One tick through TickCalls / TickPackets (sync), ...Async or ...Host with the buffers of that form.  Returns the code."""
        buf = self.host if form == "host" else self.dev
        ptr = (lambda a: a.ctypes.data) if form == "host" else (lambda a: a.data_ptr())
        fl = None if flags is None else np.ascontiguousarray(flags, dtype=np.uint8)
        args = [self.sb.h, ptr(buf["far"]) if far else None, ptr(buf["near"]) if near_out else None, ptr(buf["clean"]) if clean else None,
                ptr(buf["out"]) if near_out else None, n * calls if stride is None else stride, n, calls, 40, None if fl is None else self.ms.ctypes.data,
                None if fl is None else fl.ctypes.data, self.codes.ctypes.data]
        name = "WebRtcAecmSessions_Tick" + ("Packets" if packets else "Calls") + {"sync": "", "async": "Async", "host": "Host"}[form]
        rc = getattr(self.sb.lib, name)(*args, *((None, None) if form == "async" else ()))
        if form == "async" and rc == 0:
            assert self.sb.synchronize() == 0
        return rc

    def accepted(self, rows, flags, n, calls, clean):
        """An accepted tick on device rows; returns (out, the snapshots of all sessions)."""
        for k in ("far", "near", "clean"):
            self.dev[k].copy_(self.torch.from_numpy(rows[k]))
        self.dev["out"].fill_(0x7b7b)
        self.torch.cuda.synchronize()
        assert self.call("sync", flags=flags, n=n, calls=calls, clean=clean, packets=True, stride=ROW) == 0
        rc, snaps = self.sb.export_sessions()
        assert rc == 0
        return self.dev["out"].cpu().numpy(), snaps

    def modes(self):
        got = [self.sb.get_session_clean_mode(s) for s in range(self.S)]
        assert all(rc == 0 for rc, _ in got)
        return [m for _, m in got]


@pytest.mark.parametrize("two_rates", [False, True], ids=["one_rate", "two_rates"])
@pytest.mark.parametrize("S", [5, 257])
def test_refused_ticks_change_nothing(S, two_rates):
    """S = 5: no multiple of the 4 sessions of a tick workgroup; 257: two planning workgroups, so the bases arrays have two entries.
    two_rates: session 1, 3, ... at 8 kHz in a 16 kHz object (its K-call ticks are packet ticks; the table's rows for such an object)."""
    rates = T.pattern(S, 16000, 8000) if two_rates else None
    a, b = Twin(S, rates), Twin(S, rates)
    plan = T.Object(S, rates=rates)
    rows_of = [c for c in T.COINCIDING if c["gpu"] and ("rates" in c) == two_rates]
    assert rows_of
    rng = np.random.default_rng(S)
    families, refusals, split_used = [], 0, False
    for tick in accepted_ticks(S):
        if tick == "init":
            for s in range(2, S, ALWAYS_EVERY):
                assert a.sb.init_session_rate(s, 16000) == 0 and b.sb.init_session_rate(s, 16000) == 0
                plan.init_session(s, 16000)
            continue
        # the refused ticks, on one twin only
        for case in rows_of:
            if case.get("after_split") and not split_used:
                continue
            kw = dict(case["tick"])
            if "flags" in kw:
                kw["flags"] = T.pattern(S, *kw["flags"])
            for form in ("sync", "async", "host"):
                assert a.call(form, **kw) == case["code"], (case["name"], form)
                refusals += 1
        flags, n, calls, clean = tick
        rows = {k: rng.integers(-3000, 3000, (S, ROW)).astype(np.int16) for k in ("far", "near", "clean")}
        out_a, snaps_a = a.accepted(rows, flags, n, calls, clean)
        out_b, snaps_b = b.accepted(rows, flags, n, calls, clean)
        rc, got = plan.tick(flags=flags, n=n, calls=calls, clean=clean, packets=True, ms_per_session=flags is not None)
        assert rc == 0
        families.append(got["family"])
        split_used = split_used or got["family"] == "split"
        assert np.array_equal(out_a, out_b), (len(families), got["family"])
        assert snaps_a == snaps_b, (len(families), got["family"])
        assert a.modes() == b.modes() == plan.state()["modes"]
    want = {"nothing", "mixed", "packets", "split"} if two_rates else set(T.families())
    assert set(families) == want and families[-1] == "split", families
    assert refusals == 3 * (len(families) * len([c for c in rows_of if not c.get("after_split")]) + len([c for c in rows_of if c.get("after_split")]))
    a.sb.close()
    b.sb.close()
