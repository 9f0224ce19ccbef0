"""The session-flow decision corpus (tests/flow_corpus.py) through every entry point that reaches a different planning kernel, one
object of 300 sessions per test -- two planning workgroups, the last wavefront partial, neighbouring lanes in different scenarios
and phases, so that the wrapper's decisions are taken DIVERGENTLY inside aecm_flow_plan_kernel (dense ticks),
aecm_flow_plan_sparse_kernel (idle lanes; force_sparse_ticks), aecm_flow_plan_mixed_kernel (both rates, half calls),
aecm_flow_plan_calls_kernel (TickCalls, K = 2, 3, 6 and the replay-row spill inside a K-call tick), aecm_flow_plan_packets_kernel
(TickPackets on the mixed object) and, one wavefront per session, aecm_buffer_farend_kernel (the bursts of every object); the dense
object once more on the checked library.  Two comparisons per object:
  - against the unmodified reference, one WebRtcAecm_* instance per session at its own rate and call sizes (where oracle/_ref did not
    travel: the single-session ABI, and in both cases the reference's recorded run, tests/golden/sessflow_*.npz): every output
    sample, every return code, the echo path at the end, bit for bit;
  - against the host compile of the same source: after every tick the wrapper words of every session's snapshot (export_sessions,
    offset 16 192) equal the FlowRegs tests/sim/sim_flowcov.cpp computes for that session and tick, field by field (F_NEAR_LAG is
    exported as 0 and left out).  That catches a planner whose compiled code differs from its source even where the audio survives."""
import functools
import os
import subprocess
import sys
import textwrap
import importlib.util
from pathlib import Path

import numpy as np
import pytest

import flow_corpus as fc
import webrtc_aecm_amd as aecm
from helpers import GOLDEN
from oracle import pyoracle

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
_spec = importlib.util.spec_from_file_location("flow_coverage", ROOT / "tools" / "flow_coverage.py")
F = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(F)

SNAPSHOT_BYTES, FLOW_AT, FLOW_WORDS = 34304, 16192, 32
FIELDS = ("F_BUF_SIZE_START", "F_KNOWN_DELAY", "F_COUNTER", "F_SUM", "F_FIRST_VAL", "F_CHECK_BUF_SIZE_CTR", "F_MS", "F_FILT_DELAY",
          "F_TIME_FOR_DELAY_CHANGE", "F_EC_STARTUP", "F_CHECK_BUFF_SIZE", "F_DELAY_CHANGE", "F_LAST_DELAY_DIFF", "F_FAR_RP", "F_FAR_WP", "F_FRM_POS",
          "F_BLK_POS", "F_OUT_RP", "F_RUN_POS", "F_RUN_DELTA", "F_FF_VALID", "F_OLD_POS0", "F_OLD_POS1", "F_OLD_ROW0", "F_OLD_ROW1")        # (then F_NEAR_LAG)
JUNK_FAR, JUNK_NEAR = 12345, -12345
FAMILIES = list(fc.GOLDEN_NAMES)


@functools.lru_cache(maxsize=None)
def _case(family):
    """(schedule, far, near, the host harness's run) of a family, once."""
    sch = fc.family_schedule(family)
    far, near = fc.signals(sch)
    for a in (far, near):
        a.flags.writeable = False
    host = F.Harness(coverage=False).run(sch)
    assert host["first_difference"] == -1, (family, host["first_difference"], host["detail"])
    return sch, far, near, host


@pytest.fixture(scope="module")
def reference():
    """family -> (out, codes, paths) of one instance per session, computed once per family and shared by the tests that need it; the
    unmodified reference where it is built, else the single-session ABI -- in both cases it must be the reference's recorded run."""
    @functools.lru_cache(maxsize=None)
    def run(family):
        sch, far, near, _ = _case(family)
        if pyoracle.have_reference():
            make = lambda fs: pyoracle.RefSession(fs, 1, 3)
        else:
            def make(fs):
                s = aecm.Aecm()
                assert s.init(fs) == 0 and s.set_config(1, 3) == 0
                return s
        out, codes, paths = fc.drive_reference(sch, far, near, make)
        g, mine = np.load(GOLDEN / f"{fc.GOLDEN_NAMES[family]}.npz"), fc.summary(out, codes, paths)
        assert all(np.array_equal(g[k], mine[k]) for k in ("sha256", "codes", "paths")), (family, "differs from the reference's recorded run")
        out.flags.writeable = False
        return out, codes, paths
    return run


def _wrapper_words(blob, sessions):
    snaps = np.frombuffer(blob, dtype=np.int32).reshape(sessions, SNAPSHOT_BYTES // 4)
    return snaps[:, FLOW_AT // 4:FLOW_AT // 4 + FLOW_WORDS]


def _run_object(family, expected):
    """The family's schedule on an AecmSessions object; after every tick that launches, the wrapper words against the host harness.
    Returns the measured seconds of the device side."""
    import time
    sch, far, near, host = _case(family)
    exp_out, exp_codes, exp_paths = expected
    T, S = sch["flags"].shape
    assert S == 300 and aecm.load().WebRtcAecmSessions_session_size_bytes() == SNAPSHOT_BYTES
    mixed = len(set(sch["rates"].tolist())) > 1
    t0 = time.time()
    sb = aecm.AecmSessions(S, int(sch["fs"]), 1, 3, rates=sch["rates"] if mixed else None)
    if sch["force"]:
        assert sb.force_sparse_ticks(True) == 0
    # the imported start states: the wrapper words the harness gives, in the snapshots of fresh sessions
    fresh = np.zeros(FLOW_WORDS, dtype=np.int32)
    fresh[[9, 10, 11, 20, 23, 24]] = 1
    rc, blob = sb.export_sessions()
    assert rc == 0 and len(blob) == S * SNAPSHOT_BYTES
    assert np.array_equal(_wrapper_words(blob, S), np.broadcast_to(fresh, (S, FLOW_WORDS)))
    imported = np.flatnonzero((host["start"] != fresh).any(axis=1))
    if imported.size:
        snaps = np.frombuffer(blob, dtype=np.int32).reshape(S, -1).copy()
        snaps[imported, FLOW_AT // 4:FLOW_AT // 4 + FLOW_WORDS] = host["start"][imported]
        assert sb.import_sessions(imported, np.ascontiguousarray(snaps[imported]).view(np.uint8), any_rate=mixed) == 0         # (a session of the other rate keeps it)
    cf, cn = np.zeros(S, dtype=np.int64), np.zeros(S, dtype=np.int64)
    out = np.zeros_like(exp_out)
    blen = int(sch["burst_len"])
    for t in range(T):
        n, K, kind, n_s, calls = fc.tick_layout(sch, t)
        fl, ms, b = sch["flags"][t], sch["ms"][t], sch["burst"][t].astype(np.int64)
        if b.any():
            fx = np.full((S, int(b.max()) * blen), JUNK_FAR, dtype=np.int16)
            for s in np.flatnonzero(b):
                fx[s, :b[s] * blen] = far[s, cf[s]:cf[s] + b[s] * blen]
            cf += b * blen
            assert sb.buffer_farend_host(fx, blen, int(b.max()), calls_per_session=b.astype(np.uint8)) == 0, (family, t)
        own, span = n_s * calls, n * K
        f, d = np.full((S, span), JUNK_FAR, dtype=np.int16), np.full((S, span), JUNK_NEAR, dtype=np.int16)
        farend = (fl & fc.NO_FAREND) == 0
        for s in np.flatnonzero(own):
            if farend[s]:
                f[s, :own[s]] = far[s, cf[s]:cf[s] + own[s]]
            d[s, :own[s]] = near[s, cn[s]:cn[s] + own[s]]
        if kind == 0:
            rc, o, codes = sb.tick_host_per_session(f, d, ms, flags=fl)
        elif kind == 1:
            rc, o, codes = sb.tick_calls_host(f, d, K, ms, flags=fl)
        else:
            rc, o, codes = sb.tick_packets_host(f, d, K, ms, flags=fl)
        nz = exp_codes[t][exp_codes[t] != 0]
        assert rc == (int(nz[0]) if nz.size else 0) and np.array_equal(codes, exp_codes[t]), (family, "return codes of tick", t)
        for s in np.flatnonzero(own):
            out[s, cn[s]:cn[s] + own[s]] = o[s, :own[s]]
            assert not o[s, own[s]:].any(), (family, "zeros behind a session's calls", t, s)
        assert not o[own == 0].any(), (family, "an idle session's row", t)
        cf += np.where(farend, own, 0)
        cn += own
        if host["kernels"][t] == 0:
            continue                                          # nobody called: nothing was launched, nothing moved
        rc, blob = sb.export_sessions()
        assert rc == 0
        dev, want = _wrapper_words(blob, S)[:, :len(FIELDS)], host["regs"][t][:, :len(FIELDS)]
        if not np.array_equal(dev, want):
            s, k = (int(x[0]) for x in np.nonzero(dev != want))
            pytest.fail(f"{family}: the wrapper state after tick {t} ({F.KERNELS[host['kernels'][t]]} planner) differs from the host compile of "
                        f"aecm_flow_plan.h first in session {s} (lane {s % 64} of wavefront {s // 64}, scenario {sch['names'][s]}), field {FIELDS[k]}: "
                        f"device {dev[s, k]}, host {want[s, k]}; flags {fl[s]}, ms {ms[s]}")
        assert not _wrapper_words(blob, S)[:, len(FIELDS):].any(), (family, "F_NEAR_LAG is exported as 0; the words behind it are 0", t)
    bad = np.argwhere(out != exp_out)
    assert bad.size == 0, (family, "output: first difference in session, sample", int(bad[0][0]), int(bad[0][1]), sch["names"][int(bad[0][0])])
    for s in range(S):
        rc, path = sb.get_echo_path(s)
        assert rc == 0 and np.array_equal(path, exp_paths[s]), (family, "echo path of session", s, sch["names"][s])
    sb.close()
    return time.time() - t0


def test_the_schedules_reach_every_planner():
    """What each object's ticks are routed to (the host harness routes as SessionBatch::Enqueue does)."""
    want = {"dense16": {"dense"}, "dense8": {"dense"}, "sparse16": {"sparse"}, "forced8": {"sparse"}, "mixed": {"mixed"}, "calls2": {"calls"},
            "calls3": {"calls"}, "calls6": {"calls"}, "packets2": {"packets"}, "calls6_spill": {"dense", "sparse", "calls"}}
    for family in FAMILIES:
        sch, _, _, host = _case(family)
        assert {F.KERNELS[k] for k in set(host["kernels"].tolist()) if k} == want[family], family
        assert sch["burst"].any() or family == "calls6_spill", family          # aecm_buffer_farend_kernel runs in every object


@pytest.mark.parametrize("family", FAMILIES)
def test_flow_corpus(family, reference):
    seconds = _run_object(family, reference(family))
    print(f"{family}: device side {seconds:.2f} s")


def test_flow_corpus_on_the_checked_library(tmp_path, reference):
    """libaecm_mi355x_checked.so (-DAECM_CHECKED), the dense object, in a child process: outputs, codes, echo paths and wrapper words as
    above, and both audit counters stay 0."""
    from webrtc_aecm_amd import build
    assert build.LIB_CHECKED.exists()
    out, codes, paths = reference("dense16")
    np.savez(tmp_path / "expected.npz", out=out, codes=codes, paths=paths)
    script = tmp_path / "checked_flow.py"
    script.write_text(textwrap.dedent(f"""
        import numpy as np
        import webrtc_aecm_amd as aecm
        import test_gpu_flow_corpus as T
        assert aecm.check_counters(0, reset=True) is not None
        g = np.load(r"{tmp_path / 'expected.npz'}")
        T._run_object("dense16", (g["out"], g["codes"], g["paths"]))
        c = aecm.check_counters(0)
        print("AUDIT", int(c[0]), int(c[1]))
    """))
    env = dict(os.environ, AECM_LIB_PATH=str(build.LIB_CHECKED),
               PYTHONPATH=os.pathsep.join([str(GOLDEN.parent.parent), str(GOLDEN.parent), os.environ.get("PYTHONPATH", "")]))
    r = subprocess.run([sys.executable, str(script)], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("AUDIT")]
    assert line and line[-1].split()[1:] == ["0", "0"], r.stdout[-500:]
