"""The ops probe on the GPU (WebRtcAecmBatch_DebugOps, aecm_ops_probe_kernels.hip): the DEVICE branch of every entry of
webrtc_aecm_amd/csrc/aecm_ops_table.inc -- builtins, LLVM intrinsics reached by name, inline assembly with operand modifiers --
alone, against the HOST branch of the same entry (tests/_build/libaecm_ops.so, what the lane simulator runs) and against the
independent definition of tests/ops_ref.py, over the entry's admissible grid (tests/ops_grid.py), in lane form (operands in vector
registers) and in uniform form (wave-uniform operands, which the compiler may keep on the scalar unit).  One launch per entry and
form.  Then the same through the audit twin of the library, with the positive control its counters never had: tuples that violate
a claim make them count, exactly, and the checked primitives still return the exact result."""
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys
import textwrap
from functools import lru_cache

import numpy as np
import pytest

import ops_grid
import ops_ref
import ops_sim
import webrtc_aecm_amd as aecm

pytestmark = pytest.mark.gpu

NAMES = ops_grid.names()
FORMS = {0: "lane form", 1: "uniform form"}
SHIPPED_ONLY = ("mul24_insn_raw",)          # the raw instruction: the audit build's mul24_insn is the checked mul24
_shipped = {}                               # (name, form) -> digest of the shipped library's results


@lru_cache(maxsize=None)
def expected(name):
    """(a, b, c, host branch, independent reference) over the admissible grid: computed once, shared, never written to."""
    a, b, c = ops_grid.admissible(name)
    host, flags = ops_sim.evaluate(name, a, b, c)
    assert not flags.any()
    ref = ops_ref.evaluate(name, a, b, c)
    for x in (host, ref):
        x.flags.writeable = False
    return a, b, c, host, ref


def digest(out):
    return hashlib.sha256(np.ascontiguousarray(out, dtype=np.int32).tobytes()).hexdigest()


def run_shipped(name, form):
    a, b, c, host, ref = expected(name)
    out, nonuniform = aecm.debug_ops(name, a, b, c, form=form)
    _shipped[(name, form)] = digest(out)
    return out, nonuniform


def describe_first_difference(name, form, a, b, c, dev, host, ref):
    bad = np.flatnonzero((dev != host) | (dev != ref))
    if not bad.size:
        return None
    i = int(bad[0])
    ops = ", ".join(str(int(o[i])) for o in (a, b, c) if o is not None)
    return (f"{name}, {FORMS[form]}: {bad.size} of {a.size} tuples differ; first: tuple {i} = ({ops}): "
            f"device {int(dev[i])}, host branch {int(host[i])}, reference {int(ref[i])}")


def test_library_lists_the_same_table():
    assert aecm.debug_ops_names() == NAMES == ops_sim.names()
    lib = aecm.load()
    assert lib.WebRtcAecmBatch_DebugOpName(-1) is None and lib.WebRtcAecmBatch_DebugOpName(len(NAMES)) is None


@pytest.mark.parametrize("name", NAMES)
def test_device_equals_host_branch_and_reference(name):
    a, b, c, host, ref = expected(name)
    assert a.size >= 1000
    for form in FORMS:
        dev, nonuniform = run_shipped(name, form)
        msg = describe_first_difference(name, form, a, b, c, dev, host, ref)
        assert msg is None, msg
        assert not nonuniform.any(), (f"{name}, {FORMS[form]}: lanes of one wave disagree on wave-uniform operands, first at tuple "
                                      f"{int(np.flatnonzero(nonuniform)[0])}")


def test_refusals():
    """Bad op / form / n and a missing operand array: AECM_BAD_PARAMETER_ERROR, and the output is not touched."""
    lib = aecm.load()
    bad = aecm.ffi.AECM_BAD_PARAMETER_ERROR
    a = np.arange(8, dtype=np.int32)
    out = np.full(8, 0x5A5A5A5A, dtype=np.int32)
    non = np.full(8, 0x5A5A5A5A, dtype=np.int32)
    add, dot2 = NAMES.index("add"), NAMES.index("dot2_i16")
    p = lambda x: None if x is None else x.ctypes.data      # noqa: E731
    calls = [(-1, 0, a, a, a, 8), (len(NAMES), 0, a, a, a, 8), (1 << 30, 1, a, a, a, 8),          # no such op
             (add, 2, a, a, None, 8), (add, -1, a, a, None, 8),                                   # no such form
             (add, 0, a, a, None, 0), (add, 0, a, a, None, -5), (add, 1, a, a, None, (1 << 20) + 1),      # n <= 0, n > 2^20
             (add, 0, a, None, None, 8), (add, 0, None, a, None, 8), (dot2, 1, a, a, None, 8)]    # an operand the arity needs
    for op, form, x, y, z, n in calls:
        assert lib.WebRtcAecmBatch_DebugOps(0, op, form, p(x), p(y), p(z), p(out), p(non), n) == bad, (op, form, n)
        assert (out == 0x5A5A5A5A).all() and (non == 0x5A5A5A5A).all()
    assert lib.WebRtcAecmBatch_DebugOps(0, add, 0, p(a), p(a), None, None, None, 8) == bad          # no output array
    # and the smallest good call, without the optional array
    assert lib.WebRtcAecmBatch_DebugOps(0, add, 1, p(a), p(a), None, p(out), None, 8) == 0
    assert np.array_equal(out, 2 * a)


def test_audit_build_counts_violations_and_stays_exact(tmp_path):
    """libaecm_mi355x_checked.so in a fresh child process (AECM_LIB_PATH): over the admissible grids its results are the shipped
    library's and both counters stay 0; over the tuples that violate a claim of mul24 / as_i16 / as_nonneg / checked_shift31 the
    claim's counter rises by exactly their number in lane form (by 64 times that in uniform form: every lane of the wave counts)
    and the other stays 0, and the results are the exact ones the header promises (mul24: mul(a, b); as_i16: sext16(v))."""
    from webrtc_aecm_amd import build
    with pytest.raises(aecm.AecmError) as e:
        aecm.check_counters(0)
    assert e.value.code == aecm.ffi.AECM_UNSUPPORTED_FUNCTION_ERROR
    assert build.LIB_CHECKED.exists()
    audited = [n for n in NAMES if n not in SHIPPED_ONLY]
    for name in audited:
        for form in FORMS:
            if (name, form) not in _shipped:               # (this test run on its own)
                run_shipped(name, form)
    script = tmp_path / "audit_ops.py"
    script.write_text(textwrap.dedent("""
        import hashlib, json, sys
        import numpy as np
        import webrtc_aecm_amd as aecm
        import ops_grid, ops_ref
        names = json.loads(sys.argv[1])
        report = {"digests": {}, "violations": {}}
        assert aecm.check_counters(0, reset=True) is not None
        for name in names:
            a, b, c = ops_grid.admissible(name)
            for form in (0, 1):
                out, non = aecm.debug_ops(name, a, b, c, form=form)
                assert not non.any(), (name, form)
                report["digests"][f"{name}/{form}"] = hashlib.sha256(out.tobytes()).hexdigest()
        report["admissible_counters"] = [int(v) for v in aecm.check_counters(0, reset=True)]
        for name in sorted(ops_ref.AUDIT_REF):
            a, b, c = ops_grid.violating(name)
            want = ops_ref.evaluate(name, a, b, c, table=ops_ref.AUDIT_REF)
            for form in (0, 1):
                out, non = aecm.debug_ops(name, a, b, c, form=form)
                counters = [int(v) for v in aecm.check_counters(0, reset=True)]
                bad = np.flatnonzero(out != want)
                first = None if not bad.size else [int(bad[0])] + [int(o[bad[0]]) for o in (a, b, c, out, want) if o is not None]
                report["violations"][f"{name}/{form}"] = {"n": int(a.size), "counters": counters, "wrong": int(bad.size), "first": first,
                                                          "nonuniform": int(np.count_nonzero(non))}
        print("REPORT " + json.dumps(report))
    """))
    root = str(ops_grid.ROOT)
    env = dict(os.environ, AECM_LIB_PATH=str(build.LIB_CHECKED),
               PYTHONPATH=os.pathsep.join([root, os.path.join(root, "tests"), os.environ.get("PYTHONPATH", "")]))
    r = subprocess.run([sys.executable, str(script), json.dumps(audited)], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("REPORT ")]
    assert line, r.stdout[-500:]
    report = json.loads(line[-1][len("REPORT "):])
    differing = [k for k in report["digests"] if report["digests"][k] != _shipped[(k.rsplit("/", 1)[0], int(k.rsplit("/", 1)[1]))]]
    assert not differing, f"the audit build's results differ from the shipped library's: {differing}"
    assert len(report["digests"]) == 2 * len(audited)
    assert report["admissible_counters"] == [0, 0]
    which = {"mul24": 0, "as_i16": 1, "as_nonneg": 1, "checked_shift31": 1}          # aecm_ops.h: [0] mul24 operands, [1] the narrowings
    assert set(which) == set(ops_ref.AUDIT_REF)
    for name, counter in which.items():
        for form in FORMS:
            v = report["violations"][f"{name}/{form}"]
            assert v["n"] >= 63, (name, v)
            want = [0, 0]
            want[counter] = v["n"] * (1 if form == 0 else 64)
            assert v["counters"] == want, (name, FORMS[form], v)
            assert v["wrong"] == 0 and v["nonuniform"] == 0, (name, FORMS[form], v)
