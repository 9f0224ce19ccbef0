"""The ops probe on the CPU: the list of probed primitives (webrtc_aecm_amd/csrc/aecm_ops_table.inc) is complete, the HOST branch
of every entry (tests/sim/sim_ops.cpp -> tests/_build/libaecm_ops.so, the definitions the lane simulator runs) equals the
independent definition of tests/ops_ref.py bit for bit over the entry's whole grid, and the grids (tests/ops_grid.py) hold what
they must.  The device branch of the same list is compared with both in tests/test_gpu_ops_probe.py."""
import json
import re

import numpy as np
import pytest

import ops_grid
import ops_ref
import ops_sim

ROOT = ops_grid.ROOT
OPS_H = ROOT / "webrtc_aecm_amd" / "csrc" / "aecm_ops.h"
ALLOWLIST = ROOT / "tests" / "ops_allowlist.json"
NAMES = ops_grid.names()
# entries of the table that are not a function of aecm_ops.h by that name: second results, raw forms and the helpers of aecm_wave.h
DERIVED = {"div_magic_magic": "div_magic", "div_magic_shift": "div_magic", "mul24_insn_raw": "mul24_insn"}
WAVE_HELPERS = ("asym_filt", "log_energy_q8", "aligned_slot", "bitrev6")


def functions_of_ops_h(text):
    """Every function defined under namespace aecm in aecm_ops.h: AECM_HD definitions (template or not) and the packed binary
    ops that the AECM_PK_BINOP macro defines."""
    text = re.sub(r"//.*", "", text)
    body = text[text.index("namespace aecm {"):]
    found = set(re.findall(r"\bAECM_HD\s+[\w:<> ]*?[\s*&](\w+)\s*\(", body))
    found |= {n for n in re.findall(r"^AECM_PK_BINOP\(\s*(\w+)\s*,", body, re.M)}
    found.discard("NAME")                                  # the macro's own parameter
    return found


def probed_functions():
    out = set()
    for n in NAMES:
        if n in DERIVED:
            out.add(DERIVED[n])
        elif not n.startswith(WAVE_HELPERS):
            out.add(n)
    return out


def test_table_is_well_formed():
    entries = ops_grid.table_entries()
    assert [i for i, _, _ in entries] == list(range(len(entries))) and len(entries) >= 80
    assert len(set(NAMES)) == len(NAMES)
    assert all(1 <= k <= 3 for _, _, k in entries)
    # the compiled host library expanded the same list
    assert ops_sim.names() == NAMES
    assert [ops_sim.arity(i) for i in range(len(NAMES))] == [k for _, _, k in entries]
    for helper in WAVE_HELPERS:
        assert any(n.startswith(helper) for n in NAMES), helper
    # asym_filt: one entry per (step_pos, step_neg) pair calc_energies passes
    wave = (ROOT / "webrtc_aecm_amd" / "csrc" / "aecm_wave.h").read_text()
    m = re.search(r"int inc_max = (\d+), dec_max = (\d+), inc_min = (\d+), dec_min = (\d+);\s*if \(AECM_STEADY_NEVER\(u\.startup == 0\)\) "
                  r"\{ inc_max = (\d+); dec_min = (\d+); inc_min = (\d+); \}", wave)
    assert m and len(re.findall(r"asym_filt\(u\.fe_m", wave)) == 2, "calc_energies no longer passes the step pairs the table lists"
    inc_max, dec_max, inc_min, dec_min, inc_max0, dec_min0, inc_min0 = map(int, m.groups())
    pairs = {(inc_min, dec_min), (inc_max, dec_max), (inc_min0, dec_min0), (inc_max0, dec_max)}
    assert {f"asym_filt_{p}_{n}" for p, n in pairs} == {n for n in NAMES if re.fullmatch(r"asym_filt_\d+_\d+", n)}
    assert {f"asym_filt_lean_{p}_{n}" for p, n in pairs} == {n for n in NAMES if n.startswith("asym_filt_lean_")}


def test_every_function_of_ops_h_is_probed_or_excused():
    """A primitive added to aecm_ops.h without an entry in the table (or a reasoned line in tests/ops_allowlist.json) fails here."""
    allow = json.loads(ALLOWLIST.read_text())
    assert all(isinstance(r, str) and len(r.strip()) >= 10 for r in allow.values()), "every excused name carries a reason"
    defined = functions_of_ops_h(OPS_H.read_text())
    assert len(defined) >= 70
    probed = probed_functions()
    assert not (probed & set(allow)), "probed and excused at once"
    missing = defined - probed - set(allow)
    assert not missing, f"functions of aecm_ops.h without an entry in aecm_ops_table.inc: {sorted(missing)}"
    stale = (probed | set(allow)) - defined
    assert not stale, f"table entries or excuses for functions aecm_ops.h does not define: {sorted(stale)}"
    # the parser itself: it must see a function that is added
    grown = OPS_H.read_text().replace("}  // namespace aecm", "AECM_HD int brand_new_op(int a) { return a; }\n"
                                      "template <class I> AECM_HD I brand_new_template(I a) { return a; }\n}  // namespace aecm")
    assert functions_of_ops_h(grown) - defined == {"brand_new_op", "brand_new_template"}


def test_reference_and_predicates_cover_the_table():
    assert set(ops_ref.REF) == set(NAMES)
    for table in (ops_grid.CLAIMS, ops_grid.DOMAINS, ops_grid.NAMED, ops_ref.AUDIT_REF):
        assert set(table) <= set(NAMES), sorted(set(table) - set(NAMES))
    assert set(ops_grid.UNIFORM_C) <= set(NAMES)
    assert set(ops_ref.AUDIT_REF) <= set(ops_grid.CLAIMS)


def test_edge_set():
    e = set(int(v) for v in ops_grid.E32)
    want = [0, 1, -1, 2, -2, ops_grid.INT_MAX, ops_grid.INT_MIN, ops_grid.INT_MIN + 1, 1 << 23, -(1 << 23), (1 << 23) - 1, -(1 << 23) - 1,
            32767, -32767, 32768, -32768, 65535, 65536]
    want += [v - (1 << 32) if v >= 1 << 31 else v for v in (0x80008000, 0x7fff7fff, 0x8000ffff, 0xffff8000, 0x00018000, 0x7fff0001)]
    for k in range(31):
        want += [1 << k, -(1 << k), (1 << k) + 1, (1 << k) - 1, ~(1 << k)]
    assert not [v for v in want if v not in e]
    s = set(int(v) for v in ops_grid.sparse_words())
    assert len(s) == 2 * (1 + 32 + 32 * 31 // 2) and 0x00010001 in s and ~0x00010001 in s


@pytest.mark.parametrize("name", NAMES)
def test_grid(name):
    """At most 2^20 tuples; at least 1 000 inside the claim, with every named case that lies inside it; deterministic; the host
    library's "claim violated" flag is set for exactly the tuples outside the claim (the predicates here are the header's checks)."""
    a, b, c = ops_grid.full_grid(name)
    k = ops_grid.arity(name)
    assert [o is not None for o in (a, b, c)] == [j < k for j in range(3)]
    assert a.size <= ops_grid.MAX_TUPLES
    inside = ops_grid.claim_mask(name, a, b, c)
    assert int(inside.sum()) >= 1000, int(inside.sum())
    ops_grid._full_grid.cache_clear()
    again = ops_grid.full_grid(name)
    assert all((x is None and y is None) or np.array_equal(x, y) for x, y in zip((a, b, c), again))
    # named cases
    adm = ops_grid.admissible(name)
    rows = set(zip(*[o.tolist() for o in adm if o is not None]))
    z = np.zeros(1, dtype=np.int64)
    for case in ops_grid.NAMED.get(name, []):
        w = [None if v is None else np.array([v], dtype=np.int64) for v in case]
        in_claim = ops_grid._mask(ops_grid.CLAIMS, name, *w)[0] and ops_grid._mask(ops_grid.DOMAINS, name, *w)[0]
        if in_claim:
            assert tuple(v for v in case if v is not None) in rows, case
    # the wave-uniform operand of the _uc forms: one value per aligned group of 64
    if name in ops_grid.UNIFORM_C:
        assert np.array_equal(adm[2], np.repeat(adm[2][::64], 64)[:adm[2].size])
    # the header's own checks fire exactly outside the claim
    _, flags = ops_sim.evaluate(name, a, b, c)
    assert np.array_equal(flags != 0, ~inside), (name, int((flags != 0).sum()), int((~inside).sum()))
    if name not in ops_grid.CLAIMS:
        assert inside.all()


@pytest.mark.parametrize("name", NAMES)
def test_host_branch_equals_the_independent_reference(name):
    a, b, c = ops_grid.admissible(name)
    got, flags = ops_sim.evaluate(name, a, b, c)
    assert not flags.any()
    want = ops_ref.evaluate(name, a, b, c)
    bad = np.flatnonzero(got != want)
    if bad.size:
        i = int(bad[0])
        pytest.fail(f"{name}: {bad.size} of {a.size} tuples differ; first: tuple {i} = "
                    f"({', '.join(str(int(o[i])) for o in (a, b, c) if o is not None)}): host {int(got[i])}, reference {int(want[i])}")


def test_named_cases_have_the_values_the_reference_lines_give():
    """A handful of the named cases by hand, so that a mistake shared by ops_ref.py and the header cannot pass unseen."""
    def ref(name, *t):
        return int(ops_ref.evaluate(name, *[None if v is None else [v] for v in t])[0])
    INT_MIN, INT_MAX = ops_grid.INT_MIN, ops_grid.INT_MAX
    assert ref("divi", 5, 0) == INT_MAX and ref("divi", INT_MIN, -1) == INT_MIN and ref("divi", -7, 2) == -3
    assert ref("divu", 5, 0) == -1
    assert [ref("norm_w32", v) for v in (0, -1, INT_MIN, 1, INT_MAX)] == [0, 31, 0, 30, 0]
    assert [ref("norm_w16", v) for v in (0, -1, -32768, 1, 32767)] == [0, 15, 0, 14, 0]
    assert [ref("norm_w32_nz", v) for v in (0, -1)] == [31, 31] and [ref("norm_w16_nz", v) for v in (0, -1)] == [15, 15]
    assert [ref("ffbh_i", v) for v in (0, -1, 1, -2, INT_MIN)] == [-1, -1, 31, 31, 1]
    assert ref("norm_u32_v", 0) == 0 and ref("clz32", 0) == 32 and ref("norm_u32", -1) == 0
    h = -0x7fff8000                                        # 0x80008000
    assert ref("dot2_i16", h, h, -1) == INT_MAX and ref("dot2_i16_c0", h, h) == INT_MIN and ref("dot2_i16_cm1", h, h) == INT_MAX
    assert ref("pk_neg_i16", h) == h and ref("pk_abs_sat_i16", h) == 0x7fff7fff
    assert ref("add_sat32", INT_MAX, 1) == INT_MAX and ref("add_sat32", INT_MIN, -1) == INT_MIN
    assert ref("shift_i31", -1, -31) == -1 and ref("shift_u31", -1, -31) == 1 and ref("shift_i31", 1, 31) == INT_MIN
    assert ref("mean_step", INT_MAX, 1, -2) == w32_int(-2 + -((1 << 31) - 1 >> 1))
    assert ref("mul24_insn_raw", 1 << 23, 1) == -(1 << 23) and ref("mul24_insn_raw", (1 << 24) + 3, 5) == 15
    assert ref("log_energy_q8", 0, 5) == 896 and ref("log_energy_q8", 1, 0) == 896 and ref("log_energy_q8", -1, 0) == 896 + (31 << 8) + 255
    assert ref("asym_filt_4_11", 32767, 5) == 5 and ref("asym_filt_4_11", 0, 32) == 2 and ref("asym_filt_4_11", 0, -4096) == -2
    assert ref("aligned_slot", 0, 1) == 99 and ref("bitrev6", 1) == 32
    assert ref("div_magic_magic", 65) == 4162814457 - (1 << 32) and ref("div_magic_shift", 65) == 7          # init_lane_constants' pair


def w32_int(x):
    return ((x + (1 << 31)) & 0xffffffff) - (1 << 31)
