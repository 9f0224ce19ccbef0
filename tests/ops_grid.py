"""TEST INFRASTRUCTURE: the operand tuples of the ops probe, per entry of webrtc_aecm_amd/csrc/aecm_ops_table.inc.  Deterministic
(seeded RandomState per entry), at most 2^20 tuples per entry.

Three things per entry, by name:
  full_grid(name)     every tuple the entry is ever given (int32 arrays a, b, c; None above the arity)
  CLAIMS[name]        the range the header CLAIMS and checks (mul24's 24-bit operands, as_i16 ...): the host branch calls its
                      aecm_*_violation hook, the audit build counts, exactly where the predicate is false.  Tuples outside it
                      are dropped for the shipped library (admissible) and kept for the audit test (violating).
  DOMAINS[name]       the contract of the call sites that nothing checks (a != 0 for clz32_nz, per-half shift counts < 16, the
                      int16 arguments of asym_filt ...).  Nothing is defined outside it, on either side: full_grid never
                      leaves it.  Each states where the contract comes from.
"""
from __future__ import annotations

import re
import zlib
from functools import lru_cache
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
TABLE = ROOT / "webrtc_aecm_amd" / "csrc" / "aecm_ops_table.inc"
INT_MIN, INT_MAX = -(1 << 31), (1 << 31) - 1
MAX_TUPLES = 1 << 20
kHistory = 100


def table_entries():
    """[(id, name, arity)] as aecm_ops_table.inc lists them (parsed, so that collecting the tests needs no compiler)."""
    text = re.sub(r"//.*", "", TABLE.read_text())
    return [(int(i), n, int(k)) for i, n, k in re.findall(r"^AECM_OP\(\s*(\d+)\s*,\s*(\w+)\s*,\s*(\d)\s*,", text, re.M)]


def names():
    return [n for _, n, _ in table_entries()]


def arity(name):
    return {n: k for _, n, k in table_entries()}[name]


def _w32(values):
    v = np.asarray(list(values), dtype=object)
    return np.array([((int(x) + (1 << 31)) & 0xffffffff) - (1 << 31) for x in v], dtype=np.int64)


def _unique(v):
    """Order-preserving."""
    _, idx = np.unique(v, return_index=True)
    return v[np.sort(idx)]


def e32():
    """The 32-bit edge set."""
    v = [0, 1, -1, 2, -2, INT_MAX, INT_MIN, INT_MIN + 1]
    for k in range(32):
        p = 1 << k
        v += [p, -p, p + 1, p - 1, ~p]
    v += [1 << 23, -(1 << 23), (1 << 23) - 1, -(1 << 23) - 1]                 # the 24-bit boundaries
    v += [32767, -32767, 32768, -32768, 65535, 65536]                         # the int16 boundaries
    v += [0x80008000, 0x7fff7fff, 0x8000ffff, 0xffff8000, 0x00018000, 0x7fff0001]      # packed words
    return _unique(_w32(v))


E32 = e32()
E16 = E32[(E32 >= -32768) & (E32 <= 32767)]                                   # its int16 subset


def sparse_words():
    """Every word with at most two set or at most two clear bits."""
    v = [0]
    for i in range(32):
        v.append(1 << i)
        for j in range(i):
            v.append((1 << i) | (1 << j))
    v = _w32(v)
    return _unique(np.concatenate([v, ~v]))


def _rs(name):
    return np.random.RandomState(zlib.crc32(name.encode()) & 0x7fffffff)


def _rand32(rs, n):
    return rs.randint(INT_MIN, INT_MAX + 1, size=n, dtype=np.int64)


def _cross(*axes):
    """All combinations, the LAST axis varying slowest (so that aligned groups of 64 tuples mostly share the last operand)."""
    grids = np.meshgrid(*axes[::-1], indexing="ij")[::-1]
    return [g.ravel() for g in grids]


def _cat(*parts):
    return [np.concatenate([p[k] for p in parts]) for k in range(len(parts[0]))]


def unary32(name, extra=()):
    rs = _rs(name)
    return [np.concatenate([E32, sparse_words(), _rand32(rs, 1 << 18), np.asarray(extra, dtype=np.int64)])]


def unary_packed(name):
    full = np.arange(1 << 16, dtype=np.int64)
    other = np.array([0, 1, 0x7fff, 0x8000, 0xffff], dtype=np.int64)
    f, o = _cross(full, other)
    words = np.concatenate([f | (o << 16), o | (f << 16)])
    return [np.concatenate([E32, _w32(words)])]


def binary(name, n_random=1 << 17):
    rs = _rs(name)
    return _cat(_cross(E32, E32), [_rand32(rs, n_random), _rand32(rs, n_random)])


def binary_count(name, lo, hi):
    """A value and a shift-like count: E32 x every count in [lo, hi], E32 x E32, random values with random counts."""
    rs = _rs(name)
    counts = np.arange(lo, hi + 1, dtype=np.int64)
    return _cat(_cross(E32, counts), _cross(E32, E32), [_rand32(rs, 1 << 16), _rand32(rs, 1 << 16)],
                [_rand32(rs, 1 << 16), rs.randint(lo, hi + 1, size=1 << 16).astype(np.int64)])


def third_operands(rs):
    return np.concatenate([np.array([0, -1, 1, INT_MAX, INT_MIN], dtype=np.int64), _rand32(rs, 4)])


def ternary(name):
    rs = _rs(name)
    n = 1 << 17
    return _cat(_cross(E32, E32, third_operands(rs)), [_rand32(rs, n), _rand32(rs, n), _rand32(rs, n)])


def _shl_add(name):
    rs = _rs(name)
    n = 1 << 17
    return _cat(_cross(E32, np.arange(-64, 65, dtype=np.int64), third_operands(rs)), [_rand32(rs, n), _rand32(rs, n), _rand32(rs, n)])


def _shift31(name):
    rs = _rs(name)
    n = 1 << 17
    counts = np.arange(-31, 32, dtype=np.int64)
    outside = _w32([32, -32, 33, -33, 64, -64, INT_MAX, INT_MIN])            # violate the claim: for the host flags only
    return _cat(_cross(E32, counts), [_rand32(rs, n), rs.randint(-31, 32, size=n).astype(np.int64)], _cross(E32, outside))


def _pk_shift(name):
    rs = _rs(name)
    n = 1 << 17
    c = np.arange(16, dtype=np.int64)
    cl, ch = _cross(c, c)
    pairs = cl | (ch << 16)                                                   # every pair of per-half counts in [0, 15]^2
    return _cat(_cross(E32, pairs), [_rand32(rs, n), rs.randint(0, 16, size=n).astype(np.int64) | (rs.randint(0, 16, size=n).astype(np.int64) << 16)])


def _mean_step(name):
    rs = _rs(name)
    n = 1 << 17
    few = np.array([0, 1, 2, 15, 16, 30, 31], dtype=np.int64)
    small = np.array([0, 1, -1, 2, -2, INT_MAX, INT_MIN, INT_MIN + 1, 1 << 30], dtype=np.int64)
    v1, m1, f1 = _cross(E32, E32, few)
    v2, m2, f2 = _cross(E32, small, np.arange(32, dtype=np.int64))           # every factor 0..31
    return _cat([v1, f1, m1], [v2, f2, m2], [_rand32(rs, n), rs.randint(0, 32, size=n).astype(np.int64), _rand32(rs, n)])


def _divu_by_magic(name):
    rs = _rs(name)
    ns, ds = [], []
    for d in range(1, 66):                                                    # the bins' divisors
        ks = np.unique(np.concatenate([np.arange(1, 33), rs.randint(1, (1 << 31) // d + 1, size=32)])).astype(np.int64)
        n = np.concatenate([[0, 1, d - 1, d, (1 << 31) - 1, 1 << 31], ks * d - 1, ks * d, ks * d + 1, rs.randint(0, (1 << 31) + 1, size=2048, dtype=np.int64)])
        n = n[(n >= 0) & (n <= (1 << 31))]
        ns.append(n)
        ds.append(np.full(n.size, d, dtype=np.int64))
    # larger divisors of the stated range, at random
    n = rs.randint(0, (1 << 31) + 1, size=1 << 16, dtype=np.int64)
    ns.append(n)
    ds.append(rs.randint(1, (1 << 16) + 1, size=n.size).astype(np.int64))
    return [_w32(np.concatenate(ns)), np.concatenate(ds)]


def _asym_filt(step_pos, step_neg):
    def build(name):
        rs = _rs(name)
        old, new = _cross(E16, E16)
        near_old, near_new = [], []
        for delta in (1, -1, 1 << step_pos, -(1 << step_pos), 1 << step_neg, -(1 << step_neg)):
            near_old.append(E16)
            near_new.append(np.clip(E16 + delta, -32768, 32767))             # old +- 1, old +- 2^step, inside int16
        n = 1 << 16
        return _cat([old, new], [np.concatenate(near_old), np.concatenate(near_new)],
                    [rs.randint(-32768, 32768, size=n).astype(np.int64), rs.randint(-32768, 32768, size=n).astype(np.int64)])
    return build


def _log_energy(name):
    rs = _rs(name)
    n = 1 << 17
    e = np.concatenate([E32, sparse_words()])
    return _cat(_cross(e, np.arange(27, dtype=np.int64)), [_rand32(rs, n), rs.randint(0, 27, size=n).astype(np.int64)])


def _aligned_slot(name):
    return _cross(np.arange(0, kHistory + 1, dtype=np.int64), np.arange(0, kHistory, dtype=np.int64))


def _int16_exhaustive(name):
    return [np.arange(-32768, 32768, dtype=np.int64)]


def _mul24(name):
    rs = _rs(name)
    n = 1 << 17
    lim = 1 << 23
    return _cat(_cross(E32, E32), [_rand32(rs, 1 << 15), _rand32(rs, 1 << 15)],
                [rs.randint(-lim, lim, size=n).astype(np.int64), rs.randint(-lim, lim, size=n).astype(np.int64)])


_COUNT_OPS = ("shl", "sar", "lsr", "shift_i", "shift_u")
_UNARY_PACKED = ("pk_abs_sat_i16", "pk_neg_i16", "pk_nonzero_u16", "max_halves_i16")
UNIFORM_C = ("dot2_i16_uc", "mad16_lo_uc", "mad16_hi_uc")                    # the last operand is wave-uniform by contract

_BUILDERS = {
    **{n: (lambda name: binary_count(name, -64, 64)) for n in _COUNT_OPS},
    **{n: unary_packed for n in _UNARY_PACKED},
    "shl_add": _shl_add,
    "low_mask": lambda name: unary32(name, np.arange(-64, 65)),
    "shift_u31": _shift31, "shift_i31": _shift31,
    "checked_shift31": lambda name: unary32(name, np.tile(np.arange(-31, 32), 16)),      # only 63 values are inside the claim: 16 times each
    "pk_shl_b16": _pk_shift, "pk_lshr_b16": _pk_shift, "pk_ashr_i16": _pk_shift,
    "mean_step": _mean_step,
    "divu_by_magic": _divu_by_magic,
    "div_magic_magic": lambda name: [np.arange(1, (1 << 16) + 1, dtype=np.int64)],
    "div_magic_shift": lambda name: [np.arange(1, (1 << 16) + 1, dtype=np.int64)],
    "norm_w16": _int16_exhaustive, "norm_w16_nz": _int16_exhaustive,
    "as_i16": lambda name: unary32(name, np.arange(-32768, 32768)),
    "mul24": _mul24, "mul24_insn": _mul24,
    "log_energy_q8": _log_energy,
    "aligned_slot": _aligned_slot,
    "bitrev6": lambda name: unary32(name, np.arange(64)),
}
for _pos, _neg in ((11, 3), (8, 2), (4, 11), (2, 11)):
    _BUILDERS[f"asym_filt_{_pos}_{_neg}"] = _BUILDERS[f"asym_filt_lean_{_pos}_{_neg}"] = _asym_filt(_pos, _neg)

_i24 = lambda x: (x >= -(1 << 23)) & (x < (1 << 23))            # noqa: E731
# What the header checks (aecm_ops.h: the aecm_*_violation hooks on the host, g_aecm_check_fail in the audit build).
CLAIMS = {
    "mul24": lambda a, b, c: _i24(a) & _i24(b),
    "mul24_insn": lambda a, b, c: _i24(a) & _i24(b),
    "as_i16": lambda a, b, c: (a >= -32768) & (a <= 32767),
    "as_nonneg": lambda a, b, c: a >= 0,
    "norm_u32_nn": lambda a, b, c: a >= 0,
    "checked_shift31": lambda a, b, c: (a >= -31) & (a <= 31),
    "shift_u31": lambda a, b, c: (b >= -31) & (b <= 31),
    "shift_i31": lambda a, b, c: (b >= -31) & (b <= 31),
}
_is16 = lambda x: (x >= -32768) & (x <= 32767)                  # noqa: E731
_diff_wraps_to_int_min = lambda v, m: ((v - m) & 0xffffffff) == 0x80000000      # noqa: E731
# What the call sites guarantee and nothing checks.
DOMAINS = {
    # "an operand the caller knows to be non-zero -- or whose count it then ignores": the device branch has no zero fix-up
    "clz32_nz": lambda a, b, c: a != 0,
    # spl_inl.h:108: WebRtcSpl_NormW16 takes an int16_t; the header's formula is "for a in int16 range"
    "norm_w16": lambda a, b, c: _is16(a),
    "norm_w16_nz": lambda a, b, c: _is16(a),
    # "counts are < 16 at every call site" (the portable definition takes them modulo 16, the device's vector shift does not promise to)
    "pk_shl_b16": lambda a, b, c: ((b & 0xfff0fff0) == 0),
    "pk_lshr_b16": lambda a, b, c: ((b & 0xfff0fff0) == 0),
    "pk_ashr_i16": lambda a, b, c: ((b & 0xfff0fff0) == 0),
    # div_magic: "a small divisor 1 <= d <= 2^16"; divu_by_magic: "0 <= n <= 2^31"
    "div_magic_magic": lambda a, b, c: (a >= 1) & (a <= (1 << 16)),
    "div_magic_shift": lambda a, b, c: (a >= 1) & (a <= (1 << 16)),
    "divu_by_magic": lambda a, b, c: ((a >= 0) | (a == INT_MIN)) & (b >= 1) & (b <= (1 << 16)),
    # delay_estimator.cc:690-702: factor is a shift count (0..31).  A difference of exactly 2^31 makes the reference negate
    # INT_MIN, which C leaves undefined (the header's form gives -2^(31-factor) there, a wrapping negation +2^(31-factor)); the
    # one caller (binary_spectra, factor 6) passes v = mag << (15 - q) with mag <= 46340, in [0, 2^31), and a mean that starts at
    # v >> 1 or 0 and only ever moves towards such a v: the difference lies strictly inside (-2^31, 2^31)
    "mean_step": lambda a, b, c: (b >= 0) & (b <= 31) & ~_diff_wraps_to_int_min(a, c),
    # aecm_core.cc:588: int16_t filtOld, inVal (far-energy logs and their filtered extremes)
    **{f"asym_filt{lean}_{p}_{n}": (lambda a, b, c: _is16(a) & _is16(b)) for lean in ("", "_lean") for p, n in ((11, 3), (8, 2), (4, 11), (2, 11))},
    # the Q domains a valid state can hold: "for 0 <= q <= 26"
    "log_energy_q8": lambda a, b, c: (b >= 0) & (b <= 26),
    # hist_pos as update_far_history leaves it (0..kHistory, aecm_state_check.h), delay as effective_delay returns it
    "aligned_slot": lambda a, b, c: (a >= 0) & (a <= kHistory) & (b >= 0) & (b <= kHistory - 1),
}

# Cases every grid must hold (where they lie inside the entry's claim and domain): (a, b, c), None above the arity.
_H = -32768
NAMED = {
    "divi": [(5, 0, None), (-5, 0, None), (INT_MIN, 0, None), (INT_MIN, -1, None), (-7, 2, None), (7, -2, None)],
    "divu": [(5, 0, None), (-1, 0, None), (0, 0, None)],
    "norm_w32": [(0, None, None), (-1, None, None), (INT_MIN, None, None)],
    "norm_w32_nz": [(0, None, None), (-1, None, None), (INT_MIN, None, None)],
    "norm_w16": [(0, None, None), (-1, None, None), (_H, None, None)],
    "norm_w16_nz": [(0, None, None), (-1, None, None), (_H, None, None)],
    "ffbh_i": [(0, None, None), (-1, None, None)],
    "norm_u32_v": [(0, None, None)],
    "norm_u32": [(0, None, None)],
    "clz32": [(0, None, None)],
    "dot2_i16": [(-0x7fff8000, -0x7fff8000, -1), (-0x7fff8000, -0x7fff8000, 0)],      # 0x80008000: both halves -32768, 2^31 wraps
    "dot2_i16_uc": [(-0x7fff8000, -0x7fff8000, -1), (-0x7fff8000, -0x7fff8000, 0)],
    "dot2_i16_c0": [(-0x7fff8000, -0x7fff8000, None)],
    "dot2_i16_cm1": [(-0x7fff8000, -0x7fff8000, None)],
    "pk_neg_i16": [(-0x7fff8000, None, None), (0x8000, None, None), (INT_MIN, None, None)],
    "pk_abs_sat_i16": [(-0x7fff8000, None, None)],
    "add_sat32": [(INT_MAX, 1, None), (INT_MIN, -1, None), (INT_MAX, INT_MAX, None), (INT_MIN, INT_MIN, None)],
    "shift_i31": [(-1, 31, None), (-1, -31, None), (INT_MIN, -31, None), (1, 31, None)],
    "shift_u31": [(-1, 31, None), (-1, -31, None), (INT_MIN, -31, None), (1, 31, None)],
    "mean_step": [(INT_MAX, 1, -2), (INT_MIN + 1, 3, 5), (INT_MIN, 31, 1)],           # differences that wrap
}


def _mask(table, name, a, b, c):
    z = np.zeros_like(a)
    f = table.get(name)
    return np.ones(a.shape, dtype=bool) if f is None else np.asarray(f(a, z if b is None else b, z if c is None else c), dtype=bool)


@lru_cache(maxsize=None)
def _full_grid(name):
    k = arity(name)
    build = _BUILDERS.get(name) or {1: unary32, 2: binary, 3: ternary}[k]
    ops = [np.asarray(x, dtype=np.int64) for x in build(name)]
    assert len(ops) == k, name
    if name in UNIFORM_C:                                  # the kernel takes c of the first lane of each wave: one value per group of 64
        ops[2] = np.repeat(ops[2][::64], 64)[:ops[2].size]
    named = NAMED.get(name, [])
    if named:
        rep = 64 if name in UNIFORM_C else 1               # (a named case of a _uc form is a whole group of its own)
        head = [np.repeat(np.array([t[j] for t in named], dtype=np.int64), rep) for j in range(k)]
        ops = [np.concatenate([h, o]) for h, o in zip(head, ops)]
    ops += [None] * (3 - k)
    keep = _mask(DOMAINS, name, *ops)
    if name in UNIFORM_C:
        assert keep.all()
    ops = [None if o is None else o[keep] for o in ops]
    assert 0 < ops[0].size <= MAX_TUPLES, (name, ops[0].size)
    assert all(o is None or (o.min() >= INT_MIN and o.max() <= INT_MAX) for o in ops)
    out = tuple(None if o is None else np.ascontiguousarray(o, dtype=np.int32) for o in ops)
    for o in out:
        if o is not None:
            o.flags.writeable = False                      # shared by every test that asks for it
    return out


def full_grid(name):
    return _full_grid(name)


def claim_mask(name, a, b, c):
    """True where the tuple is inside what the header claims (and checks) for the entry."""
    w = [None if o is None else o.astype(np.int64) for o in (a, b, c)]
    return _mask(CLAIMS, name, *w)


def _select(name, inside):
    a, b, c = full_grid(name)
    m = claim_mask(name, a, b, c)
    m = m if inside else ~m
    if name in UNIFORM_C:
        assert m.all() == inside
    return tuple(None if o is None else np.ascontiguousarray(o[m]) for o in (a, b, c))


def admissible(name):
    """The tuples a shipped kernel may be given."""
    return _select(name, True)


def violating(name):
    """The tuples outside the entry's claim: for the host flags and the audit build."""
    return _select(name, False)
