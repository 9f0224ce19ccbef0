"""TEST INFRASTRUCTURE: an independent definition of every entry of webrtc_aecm_amd/csrc/aecm_ops_table.inc, keyed by name.

Written from the MEANING each function has -- the reference's lines that aecm_ops.h cites, or the one-line statement in the
function's comment -- in numpy int64 arithmetic on mathematical integers with explicit wrapping to 32 (16) bits, not from the C of
either branch of the header: this is what catches a host branch that is wrong.  Cited lines of the reference:
  aecm/spl_inl.h:59-111                           SatW32ToW16, AddSatW32, NormW32 / NormU32 / NormW16
  aecm/signal_processing_library.h:128            WEBRTC_SPL_SHIFT_W32
  aecm/signal_processing_library.cc:107-123       DivU32U16, DivW32W16
  aecm/delay_estimator.cc:690-702                 WebRtc_MeanEstimatorFix
  aecm/aecm_core.cc:588-605, 612-628, 157-172     AsymFilt, LogOfEnergyInQ8, AlignedFarend
Where the reference's C is undefined (a shift count outside 0..31, INT_MIN / -1, -INT_MIN) the header's opening comment is the
definition: two's complement wrap, 5-bit shift counts, arithmetic >> on signed.

Every function takes and returns int64 arrays that hold int32 values.  REF[name](a, b, c) for the tuples inside the entry's
precondition (tests/ops_grid.py); AUDIT_REF[name] is what the header promises of the audit build OUTSIDE it."""
from __future__ import annotations

import numpy as np

I64 = np.int64
INT_MIN, INT_MAX = -(1 << 31), (1 << 31) - 1
kHistory = 100          # aecm_state.h (MAX_DELAY, aecm_defines.h:26)


def w32(x):
    """The integer x (|x| < 2^62) as the int32 with the same low 32 bits."""
    x = np.asarray(x, dtype=I64)
    return ((x + (1 << 31)) & 0xffffffff) - (1 << 31)


def u32(x):
    return np.asarray(x, dtype=I64) & 0xffffffff


def s16(x):
    """The low 16 bits as a signed number."""
    return ((np.asarray(x, dtype=I64) & 0xffff) ^ 0x8000) - 0x8000


def u16(x):
    return np.asarray(x, dtype=I64) & 0xffff


def lo(x):
    return s16(x)


def hi(x):
    return s16(np.asarray(x, dtype=I64) >> 16)


def ulo(x):
    return u16(x)


def uhi(x):
    return u16(np.asarray(x, dtype=I64) >> 16)


def pack(l, h):
    """Two 16-bit halves (any integers: their low 16 bits) as one int32 word."""
    return w32(u16(l) | (u16(h) << 16))


def bit_length(x):
    """Of 0 <= x < 2^32."""
    x = np.array(x, dtype=I64)
    n = np.zeros_like(x)
    for s in (16, 8, 4, 2, 1):
        m = (x >> s) != 0
        n += np.where(m, s, 0)
        x = np.where(m, x >> s, x)
    return n + (x != 0)


def lead_zeros(x):
    """Leading zero bits of the 32-bit word, 32 for 0 (spl_inl.h:40-47)."""
    return 32 - bit_length(u32(x))


def sign_run(x):
    """The number of leading bits equal to the sign bit (bit 31 included): 32 for 0 and -1."""
    return lead_zeros(np.where(x < 0, ~x, x))


def trunc_div(a, b):
    """a / b rounded toward zero, b != 0 (mathematical integers)."""
    q = np.abs(a) // np.abs(b)
    return np.where((a < 0) != (b < 0), -q, q)


def obj(x):
    return np.asarray(x, dtype=I64).astype(object)


def from_obj(x):
    return np.array([int(v) for v in x], dtype=I64) if len(x) else np.zeros(0, dtype=I64)


def mulhi_u(a, b):
    """floor(u32(a) * u32(b) / 2^32), the products in unbounded integers."""
    return from_obj((obj(u32(a)) * obj(u32(b))) >> 32)


def shift5(n):
    return np.asarray(n, dtype=I64) & 31


def shl(a, n):
    return w32(u32(a) << shift5(n))


def sar(a, n):
    return np.asarray(a, dtype=I64) >> shift5(n)


def lsr(a, n):
    return w32(u32(a) >> shift5(n))


def dot2(a, b, c):
    return w32(lo(a) * lo(b) + hi(a) * hi(b) + c)


def shift_w32(x, c, right):
    """WEBRTC_SPL_SHIFT_W32: x * 2^c for c >= 0, x >> -c otherwise; counts taken modulo 32."""
    return np.where(c >= 0, shl(x, c), right(x, -c))


def shift31(x, c, signed):
    """The same for -31 <= c <= 31, on integers: floor(x * 2^c) of the (un)signed x, low 32 bits."""
    x = obj(x if signed else u32(x))
    c = np.asarray(c, dtype=I64)
    r = [(int(v) << int(k)) if k >= 0 else (int(v) >> int(-k)) for v, k in zip(x, c)]
    return w32(np.array([v & 0xffffffff for v in r], dtype=I64))


def norm_w32(a):
    return np.where(a == 0, 0, sign_run(a) - 1)            # spl_inl.h:96-98


def norm_w16(a):
    return np.where(a == 0, 0, sign_run(a) - 17)           # spl_inl.h:108-111 (a an int16)


def div_magic(d):
    """(L, M - 2^32) with L = ceil(log2 d), M = ceil(2^(32+L) / d), 1 <= d <= 2^16 (the comment of div_magic)."""
    d = np.asarray(d, dtype=I64)
    L = bit_length(d - 1)                                  # ceil(log2 d): bits of d - 1
    M = from_obj(-((-(obj(np.ones_like(d)) << obj(32 + L))) // obj(d)))
    return L, M - (1 << 32)


def mean_step(value, factor, mean):
    """delay_estimator.cc:690-702: the difference's magnitude is shifted."""
    diff = w32(value - mean)
    step = np.where(diff < 0, -((-diff) >> factor), diff >> factor)
    return w32(mean + step)


def asym_filt(step_pos, step_neg):
    def f(old, new, _c=None):                              # aecm_core.cc:588-605, old and new int16
        down = s16(old - ((old - new) >> step_neg))
        up = s16(old + ((new - old) >> step_pos))
        return np.where((old == 32767) | (old == -32768), new, np.where(old > new, down, up))
    return f


def log_energy_q8(energy, q):
    """aecm_core.cc:612-628: (7 << 7) + log2(energy) in Q8 with a linear fraction, minus q << 8; (7 << 7) for energy == 0."""
    e = u32(energy)
    zeros = np.where(e == 0, 0, lead_zeros(e))
    frac = ((e << zeros) & 0x7fffffff) >> 23
    return np.where(e > 0, s16((7 << 7) + ((31 - zeros) << 8) + frac - (q << 8)), 7 << 7)


def bitrev6(t):
    r = np.zeros_like(t)
    for k in range(6):
        r |= ((t >> k) & 1) << (5 - k)
    return r


def sext24(x):
    return ((np.asarray(x, dtype=I64) & 0xffffff) ^ 0x800000) - 0x800000


def per_half(f, signed):
    """A packed op from its per-half meaning f(x, y[, z]) on the signed / unsigned halves."""
    lo_, hi_ = (lo, hi) if signed else (ulo, uhi)

    def g(a, b=None, c=None):
        args_lo = [lo_(v) for v in (a, b, c) if v is not None]
        args_hi = [hi_(v) for v in (a, b, c) if v is not None]
        return pack(f(*args_lo), f(*args_hi))
    return g


def _sat16(v):
    return np.clip(v, -32768, 32767)


REF = {
    "shl": lambda a, b, c: shl(a, b),
    "sar": lambda a, b, c: sar(a, b),
    "lsr": lambda a, b, c: lsr(a, b),
    "mul": lambda a, b, c: w32(a * b),
    "add": lambda a, b, c: w32(a + b),
    "sub": lambda a, b, c: w32(a - b),
    "neg": lambda a, b, c: w32(-a),
    "sext16": lambda a, b, c: s16(a),
    "shl_add": lambda a, b, c: w32(shl(a, b) + c),
    "zext16": lambda a, b, c: u16(a),
    "sel": lambda a, b, c: np.where(a != 0, b, c),
    "imin": lambda a, b, c: np.minimum(a, b),
    "imax": lambda a, b, c: np.maximum(a, b),
    "iabs": lambda a, b, c: w32(np.abs(a)),
    "ltu": lambda a, b, c: (u32(a) < u32(b)).astype(I64),
    "gtu": lambda a, b, c: (u32(a) > u32(b)).astype(I64),
    "clz32": lambda a, b, c: lead_zeros(a),
    "clz32_nz": lambda a, b, c: lead_zeros(a),                               # a != 0
    "popc": lambda a, b, c: sum(((u32(a) >> k) & 1) for k in range(32)),
    # signal_processing_library.cc:107-123; INT_MIN / -1 = 2^31 wraps to INT_MIN
    "divi": lambda a, b, c: np.where(b == 0, INT_MAX, w32(trunc_div(a, np.where(b == 0, 1, b)))),
    "divu": lambda a, b, c: np.where(b == 0, -1, w32(u32(a) // np.where(b == 0, 1, u32(b)))),
    "mul24": lambda a, b, c: w32(a * b),                                     # both operands inside 24 signed bits
    "mul24_insn": lambda a, b, c: w32(a * b),
    "mul24_insn_raw": lambda a, b, c: w32(sext24(a) * sext24(b)),            # the instruction: the low 24 bits of each operand
    "as_i16": lambda a, b, c: a,
    "as_nonneg": lambda a, b, c: a,
    "dot2_i16": dot2,
    "dot2_i16_c0": lambda a, b, c: dot2(a, b, 0),
    "dot2_i16_cm1": lambda a, b, c: dot2(a, b, -1),
    "dot2_i16_uc": dot2,
    "mad16_lo": lambda a, b, c: w32(lo(a) * lo(b) + c),
    "mad16_hi": lambda a, b, c: w32(hi(a) * lo(b) + c),
    "mad16_lo_uc": lambda a, b, c: w32(lo(a) * lo(b) + c),
    "mad16_hi_uc": lambda a, b, c: w32(hi(a) * lo(b) + c),
    "pack_hi16": lambda a, b, c: pack(uhi(a), uhi(b)),
    "pk_abs_sat_i16": lambda a, b, c: per_half(lambda x: np.minimum(np.abs(x), 32767), True)(a),
    "pk_neg_i16": lambda a, b, c: per_half(lambda x: -x, True)(a),
    "pk_add_i16": lambda a, b, c: per_half(lambda x, y: x + y, True)(a, b),
    "pk_sub_i16": lambda a, b, c: per_half(lambda x, y: x - y, True)(a, b),
    "pk_mul_lo_u16": lambda a, b, c: per_half(lambda x, y: x * y, False)(a, b),
    "pk_shl_b16": lambda a, b, c: per_half(lambda x, y: x << (y & 15), False)(a, b),       # counts < 16 at every call site
    "pk_lshr_b16": lambda a, b, c: per_half(lambda x, y: x >> (y & 15), False)(a, b),
    "pk_ashr_i16": lambda a, b, c: per_half(lambda x, y: x >> (y & 15), True)(a, b),
    "pk_min_u16": lambda a, b, c: per_half(np.minimum, False)(a, b),
    "pk_mad_u16": lambda a, b, c: per_half(lambda x, y, z: x * y + z, False)(a, b, c),
    "pk_nonzero_u16": lambda a, b, c: per_half(lambda x: (x != 0).astype(I64), False)(a),
    "opaque_v": lambda a, b, c: a,
    "pk_max_i16": lambda a, b, c: per_half(np.maximum, True)(a, b),
    "pk_add_u16": lambda a, b, c: per_half(lambda x, y: x + y, False)(a, b),
    "pk_max_u16": lambda a, b, c: per_half(np.maximum, False)(a, b),
    "pk_sub_sat_u16": lambda a, b, c: per_half(lambda x, y: np.maximum(x - y, 0), False)(a, b),
    "pk_add_sat_i16": lambda a, b, c: per_half(lambda x, y: _sat16(x + y), True)(a, b),
    "max_halves_i16": lambda a, b, c: np.maximum(lo(a), hi(a)),
    # v_ffbh_i32: the leading bits equal to the sign bit, -1 when all 32 are (0 and -1)
    "ffbh_i": lambda a, b, c: np.where((a == 0) | (a == -1), -1, sign_run(a)),
    "norm_u32": lambda a, b, c: np.where(a == 0, 0, lead_zeros(a)),          # spl_inl.h:102-104
    "norm_u32_v": lambda a, b, c: np.where(a == 0, 0, lead_zeros(a)),
    "min_u32": lambda a, b, c: np.where(u32(a) < u32(b), a, b),
    "norm_u32_nn": lambda a, b, c: np.where(a == 0, 0, lead_zeros(a)),       # a >= 0 as a signed number
    "norm_w32": lambda a, b, c: norm_w32(a),
    "norm_w16": lambda a, b, c: norm_w16(a),
    "norm_w32_nz": lambda a, b, c: np.where(a == 0, 31, norm_w32(a)),        # "as many redundant sign bits as there can be" for 0
    "norm_w16_nz": lambda a, b, c: np.where(a == 0, 15, norm_w16(a)),
    "mulhi_i32": lambda a, b, c: (a * b) >> 32,
    "mulhi_u32": lambda a, b, c: w32(mulhi_u(a, b)),
    "div_magic_magic": lambda a, b, c: w32(div_magic(a)[1]),
    "div_magic_shift": lambda a, b, c: div_magic(a)[0],
    "divu_by_magic": lambda a, b, c: w32(u32(a) // b),                       # floor(n / d), 0 <= n <= 2^31, 1 <= d <= 2^16
    "add_sat32": lambda a, b, c: np.clip(a + b, INT_MIN, INT_MAX),           # spl_inl.h:70-82
    "sat16": lambda a, b, c: _sat16(a),                                      # spl_inl.h:59-68
    "shift_i": lambda a, b, c: shift_w32(a, b, sar),
    "shift_u": lambda a, b, c: shift_w32(a, b, lsr),
    "checked_shift31": lambda a, b, c: a,
    "shift_u31": lambda a, b, c: shift31(a, b, False),
    "shift_i31": lambda a, b, c: shift31(a, b, True),
    "low_mask": lambda a, b, c: w32((I64(1) << shift5(a)) - 1),
    "mean_step": mean_step,
    "asym_filt_11_3": asym_filt(11, 3),
    "asym_filt_8_2": asym_filt(8, 2),
    "asym_filt_4_11": asym_filt(4, 11),
    "asym_filt_2_11": asym_filt(2, 11),
    "asym_filt_lean_11_3": asym_filt(11, 3),
    "asym_filt_lean_8_2": asym_filt(8, 2),
    "asym_filt_lean_4_11": asym_filt(4, 11),
    "asym_filt_lean_2_11": asym_filt(2, 11),
    "log_energy_q8": lambda a, b, c: log_energy_q8(a, b),
    # aecm_core.cc:157-172: far_history_pos - delay, plus MAX_DELAY if negative
    "aligned_slot": lambda a, b, c: np.where(a - b < 0, a - b + kHistory, a - b),
    "bitrev6": lambda a, b, c: bitrev6(a & 63),
}

# What the audit build (-DAECM_CHECKED) returns for a tuple OUTSIDE the claimed range, as aecm_ops.h states it: the exact result.
AUDIT_REF = {
    "mul24": lambda a, b, c: w32(a * b),                   # "computes the exact result": mul(a, b)
    "as_i16": lambda a, b, c: s16(a),                      # "what the reference's (int16_t) cast does"
    "as_nonneg": lambda a, b, c: a,
    "checked_shift31": lambda a, b, c: a,
}


def evaluate(name, a, b=None, c=None, table=REF):
    a = np.asarray(a, dtype=I64)
    z = np.zeros_like(a)
    r = table[name](a, z if b is None else np.asarray(b, dtype=I64), z if c is None else np.asarray(c, dtype=I64))
    r = np.asarray(r, dtype=I64)
    assert r.shape == a.shape and (r >= INT_MIN).all() and (r <= INT_MAX).all(), name
    return r.astype(np.int32)
