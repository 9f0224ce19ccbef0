// The one list of the fixed-point primitives that the ops probe evaluates: every function of aecm_ops.h and the plain-integer
// helpers of aecm_wave.h with closed definitions.  Two includers expand it -- the device kernel (aecm_ops_probe_kernels.hip: the
// DEVICE branch of each primitive, as builtins and inline assembly) and the host library of the test suite (tests/sim/sim_ops.cpp:
// the HOST branch, the one the lane simulator runs) -- so the two sides cannot list different functions; tests/test_ops_probe.py
// holds the list against aecm_ops.h itself and against the independent definitions of tests/ops_ref.py.
//
//   AECM_OP(id, name, arity, call)     ids are dense from 0 in list order; the call is an int expression of the int operands
//                                      a, b, c (the first `arity` of them), in namespace aecm
//
// The includer defines, before it includes this file with AECM_OPS_TABLE_HELPERS set (once, at namespace scope, outside
// namespace aecm) and again wherever it expands the list:
//   AECM_OPS_ENGINE        BlockEngine<policy, false> of the non-lean block loop  (device: Gfx950Wave<true>, host: the simulator's)
//   AECM_OPS_ENGINE_LEAN   the same with the lean forms on                        (device: the chunk queue's policy)
//   AECM_OPS_VI(x)         the int x as the policy's lane vector;  AECM_OPS_LANE0(v)  a lane vector's (uniform) value as an int
//   AECM_OPS_UNIFORM(x)    x as a wave-uniform value: the addend of the _uc forms, an SGPR operand by their contract
//                          (device: the first active lane's x; host: x)
//
// Preconditions (the range a call site guarantees) are not stated here: tests/ops_grid.py names one predicate per entry and
// drops the tuples outside it before a shipped kernel sees them.
#if defined(AECM_OPS_TABLE_HELPERS)
namespace aecm {
// the (magic, shift) pair of a divisor, one result per entry
AECM_HD int ops_div_magic_magic(int d) { int m, s; div_magic(d, &m, &s); return m; }
AECM_HD int ops_div_magic_shift(int d) { int m, s; div_magic(d, &m, &s); return s; }
// floor(n / d) through the pair div_magic gives for d
AECM_HD int ops_divu_by_magic(int n, int d) { int m, s; div_magic(d, &m, &s); return divu_by_magic(n, m, s); }
// v_mul_i32_i24 on any operands: the instruction reads the low 24 bits of each.  The host branch (and the audit build) of
// mul24_insn states the product for operands inside 24 signed bits only, so there the operands are narrowed first.
AECM_HD int ops_mul24_insn_raw(int a, int b) {
#if defined(__HIP_DEVICE_COMPILE__) && !defined(AECM_CHECKED)
    return mul24_insn(a, b);
#else
    return mul24_insn(sar(shl(a, 8), 8), sar(shl(b, 8), 8));
#endif
}
}  // namespace aecm
#else
AECM_OP(0, shl, 2, shl(a, b))
AECM_OP(1, sar, 2, sar(a, b))
AECM_OP(2, lsr, 2, lsr(a, b))
AECM_OP(3, mul, 2, mul(a, b))
AECM_OP(4, add, 2, add(a, b))
AECM_OP(5, sub, 2, sub(a, b))
AECM_OP(6, neg, 1, neg(a))
AECM_OP(7, sext16, 1, sext16(a))
AECM_OP(8, shl_add, 3, shl_add(a, b, c))
AECM_OP(9, zext16, 1, zext16(a))
AECM_OP(10, sel, 3, sel(a != 0, b, c))
AECM_OP(11, imin, 2, imin(a, b))
AECM_OP(12, imax, 2, imax(a, b))
AECM_OP(13, iabs, 1, iabs(a))
AECM_OP(14, ltu, 2, (int)ltu(a, b))
AECM_OP(15, gtu, 2, (int)gtu(a, b))
AECM_OP(16, clz32, 1, clz32(a))
AECM_OP(17, clz32_nz, 1, clz32_nz(a))
AECM_OP(18, popc, 1, popc(a))
AECM_OP(19, divi, 2, divi(a, b))
AECM_OP(20, divu, 2, divu(a, b))
AECM_OP(21, mul24, 2, mul24(a, b))
AECM_OP(22, mul24_insn, 2, mul24_insn(a, b))
AECM_OP(23, mul24_insn_raw, 2, ops_mul24_insn_raw(a, b))
AECM_OP(24, as_i16, 1, as_i16(a))
AECM_OP(25, as_nonneg, 1, as_nonneg(a))
AECM_OP(26, dot2_i16, 3, dot2_i16(a, b, c))
AECM_OP(27, dot2_i16_c0, 2, dot2_i16_c0(a, b))
AECM_OP(28, dot2_i16_cm1, 2, dot2_i16_cm1(a, b))
AECM_OP(29, dot2_i16_uc, 3, dot2_i16_uc(a, b, AECM_OPS_UNIFORM(c)))
AECM_OP(30, mad16_lo, 3, mad16_lo(a, b, c))
AECM_OP(31, mad16_hi, 3, mad16_hi(a, b, c))
AECM_OP(32, mad16_lo_uc, 3, mad16_lo_uc(a, b, AECM_OPS_UNIFORM(c)))
AECM_OP(33, mad16_hi_uc, 3, mad16_hi_uc(a, b, AECM_OPS_UNIFORM(c)))
AECM_OP(34, pack_hi16, 2, pack_hi16(a, b))
AECM_OP(35, pk_abs_sat_i16, 1, pk_abs_sat_i16(a))
AECM_OP(36, pk_neg_i16, 1, pk_neg_i16(a))
AECM_OP(37, pk_add_i16, 2, pk_add_i16(a, b))
AECM_OP(38, pk_sub_i16, 2, pk_sub_i16(a, b))
AECM_OP(39, pk_mul_lo_u16, 2, pk_mul_lo_u16(a, b))
AECM_OP(40, pk_shl_b16, 2, pk_shl_b16(a, b))
AECM_OP(41, pk_lshr_b16, 2, pk_lshr_b16(a, b))
AECM_OP(42, pk_ashr_i16, 2, pk_ashr_i16(a, b))
AECM_OP(43, pk_min_u16, 2, pk_min_u16(a, b))
AECM_OP(44, pk_mad_u16, 3, pk_mad_u16(a, b, c))
AECM_OP(45, pk_nonzero_u16, 1, pk_nonzero_u16(a))
AECM_OP(46, opaque_v, 1, opaque_v(a))
AECM_OP(47, pk_max_i16, 2, pk_max_i16(a, b))
AECM_OP(48, pk_add_u16, 2, pk_add_u16(a, b))
AECM_OP(49, pk_max_u16, 2, pk_max_u16(a, b))
AECM_OP(50, pk_sub_sat_u16, 2, pk_sub_sat_u16(a, b))
AECM_OP(51, pk_add_sat_i16, 2, pk_add_sat_i16(a, b))
AECM_OP(52, max_halves_i16, 1, max_halves_i16(a))
AECM_OP(53, ffbh_i, 1, ffbh_i(a))
AECM_OP(54, norm_u32, 1, norm_u32(a))
AECM_OP(55, norm_u32_v, 1, norm_u32_v(a))
AECM_OP(56, min_u32, 2, min_u32(a, b))
AECM_OP(57, norm_u32_nn, 1, norm_u32_nn(a))
AECM_OP(58, norm_w32, 1, norm_w32(a))
AECM_OP(59, norm_w16, 1, norm_w16(a))
AECM_OP(60, norm_w32_nz, 1, norm_w32_nz(a))
AECM_OP(61, norm_w16_nz, 1, norm_w16_nz(a))
AECM_OP(62, mulhi_i32, 2, mulhi_i32(a, b))
AECM_OP(63, mulhi_u32, 2, mulhi_u32(a, b))
AECM_OP(64, div_magic_magic, 1, ops_div_magic_magic(a))
AECM_OP(65, div_magic_shift, 1, ops_div_magic_shift(a))
AECM_OP(66, divu_by_magic, 2, ops_divu_by_magic(a, b))
AECM_OP(67, add_sat32, 2, add_sat32(a, b))
AECM_OP(68, sat16, 1, sat16(a))
AECM_OP(69, shift_i, 2, shift_i(a, b))
AECM_OP(70, shift_u, 2, shift_u(a, b))
AECM_OP(71, checked_shift31, 1, checked_shift31(a))
AECM_OP(72, shift_u31, 2, shift_u31(a, b))
AECM_OP(73, shift_i31, 2, shift_i31(a, b))
AECM_OP(74, low_mask, 1, low_mask(a))
AECM_OP(75, mean_step, 3, mean_step(a, b, c))                   // (value, factor, mean)
// aecm_wave.h.  asym_filt(old, in): one entry per (step_pos, step_neg) pair calc_energies passes -- far-energy minimum
// (11, 3) and maximum (4, 11), and (8, 2) / (2, 11) during start-up -- in the plain and in the lean block loop.
AECM_OP(76, asym_filt_11_3, 2, AECM_OPS_ENGINE::asym_filt(a, b, 11, 3))
AECM_OP(77, asym_filt_8_2, 2, AECM_OPS_ENGINE::asym_filt(a, b, 8, 2))
AECM_OP(78, asym_filt_4_11, 2, AECM_OPS_ENGINE::asym_filt(a, b, 4, 11))
AECM_OP(79, asym_filt_2_11, 2, AECM_OPS_ENGINE::asym_filt(a, b, 2, 11))
AECM_OP(80, asym_filt_lean_11_3, 2, AECM_OPS_ENGINE_LEAN::asym_filt(a, b, 11, 3))
AECM_OP(81, asym_filt_lean_8_2, 2, AECM_OPS_ENGINE_LEAN::asym_filt(a, b, 8, 2))
AECM_OP(82, asym_filt_lean_4_11, 2, AECM_OPS_ENGINE_LEAN::asym_filt(a, b, 4, 11))
AECM_OP(83, asym_filt_lean_2_11, 2, AECM_OPS_ENGINE_LEAN::asym_filt(a, b, 2, 11))
AECM_OP(84, log_energy_q8, 2, AECM_OPS_ENGINE::log_energy_q8(a, b))            // (energy, q)
AECM_OP(85, aligned_slot, 2, AECM_OPS_ENGINE::aligned_slot(a, b))              // (hist_pos, delay)
AECM_OP(86, bitrev6, 1, AECM_OPS_LANE0(AECM_OPS_ENGINE::bitrev6(AECM_OPS_VI(a))))
#endif
