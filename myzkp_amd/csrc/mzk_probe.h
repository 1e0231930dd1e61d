// mzk_probe.h -- the arithmetic probe: ONE device function per call on raw limbs, nothing else.
//
// TEST SURFACE.  Operands arrive as raw u32 limbs (P::L per field element, whatever representation the caller chose: lazy,
// signed, un-normalised), the result leaves as the raw limbs the function returned -- no reduction, packing or comparison on the
// way; the judgement is made in Python integers (tests/arith_model.py).  The per-lane forms below are plain C++ over
// mzk_field.h / mzk_ec.h / mzk_g2.h, so the SAME text is compiled by hipcc for the device (mzk_probe.hip, mzk_selftest_field_probe /
// mzk_selftest_g1_probe / mzk_selftest_g2_probe) and by g++ for the bounds-checked host build (tests/hostcheck: hc_field_probe /
// hc_g1_probe / hc_g2_probe), and both sides read the same case table (G2: tests/g2_model.py).  The asm, quad, row and wave forms exist only on the device and live in mzk_probe.hip.
#pragma once
#include "mzk_ec.h"
#include "mzk_g2.h"

namespace mzk {

// field ops (numbering = MZK_PROBE_* of include/mzk.h)
enum {
  PR_MUL = 0, PR_SQR = 1, PR_MUL_ADD2 = 2, PR_SHOUP_MUL = 3, PR_SMUL = 4, PR_SMUL_C1 = 5,
  PR_SADD = 6, PR_SSUB = 7, PR_SCARRY = 8, PR_SBIAS = 9, PR_SREDUCE = 10,
  PR_ADD = 11, PR_SUB4 = 12, PR_SUB8 = 13, PR_NEG_LAZY4 = 14, PR_NEG_LAZY8 = 15, PR_DBL = 16, PR_CARRY = 17,
  PR_WEAK_REDUCE = 18, PR_REDUCE = 19, PR_COND_SUB_P = 20, PR_NEG_CANON = 21,
  PR_IS_ZERO_MOD6 = 22, PR_IS_ZERO_MOD10 = 23, PR_IS_ZERO_MOD12 = 24, PR_INV = 25,
  PR_FIELD_OPS = 26
};
enum { PR_FORM_CPP = 0, PR_FORM_ASM = 1, PR_FORM_QUAD = 2, PR_FORM_ROW = 3, PR_FORM_WAVE = 4 };
// group ops
enum { PR_G1_MADD_SIGNED = 0, PR_G1_MADD = 1, PR_G1_ADD = 2, PR_G1_DBL = 3, PR_G1_DBL_AFFINE = 4, PR_G1_TO_AFFINE = 5, PR_G1_OPS = 6 };
constexpr int PR_SLOT = 4 * FqParams::L;      // an XYZZ operand / result: 4 x 9 raw limbs, coordinate-major, all-zero = infinity
constexpr int PR_AFF = 2 * FqParams::L;       // an affine operand: 2 x 9 limbs, Montgomery form, canonical

// operands per case
MZK_HD constexpr int probe_field_arity(int op) {
  return op == PR_MUL_ADD2 ? 4 : op == PR_SHOUP_MUL ? 3
       : (op == PR_MUL || op == PR_SMUL || op == PR_SMUL_C1 || op == PR_SADD || op == PR_SSUB || op == PR_ADD || op == PR_SUB4 || op == PR_SUB8) ? 2 : 1;
}
// which ops a field has: the signed lazy family is the sparse modulus's, the precomputed-quotient product BN254 Fr's
template <class P> MZK_HD constexpr bool probe_field_has(int op) {
  if (op < 0 || op >= PR_FIELD_OPS) return false;
  if (op >= PR_SMUL && op <= PR_SREDUCE) return SparseMod<P>::value;
  if (op == PR_SHOUP_MUL) return P::L == 9 && P::P[0] == 0x10000001u;
  return true;
}

template <class P> MZK_HD Fe<P> probe_ld(const u32* w) {
  Fe<P> r;
#pragma unroll
  for (int i = 0; i < P::L; i++) r.l[i] = w[i];
  return r;
}
template <class P> MZK_HD void probe_st(const Fe<P>& a, u32* w) {
#pragma unroll
  for (int i = 0; i < P::L; i++) w[i] = a.l[i];
}
template <class P> MZK_HD void probe_st_flag(bool f, u32* w) {
#pragma unroll
  for (int i = 0; i < P::L; i++) w[i] = 0;
  w[0] = f ? 1u : 0u;
}

// the portable form of field op OP: in = arity x L limbs, out = L limbs (the zero tests: out[0] = 0 / 1)
template <class P, int OP> MZK_HD void probe_field_cpp(const u32* in, u32* out) {
  constexpr int L = P::L;
  const Fe<P> a = probe_ld<P>(in);
  if constexpr (OP == PR_MUL) probe_st<P>(fe_mul<P>(a, probe_ld<P>(in + L)), out);
  else if constexpr (OP == PR_SQR) probe_st<P>(fe_sqr<P>(a), out);
  else if constexpr (OP == PR_MUL_ADD2) probe_st<P>(fe_mul_add2<P>(a, probe_ld<P>(in + L), probe_ld<P>(in + 2 * L), probe_ld<P>(in + 3 * L)), out);
  else if constexpr (OP == PR_SHOUP_MUL) probe_st<P>(fe_shoup_mul<P>(a, in + L, in + 2 * L), out);
  else if constexpr (OP == PR_SMUL) probe_st<P>(fe_mul_sparse<P, true, 0>(a, probe_ld<P>(in + L)), out);
  else if constexpr (OP == PR_SMUL_C1) probe_st<P>(fe_mul_sparse<P, true, 1>(a, probe_ld<P>(in + L)), out);
  else if constexpr (OP == PR_SADD) probe_st<P>(fe_sadd<P>(a, probe_ld<P>(in + L)), out);
  else if constexpr (OP == PR_SSUB) probe_st<P>(fe_ssub<P>(a, probe_ld<P>(in + L)), out);
  else if constexpr (OP == PR_SCARRY) probe_st<P>(fe_scarry<P>(a), out);
  else if constexpr (OP == PR_SBIAS) probe_st<P>(fe_sbias<P>(a), out);
  else if constexpr (OP == PR_SREDUCE) probe_st<P>(fe_sreduce<P>(a), out);
  else if constexpr (OP == PR_ADD) probe_st<P>(fe_add<P>(a, probe_ld<P>(in + L)), out);
  else if constexpr (OP == PR_SUB4) probe_st<P>(fe_sub<P, 4>(a, probe_ld<P>(in + L)), out);
  else if constexpr (OP == PR_SUB8) probe_st<P>(fe_sub<P, 8>(a, probe_ld<P>(in + L)), out);
  else if constexpr (OP == PR_NEG_LAZY4) probe_st<P>(fe_neg_lazy<P, 4>(a), out);
  else if constexpr (OP == PR_NEG_LAZY8) probe_st<P>(fe_neg_lazy<P, 8>(a), out);
  else if constexpr (OP == PR_DBL) probe_st<P>(fe_dbl<P>(a), out);
  else if constexpr (OP == PR_CARRY) probe_st<P>(fe_carry<P>(a), out);
  else if constexpr (OP == PR_WEAK_REDUCE) probe_st<P>(fe_weak_reduce<P>(a), out);
  else if constexpr (OP == PR_REDUCE) probe_st<P>(fe_reduce<P>(a), out);
  else if constexpr (OP == PR_COND_SUB_P) probe_st<P>(fe_cond_sub_p<P>(a), out);
  else if constexpr (OP == PR_NEG_CANON) probe_st<P>(fe_neg_canon<P>(a), out);
  else if constexpr (OP == PR_IS_ZERO_MOD6) probe_st_flag<P>(fe_is_zero_mod<P, 6>(a), out);
  else if constexpr (OP == PR_IS_ZERO_MOD10) probe_st_flag<P>(fe_is_zero_mod<P, 10>(a), out);
  else if constexpr (OP == PR_IS_ZERO_MOD12) probe_st_flag<P>(fe_is_zero_mod<P, 12>(a), out);
  else if constexpr (OP == PR_INV) probe_st<P>(fe_inv_safegcd<P>(a), out);
}

MZK_HD Xyzz probe_ld_slot(const u32* w) {
  Xyzz p;
  p.X = probe_ld<FqParams>(w); p.Y = probe_ld<FqParams>(w + 9); p.ZZ = probe_ld<FqParams>(w + 18); p.ZZZ = probe_ld<FqParams>(w + 27);
  return p;
}
MZK_HD Affine probe_ld_affine(const u32* w) {
  Affine a;
  a.x = probe_ld<FqParams>(w); a.y = probe_ld<FqParams>(w + 9);
  return a;
}
// the limbs the function returned; infinity as all-zero (what xyzz_gstore_raw writes)
MZK_HD void probe_st_slot(const Xyzz& p, u32* w) {
  const bool inf = xyzz_is_inf(p);
#pragma unroll
  for (int i = 0; i < 9; i++) {
    w[i] = inf ? 0u : p.X.l[i]; w[9 + i] = inf ? 0u : p.Y.l[i]; w[18 + i] = inf ? 0u : p.ZZ.l[i]; w[27 + i] = inf ? 0u : p.ZZZ.l[i];
  }
}
// the single-lane forms of group op OP with the product routines A (FeCpp; FeAsm on the device): a = slot (dbl_affine: affine),
// b = slot (add) or affine (madd, madd_signed); out = one slot.  to_affine: 16 plain ABI words x || y (all-zero = infinity), rest 0.
template <int OP, template <class> class A> MZK_HD void probe_g1_lane(const u32* a, const u32* b, bool neg, u32* out) {
  if constexpr (OP == PR_G1_MADD_SIGNED) probe_st_slot(xyzz_madd_signed_with<A>(probe_ld_slot(a), probe_ld_affine(b), neg), out);
  else if constexpr (OP == PR_G1_MADD) probe_st_slot(xyzz_madd_with<A>(probe_ld_slot(a), probe_ld_affine(b)), out);
  else if constexpr (OP == PR_G1_ADD) probe_st_slot(xyzz_add_with<A>(probe_ld_slot(a), probe_ld_slot(b)), out);
  else if constexpr (OP == PR_G1_DBL) probe_st_slot(xyzz_dbl_with<A>(probe_ld_slot(a)), out);
  else if constexpr (OP == PR_G1_DBL_AFFINE) probe_st_slot(xyzz_dbl_affine(probe_ld_affine(a)), out);
  else if constexpr (OP == PR_G1_TO_AFFINE) {
    Affine af;
#pragma unroll
    for (int i = 0; i < PR_SLOT; i++) out[i] = 0;
    if (xyzz_to_affine<true>(probe_ld_slot(a), &af)) affine_store_plain(af, out);
  }
}

// ---- G2 (mzk_g2.h): Fq2 and the XYZZ group law over it.  Portable form only: G2 has no asm, quad or row variant. ----------------
enum {
  PR_G2_F2_ADD = 0, PR_G2_F2_SUB = 1, PR_G2_F2_DBL = 2, PR_G2_F2_MUL = 3, PR_G2_F2_SQR = 4, PR_G2_F2_INV = 5, PR_G2_F2_IS_ZERO = 6,
  PR_G2_MADD = 7, PR_G2_ADD = 8, PR_G2_DBL = 9, PR_G2_DBL_AFFINE = 10, PR_G2_TO_AFFINE = 11, PR_G2_SCALAR_MUL = 12, PR_G2_STORE_LOAD = 13,
  PR_G2_OPS = 14
};
constexpr int PR_F2 = 2 * FqParams::L;        // an Fq2 operand / result: c0 then c1, 9 raw limbs each
constexpr int PR_SLOT2 = 4 * PR_F2;           // an XYZZ operand / result over Fq2: X, Y, ZZ, ZZZ, coordinate-major, all-zero = infinity
constexpr int PR_AFF2 = 2 * PR_F2;            // an affine operand: x, y, Montgomery form, canonical
// limbs of operand a / operand b / the result, scalar words, per case
MZK_HD constexpr int probe_g2_a_words(int op) { return op <= PR_G2_F2_IS_ZERO ? PR_F2 : (op == PR_G2_DBL_AFFINE || op == PR_G2_SCALAR_MUL) ? PR_AFF2 : PR_SLOT2; }
MZK_HD constexpr int probe_g2_b_words(int op) {
  return (op == PR_G2_F2_ADD || op == PR_G2_F2_SUB || op == PR_G2_F2_MUL) ? PR_F2 : op == PR_G2_MADD ? PR_AFF2 : op == PR_G2_ADD ? PR_SLOT2 : 0;
}
MZK_HD constexpr int probe_g2_k_words(int op) { return op == PR_G2_SCALAR_MUL ? 8 : 0; }
MZK_HD constexpr int probe_g2_out_words(int op) { return op <= PR_G2_F2_IS_ZERO ? PR_F2 : PR_SLOT2; }

MZK_HD Fq2 probe_ld_f2(const u32* w) { Fq2 r; r.c0 = probe_ld<FqParams>(w); r.c1 = probe_ld<FqParams>(w + 9); return r; }
MZK_HD void probe_st_f2(const Fq2& a, u32* w) { probe_st<FqParams>(a.c0, w); probe_st<FqParams>(a.c1, w + 9); }
MZK_HD Xyzz2 probe_ld_slot2(const u32* w) {
  Xyzz2 p;
  p.X = probe_ld_f2(w); p.Y = probe_ld_f2(w + PR_F2); p.ZZ = probe_ld_f2(w + 2 * PR_F2); p.ZZZ = probe_ld_f2(w + 3 * PR_F2);
  return p;
}
MZK_HD Affine2 probe_ld_affine2(const u32* w) { Affine2 a; a.x = probe_ld_f2(w); a.y = probe_ld_f2(w + PR_F2); return a; }
// the limbs the function returned, as they are: infinity has to come back as the all-zero slot by itself
MZK_HD void probe_st_slot2(const Xyzz2& p, u32* w) {
  probe_st_f2(p.X, w); probe_st_f2(p.Y, w + PR_F2); probe_st_f2(p.ZZ, w + 2 * PR_F2); probe_st_f2(p.ZZZ, w + 3 * PR_F2);
}
// G2 op OP on one case.  Fq2 ops: a, b, out = Fq2 (is_zero: out[0] = 0 / 1, rest 0).  Group ops: a = slot (dbl_affine, scalar_mul:
// affine), b = affine (madd) or slot (add), k = 8 canonical scalar words (scalar_mul); out = one slot.  to_affine: the 32 plain wire
// words of g2_store_plain (all-zero = infinity), rest 0.  store_load: the slot x2_load reads back from what x2_store wrote.
template <int OP> MZK_HD void probe_g2_lane(const u32* a, const u32* b, const u32* k, u32* out) {
  if constexpr (OP == PR_G2_F2_ADD) probe_st_f2(f2_add(probe_ld_f2(a), probe_ld_f2(b)), out);
  else if constexpr (OP == PR_G2_F2_SUB) probe_st_f2(f2_sub(probe_ld_f2(a), probe_ld_f2(b)), out);
  else if constexpr (OP == PR_G2_F2_DBL) probe_st_f2(f2_dbl(probe_ld_f2(a)), out);
  else if constexpr (OP == PR_G2_F2_MUL) probe_st_f2(f2_mul(probe_ld_f2(a), probe_ld_f2(b)), out);
  else if constexpr (OP == PR_G2_F2_SQR) probe_st_f2(f2_sqr(probe_ld_f2(a)), out);
  else if constexpr (OP == PR_G2_F2_INV) probe_st_f2(f2_inv(probe_ld_f2(a)), out);
  else if constexpr (OP == PR_G2_F2_IS_ZERO) {
    const bool z = f2_is_zero(probe_ld_f2(a));
    for (int i = 0; i < PR_F2; i++) out[i] = 0;
    out[0] = z ? 1u : 0u;
  }
  else if constexpr (OP == PR_G2_MADD) probe_st_slot2(x2_madd(probe_ld_slot2(a), probe_ld_affine2(b)), out);
  else if constexpr (OP == PR_G2_ADD) probe_st_slot2(x2_add(probe_ld_slot2(a), probe_ld_slot2(b)), out);
  else if constexpr (OP == PR_G2_DBL) probe_st_slot2(x2_dbl(probe_ld_slot2(a)), out);
  else if constexpr (OP == PR_G2_DBL_AFFINE) probe_st_slot2(x2_dbl_affine(probe_ld_affine2(a)), out);
  else if constexpr (OP == PR_G2_TO_AFFINE) {
    for (int i = 0; i < PR_SLOT2; i++) out[i] = 0;
    g2_store_plain(probe_ld_slot2(a), out);
  }
  else if constexpr (OP == PR_G2_SCALAR_MUL) probe_st_slot2(x2_scalar_mul(probe_ld_affine2(a), k), out);
  else if constexpr (OP == PR_G2_STORE_LOAD) {
    u32 rec[64];
    x2_store(probe_ld_slot2(a), rec);
    probe_st_slot2(x2_load(rec), out);
  }
}

}  // namespace mzk
