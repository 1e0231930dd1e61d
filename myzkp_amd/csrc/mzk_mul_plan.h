// mzk_mul_plan.h -- what the two polynomial products (mzk_fft_multiply, mzk_fast_multiply: mzk_api.hip) decide on the host before they
// touch the device: the error code, whether the result is empty and nothing runs, the transform order, how often the root is squared,
// how many elements of each operand are copied, and which prefix of the result is kept and whether it is trimmed.  A pure function of
// the lengths and root_order.  Host-only C++17 with no HIP include, so that it can be compiled and checked on its own against a
// restatement of polynomial.rs:242-276 and ntt.rs:66-116 (tests/test_hostcheck_mul_plan.py).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include "../../include/mzk.h"

namespace mzk {

constexpr size_t MUL_SMALL_ORDER = 16;      // fast_multiply below degree 8: a 16-point cyclic convolution cannot wrap around
constexpr int MUL_SMALL_LOG = 4;

// In every admitted case (err == MZK_OK && !empty): order >= 1, copy_a <= order and copy_b <= order -- the device buffers hold `order`
// elements -- and keep <= order.
struct MulPlan {
  int err = MZK_OK;
  char msg[96] = {0};
  bool empty = false;       // the result is the empty polynomial: nothing is leased, copied or launched
  bool small = false;       // fast_multiply's `lhs * rhs` exit: the transforms take the field's own 16th root, not the caller's
  size_t order = 0;         // points of the three transforms (1: they are the identity)
  int squarings = 0;        // fast_multiply: the caller's root squared this often has order `order`
  size_t copy_a = 0, copy_b = 0;      // leading elements of each operand copied to the device; the rest of `order` is zero
  size_t keep = 0;          // the result is the first `keep` elements of the inverse transform ...
  bool trim = false;        // ... without its trailing zero elements
};

static inline MulPlan mul_plan_fail(int err, const char* msg) {
  MulPlan P;
  P.err = err;
  snprintf(P.msg, sizeof P.msg, "%s", msg);
  return P;
}

// Polynomial::fft_multiply (polynomial.rs:242-276) of la and lb stored coefficients.  m = la + lb - 1 underflows for two empty
// operands; n = m.next_power_of_two(); both operands are resized to n, which CUTS the longer one when the other is empty
// (m = lb - 1 < lb); the result is c[..m] trimmed.  An empty operand transforms to zero, so the product is the empty polynomial
// whatever omega is: it is returned before anything is sized by m.
static inline MulPlan fft_mul_plan(size_t la, size_t lb) {
  if (la == 0 && lb == 0) return mul_plan_fail(MZK_E_LENGTH, "attempt to subtract with overflow (self.coef.len() + other.coef.len() - 1)");
  MulPlan P;
  if (la == 0 || lb == 0) { P.empty = true; return P; }
  const size_t m = la + lb - 1;
  size_t n = 1;
  while (n < m) n <<= 1;
  P.order = n;
  P.copy_a = la;            // la <= m <= n as lb >= 1, and the same for lb
  P.copy_b = lb;
  P.keep = m;               // truncate(m), then trim_trailing_zeros (:271-275)
  P.trim = true;
  return P;
}

// ntt::fast_multiply (ntt.rs:66-116) once the root has passed its two assertions (:75-76): la, lb stored coefficients, of which
// da, db are left without the trailing zeros (degree + 1; 0 = the zero polynomial).
//  * a zero operand: the empty polynomial (:78-80);
//  * degree < 8: `lhs * rhs`, the trimmed schoolbook product, before root_order is looked at (:86-88).  Here: the trimmed operands
//    through a 16-point cyclic convolution, trimmed over da + db - 1;
//  * else order = root_order halved while degree < order / 2 (:90-93), operands zero-filled up to `order` (:95-102) and the `order`
//    coefficients of the inverse transform returned as they are (:111-115): a cyclic convolution when degree >= order.  An operand
//    stored longer than `order` is not cut: the reference's ntt then panics on its length or its root (MZK_E_LENGTH here), and an
//    order that is no power of two panics in ntt.rs:8-11 (MZK_E_NOT_POW2).
static inline MulPlan fast_mul_plan(size_t la, size_t lb, size_t da, size_t db, size_t root_order) {
  MulPlan P;
  if (da > la || db > lb) return mul_plan_fail(MZK_E_ARG, "fast_multiply: trimmed length above the stored length");
  if (da == 0 || db == 0) { P.empty = true; return P; }
  const size_t degree = (da - 1) + (db - 1);
  if (degree < 8) {
    P.small = true;
    P.order = MUL_SMALL_ORDER;
    P.copy_a = da;          // da, db <= 8
    P.copy_b = db;
    P.keep = da + db - 1;
    P.trim = true;
    return P;
  }
  size_t order = root_order;
  while (degree < order / 2) { order /= 2; P.squarings++; }
  if (la > order || lb > order) return mul_plan_fail(MZK_E_LENGTH, "fast_multiply: operand longer than the transform order");
  if (order & (order - 1)) return mul_plan_fail(MZK_E_NOT_POW2, "cannot compute ntt of non-power-of-two sequence");
  P.order = order;          // >= la >= da >= 1
  P.copy_a = la;
  P.copy_b = lb;
  P.keep = order;
  return P;
}

}  // namespace mzk
