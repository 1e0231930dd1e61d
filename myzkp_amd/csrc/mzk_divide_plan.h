// mzk_divide_plan.h -- what a coset division (mzk_fast_coset_divide once, mzk_fast_coset_divide_batch_dev once per row: mzk_api.hip)
// decides on the host before it touches the device: the error code and the reference's text, the exit to long division, the transform
// order, how often the root is squared, and the quotient's length.  A pure function of the trimmed lengths and root_order.  Host-only
// C++17 with no HIP include, so that it can be compiled and checked on its own against a restatement of ntt.rs:281-302 and :7-23
// (tests/test_hostcheck_divide_plan.py).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include "../../include/mzk.h"

namespace mzk {

struct DividePlan {
  int err = MZK_OK;
  char msg[96] = {0};
  bool small = false;       // degree < 8: `lhs / rhs`, long division on the host; order and squarings stay 0
  size_t order = 0;         // points of the transforms; tl <= order
  int squarings = 0;        // the caller's root squared this often has order `order`
  size_t ql = 0;            // tl - tr + 1 coefficients of the quotient; set whenever 0 < tr < tl, the inner transform's refusals included
};

static inline DividePlan divide_plan_fail(DividePlan P, int err, const char* msg) {
  P.err = err;
  snprintf(P.msg, sizeof P.msg, "%s", msg);
  return P;
}

// ntt::fast_coset_divide (ntt.rs:271-330) once the root has passed its two assertions (:281-282): tl, tr coefficients of numerator
// and denominator without their trailing zeros (degree + 1; 0 = the zero polynomial, of degree -1).
//  * a zero denominator (:283) is MZK_E_ARG, a denominator of no smaller degree than the numerator's (:284) MZK_E_LENGTH;
//  * degree < 8: `lhs / rhs`, before root_order is looked at (:294-296);
//  * else order = root_order halved while degree < order / 2, the root squared each time (:298-302), both operands zero-filled up to
//    `order` (:306-313).  A numerator longer than that is not cut: the reference's ntt then panics on its length (:8-11,
//    MZK_E_NOT_POW2) or on its root (:16-19, MZK_E_ROOT_ORDER).  An order that is no power of two but holds the numerator is passed
//    on as it is: the transforms refuse it.
static inline DividePlan coset_divide_plan(size_t tl, size_t tr, size_t root_order) {
  DividePlan P;
  if (tr == 0) return divide_plan_fail(P, MZK_E_ARG, "assertion failed: !rhs.is_zero()");
  if (!(tr < tl)) return divide_plan_fail(P, MZK_E_LENGTH, "assertion failed: rhs.degree() < lhs.degree()");
  const size_t degree = tl - 1;
  P.ql = tl - tr + 1;
  if (degree < 8) { P.small = true; return P; }
  size_t order = root_order;
  while (degree < order / 2) { order /= 2; P.squarings++; }
  if (tl > order) {
    if (tl & (tl - 1)) return divide_plan_fail(P, MZK_E_NOT_POW2, "cannot compute ntt of non-power-of-two sequence");
    return divide_plan_fail(P, MZK_E_ROOT_ORDER, "primitive root must be nth root of unity, where n is len(values)");
  }
  P.order = order;
  return P;
}

}  // namespace mzk
