// The host decisions of a coset division (myzkp_amd/csrc/mzk_divide_plan.h: coset_divide_plan) against a restatement of the reference's
// control flow on lengths alone (ntt.rs:281-302 and, for the inner transforms, :7-23), tests/test_hostcheck_divide_plan.py.
// Stand-alone: g++ -fsanitize=address,undefined; every admitted plan's operands are copied into buffers of exactly `order` bytes, so a
// numerator above the order is a heap-buffer-overflow as well as a failed check.
//   divide_plan_shim                        every check; prints "ok <cases>"
//   divide_plan_shim TL TR ROOT_ORDER       the plan: "err small order squarings ql" and the message on a second line
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <stdint.h>
#include <vector>
#include "../../myzkp_amd/csrc/mzk_divide_plan.h"

using namespace mzk;

static int g_fail = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (g_fail < 20) { printf("FAIL: " __VA_ARGS__); printf("\n"); } g_fail++; } } while (0)

static const size_t MAX_LEN = 70;
static const uint8_t g_src[MAX_LEN + 1] = {0};

// ---- the reference, on lengths ---------------------------------------------------------------------------------------------------------
enum Panic { NONE = 0, RHS_ZERO, DEGREES, NTT_POW2, NTT_ROOT, NTT_PRIM };
// ntt.rs:7-23 for a root of exact order `order`: root^len == 1 iff order | len
static Panic ntt_panics(size_t len, size_t order) {
  if (len & (len - 1)) return NTT_POW2;                    // :8-11 (len >= 1 here)
  if (len <= 1) return NONE;                               // :12-14
  if (len % order) return NTT_ROOT;                        // :16-19
  if ((len / 2) % order == 0) return NTT_PRIM;             // :20-23
  return NONE;
}
struct RefDivide { Panic panic; bool long_division; size_t order; int squarings; size_t lhs_len, out_len; };
// ntt.rs:283-325 after the assertions on the root (:281-282); tl, tr = degree + 1 (0: the zero polynomial, degree -1)
static RefDivide ref_fast_coset_divide(size_t tl, size_t tr, size_t root_order) {
  RefDivide R = {};
  if (tr == 0) { R.panic = RHS_ZERO; return R; }           // :283
  const long deg_l = (long)tl - 1, deg_r = (long)tr - 1;
  if (!(deg_r < deg_l)) { R.panic = DEGREES; return R; }   // :284 (so lhs is not zero: :286-288 never returns)
  size_t order = root_order;                               // :291
  const size_t degree = (size_t)(deg_l > deg_r ? deg_l : deg_r);      // :292
  R.out_len = (size_t)(deg_l - deg_r) + 1;                 // :325, and the quotient of the long division (its leading coefficient is not zero)
  if (degree < 8) { R.long_division = true; return R; }    // :294-296
  while (degree < order / 2) { order = order / 2; R.squarings++; }      // :298-302
  size_t lhs_len = tl, rhs_len = tr;                       // :306, :310
  while (lhs_len < order) lhs_len++;                       // :307-309
  while (rhs_len < order) rhs_len++;                       // :311-313
  R.order = order; R.lhs_len = lhs_len;
  R.panic = ntt_panics(lhs_len, order);                    // :315
  if (!R.panic) R.panic = ntt_panics(rhs_len, order);      // :316
  return R;                                                // :318-323: the zip and the inverse transform have min(lhs_len, rhs_len) = order entries
}

static void check(size_t tl, size_t tr, size_t root_order) {
  const DividePlan P = coset_divide_plan(tl, tr, root_order);
  const RefDivide R = ref_fast_coset_divide(tl, tr, root_order);
  const bool pow2 = !(R.order & (R.order - 1));
  if (R.panic == RHS_ZERO) { CHECK(P.err == MZK_E_ARG && !strcmp(P.msg, "assertion failed: !rhs.is_zero()"), "%zu %zu %zu: err %d", tl, tr, root_order, P.err); return; }
  if (R.panic == DEGREES) {
    CHECK(P.err == MZK_E_LENGTH && !strcmp(P.msg, "assertion failed: rhs.degree() < lhs.degree()"), "%zu %zu %zu: err %d", tl, tr, root_order, P.err);
    return;
  }
  CHECK(P.ql == R.out_len, "%zu %zu %zu: ql %zu, reference %zu", tl, tr, root_order, P.ql, R.out_len);
  if (R.long_division) {
    CHECK(P.err == MZK_OK && P.small && P.order == 0 && P.squarings == 0, "%zu %zu %zu: err %d small %d order %zu", tl, tr, root_order, P.err, P.small, P.order);
    return;
  }
  CHECK(!P.small, "%zu %zu %zu: small, the reference transforms", tl, tr, root_order);
  if (tl > R.order) {
    // the numerator is longer than the order: the first inner transform panics on its length or on its root.  (tr < tl: the
    // denominator's transform comes second and changes nothing.)  A power of two above a power-of-two order passes ntt.rs:16-19 and
    // fails :20-23; the library has refused both with the code and text of :16-19 since it has this call, and keeps to that.
    CHECK(R.panic != NONE, "%zu %zu %zu: the reference does not panic", tl, tr, root_order);
    const int want = (tl & (tl - 1)) ? MZK_E_NOT_POW2 : MZK_E_ROOT_ORDER;
    CHECK((R.panic == NTT_POW2) == (want == MZK_E_NOT_POW2), "%zu %zu %zu: reference panic %d", tl, tr, root_order, (int)R.panic);
    CHECK(P.err == want, "%zu %zu %zu: err %d, expected %d", tl, tr, root_order, P.err, want);
    CHECK(!strcmp(P.msg, want == MZK_E_NOT_POW2 ? "cannot compute ntt of non-power-of-two sequence" : "primitive root must be nth root of unity, where n is len(values)"),
          "%zu %zu %zu: message %s", tl, tr, root_order, P.msg);
    return;
  }
  // the numerator fits: the plan hands the order on.  The reference panics only where that order is no power of two (ntt.rs:8-11),
  // which the transforms behind the plan refuse themselves
  CHECK((R.panic != NONE) == !pow2 && (R.panic == NONE || R.panic == NTT_POW2), "%zu %zu %zu: reference panic %d at order %zu", tl, tr, root_order, (int)R.panic, R.order);
  CHECK(P.err == MZK_OK && P.order == R.order && P.squarings == R.squarings, "%zu %zu %zu: err %d order %zu squarings %d; reference order %zu squarings %d", tl, tr,
        root_order, P.err, P.order, P.squarings, R.order, R.squarings);
  size_t o = root_order;
  for (int i = 0; i < P.squarings; i++) o /= 2;
  CHECK(o == P.order && P.ql <= P.order, "%zu %zu %zu: %d halvings give %zu, order %zu, ql %zu", tl, tr, root_order, P.squarings, o, P.order, P.ql);
  if (P.err == MZK_OK && tl <= P.order) {      // what the device buffers see: `order` elements, the operands' leading tl / tr copied in
    std::vector<uint8_t> dl(P.order, 0), dr(P.order, 0), dq(P.order, 0);
    memcpy(dl.data(), g_src, tl);
    memcpy(dr.data(), g_src, tr);
    memcpy(dq.data(), g_src, P.ql);
  }
}

int main(int argc, char** argv) {
  if (argc == 4) {
    const DividePlan P = coset_divide_plan((size_t)atoll(argv[1]), (size_t)atoll(argv[2]), (size_t)atoll(argv[3]));
    printf("%d %d %zu %d %zu\n%s\n", P.err, P.small, P.order, P.squarings, P.ql, P.msg);
    return 0;
  }
  size_t n = 0;
  for (size_t tl = 0; tl <= MAX_LEN; tl++)
    for (size_t tr = 0; tr <= MAX_LEN; tr++) {
      for (size_t root_order = 2; root_order <= 4096; root_order *= 2) { check(tl, tr, root_order); n++; }
      for (size_t root_order : {24, 48}) { check(tl, tr, root_order); n++; }
    }
  if (g_fail) { printf("%d checks failed\n", g_fail); return 1; }
  printf("ok %zu\n", n);
  return 0;
}
