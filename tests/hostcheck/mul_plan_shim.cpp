// The host decisions of the two polynomial products (myzkp_amd/csrc/mzk_mul_plan.h: fft_mul_plan, fast_mul_plan) against a restatement
// of the reference's control flow on lengths alone (polynomial.rs:242-276, ntt.rs:7-23 and :66-116), tests/test_hostcheck_mul_plan.py.
// Stand-alone: g++ -fsanitize=address,undefined; every plan's copies are made into buffers of exactly `order` bytes, so a copy count
// above the order is a heap-buffer-overflow as well as a failed check.
//   mul_plan_shim                         every check; prints "ok <fft_multiply cases> <fast_multiply cases>"
//   mul_plan_shim fft LA LB               the plan: "err empty small order squarings copy_a copy_b keep trim"
//   mul_plan_shim fast LA LB DA DB ROOT_ORDER
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <stdint.h>
#include <vector>
#include "../../myzkp_amd/csrc/mzk_mul_plan.h"

using namespace mzk;

static int g_fail = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (g_fail < 20) { printf("FAIL: " __VA_ARGS__); printf("\n"); } g_fail++; } } while (0)

static const size_t MAX_LEN = 70;
static const uint8_t g_src[MAX_LEN + 1] = {0};

// what the device buffers see: `order` zero elements each, then the leading copy_a / copy_b elements of the operands
static void run_copies(const MulPlan& P, size_t la, size_t lb) {
  std::vector<uint8_t> da(P.order, 0), db(P.order, 0);
  CHECK(P.copy_a <= la && P.copy_b <= lb, "copies %zu %zu of operands of %zu %zu", P.copy_a, P.copy_b, la, lb);
  if (P.copy_a) memcpy(da.data(), g_src, P.copy_a);
  if (P.copy_b) memcpy(db.data(), g_src, P.copy_b);
}

// ---- the reference, on lengths ---------------------------------------------------------------------------------------------------------
static size_t next_power_of_two(size_t m) {      // usize::next_power_of_two: 0 -> 1
  size_t n = 1;
  while (n < m) n <<= 1;
  return n;
}

struct RefFft { bool panics; size_t n, m, from_a, from_b; bool zero; };
// polynomial.rs:242-276.  A vector is its length and how many of its leading entries are the operand's (the rest: F::zero()).
static RefFft ref_fft_multiply(size_t la, size_t lb) {
  RefFft R = {};
  if (la + lb == 0) { R.panics = true; return R; }       // :244 usize underflow
  R.m = la + lb - 1;
  R.n = next_power_of_two(R.m);                           // :245
  size_t a_len = la, a_own = la, b_len = lb, b_own = lb;
  if (R.n < a_len) a_own = R.n;                           // :249 resize: truncates ...
  a_len = R.n;                                            // ... or fills with zeros
  if (R.n < b_len) b_own = R.n;                           // :251
  b_len = R.n;
  R.from_a = a_own; R.from_b = b_own;
  // :254-269: fft of n points (no check on omega), c[i] = a[i] * b[i], inverse fft, scale: an operand without entries transforms to
  // zero and so does the product
  R.zero = a_own == 0 || b_own == 0;
  (void)a_len; (void)b_len;
  return R;                                               // :272-275 truncate(m), trim_trailing_zeros
}

// ntt.rs:7-23 for a root of exact order `order`: root^len == 1 iff order | len
static bool ntt_panics(size_t len, size_t order) {
  if (len == 0) return true;                              // :9 len - 1 underflows
  if (len & (len - 1)) return true;                       // :8-11
  if (len <= 1) return false;                             // :12-14
  if (len % order) return true;                           // :16-19
  if ((len / 2) % order == 0) return true;                // :20-23
  return false;
}

struct RefFast { bool panics, zero, schoolbook; size_t order; int squarings; size_t from_a, from_b, out_len; };
// ntt.rs:66-116 after the assertions on the root (:75-76), za / zb trailing zero coefficients among the la / lb stored ones
static RefFast ref_fast_multiply(size_t la, size_t lb, size_t za, size_t zb, size_t root_order) {
  RefFast R = {};
  const long deg_a = (long)(la - za) - 1, deg_b = (long)(lb - zb) - 1;      // Polynomial::degree: -1 for zero (polynomial.rs:101-108)
  if (deg_a == -1 || deg_b == -1) { R.zero = true; return R; }              // :78-80
  size_t order = root_order;                                                // :83
  const size_t degree = (size_t)(deg_a + deg_b);                            // :84
  if (degree < 8) {                                                         // :86-88 lhs * rhs: mul_ref trims (polynomial.rs:302-316);
    R.schoolbook = true;                                                    // a field has no zero divisors: degree + 1 coefficients
    R.out_len = degree + 1;
    return R;
  }
  while (degree < order / 2) { order = order / 2; R.squarings++; }          // :90-93
  size_t lhs_len = la, rhs_len = lb;                                        // :95-96 the stored coefficients, trailing zeros included
  while (lhs_len < order) lhs_len++;                                        // :97-99
  while (rhs_len < order) rhs_len++;                                        // :100-102
  R.order = order;
  R.from_a = la; R.from_b = lb;
  if (ntt_panics(lhs_len, order) || ntt_panics(rhs_len, order)) { R.panics = true; return R; }      // :104-105
  const size_t had = lhs_len < rhs_len ? lhs_len : rhs_len;                 // :106-110 zip
  if (had != 1 && ntt_panics(had, order)) { R.panics = true; return R; }    // :111 intt (:54-59): the inverse root has the same order
  R.out_len = had;                                                          // :113-115 untrimmed
  return R;
}

static void check_fft(size_t la, size_t lb) {
  const MulPlan P = fft_mul_plan(la, lb);
  const RefFft R = ref_fft_multiply(la, lb);
  CHECK((P.err != MZK_OK) == R.panics, "fft %zu %zu: err %d, reference panics %d", la, lb, P.err, R.panics);
  if (R.panics) { CHECK(P.err == MZK_E_LENGTH, "fft %zu %zu: err %d", la, lb, P.err); return; }
  if (P.err) return;
  CHECK(P.empty == R.zero, "fft %zu %zu: empty %d, reference's product is zero %d", la, lb, P.empty, R.zero);
  if (P.empty) return;
  CHECK(P.order == R.n && P.copy_a == R.from_a && P.copy_b == R.from_b && P.keep == R.m && P.trim && !P.small && P.squarings == 0,
        "fft %zu %zu: order %zu copies %zu %zu keep %zu trim %d; reference n %zu entries %zu %zu m %zu", la, lb, P.order, P.copy_a, P.copy_b, P.keep, P.trim,
        R.n, R.from_a, R.from_b, R.m);
  CHECK(P.copy_a <= P.order && P.copy_b <= P.order && P.keep <= P.order, "fft %zu %zu: copies %zu %zu keep %zu order %zu", la, lb, P.copy_a, P.copy_b, P.keep, P.order);
  if (P.copy_a <= P.order && P.copy_b <= P.order) run_copies(P, la, lb);
}

static void check_fast(size_t la, size_t lb, size_t za, size_t zb, size_t root_order) {
  const size_t da = la - za, db = lb - zb;
  const MulPlan P = fast_mul_plan(la, lb, da, db, root_order);
  const RefFast R = ref_fast_multiply(la, lb, za, zb, root_order);
  CHECK((P.err != MZK_OK) == R.panics, "fast %zu-%zu %zu-%zu order %zu: err %d, reference panics %d", la, za, lb, zb, root_order, P.err, R.panics);
  if (R.panics) {
    // which of the reference's panics: an operand stored longer than the order, else the order is no power of two
    const int want = (la > R.order || lb > R.order) ? MZK_E_LENGTH : MZK_E_NOT_POW2;
    CHECK(P.err == want, "fast %zu-%zu %zu-%zu order %zu: err %d, expected %d", la, za, lb, zb, root_order, P.err, want);
    return;
  }
  if (P.err) return;
  CHECK(P.empty == R.zero, "fast %zu-%zu %zu-%zu order %zu: empty %d, reference zero %d", la, za, lb, zb, root_order, P.empty, R.zero);
  if (P.empty) return;
  CHECK(P.small == R.schoolbook, "fast %zu-%zu %zu-%zu order %zu: small %d, reference schoolbook %d", la, za, lb, zb, root_order, P.small, R.schoolbook);
  if (P.small != R.schoolbook) return;
  if (P.small) {
    // the trimmed operands through MUL_SMALL_ORDER points without wrap-around, the product trimmed: the schoolbook product
    CHECK(P.order == MUL_SMALL_ORDER && P.order == (size_t)1 << MUL_SMALL_LOG && P.copy_a == da && P.copy_b == db && P.keep == R.out_len && P.trim,
          "fast %zu-%zu %zu-%zu: small order %zu copies %zu %zu keep %zu trim %d", la, za, lb, zb, P.order, P.copy_a, P.copy_b, P.keep, P.trim);
  } else {
    CHECK(P.order == R.order && P.squarings == R.squarings && (root_order >> P.squarings) == P.order && P.copy_a == R.from_a && P.copy_b == R.from_b &&
              P.keep == R.out_len && !P.trim,
          "fast %zu-%zu %zu-%zu order %zu: order %zu squarings %d copies %zu %zu keep %zu trim %d; reference order %zu squarings %d entries %zu %zu length %zu", la, za,
          lb, zb, root_order, P.order, P.squarings, P.copy_a, P.copy_b, P.keep, P.trim, R.order, R.squarings, R.from_a, R.from_b, R.out_len);
  }
  const bool fits = P.copy_a <= P.order && P.copy_b <= P.order && P.keep <= P.order;
  CHECK(fits, "fast %zu-%zu %zu-%zu order %zu: copies %zu %zu keep %zu order %zu", la, za, lb, zb, root_order, P.copy_a, P.copy_b, P.keep, P.order);
  // the buffers at the ends of the trailing-zero range (the copy counts are la / lb or da / db: every value occurs there)
  if (fits && (za == 0 || za == la - 1) && (zb == 0 || zb == lb - 1)) run_copies(P, la, lb);
}

static void print_plan(const MulPlan& P) {
  printf("%d %d %d %zu %d %zu %zu %zu %d\n", P.err, P.empty, P.small, P.order, P.squarings, P.copy_a, P.copy_b, P.keep, P.trim);
}

int main(int argc, char** argv) {
  if (argc == 4 && !strcmp(argv[1], "fft")) {
    print_plan(fft_mul_plan((size_t)atoll(argv[2]), (size_t)atoll(argv[3])));
    return 0;
  }
  if (argc == 7 && !strcmp(argv[1], "fast")) {
    print_plan(fast_mul_plan((size_t)atoll(argv[2]), (size_t)atoll(argv[3]), (size_t)atoll(argv[4]), (size_t)atoll(argv[5]), (size_t)atoll(argv[6])));
    return 0;
  }
  size_t n_fft = 0, n_fast = 0;
  for (size_t la = 0; la <= MAX_LEN; la++)
    for (size_t lb = 0; lb <= MAX_LEN; lb++) {
      // fft_multiply never looks at the values: the trailing zeros change nothing, the plan does not take them
      check_fft(la, lb);
      n_fft++;
      for (size_t za = 0; za <= la; za++)
        for (size_t zb = 0; zb <= lb; zb++)
          for (size_t root_order = 2; root_order <= 4096; root_order *= 2) {
            check_fast(la, lb, za, zb, root_order);
            n_fast++;
          }
    }
  // an order that is no power of two (ntt.rs:8-11), and a trimmed length above the stored one
  for (size_t root_order : {6, 12, 24, 48, 96, 160, 4095})
    for (size_t la = 1; la <= MAX_LEN; la++)
      for (size_t lb = 1; lb <= MAX_LEN; lb++) { check_fast(la, lb, 0, 0, root_order); n_fast++; }
  CHECK(fast_mul_plan(3, 3, 4, 3, 16).err == MZK_E_ARG && fast_mul_plan(3, 3, 3, 4, 16).err == MZK_E_ARG, "trimmed above stored is not refused");
  if (g_fail) { printf("%d checks failed\n", g_fail); return 1; }
  printf("ok %zu %zu\n", n_fft, n_fast);
  return 0;
}
