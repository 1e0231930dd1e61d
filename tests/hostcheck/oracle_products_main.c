/* The CPU oracle's two polynomial products (oracle/mzk_oracle.c: orc_fft_multiply_ref, orc_fast_multiply_ref) at the shapes with an
 * empty or an all-zero operand, every buffer of exactly the documented size (tests/test_oracle_products.py builds and runs this).
 * Stand-alone: gcc -fsanitize=address,undefined with oracle/mzk_oracle.c compiled into the program.
 * fft_multiply with la = 0 has m = lb - 1 and n = next_power_of_two(m) < lb whenever lb = 2^k + 1: the reference's resize(n)
 * (polynomial.rs:248-251) cuts the operand, and a copy of all lb coefficients into the n-element vector is a heap overflow.
 * Prints "ok <calls>". */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

typedef uint64_t u64;
int orc_m128_nth_root(int log2n, u64* out);
int orc_fft_multiply_ref(int fid, const u64* a, size_t la, const u64* b, size_t lb, const u64* omega, u64* out, size_t* out_len);
int orc_fast_multiply_ref(int fid, const u64* a, size_t la, const u64* b, size_t lb, const u64* root, size_t root_order, u64* out, size_t* out_len);

enum { FR = 0, M128 = 1 };
static int g_fail = 0, g_calls = 0;
#define CHECK(cond, ...) do { if (!(cond)) { printf("FAIL: " __VA_ARGS__); printf("\n"); g_fail++; } } while (0)

/* n elements of L limbs: i + 1 in the lowest limb (canonical, non-zero), or all zero */
static u64* poly(size_t n, int L, int zero) {
  u64* p = malloc(n ? 8 * L * n : 1);      /* exactly n elements: the sanitizer sees a read past them */
  for (size_t i = 0; i < n * (size_t)L; i++) p[i] = 0;
  if (!zero) for (size_t i = 0; i < n; i++) p[i * L] = i + 1;
  return p;
}

static void fft_case(int fid, int L, size_t la, size_t lb, const u64* omega) {
  u64 *a = poly(la, L, 0), *b = poly(lb, L, 0);
  const size_t m = la + lb - 1;
  u64* out = malloc(m ? 8 * L * m : 1);    /* "out holds la+lb-1 elements" */
  size_t out_len = 99;
  const int rc = orc_fft_multiply_ref(fid, a, la, b, lb, omega, out, &out_len);
  g_calls++;
  CHECK(rc == 0 && out_len == 0, "fft_multiply field %d (%zu, %zu): rc %d length %zu, expected the empty product", fid, la, lb, rc, out_len);
  free(a); free(b); free(out);
}

static void fast_case(int fid, int L, size_t la, int zero_a, size_t lb, int zero_b, const u64* root, size_t root_order) {
  u64 *a = poly(la, L, zero_a), *b = poly(lb, L, zero_b);
  const size_t cap = root_order > la + lb ? root_order : la + lb;      /* "out must hold max(root_order, la+lb) elements" */
  u64* out = malloc(8 * L * cap);
  size_t out_len = 99;
  const int rc = orc_fast_multiply_ref(fid, a, la, b, lb, root, root_order, out, &out_len);
  g_calls++;
  CHECK(rc == 0 && out_len == 0, "fast_multiply field %d (%zu, %zu): rc %d length %zu, expected the empty product", fid, la, lb, rc, out_len);
  free(a); free(b); free(out);
}

int main(void) {
  static const size_t lens[] = {1, 2, 3, 4, 5, 9, 17, 129, 4097};
  u64 w16[2], w4[2];
  if (orc_m128_nth_root(4, w16) || orc_m128_nth_root(2, w4)) { printf("FAIL: no root\n"); return 1; }
  /* over Fr the product of an empty operand is zero whatever omega is (the reference does not look at it): 1 */
  const u64 one_fr[4] = {1, 0, 0, 0};
  for (size_t i = 0; i < sizeof lens / sizeof lens[0]; i++) {
    fft_case(M128, 2, 0, lens[i], w16);
    fft_case(M128, 2, lens[i], 0, w16);
    fft_case(FR, 4, 0, lens[i], one_fr);
    fft_case(FR, 4, lens[i], 0, one_fr);
    fast_case(M128, 2, 0, 0, lens[i], 0, w16, 16);
    fast_case(M128, 2, lens[i], 0, 0, 0, w16, 16);
    fast_case(M128, 2, lens[i], 1, 5, 0, w16, 16);      /* Polynomial::is_zero looks through trailing zeros (ntt.rs:78-80) */
    fast_case(M128, 2, 5, 0, lens[i], 1, w16, 16);
  }
  /* and one product with both operands present, buffers as tight: (1 + 2X + 3X^2)(1 + 2X) = 1 + 4X + 7X^2 + 6X^3 */
  {
    u64 *a = poly(3, 2, 0), *b = poly(2, 2, 0), *out = malloc(8 * 2 * 4);
    size_t out_len = 99;
    const int rc = orc_fft_multiply_ref(M128, a, 3, b, 2, w4, out, &out_len);
    g_calls++;
    const u64 want[8] = {1, 0, 4, 0, 7, 0, 6, 0};
    CHECK(rc == 0 && out_len == 4 && !memcmp(out, want, sizeof want), "fft_multiply (3, 2): rc %d length %zu", rc, out_len);
    free(a); free(b); free(out);
  }
  if (g_fail) { printf("%d checks failed\n", g_fail); return 1; }
  printf("ok %d\n", g_calls);
  return 0;
}
