// mzk_prefix_plan.h -- the host parameters of interpolation and zerofier over a prefix of a power-of-two subgroup (mzk_poly.hip: the
// trace domains of FastStark::prove, fast_stark.rs:53-57 and :197-215): whether a domain looks like such a prefix, the inverse of the
// m x m system that fixes the m missing values, and the partial-fraction parameters of the zerofier.  Pure functions of the domain's
// points over mzk_hostfield.h.  Host-only C++17 with no HIP include, so that it can be compiled and checked on its own against
// Python integers (tests/test_hostcheck_prefix_plan.py; the closed forms themselves: tests/test_prefix_math.py).
#pragma once
#include <string.h>
#include <utility>
#include <vector>
#include "mzk_hostfield.h"

namespace mzk {

static inline size_t next_pow2(size_t x) { size_t p = 1; while (p < x) p <<= 1; return p; }

// a prefix with more points of the subgroup missing goes through the subproduct tree
constexpr size_t PREFIX_MAX_MISSING = 64;

// domain[i] == g^i for i < n with g = domain[1] of order exactly N = next_pow2(n), at most PREFIX_MAX_MISSING points of the subgroup
// missing and the interpolation weights C (m x n elements) within 1 GiB.  The host looks at the order of g and at three points only
// (an arbitrary domain leaves here after a few short exponentiations); the caller then compares EVERY point with its power of g on the
// device (n host products were 0.3 ms at 2^14 points -- more than the zerofier takes).
static inline bool prefix_candidate(const HostField* hf, const uint64_t* domain, size_t n, size_t* N_out) {
  if (n < 2) return false;
  const int nl = hf->nl;
  const size_t N = next_pow2(n);
  if (N - n > PREFIX_MAX_MISSING || (N - n) * n * (size_t)nl * 8 > ((size_t)1 << 30)) return false;
  if (!h_is_one(hf, domain)) return false;
  const uint64_t* g = domain + nl;
  const char* msg;
  if (h_root_check(hf, g, N, &msg) != MZK_OK) return false;
  if (n > 2) {
    uint64_t t[4] = {0, 0, 0, 0};
    h_mulmod(hf, t, g, g);
    if (memcmp(t, domain + 2 * nl, 8 * (size_t)nl)) return false;
    h_powmod_u64(hf, t, g, (uint64_t)(n - 1));
    if (memcmp(t, domain + (n - 1) * nl, 8 * (size_t)nl)) return false;
  }
  *N_out = N;
  return true;
}

// Ainv (m x m, row-major, canonical) of A[t][j] = x_(n+j)^(1+t), x_i = g^i, by Gauss-Jordan; false if a pivot is missing (cannot
// happen for distinct non-zero x: every leading minor is a Vandermonde determinant times a product of x's)
static inline bool prefix_system_inverse(const HostField* hf, const uint64_t* g, size_t n, size_t m, std::vector<uint64_t>* out) {
  const size_t nl = (size_t)hf->nl;
  std::vector<uint64_t> a(m * 2 * m * 4, 0);                  // [A | I], four limbs per entry
  auto at = [&](size_t row, size_t col) { return a.data() + (row * 2 * m + col) * 4; };
  for (size_t j = 0; j < m; j++) {
    uint64_t x[4] = {0, 0, 0, 0}, pw[4] = {0, 0, 0, 0};
    h_powmod_u64(hf, x, g, (uint64_t)(n + j));
    memcpy(pw, x, 8 * nl);
    for (size_t t = 0; t < m; t++) { memcpy(at(t, j), pw, 8 * nl); h_mulmod(hf, pw, pw, x); }
    at(j, m + j)[0] = 1;
  }
  for (size_t col = 0; col < m; col++) {
    size_t piv = col;
    while (piv < m && h_is_zero(hf, at(piv, col))) piv++;
    if (piv == m) return false;
    if (piv != col) for (size_t k = 0; k < 2 * m * 4; k++) std::swap(a[col * 2 * m * 4 + k], a[piv * 2 * m * 4 + k]);
    uint64_t inv[4] = {0, 0, 0, 0};
    h_invmod(hf, inv, at(col, col));
    for (size_t k = 0; k < 2 * m; k++) h_mulmod(hf, at(col, k), at(col, k), inv);
    for (size_t row = 0; row < m; row++) {
      if (row == col || h_is_zero(hf, at(row, col))) continue;
      uint64_t f[4] = {0, 0, 0, 0}, prod[4] = {0, 0, 0, 0};
      memcpy(f, at(row, col), 8 * nl);
      for (size_t k = 0; k < 2 * m; k++) { h_mulmod(hf, prod, at(col, k), f); h_submod(hf, at(row, k), at(row, k), prod); }
    }
  }
  out->assign(m * m * nl, 0);
  for (size_t j = 0; j < m; j++) for (size_t t = 0; t < m; t++) memcpy(out->data() + (j * m + t) * nl, at(j, m + t), 8 * nl);
  return true;
}

// The zerofier Z of such a prefix: Z D = X^N - 1 with D = prod_j (X - x_(n+j)) over the m = N - n missing points, so the coefficients
// of Z are minus those of the power series 1 / D, and by partial fractions  z_k = sum_j rho_j w_j^(k+1),  k <= n,  w_j = 1 / x_(n+j),
// rho_j = 1 / prod_(l != j) (x_(n+j) - x_(n+l))  (m^2 products).  out: (rho_j, w_j) for j < m, canonical, interleaved; false if two
// missing points coincide (cannot happen in a subgroup)
static inline bool prefix_zerofier_params(const HostField* hf, const uint64_t* g, size_t n, size_t N, std::vector<uint64_t>* out) {
  const size_t nl = (size_t)hf->nl, m = N - n;
  std::vector<uint64_t> x(m * 4, 0);
  for (size_t j = 0; j < m; j++) h_powmod_u64(hf, x.data() + 4 * j, g, (uint64_t)(n + j));
  out->assign(2 * m * nl, 0);
  for (size_t j = 0; j < m; j++) {
    uint64_t prod[4] = {1, 0, 0, 0}, d[4] = {0, 0, 0, 0}, inv[4] = {0, 0, 0, 0}, w[4] = {0, 0, 0, 0};
    for (size_t l = 0; l < m; l++) {
      if (l == j) continue;
      h_submod(hf, d, x.data() + 4 * j, x.data() + 4 * l);
      if (h_is_zero(hf, d)) return false;
      h_mulmod(hf, prod, prod, d);
    }
    h_invmod(hf, inv, prod);
    h_powmod_u64(hf, w, g, (uint64_t)(N - (n + j)));           // 1 / x_(n+j) = g^(N - n - j)
    memcpy(out->data() + (2 * j) * nl, inv, 8 * nl);
    memcpy(out->data() + (2 * j + 1) * nl, w, 8 * nl);
  }
  return true;
}

}  // namespace mzk
