/* mzk_oracle.c -- CPU restatement of the MyZKP prover hot path.  TEST INFRASTRUCTURE ONLY.
 *
 * This file is the parity oracle for the HIP kernels.  Only tests/, __graft_entry__.smoke() and the
 * cpu_baseline leg of bench.py may load it; the product library (myzkp_amd/csrc) never links,
 * includes or calls anything in oracle/.
 *
 * The reference (Koukyosyumei/MyZKP, Rust) cannot be built in this environment (no rustc/cargo,
 * SURVEY.md F5), so this is a from-scratch C restatement of its algorithms, function by function,
 * each citing the reference lines it follows.  Paths are relative to myzkp/src/modules/.
 * Arithmetic is on 64-bit limbs with unsigned __int128 (radix-2^64 Montgomery internally); that is a
 * deliberately different limb size and radix from the device code (29-bit limbs, R = 2^261), so an
 * arithmetic slip on one side does not cancel on the other.
 *
 * Pinning status: pinned against every known-answer test the reference holds for this path
 * (tests/test_oracle_kats.py: field.rs:491-504,544-550; curve.rs:494-495; bn128.rs:285-301;
 * rescueprime.rs:606-620; fri.rs:436-438; ntt.rs:346-374; cuda/test_fr.cu:16-42;
 * cuda/kernels/field.hpp:9-31) and against fixtures produced by an independent Python big-integer
 * transcription (tests/golden/, generator tests/golden/make_golden.py).
 *
 * Two layers:
 *   orc_*_ref  : literal restatements of the reference's algorithms (recursive NTT with one pow per
 *                output, affine double-and-add MSM with one inversion per group operation, ...).
 *   orc_*_fast : CPU implementations of the same functions with better algorithms (iterative NTT,
 *                Pippenger), validated against the *_ref layer, used to check 2^20..2^24 GPU results
 *                and as the multi-core "cpu_fast" figure in bench.py.
 *
 * Encoding at this API = the library ABI: canonical little-endian u64 limbs (4 for Fr/Fq, 2 for
 * M128, 1 for the toy field); affine points are x||y, all-zero = point at infinity.
 */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#ifdef _OPENMP
#include <omp.h>
#endif

typedef uint64_t u64;
typedef unsigned __int128 u128;
#define MAXN 4

/* ------------------------------------------------------------------------------------------- */
/* Field descriptors                                                                            */
/* ------------------------------------------------------------------------------------------- */
typedef struct {
  int n;          /* 64-bit limbs */
  u64 p[MAXN];    /* modulus */
  u64 n0;         /* -p^-1 mod 2^64 */
  u64 one[MAXN];  /* R mod p */
  u64 r2[MAXN];   /* R^2 mod p */
} fld_t;

enum { FID_FR = 0, FID_M128 = 1, FID_FQ = 2, FID_F631 = 3, FID_F17 = 4, FID_F31 = 5, FID_COUNT = 6 };
static fld_t g_fld[FID_COUNT];
static int g_init = 0;

static int ge(const u64* a, const u64* b, int n) {
  for (int i = n - 1; i >= 0; i--) {
    if (a[i] != b[i]) return a[i] > b[i];
  }
  return 1;
}
static u64 sub_n(u64* r, const u64* a, const u64* b, int n) {
  u64 br = 0;
  for (int i = 0; i < n; i++) {
    u128 d = (u128)a[i] - b[i] - br;
    r[i] = (u64)d;
    br = (u64)(d >> 64) & 1;
  }
  return br;
}
static u64 add_n(u64* r, const u64* a, const u64* b, int n) {
  u64 c = 0;
  for (int i = 0; i < n; i++) {
    u128 s = (u128)a[i] + b[i] + c;
    r[i] = (u64)s;
    c = (u64)(s >> 64);
  }
  return c;
}
static int is_zero_n(const u64* a, int n) {
  u64 acc = 0;
  for (int i = 0; i < n; i++) acc |= a[i];
  return acc == 0;
}
static int eq_n(const u64* a, const u64* b, int n) { return memcmp(a, b, 8 * n) == 0; }

/* (a + b) mod p, inputs < p.  Ring::add_ref, algebra/field.rs:166-169. */
static void f_add(const fld_t* f, u64* r, const u64* a, const u64* b) {
  u64 t[MAXN];
  u64 c = add_n(t, a, b, f->n);
  if (c || ge(t, f->p, f->n)) sub_n(t, t, f->p, f->n);
  memcpy(r, t, 8 * f->n);
}
/* (a - b) mod p.  Ring::sub_ref, field.rs:171-174 (canonical representative). */
static void f_sub(const fld_t* f, u64* r, const u64* a, const u64* b) {
  u64 t[MAXN];
  if (sub_n(t, a, b, f->n)) add_n(t, t, f->p, f->n);
  memcpy(r, t, 8 * f->n);
}
static void f_neg(const fld_t* f, u64* r, const u64* a) {
  u64 z[MAXN] = {0};
  f_sub(f, r, z, a);
}
/* Montgomery product a*b/R mod p (CIOS). */
static void f_mmul(const fld_t* f, u64* r, const u64* a, const u64* b) {
  const int n = f->n;
  u64 t[MAXN + 2];
  memset(t, 0, sizeof t);
  for (int i = 0; i < n; i++) {
    u64 c = 0;
    for (int j = 0; j < n; j++) {
      u128 s = (u128)a[j] * b[i] + t[j] + c;
      t[j] = (u64)s;
      c = (u64)(s >> 64);
    }
    u128 s = (u128)t[n] + c;
    t[n] = (u64)s;
    t[n + 1] = (u64)(s >> 64);
    u64 m = t[0] * f->n0;
    s = (u128)m * f->p[0] + t[0];
    c = (u64)(s >> 64);
    for (int j = 1; j < n; j++) {
      s = (u128)m * f->p[j] + t[j] + c;
      t[j - 1] = (u64)s;
      c = (u64)(s >> 64);
    }
    s = (u128)t[n] + c;
    t[n - 1] = (u64)s;
    t[n] = t[n + 1] + (u64)(s >> 64);
  }
  if (t[n] || ge(t, f->p, n)) sub_n(t, t, f->p, n);
  memcpy(r, t, 8 * n);
}
static void f_tomont(const fld_t* f, u64* r, const u64* a) { f_mmul(f, r, a, f->r2); }
static void f_frommont(const fld_t* f, u64* r, const u64* a) {
  u64 one[MAXN] = {1, 0, 0, 0};
  f_mmul(f, r, a, one);
}
/* Montgomery-domain pow, exponent as n_e limbs.  LSB-first square-and-multiply exactly as
 * mod_pow, algebra/utils.rs:108-137. */
static void f_mpow(const fld_t* f, u64* r, const u64* a, const u64* e, int ne) {
  u64 result[MAXN], base[MAXN];
  memcpy(result, f->one, 8 * f->n);
  memcpy(base, a, 8 * f->n);
  int top = ne * 64 - 1;
  while (top >= 0 && !((e[top / 64] >> (top % 64)) & 1)) top--;
  for (int i = 0; i <= top; i++) {
    if ((e[i / 64] >> (i % 64)) & 1) f_mmul(f, result, result, base);
    f_mmul(f, base, base, base);
  }
  memcpy(r, result, 8 * f->n);
}
/* Montgomery-domain inverse.  The reference runs extended Euclid on BigInts (field.rs:210-237);
 * Fermat's a^(p-2) returns the same canonical residue (0 -> 0, as extended Euclid's t = 0). */
static void f_minv(const fld_t* f, u64* r, const u64* a) {
  u64 e[MAXN], two[MAXN] = {2, 0, 0, 0};
  sub_n(e, f->p, two, f->n);
  f_mpow(f, r, a, e, f->n);
}

static void fld_setup(fld_t* f, int n, const u64* p) {
  memset(f, 0, sizeof *f);
  f->n = n;
  memcpy(f->p, p, 8 * n);
  u64 inv = 1; /* Newton: inv = p^-1 mod 2^64 */
  for (int i = 0; i < 6; i++) inv *= 2 - p[0] * inv;
  f->n0 = (u64)0 - inv;
  /* one = 2^(64n) mod p, r2 = 2^(128n) mod p by doubling */
  u64 t[MAXN] = {1, 0, 0, 0};
  for (int i = 0; i < 128 * n; i++) {
    f_add(f, t, t, t);
    if (i == 64 * n - 1) memcpy(f->one, t, 8 * n);
  }
  memcpy(f->r2, t, 8 * n);
}

static void orc_init(void) {
  if (g_init) return;
  /* ModEIP197, field.rs:428-431 */
  static const u64 FR[4] = {0x43e1f593f0000001ULL, 0x2833e84879b97091ULL, 0xb85045b68181585dULL, 0x30644e72e131a029ULL};
  /* BN128Modulus, curve/bn128.rs:19-22 */
  static const u64 FQ[4] = {0x3c208c16d87cfd47ULL, 0x97816a916871ca8dULL, 0xb85045b68181585dULL, 0x30644e72e131a029ULL};
  /* M128 = 1 + 407 * 2^119, zkstark/fri.rs:408 */
  static const u64 M128[2] = {1ULL, 407ULL << 55};
  static const u64 F631[1] = {631}, F17[1] = {17}, F31[1] = {31};
  fld_setup(&g_fld[FID_FR], 4, FR);
  fld_setup(&g_fld[FID_FQ], 4, FQ);
  fld_setup(&g_fld[FID_M128], 2, M128);
  fld_setup(&g_fld[FID_F631], 1, F631);
  fld_setup(&g_fld[FID_F17], 1, F17);
  fld_setup(&g_fld[FID_F31], 1, F31);
  g_init = 1;
}
static const fld_t* fld_of(int fid) {
  orc_init();
  if (fid < 0 || fid >= FID_COUNT) return NULL;
  return &g_fld[fid];
}

int orc_field_limbs(int fid) { const fld_t* f = fld_of(fid); return f ? f->n : -1; }
int orc_field_modulus(int fid, u64* out) {
  const fld_t* f = fld_of(fid);
  if (!f) return -1;
  memcpy(out, f->p, 8 * f->n);
  return 0;
}

/* ---- canonical-in / canonical-out scalar field API (FiniteFieldElement ops, field.rs:157-279) */
/* FiniteFieldElement::new + sanitize (field.rs:102-110, 260-270): reduce an arbitrary n-limb value. */
int orc_field_reduce(int fid, const u64* a, u64* out) {
  const fld_t* f = fld_of(fid);
  if (!f) return -1;
  u64 t[MAXN];
  memcpy(t, a, 8 * f->n);
  /* value < 2^(64n) < 2^64 p for every field here except tiny ones; use Montgomery round trip */
  u64 m[MAXN];
  f_mmul(f, m, t, f->r2); /* t*R mod p (valid for any t < 2^(64n)) */
  f_frommont(f, out, m);
  return 0;
}
int orc_field_add(int fid, const u64* a, const u64* b, u64* out) {
  const fld_t* f = fld_of(fid); if (!f) return -1;
  f_add(f, out, a, b); return 0;
}
int orc_field_sub(int fid, const u64* a, const u64* b, u64* out) {
  const fld_t* f = fld_of(fid); if (!f) return -1;
  f_sub(f, out, a, b); return 0;
}
int orc_field_neg(int fid, const u64* a, u64* out) {
  const fld_t* f = fld_of(fid); if (!f) return -1;
  f_neg(f, out, a); return 0;
}
int orc_field_mul(int fid, const u64* a, const u64* b, u64* out) {
  const fld_t* f = fld_of(fid); if (!f) return -1;
  u64 am[MAXN];
  f_tomont(f, am, a);
  f_mmul(f, out, am, b); /* (aR)*b/R = ab */
  return 0;
}
int orc_field_inv(int fid, const u64* a, u64* out) {
  const fld_t* f = fld_of(fid); if (!f) return -1;
  u64 am[MAXN];
  f_tomont(f, am, a);
  f_minv(f, am, am);
  f_frommont(f, out, am);
  return 0;
}
int orc_field_pow(int fid, const u64* a, const u64* e, int ne, u64* out) {
  const fld_t* f = fld_of(fid); if (!f) return -1;
  u64 am[MAXN];
  f_tomont(f, am, a);
  f_mpow(f, am, am, e, ne);
  f_frommont(f, out, am);
  return 0;
}

/* get_nth_root_of_m128, zkstark/fri.rs:423-447: square the order-2^119 generator down to order n. */
int orc_m128_nth_root(int log2n, u64* out) {
  const fld_t* f = fld_of(FID_M128);
  if (log2n < 0 || log2n > 119) return -2; /* the reference asserts n <= 2^119, power of two */
  /* 85408008396924667383611388730472331217, fri.rs:436-438 */
  u64 root[2] = {0xb5038f9c18f6f7d1ULL, 0x4040fbed12ee470fULL};
  /* limbs are checked against the decimal literal by tests/test_oracle_kats.py */
  u64 rm[MAXN];
  f_tomont(f, rm, root);
  for (int order = 119; order > log2n; order--) f_mmul(f, rm, rm, rm);
  f_frommont(f, out, rm);
  return 0;
}

/* ------------------------------------------------------------------------------------------- */
/* Polynomials and NTT -- literal restatements                                                  */
/* ------------------------------------------------------------------------------------------- */
static void to_mont_vec(const fld_t* f, u64* dst, const u64* src, size_t cnt) {
  for (size_t i = 0; i < cnt; i++) f_tomont(f, dst + i * f->n, src + i * f->n);
}
static void from_mont_vec(const fld_t* f, u64* dst, const u64* src, size_t cnt) {
  for (size_t i = 0; i < cnt; i++) f_frommont(f, dst + i * f->n, src + i * f->n);
}
static void f_mpow_u64(const fld_t* f, u64* r, const u64* a, u64 e) { f_mpow(f, r, a, &e, 1); }

/* ntt::ntt, algebra/ntt.rs:7-48, Montgomery-domain values.  Returns 0, or -3/-4 for the two root
 * assertions (:15-22), -2 for the power-of-two assertion (:8-11). */
static int ntt_ref_rec(const fld_t* f, const u64* root, const u64* v, u64* out, size_t n) {
  const int L = f->n;
  if (n & (n - 1)) return -2;
  if (n <= 1) { if (n) memcpy(out, v, 8 * L); return 0; }
  u64 t[MAXN];
  f_mpow_u64(f, t, root, n);
  if (!eq_n(t, f->one, L)) return -3;
  f_mpow_u64(f, t, root, n / 2);
  if (eq_n(t, f->one, L)) return -4;
  size_t half = n / 2;
  u64* odds_in = malloc(8 * L * half), *evens_in = malloc(8 * L * half);
  u64* odds = malloc(8 * L * half), *evens = malloc(8 * L * half);
  for (size_t i = 0; i < n; i++) memcpy(((i & 1) ? odds_in : evens_in) + (i / 2) * L, v + i * L, 8 * L);
  u64 root2[MAXN];
  f_mpow_u64(f, root2, root, 2);
  int rc = ntt_ref_rec(f, root2, odds_in, odds, half);
  if (!rc) rc = ntt_ref_rec(f, root2, evens_in, evens, half);
  if (!rc) {
    for (size_t i = 0; i < n; i++) { /* ntt.rs:45-47: evens[i % half] + root^i * odds[i % half] */
      u64 w[MAXN];
      f_mpow_u64(f, w, root, i);
      f_mmul(f, w, w, odds + (i % half) * L);
      f_add(f, out + i * L, evens + (i % half) * L, w);
    }
  }
  free(odds_in); free(evens_in); free(odds); free(evens);
  return rc;
}
int orc_ntt_ref(int fid, const u64* root, const u64* in, u64* out, size_t n) {
  const fld_t* f = fld_of(fid); if (!f) return -1;
  if (n == 0) return 0;
  if (n & (n - 1)) return -2;
  const int L = f->n;
  u64* vin = malloc(8 * L * n), *vout = malloc(8 * L * n);
  u64 rm[MAXN];
  to_mont_vec(f, vin, in, n);
  f_tomont(f, rm, root);
  int rc = ntt_ref_rec(f, rm, vin, vout, n);
  if (!rc) from_mont_vec(f, out, vout, n);
  free(vin); free(vout);
  return rc;
}
/* ntt::intt, algebra/ntt.rs:50-64: n^-1 * ntt(root^-1, values); len 1 returns the input. */
int orc_intt_ref(int fid, const u64* root, const u64* in, u64* out, size_t n) {
  const fld_t* f = fld_of(fid); if (!f) return -1;
  const int L = f->n;
  if (n == 0) return 0;
  if (n == 1) { memcpy(out, in, 8 * L); return 0; }
  if (n & (n - 1)) return -2;
  u64* vin = malloc(8 * L * n), *vout = malloc(8 * L * n);
  u64 rm[MAXN], rinv[MAXN], nn[MAXN] = {0}, ninv[MAXN];
  to_mont_vec(f, vin, in, n);
  f_tomont(f, rm, root);
  f_minv(f, rinv, rm);
  nn[0] = (u64)n;
  f_tomont(f, ninv, nn);
  f_minv(f, ninv, ninv);
  int rc = ntt_ref_rec(f, rinv, vin, vout, n);
  if (!rc) {
    for (size_t i = 0; i < n; i++) f_mmul(f, vout + i * L, ninv, vout + i * L);
    from_mont_vec(f, out, vout, n);
  }
  free(vin); free(vout);
  return rc;
}

/* Polynomial::eval, algebra/polynomial.rs:120-128 (power-accumulate, not Horner). */
int orc_poly_eval(int fid, const u64* coef, size_t n, const u64* x, u64* out) {
  const fld_t* f = fld_of(fid); if (!f) return -1;
  const int L = f->n;
  u64 res[MAXN] = {0}, tp[MAXN], xm[MAXN], c[MAXN], t[MAXN];
  memcpy(tp, f->one, 8 * L);
  f_tomont(f, xm, x);
  for (size_t i = 0; i < n; i++) {
    f_tomont(f, c, coef + i * L);
    f_mmul(f, t, tp, c);
    f_add(f, res, res, t);
    f_mmul(f, tp, tp, xm);
  }
  f_frommont(f, out, res);
  return 0;
}

/* Polynomial::scale, polynomial.rs:167-174: coef[i] * factor^i (one pow per coefficient). */
static void poly_scale_m(const fld_t* f, u64* dst, const u64* coef_m, size_t n, const u64* factor_m) {
  for (size_t i = 0; i < n; i++) {
    u64 w[MAXN];
    f_mpow_u64(f, w, factor_m, i);
    f_mmul(f, dst + i * f->n, w, coef_m + i * f->n);
  }
}
/* ntt::fast_coset_evaluate, algebra/ntt.rs:254-269.  n_coef > order panics in the reference
 * (usize underflow at :265) -> -5. */
int orc_fast_coset_evaluate_ref(int fid, const u64* coef, size_t n_coef, const u64* offset,
                                const u64* generator, u64* out, size_t order) {
  const fld_t* f = fld_of(fid); if (!f) return -1;
  const int L = f->n;
  if (n_coef > order) return -5;
  if (order == 0) return 0;
  u64* v = calloc(order, 8 * L), *vo = malloc(8 * L * order), *cm = malloc(8 * L * (n_coef ? n_coef : 1));
  u64 om[MAXN], gm[MAXN];
  f_tomont(f, om, offset);
  f_tomont(f, gm, generator);
  to_mont_vec(f, cm, coef, n_coef);
  poly_scale_m(f, v, cm, n_coef, om);
  int rc = ntt_ref_rec(f, gm, v, vo, order);
  if (!rc) from_mont_vec(f, out, vo, order);
  free(v); free(vo); free(cm);
  return rc;
}

static size_t trimmed_len(const fld_t* f, const u64* c, size_t n) {
  while (n > 0 && is_zero_n(c + (n - 1) * f->n, f->n)) n--;
  return n;
}
/* schoolbook product, Polynomial::mul_ref polynomial.rs:302-316; returns trimmed length */
static size_t poly_mul_school_m(const fld_t* f, const u64* a, size_t la, const u64* b, size_t lb, u64* out) {
  const int L = f->n;
  la = trimmed_len(f, a, la); lb = trimmed_len(f, b, lb);
  if (la == 0 || lb == 0) return 0;
  size_t lo = la + lb - 1;
  memset(out, 0, 8 * L * lo);
  for (size_t i = 0; i < la; i++)
    for (size_t j = 0; j < lb; j++) {
      u64 t[MAXN];
      f_mmul(f, t, a + i * L, b + j * L);
      f_add(f, out + (i + j) * L, out + (i + j) * L, t);
    }
  return trimmed_len(f, out, lo);
}
/* ntt::fast_multiply, algebra/ntt.rs:66-116.  out must hold max(root_order, la+lb) elements;
 * *out_len receives the reference's result length (untrimmed `order` on the NTT path, trimmed on the
 * schoolbook path (degree < 8), 0 for a zero operand). */
int orc_fast_multiply_ref(int fid, const u64* a, size_t la, const u64* b, size_t lb, const u64* root,
                          size_t root_order, u64* out, size_t* out_len) {
  const fld_t* f = fld_of(fid); if (!f) return -1;
  const int L = f->n;
  u64 rm[MAXN], t[MAXN];
  f_tomont(f, rm, root);
  f_mpow_u64(f, t, rm, root_order);
  if (!eq_n(t, f->one, L)) return -3;
  f_mpow_u64(f, t, rm, root_order / 2);
  if (eq_n(t, f->one, L)) return -4;
  u64* am = malloc(8 * L * (la ? la : 1)), *bm = malloc(8 * L * (lb ? lb : 1));
  to_mont_vec(f, am, a, la); to_mont_vec(f, bm, b, lb);
  size_t da = trimmed_len(f, am, la), db = trimmed_len(f, bm, lb);
  int rc = 0;
  if (da == 0 || db == 0) { *out_len = 0; goto done; }
  {
    size_t degree = (da - 1) + (db - 1);
    if (degree < 8) {
      u64* o = malloc(8 * L * (da + db));
      size_t lo = poly_mul_school_m(f, am, la, bm, lb, o);
      from_mont_vec(f, out, o, lo);
      *out_len = lo;
      free(o);
      goto done;
    }
    size_t order = root_order;
    while (degree < order / 2) { f_mmul(f, rm, rm, rm); order /= 2; }
    /* the reference pushes zeros "while len < order" (:98-103): len > order cannot happen because
       degree >= order/2 ... but la may exceed order when trailing zeros are present; ntt then
       asserts on the length.  Mirror: operands longer than order -> -5. */
    if (la > order || lb > order) { rc = -5; goto done; }
    u64* x = calloc(order, 8 * L), *y = calloc(order, 8 * L), *X = malloc(8 * L * order), *Y = malloc(8 * L * order);
    memcpy(x, am, 8 * L * la); memcpy(y, bm, 8 * L * lb);
    rc = ntt_ref_rec(f, rm, x, X, order);
    if (!rc) rc = ntt_ref_rec(f, rm, y, Y, order);
    if (!rc) {
      for (size_t i = 0; i < order; i++) f_mmul(f, X + i * L, X + i * L, Y + i * L);
      u64 rinv[MAXN], nn[MAXN] = {0}, ninv[MAXN];
      f_minv(f, rinv, rm);
      nn[0] = order; f_tomont(f, ninv, nn); f_minv(f, ninv, ninv);
      rc = ntt_ref_rec(f, rinv, X, Y, order);
      if (!rc) {
        for (size_t i = 0; i < order; i++) f_mmul(f, Y + i * L, ninv, Y + i * L);
        from_mont_vec(f, out, Y, order);
        *out_len = order;
      }
    }
    free(x); free(y); free(X); free(Y);
  }
done:
  free(am); free(bm);
  return rc;
}

/* private Polynomial::fft, polynomial.rs:278-300: recursive DIT with a running twiddle; natural
 * order in, natural order out; no checks on omega. */
static void fft_ref_rec(const fld_t* f, u64* a, size_t n, const u64* omega) {
  const int L = f->n;
  if (n == 1) return;
  size_t h = n / 2;
  u64* even = malloc(8 * L * h), *odd = malloc(8 * L * h);
  for (size_t i = 0; i < h; i++) {
    memcpy(even + i * L, a + (2 * i) * L, 8 * L);
    memcpy(odd + i * L, a + (2 * i + 1) * L, 8 * L);
  }
  u64 w2[MAXN];
  f_mmul(f, w2, omega, omega);
  fft_ref_rec(f, even, h, w2);
  fft_ref_rec(f, odd, h, w2);
  u64 wi[MAXN], t[MAXN];
  memcpy(wi, f->one, 8 * L);
  for (size_t i = 0; i < h; i++) {
    f_mmul(f, t, wi, odd + i * L);
    f_add(f, a + i * L, even + i * L, t);
    f_sub(f, a + (i + h) * L, even + i * L, t);
    f_mmul(f, wi, wi, omega);
  }
  free(even); free(odd);
}
/* Polynomial::fft_multiply, polynomial.rs:242-276.  out holds la+lb-1 elements; *out_len = trimmed
 * length (the reference trims trailing zeros, :273-275).  la + lb - 1 underflows for two empty
 * operands in the reference (usize) -> -5. */
int orc_fft_multiply_ref(int fid, const u64* a, size_t la, const u64* b, size_t lb, const u64* omega,
                         u64* out, size_t* out_len) {
  const fld_t* f = fld_of(fid); if (!f) return -1;
  const int L = f->n;
  if (la + lb == 0) return -5;
  size_t m = la + lb - 1, n = 1;
  while (n < m) n <<= 1;
  if (m == 0) n = 1; /* usize::next_power_of_two(0) == 1 */
  u64* x = calloc(n, 8 * L), *y = calloc(n, 8 * L);
  /* resize(n) (:248-251) cuts the longer operand when the other one is empty: m = lb - 1 < lb */
  to_mont_vec(f, x, a, la < n ? la : n); to_mont_vec(f, y, b, lb < n ? lb : n);
  u64 wm[MAXN], winv[MAXN], nn[MAXN] = {0}, ninv[MAXN];
  f_tomont(f, wm, omega);
  fft_ref_rec(f, x, n, wm);
  fft_ref_rec(f, y, n, wm);
  for (size_t i = 0; i < n; i++) f_mmul(f, x + i * L, x + i * L, y + i * L);
  f_minv(f, winv, wm);
  fft_ref_rec(f, x, n, winv);
  nn[0] = n; f_tomont(f, ninv, nn); f_minv(f, ninv, ninv);
  for (size_t i = 0; i < n; i++) f_mmul(f, x + i * L, x + i * L, ninv);
  size_t lo = trimmed_len(f, x, m);
  from_mont_vec(f, out, x, lo);
  *out_len = lo;
  free(x); free(y);
  return 0;
}

/* ------------------------------------------------------------------------------------------- */
/* Affine short-Weierstrass group law, algebra/curve/curve.rs:44-191                            */
/* ------------------------------------------------------------------------------------------- */
typedef struct { u64 x[MAXN], y[MAXN]; int inf; } pt_t; /* Montgomery-domain coordinates */
typedef struct { const fld_t* f; u64 a[MAXN]; } crv_t;   /* y^2 = x^3 + a x + b; b is not needed */

static void pt_set_inf(pt_t* p) { memset(p, 0, sizeof *p); p->inf = 1; }

/* line_slope, curve.rs:56-70 */
static void pt_slope(const crv_t* c, u64* s, const pt_t* p, const pt_t* q) {
  const fld_t* f = c->f;
  u64 num[MAXN], den[MAXN], t[MAXN];
  if (eq_n(p->x, q->x, f->n)) {
    f_mmul(f, t, p->x, p->x);   /* x1^2 */
    f_add(f, num, t, t);
    f_add(f, num, num, t);      /* 3 x1^2 */
    f_add(f, num, num, c->a);   /* + a */
    f_add(f, den, p->y, p->y);  /* 2 y1 */
  } else {
    f_sub(f, num, q->y, p->y);
    f_sub(f, den, q->x, p->x);
  }
  f_minv(f, den, den);
  f_mmul(f, s, num, den);
}
/* double / inplace_double, curve.rs:72-101 */
static void pt_double(const crv_t* c, pt_t* r, const pt_t* p) {
  const fld_t* f = c->f;
  if (p->inf) { *r = *p; return; }
  u64 s[MAXN], nx[MAXN], ny[MAXN], t[MAXN];
  pt_slope(c, s, p, p);
  f_mmul(f, nx, s, s);
  f_sub(f, nx, nx, p->x);
  f_sub(f, nx, nx, p->x);          /* s^2 - x - x */
  f_mmul(f, t, s, nx);
  f_neg(f, ny, t);                 /* -s*new_x */
  f_mmul(f, t, s, p->x);
  f_add(f, ny, ny, t);             /* + s*x */
  f_sub(f, ny, ny, p->y);          /* - y */
  memcpy(r->x, nx, 8 * f->n); memcpy(r->y, ny, 8 * f->n); r->inf = 0;
}
/* add_ref / add_assign_ref, curve.rs:103-161, all four special cases */
static void pt_add(const crv_t* c, pt_t* r, const pt_t* p, const pt_t* q) {
  const fld_t* f = c->f;
  if (p->inf) { *r = *q; return; }
  if (q->inf) { *r = *p; return; }
  if (eq_n(p->x, q->x, f->n)) {
    if (eq_n(p->y, q->y, f->n)) { pt_double(c, r, p); return; }
    pt_set_inf(r); return;
  }
  u64 s[MAXN], nx[MAXN], ny[MAXN], t[MAXN];
  pt_slope(c, s, p, q);
  f_mmul(f, nx, s, s);
  f_sub(f, nx, nx, p->x);
  f_sub(f, nx, nx, q->x);
  f_mmul(f, t, s, nx);
  f_neg(f, ny, t);                 /* (-s)*new_x */
  f_mmul(f, t, s, p->x);
  f_sub(f, t, t, p->y);            /* s*x1 - y1 */
  f_add(f, ny, ny, t);
  memcpy(r->x, nx, 8 * f->n); memcpy(r->y, ny, 8 * f->n); r->inf = 0;
}
/* mul_ref_bigint, curve.rs:168-191: LSB-first double-and-add; scalar 0 -> infinity.  (Negative
 * scalars panic in the reference; this API only carries non-negative limbs.) */
static void pt_mul(const crv_t* c, pt_t* r, const pt_t* p, const u64* k, int nk) {
  pt_t result, cur = *p;
  pt_set_inf(&result);
  int top = nk * 64 - 1;
  while (top >= 0 && !((k[top / 64] >> (top % 64)) & 1)) top--;
  for (int i = 0; i <= top; i++) {
    if ((k[i / 64] >> (i % 64)) & 1) pt_add(c, &result, &result, &cur);
    pt_double(c, &cur, &cur);
  }
  *r = result;
}
static void pt_load(const fld_t* f, pt_t* p, const u64* xy) {
  if (is_zero_n(xy, 2 * f->n)) { pt_set_inf(p); return; }
  f_tomont(f, p->x, xy); f_tomont(f, p->y, xy + f->n); p->inf = 0;
}
static void pt_store(const fld_t* f, u64* xy, const pt_t* p) {
  if (p->inf) { memset(xy, 0, 16 * f->n); return; }
  f_frommont(f, xy, p->x); f_frommont(f, xy + f->n, p->y);
}
static void crv_setup(crv_t* c, int fid, u64 a_small) {
  c->f = fld_of(fid);
  u64 a[MAXN] = {a_small, 0, 0, 0};
  f_tomont(c->f, c->a, a);
}
/* curve ids: 0 = BN128Curve a=0,b=3 over Fq (bn128.rs:23); 1 = y^2=x^3+30x+34 over F_631
 * (curve.rs:429-497 test curve) */
static int crv_of(int cid, crv_t* c) {
  if (cid == 0) { crv_setup(c, FID_FQ, 0); return 0; }
  if (cid == 1) { crv_setup(c, FID_F631, 30); return 0; }
  return -1;
}
int orc_ec_add(int cid, const u64* p_xy, const u64* q_xy, u64* out_xy) {
  crv_t c; if (crv_of(cid, &c)) return -1;
  pt_t p, q, r;
  pt_load(c.f, &p, p_xy); pt_load(c.f, &q, q_xy);
  pt_add(&c, &r, &p, &q);
  pt_store(c.f, out_xy, &r);
  return 0;
}
int orc_ec_double(int cid, const u64* p_xy, u64* out_xy) {
  crv_t c; if (crv_of(cid, &c)) return -1;
  pt_t p, r;
  pt_load(c.f, &p, p_xy);
  pt_double(&c, &r, &p);
  pt_store(c.f, out_xy, &r);
  return 0;
}
int orc_ec_mul(int cid, const u64* p_xy, const u64* k, int nk, u64* out_xy) {
  crv_t c; if (crv_of(cid, &c)) return -1;
  pt_t p, r;
  pt_load(c.f, &p, p_xy);
  pt_mul(&c, &r, &p, k, nk);
  pt_store(c.f, out_xy, &r);
  return 0;
}
/* is the affine point on y^2 = x^3 + 3 (BN254 G1)?  bn128.rs:285-289 checks this for the generator */
int orc_g1_on_curve(const u64* xy) {
  const fld_t* f = fld_of(FID_FQ);
  if (is_zero_n(xy, 8)) return 1;
  u64 x[MAXN], y[MAXN], l[MAXN], r[MAXN], three[MAXN] = {3, 0, 0, 0};
  if (ge(xy, f->p, 4) || ge(xy + 4, f->p, 4)) return 0;
  f_tomont(f, x, xy); f_tomont(f, y, xy + 4);
  f_mmul(f, l, y, y);
  f_mmul(f, r, x, x); f_mmul(f, r, r, x);
  f_tomont(f, three, three);
  f_add(f, r, r, three);
  return eq_n(l, r, 4);
}

/* Polynomial::eval_with_powers_on_curve, algebra/polynomial.rs:156-165 -- THE MSM, literally:
 * result += powers[i].mul_ref(coef[i].sanitize()), in index order. */
int orc_msm_ref(const u64* scalars, const u64* points_xy, size_t n, u64* out_xy) {
  crv_t c; crv_of(0, &c);
  const fld_t* fr = fld_of(FID_FR);
  pt_t acc, p, t;
  pt_set_inf(&acc);
  for (size_t i = 0; i < n; i++) {
    u64 k[4];
    if (ge(scalars + 4 * i, fr->p, 4)) orc_field_reduce(FID_FR, scalars + 4 * i, k); /* sanitize */
    else memcpy(k, scalars + 4 * i, 32);
    pt_load(c.f, &p, points_xy + 8 * i);
    pt_mul(&c, &t, &p, k, 4);
    pt_add(&c, &acc, &acc, &t);
  }
  pt_store(c.f, out_xy, &acc);
  return 0;
}

/* setup_kzg, algebra/kzg.rs:27-40, G1 part, with the trapdoor alpha supplied by the caller (the
 * reference draws it from thread_rng): powers[i] = g1 * alpha^i, i = 0..=max_d. */
int orc_kzg_setup_g1_ref(const u64* g1_xy, const u64* alpha, size_t max_d, u64* powers_xy) {
  crv_t c; crv_of(0, &c);
  const fld_t* fr = fld_of(FID_FR);
  pt_t g, t;
  pt_load(c.f, &g, g1_xy);
  u64 ap[MAXN], am[MAXN], k[MAXN];
  memcpy(ap, fr->one, 32);
  f_tomont(fr, am, alpha);
  for (size_t i = 0; i <= max_d; i++) {
    f_frommont(fr, k, ap);
    pt_mul(&c, &t, &g, k, 4);
    pt_store(c.f, powers_xy + 8 * i, &t);
    f_mmul(fr, ap, ap, am);
  }
  return 0;
}
/* commit_kzg, kzg.rs:57-59 */
int orc_kzg_commit_ref(const u64* coef, size_t n, const u64* powers_xy, u64* out_xy) {
  return orc_msm_ref(coef, powers_xy, n, out_xy);
}
/* open_kzg, kzg.rs:61-72: y = f(u); f_u = (f - y) / (X - u) by the reference's long division
 * (div_rem_ref, polynomial.rs:371-405); w = MSM(f_u, powers). */
int orc_kzg_open_ref(const u64* coef, size_t n, const u64* u, const u64* powers_xy, u64* y_out, u64* w_xy) {
  const fld_t* f = fld_of(FID_FR);
  const int L = 4;
  orc_poly_eval(FID_FR, coef, n, u, y_out);
  /* f - y (Sub trims trailing zeros, polynomial.rs:517-523) */
  u64* rem = malloc(8 * L * (n ? n : 1));
  to_mont_vec(f, rem, coef, n);
  u64 ym[MAXN], um[MAXN];
  f_tomont(f, ym, y_out); f_tomont(f, um, u);
  size_t rl = n;
  if (n == 0) { rem[0] = rem[1] = rem[2] = rem[3] = 0; f_neg(f, rem, ym); rl = 1; }
  else f_sub(f, rem, rem, ym);
  rl = trimmed_len(f, rem, rl);
  /* divisor X - u = [-u, 1] (from_monomials, polynomial.rs:202-212) */
  u64 d0[MAXN];
  f_neg(f, d0, um);
  size_t ql = rl >= 2 ? rl - 1 : 0;
  u64* quo = calloc(ql ? ql : 1, 8 * L);
  while (rl >= 2) { /* polynomial.rs:385-395, divisor_lead_inv = 1 */
    u64 lead[MAXN], t[MAXN];
    memcpy(lead, rem + (rl - 1) * L, 8 * L);
    size_t dd = rl - 2;
    memcpy(quo + dd * L, lead, 8 * L);
    f_mmul(f, t, lead, d0);
    f_sub(f, rem + dd * L, rem + dd * L, t);
    f_sub(f, rem + (dd + 1) * L, rem + (dd + 1) * L, lead);
    rl = trimmed_len(f, rem, rl);
  }
  ql = trimmed_len(f, quo, ql);
  u64* qc = malloc(8 * L * (ql ? ql : 1));
  from_mont_vec(f, qc, quo, ql);
  int rc = orc_msm_ref(qc, powers_xy, ql, w_xy);
  free(rem); free(quo); free(qc);
  return rc;
}

/* ------------------------------------------------------------------------------------------- */
/* Fast CPU layer (validated against the *_ref layer by tests/test_oracle_fast.py)              */
/* ------------------------------------------------------------------------------------------- */
static size_t bitrev(size_t x, int bits) {
  size_t r = 0;
  for (int i = 0; i < bits; i++) { r = (r << 1) | (x & 1); x >>= 1; }
  return r;
}
/* Iterative radix-2 DIT; same map as orc_ntt_ref / orc_intt_ref (natural in, natural out). */
int orc_ntt_fast(int fid, const u64* root, const u64* in, u64* out, size_t n, int inverse, int nthreads) {
  const fld_t* f = fld_of(fid); if (!f) return -1;
  const int L = f->n;
  if (n == 0) return 0;
  if (n & (n - 1)) return -2;
  if (n == 1) { memcpy(out, in, 8 * L); return 0; }
  int lg = 0; while (((size_t)1 << lg) < n) lg++;
  u64 rm[MAXN], t[MAXN];
  f_tomont(f, rm, root);
  f_mpow_u64(f, t, rm, n);
  if (!eq_n(t, f->one, L)) return -3;
  f_mpow_u64(f, t, rm, n / 2);
  if (eq_n(t, f->one, L)) return -4;
  if (inverse) f_minv(f, rm, rm);
  if (nthreads < 1) nthreads = 1;
  u64* tw = malloc(8 * L * (n / 2));
  memcpy(tw, f->one, 8 * L);
  for (size_t i = 1; i < n / 2; i++) f_mmul(f, tw + i * L, tw + (i - 1) * L, rm);
  /* Values stay in the plain domain: multiplying a plain x by a Montgomery-form twiddle wR gives wx. */
  u64* a = malloc(8 * L * n);
#pragma omp parallel for num_threads(nthreads) schedule(static)
  for (size_t i = 0; i < n; i++) memcpy(a + bitrev(i, lg) * L, in + i * L, 8 * L);
  for (int s = 1; s <= lg; s++) {
    size_t half = (size_t)1 << (s - 1), step = n >> s;
#pragma omp parallel for num_threads(nthreads) schedule(static)
    for (size_t b = 0; b < n / 2; b++) {
      size_t grp = b / half, j = b % half;
      u64* lo = a + (grp * 2 * half + j) * L, *hi = lo + half * L;
      u64 tt[MAXN], u[MAXN];
      f_mmul(f, tt, tw + (j * step) * L, hi);
      memcpy(u, lo, 8 * L);
      f_add(f, lo, u, tt);
      f_sub(f, hi, u, tt);
    }
  }
  if (inverse) {
    u64 nn[MAXN] = {0}, ninv[MAXN];
    nn[0] = n; f_tomont(f, ninv, nn); f_minv(f, ninv, ninv);
#pragma omp parallel for num_threads(nthreads) schedule(static)
    for (size_t i = 0; i < n; i++) f_mmul(f, a + i * L, ninv, a + i * L);
  }
  memcpy(out, a, 8 * L * n);
  free(a); free(tw);
  return 0;
}

/* Jacobian arithmetic for the fast MSM (a = 0).  Z = 0 encodes infinity. */
typedef struct { u64 X[4], Y[4], Z[4]; } jac_t;
static void jac_set_inf(jac_t* p) { memset(p, 0, sizeof *p); }
static void jac_double(const fld_t* f, jac_t* r, const jac_t* p) {
  if (is_zero_n(p->Z, 4)) { *r = *p; return; }
  u64 A[4], B[4], C[4], D[4], E[4], F[4], t[4], X3[4], Y3[4], Z3[4];
  f_mmul(f, A, p->X, p->X);
  f_mmul(f, B, p->Y, p->Y);
  f_mmul(f, C, B, B);
  f_add(f, t, p->X, B); f_mmul(f, t, t, t); f_sub(f, t, t, A); f_sub(f, t, t, C); f_add(f, D, t, t);
  f_add(f, E, A, A); f_add(f, E, E, A);
  f_mmul(f, F, E, E);
  f_sub(f, X3, F, D); f_sub(f, X3, X3, D);
  f_sub(f, t, D, X3); f_mmul(f, Y3, E, t);
  f_add(f, t, C, C); f_add(f, t, t, t); f_add(f, t, t, t); f_sub(f, Y3, Y3, t);
  f_mmul(f, Z3, p->Y, p->Z); f_add(f, Z3, Z3, Z3);
  memcpy(r->X, X3, 32); memcpy(r->Y, Y3, 32); memcpy(r->Z, Z3, 32);
}
static void jac_add(const fld_t* f, jac_t* r, const jac_t* p, const jac_t* q) {
  if (is_zero_n(p->Z, 4)) { *r = *q; return; }
  if (is_zero_n(q->Z, 4)) { *r = *p; return; }
  u64 Z1Z1[4], Z2Z2[4], U1[4], U2[4], S1[4], S2[4], H[4], I[4], J[4], rr[4], V[4], t[4], X3[4], Y3[4], Z3[4];
  f_mmul(f, Z1Z1, p->Z, p->Z); f_mmul(f, Z2Z2, q->Z, q->Z);
  f_mmul(f, U1, p->X, Z2Z2); f_mmul(f, U2, q->X, Z1Z1);
  f_mmul(f, S1, p->Y, q->Z); f_mmul(f, S1, S1, Z2Z2);
  f_mmul(f, S2, q->Y, p->Z); f_mmul(f, S2, S2, Z1Z1);
  if (eq_n(U1, U2, 4)) {
    if (eq_n(S1, S2, 4)) { jac_double(f, r, p); return; }
    jac_set_inf(r); return;
  }
  f_sub(f, H, U2, U1);
  f_add(f, I, H, H); f_mmul(f, I, I, I);
  f_mmul(f, J, H, I);
  f_sub(f, rr, S2, S1); f_add(f, rr, rr, rr);
  f_mmul(f, V, U1, I);
  f_mmul(f, X3, rr, rr); f_sub(f, X3, X3, J); f_sub(f, X3, X3, V); f_sub(f, X3, X3, V);
  f_sub(f, t, V, X3); f_mmul(f, Y3, rr, t); f_mmul(f, t, S1, J); f_add(f, t, t, t); f_sub(f, Y3, Y3, t);
  f_add(f, Z3, p->Z, q->Z); f_mmul(f, Z3, Z3, Z3); f_sub(f, Z3, Z3, Z1Z1); f_sub(f, Z3, Z3, Z2Z2); f_mmul(f, Z3, Z3, H);
  memcpy(r->X, X3, 32); memcpy(r->Y, Y3, 32); memcpy(r->Z, Z3, 32);
}
static void jac_from_affine(const fld_t* f, jac_t* r, const u64* xm, const u64* ym) {
  memcpy(r->X, xm, 32); memcpy(r->Y, ym, 32); memcpy(r->Z, f->one, 32);
}
static void jac_store_affine(const fld_t* f, u64* xy, const jac_t* p) {
  if (is_zero_n(p->Z, 4)) { memset(xy, 0, 64); return; }
  u64 zi[4], zi2[4], x[4], y[4];
  f_minv(f, zi, p->Z);
  f_mmul(f, zi2, zi, zi);
  f_mmul(f, x, p->X, zi2);
  f_mmul(f, zi2, zi2, zi);
  f_mmul(f, y, p->Y, zi2);
  f_frommont(f, xy, x); f_frommont(f, xy + 4, y);
}
/* Pippenger bucket MSM, unsigned c-bit windows.  Same function as orc_msm_ref.
 * Threads: task (w, s) = window w over slice s of the pairs, each with its own bucket array (round 3: threads over windows
 * alone left all but `nwin` cores of the GPU box idle; this is still the oracle's plain, un-tuned code -- general Jacobian
 * additions, no signed digits, no endomorphism -- only spread over the cores), then the slices' bucket arrays are summed
 * per window and each window takes its running sum. */
int orc_msm_fast(const u64* scalars, const u64* points_xy, size_t n, u64* out_xy, int nthreads) {
  const fld_t* f = fld_of(FID_FQ);
  const fld_t* fr = fld_of(FID_FR);
  if (nthreads < 1) nthreads = 1;
  int c = 1; while (((size_t)1 << (c + 3)) < n && c < 16) c++;
  if (c < 4) c = 4;
  const int nwin = (254 + c - 1) / c;
  const size_t nb = ((size_t)1 << c) - 1;
  int S = nthreads / nwin;                         /* slices per window */
  if (S < 1) S = 1;
  if (S > 16) S = 16;                              /* 16 x 16 bucket arrays of 6 MiB at c = 16 */
  while (S > 1 && n / (size_t)S < 2 * nb) S--;     /* a slice should at least fill its buckets */
  u64* pm = malloc(64 * (n ? n : 1));
  u64* sc = malloc(32 * (n ? n : 1));
  unsigned char* isinf = malloc(n ? n : 1);
#pragma omp parallel for num_threads(nthreads) schedule(static)
  for (size_t i = 0; i < n; i++) {
    isinf[i] = is_zero_n(points_xy + 8 * i, 8);
    f_tomont(f, pm + 8 * i, points_xy + 8 * i);
    f_tomont(f, pm + 8 * i + 4, points_xy + 8 * i + 4);
    if (ge(scalars + 4 * i, fr->p, 4)) orc_field_reduce(FID_FR, scalars + 4 * i, sc + 4 * i);
    else memcpy(sc + 4 * i, scalars + 4 * i, 32);
  }
  jac_t* wsum = malloc(sizeof(jac_t) * nwin);
  jac_t* bk_all = malloc(sizeof(jac_t) * nb * (size_t)nwin * (size_t)S);
#pragma omp parallel for num_threads(nthreads) schedule(dynamic, 1)
  for (int task = 0; task < nwin * S; task++) {
    const int w = task / S, sl = task % S;
    jac_t* bk = bk_all + (size_t)task * nb;
    for (size_t b = 0; b < nb; b++) jac_set_inf(&bk[b]);
    const size_t lo = n * (size_t)sl / (size_t)S, hi = n * (size_t)(sl + 1) / (size_t)S;
    for (size_t i = lo; i < hi; i++) {
      if (isinf[i]) continue;
      int bit = w * c;
      u64 d = sc[4 * i + bit / 64] >> (bit % 64);
      if (bit % 64 + c > 64 && bit / 64 + 1 < 4) d |= sc[4 * i + bit / 64 + 1] << (64 - bit % 64);
      d &= ((u64)1 << c) - 1;
      if (!d) continue;
      jac_t q;
      jac_from_affine(f, &q, pm + 8 * i, pm + 8 * i + 4);
      jac_add(f, &bk[d - 1], &bk[d - 1], &q);
    }
  }
  if (S > 1) {                                     /* bucket b of window w: slice 0 += slices 1 .. S-1 */
#pragma omp parallel for num_threads(nthreads) schedule(static)
    for (size_t wb = 0; wb < (size_t)nwin * nb; wb++) {
      const size_t w = wb / nb, b = wb % nb;
      jac_t* dst = bk_all + (w * (size_t)S) * nb + b;
      for (int sl = 1; sl < S; sl++) jac_add(f, dst, dst, bk_all + (w * (size_t)S + (size_t)sl) * nb + b);
    }
  }
#pragma omp parallel for num_threads(nthreads) schedule(dynamic, 1)
  for (int w = 0; w < nwin; w++) {
    const jac_t* bk = bk_all + ((size_t)w * (size_t)S) * nb;
    jac_t run, acc;
    jac_set_inf(&run); jac_set_inf(&acc);
    for (size_t b = nb; b-- > 0;) {
      jac_add(f, &run, &run, &bk[b]);
      jac_add(f, &acc, &acc, &run);
    }
    wsum[w] = acc;
  }
  jac_t tot;
  jac_set_inf(&tot);
  for (int w = nwin - 1; w >= 0; w--) {
    for (int k = 0; k < c; k++) jac_double(f, &tot, &tot);
    jac_add(f, &tot, &tot, &wsum[w]);
  }
  jac_store_affine(f, out_xy, &tot);
  free(pm); free(sc); free(isinf); free(wsum); free(bk_all);
  return 0;
}

/* [k_i] G for a batch of scalars (fixed base, 8-bit windows; used to build big SRS fixtures and
 * trapdoor checks quickly): out[i] = k[i] * base. */
int orc_g1_fixed_base_mul_batch(const u64* base_xy, const u64* scalars, size_t n, u64* out_xy, int nthreads) {
  const fld_t* f = fld_of(FID_FQ);
  if (nthreads < 1) nthreads = 1;
  /* table[w][d] = d * 2^(8w) * base, d = 1..255 */
  jac_t (*tab)[255] = malloc(sizeof(jac_t) * 255 * 32);
  jac_t b;
  u64 bx[4], by[4];
  if (is_zero_n(base_xy, 8)) { memset(out_xy, 0, 64 * n); free(tab); return 0; }
  f_tomont(f, bx, base_xy); f_tomont(f, by, base_xy + 4);
  jac_from_affine(f, &b, bx, by);
  for (int w = 0; w < 32; w++) {
    tab[w][0] = b;
    for (int d = 1; d < 255; d++) jac_add(f, &tab[w][d], &tab[w][d - 1], &b);
    jac_t nb2 = tab[w][254];
    jac_add(f, &nb2, &nb2, &b); /* 256 * b */
    b = nb2;
  }
#pragma omp parallel for num_threads(nthreads) schedule(static)
  for (size_t i = 0; i < n; i++) {
    jac_t acc;
    jac_set_inf(&acc);
    for (int w = 0; w < 32; w++) {
      unsigned d = (unsigned)(scalars[4 * i + w / 8] >> (8 * (w % 8))) & 255u;
      if (d) jac_add(f, &acc, &acc, &tab[w][d - 1]);
    }
    jac_store_affine(f, out_xy + 8 * i, &acc);
  }
  free(tab);
  return 0;
}

/* ------------------------------------------------------------------------------------------- */
/* Deterministic synthetic inputs shared by tests and bench: SplitMix64 stream,       */
/* rejection-sampled below the modulus.  The GPU generator kernels reproduce these bit for bit.   */
/* ------------------------------------------------------------------------------------------- */
static u64 splitmix64(u64* s) {
  u64 z = (*s += 0x9e3779b97f4a7c15ULL);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ULL;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebULL;
  return z ^ (z >> 31);
}
/* element i of stream `seed`: limbs from SplitMix64 seeded with seed ^ (i * GOLD) ^ try, masked to
 * the modulus bit length, rejected until < p. */
void orc_synth_element(int fid, u64 seed, u64 index, u64* out) {
  const fld_t* f = fld_of(fid);
  int bits = 0;
  for (int b = f->n * 64 - 1; b >= 0; b--) if ((f->p[b / 64] >> (b % 64)) & 1) { bits = b + 1; break; }
  for (u64 attempt = 0;; attempt++) {
    u64 s = seed ^ (index * 0xd1342543de82ef95ULL) ^ (attempt * 0xa0761d6478bd642fULL);
    for (int i = 0; i < f->n; i++) out[i] = splitmix64(&s);
    int topbits = bits - 64 * (f->n - 1);
    if (topbits < 64) out[f->n - 1] &= (((u64)1 << topbits) - 1);
    if (!ge(out, f->p, f->n)) return;
  }
}
void orc_synth_vector(int fid, u64 seed, size_t n, u64* out, int nthreads) {
  const fld_t* f = fld_of(fid);
  if (nthreads < 1) nthreads = 1;
#pragma omp parallel for num_threads(nthreads) schedule(static)
  for (size_t i = 0; i < n; i++) orc_synth_element(fid, seed, i, out + i * f->n);
}
/* Try-and-increment G1 points: x = synth(seed, i) + t, smallest t >= 0 with x^3 + 3 a
 * square; y = (x^3+3)^((q+1)/4) (q = 3 mod 4), then the smaller of y, q - y ... no: y as computed. */
void orc_synth_g1_points(u64 seed, size_t n, u64* out_xy, int nthreads) {
  const fld_t* f = fld_of(FID_FQ);
  if (nthreads < 1) nthreads = 1;
  u64 e[4], one[4] = {1, 0, 0, 0}, three[4] = {3, 0, 0, 0}, b3[4];
  add_n(e, f->p, one, 4); /* (q+1)/4 */
  for (int i = 0; i < 3; i++) e[i] = (e[i] >> 2) | (e[i + 1] << 62);
  e[3] >>= 2;
  f_tomont(f, b3, three);
#pragma omp parallel for num_threads(nthreads) schedule(static)
  for (size_t i = 0; i < n; i++) {
    u64 x[4], xm[4], rhs[4], y[4], y2[4];
    orc_synth_element(FID_FQ, seed, i, x);
    for (;;) {
      f_tomont(f, xm, x);
      f_mmul(f, rhs, xm, xm); f_mmul(f, rhs, rhs, xm); f_add(f, rhs, rhs, b3);
      f_mpow(f, y, rhs, e, 4);
      f_mmul(f, y2, y, y);
      if (eq_n(y2, rhs, 4) && !is_zero_n(rhs, 4)) break;
      f_add(f, x, x, one); /* x + 1 mod q */
    }
    memcpy(out_xy + 8 * i, x, 32);
    f_frommont(f, out_xy + 8 * i + 4, y);
  }
}

/* ------------------------------------------------------------------------------------------- */
/* "Next" rows: FRI split-and-fold, batch_open_kzg, prove_degree_bound              */
/* ------------------------------------------------------------------------------------------- */
/* FRI commit-loop fold, zkstark/fri.rs:182-193, literally (one pow and one inversion-by-division per
 * element, twice):  out[i] = 2^-1 * ((1 + alpha/(offset*omega^i)) * c[i] + (1 - alpha/(offset*omega^i)) * c[n/2 + i]),
 * sanitized.  out holds n/2 elements. */
int orc_fri_fold_ref(int fid, const u64* codeword, size_t n, const u64* alpha, const u64* offset,
                     const u64* omega, u64* out) {
  const fld_t* f = fld_of(fid); if (!f) return -1;
  const int L = f->n;
  u64 am[MAXN], om[MAXN], wm[MAXN], two[MAXN] = {2, 0, 0, 0}, twoinv[MAXN];
  f_tomont(f, am, alpha); f_tomont(f, om, offset); f_tomont(f, wm, omega);
  f_tomont(f, twoinv, two); f_minv(f, twoinv, twoinv);
  const size_t h = n / 2;
  for (size_t i = 0; i < h; i++) {
    u64 wi[MAXN], d[MAXN], q[MAXN], lhs[MAXN], rhs[MAXN], a[MAXN], b[MAXN], t[MAXN];
    f_mpow_u64(f, wi, wm, i);
    f_mmul(f, d, om, wi);               /* offset * omega^i */
    f_minv(f, d, d);
    f_mmul(f, q, am, d);                /* alpha / (offset * omega^i) */
    f_add(f, lhs, f->one, q);
    f_sub(f, rhs, f->one, q);
    f_tomont(f, a, codeword + i * L);
    f_tomont(f, b, codeword + (h + i) * L);
    f_mmul(f, lhs, lhs, a);
    f_mmul(f, rhs, rhs, b);
    f_add(f, t, lhs, rhs);
    f_mmul(f, t, twoinv, t);
    f_frommont(f, out + i * L, t);
  }
  return 0;
}

/* general long division, Polynomial::div_rem_ref polynomial.rs:371-405 (Montgomery-domain arrays).
 * quo must hold max(la - lb + 1, 1) elements; returns trimmed quotient length; rem (la elements) is
 * overwritten with the remainder, *rem_len its trimmed length. */
static size_t poly_divrem_m(const fld_t* f, u64* rem, size_t la, const u64* b, size_t lb, u64* quo, size_t* rem_len) {
  const int L = f->n;
  la = trimmed_len(f, rem, la); lb = trimmed_len(f, b, lb);
  if (lb == 0 || la < lb) { *rem_len = la; return 0; }
  u64 leadinv[MAXN];
  f_minv(f, leadinv, b + (lb - 1) * L);
  size_t ql = la - lb + 1;
  memset(quo, 0, 8 * L * ql);
  size_t rl = la;
  while (rl >= lb) {
    u64 lead[MAXN], t[MAXN];
    f_mmul(f, lead, rem + (rl - 1) * L, leadinv);
    size_t dd = rl - lb;
    memcpy(quo + dd * L, lead, 8 * L);
    for (size_t i = 0; i < lb; i++) {
      f_mmul(f, t, lead, b + i * L);
      f_sub(f, rem + (dd + i) * L, rem + (dd + i) * L, t);
    }
    rl = trimmed_len(f, rem, rl);
  }
  *rem_len = rl;
  return trimmed_len(f, quo, ql);
}
/* from_monomials, polynomial.rs:202-212: prod (X - x_i); out holds k+1 elements */
static void poly_from_monomials_m(const fld_t* f, const u64* xs, size_t k, u64* out) {
  const int L = f->n;
  memset(out, 0, 8 * L * (k + 1));
  memcpy(out, f->one, 8 * L);
  size_t len = 1;
  for (size_t i = 0; i < k; i++) {
    /* out <- out * (X - x_i):  new[j] = old[j-1] - x_i * old[j], from the top down */
    for (size_t j = len + 1; j-- > 0;) {
      u64 t[MAXN], lo[MAXN];
      memset(lo, 0, sizeof lo);
      if (j > 0) memcpy(lo, out + (j - 1) * L, 8 * L);
      if (j < len) { f_mmul(f, t, out + j * L, xs + i * L); f_sub(f, lo, lo, t); }
      memcpy(out + j * L, lo, 8 * L);
    }
    len++;
  }
}
/* batch_open_kzg, algebra/kzg.rs:74-88: ys[i] = f(us[i]); ip = Lagrange interpolant (polynomial.rs:177-200);
 * f_u = (f - ip) / prod (X - us[i]) by long division; w = MSM(f_u, powers).  Distinct us required (as in
 * the reference, whose interpolate divides by prod (x_j - x_i)). */
int orc_kzg_batch_open_ref(const u64* coef, size_t n, const u64* us, size_t k, const u64* powers_xy,
                           u64* ys_out, u64* w_xy) {
  const fld_t* f = fld_of(FID_FR);
  const int L = 4;
  for (size_t i = 0; i < k; i++) orc_poly_eval(FID_FR, coef, n, us + i * L, ys_out + i * L);
  u64* usm = malloc(8 * L * (k ? k : 1)), *ysm = malloc(8 * L * (k ? k : 1));
  to_mont_vec(f, usm, us, k); to_mont_vec(f, ysm, ys_out, k);
  /* numerators = from_monomials(us) */
  u64* z = malloc(8 * L * (k + 1));
  poly_from_monomials_m(f, usm, k, z);
  /* ip = sum_j y_j * numerators / ((X - u_j) * prod_{i != j} (u_j - u_i)) */
  size_t ipcap = k + 1;
  u64* ip = calloc(ipcap, 8 * L);
  for (size_t j = 0; j < k; j++) {
    u64 den[MAXN];
    memcpy(den, f->one, 8 * L);
    for (size_t i = 0; i < k; i++) {
      if (i == j) continue;
      u64 t[MAXN];
      f_sub(f, t, usm + j * L, usm + i * L);
      f_mmul(f, den, den, t);
    }
    /* divisor = (X - u_j) * den = [-u_j * den, den] */
    u64 dv[2 * MAXN];
    f_mmul(f, dv, usm + j * L, den); f_neg(f, dv, dv);
    memcpy(dv + L, den, 8 * L);
    u64* num = malloc(8 * L * (k + 1)), *q = calloc(k + 1, 8 * L);
    memcpy(num, z, 8 * L * (k + 1));
    size_t rl, ql = poly_divrem_m(f, num, k + 1, dv, 2, q, &rl);
    for (size_t i = 0; i < ql; i++) {
      u64 t[MAXN];
      f_mmul(f, t, q + i * L, ysm + j * L);
      f_add(f, ip + i * L, ip + i * L, t);
    }
    free(num); free(q);
  }
  /* f - ip */
  size_t fl = n > ipcap ? n : ipcap;
  u64* fm = calloc(fl ? fl : 1, 8 * L);
  to_mont_vec(f, fm, coef, n);
  for (size_t i = 0; i < ipcap; i++) f_sub(f, fm + i * L, fm + i * L, ip + i * L);
  u64* quo = calloc(fl ? fl : 1, 8 * L);
  size_t rl, ql = poly_divrem_m(f, fm, fl, z, k + 1, quo, &rl);
  u64* qc = malloc(8 * L * (ql ? ql : 1));
  from_mont_vec(f, qc, quo, ql);
  int rc = orc_msm_ref(qc, powers_xy, ql, w_xy);
  free(usm); free(ysm); free(z); free(ip); free(fm); free(quo); free(qc);
  return rc;
}
/* prove_degree_bound, kzg.rs:121-134: r = f * X^(max_d - d); MSM(r, powers).  n_powers = max_d + 1.
 * d > max_d is the reference's usize underflow -> -5; result longer than the SRS -> index panic -> -5. */
int orc_kzg_prove_degree_bound_ref(const u64* coef, size_t n, const u64* powers_xy, size_t n_powers, size_t d, u64* out_xy) {
  const fld_t* f = fld_of(FID_FR);
  if (n_powers == 0 || d > n_powers - 1) return -5;
  const size_t shift = n_powers - 1 - d;
  size_t tl = 0;
  { u64* cm = malloc(32 * (n ? n : 1)); to_mont_vec(f, cm, coef, n); tl = trimmed_len(f, cm, n); free(cm); }
  if (tl == 0) { memset(out_xy, 0, 64); return 0; }   /* zero polynomial: product is zero */
  if (shift + tl > n_powers) return -5;
  u64* r = calloc(shift + tl, 32);
  memcpy(r + 4 * shift, coef, 32 * tl);
  int rc = orc_msm_ref(r, powers_xy, shift + tl, out_xy);
  free(r);
  return rc;
}

/* ntt::fast_coset_divide, algebra/ntt.rs:271-330 (the quotient step of FastStark::prove, fast_stark.rs:265).
 * Returns: -3 / -4 root order assertions (ntt.rs:282-283), -1 rhs zero (:284), -5 rhs.degree() >= lhs.degree()
 * (:285; a zero lhs has degree -1 and therefore lands here too, before the is_zero early return can be reached).
 * out receives lhs.degree() - rhs.degree() + 1 coefficients (degree < 8: the trimmed quotient of lhs / rhs). */
int orc_fast_coset_divide_ref(int fid, const u64* lhs, size_t ll, const u64* rhs, size_t lr, const u64* offset,
                              const u64* root, size_t root_order, u64* out, size_t* out_len) {
  const fld_t* f = fld_of(fid); if (!f) return -1;
  const int L = f->n;
  u64 rm[MAXN], t[MAXN], om[MAXN];
  f_tomont(f, rm, root);
  f_mpow_u64(f, t, rm, (u64)root_order);
  if (memcmp(t, f->one, 8 * L) != 0) return -3;
  f_mpow_u64(f, t, rm, (u64)(root_order / 2));
  if (memcmp(t, f->one, 8 * L) == 0) return -4;
  u64* lm = malloc(8 * L * (ll ? ll : 1)), *rhm = malloc(8 * L * (lr ? lr : 1));
  to_mont_vec(f, lm, lhs, ll);
  to_mont_vec(f, rhm, rhs, lr);
  const size_t tl = trimmed_len(f, lm, ll), tr = trimmed_len(f, rhm, lr);
  int rc = 0;
  if (tr == 0) rc = -1;
  else if (!((long)tr - 1 < (long)tl - 1)) rc = -5;
  if (rc) { free(lm); free(rhm); return rc; }
  const size_t degree = tl - 1;                       /* max(lhs.degree(), rhs.degree()) */
  if (degree < 8) {                                   /* ntt.rs:295-297: lhs / rhs */
    u64* rem = malloc(8 * L * tl), *quo = malloc(8 * L * tl);
    memcpy(rem, lm, 8 * L * tl);
    size_t rl, ql = poly_divrem_m(f, rem, tl, rhm, tr, quo, &rl);
    from_mont_vec(f, out, quo, ql);
    *out_len = ql;
    free(rem); free(quo); free(lm); free(rhm);
    return 0;
  }
  size_t order = root_order;
  while (degree < order / 2) { f_mmul(f, rm, rm, rm); order /= 2; }      /* ntt.rs:299-302 */
  if (tl > order) {   /* more coefficients than the root's order: the ntt call's own assertions fire (ntt.rs:8-18) */
    free(lm); free(rhm);
    return (tl & (tl - 1)) ? -2 : -3;
  }
  f_tomont(f, om, offset);
  u64* a = calloc(order, 8 * L), *b = calloc(order, 8 * L), *ea = malloc(8 * L * order), *eb = malloc(8 * L * order);
  poly_scale_m(f, a, lm, tl, om);                     /* scaled_lhs.coef[..=deg], zero-padded to order */
  poly_scale_m(f, b, rhm, tr, om);
  rc = ntt_ref_rec(f, rm, a, ea, order);
  if (!rc) rc = ntt_ref_rec(f, rm, b, eb, order);
  if (!rc) {
    for (size_t i = 0; i < order; i++) {              /* el.div_ref(r): el * r.inverse(), inverse(0) = 0 */
      u64 inv[MAXN];
      f_minv(f, inv, eb + i * L);
      f_mmul(f, ea + i * L, ea + i * L, inv);
    }
    /* intt (ntt.rs:50-64): n^-1 * ntt(root^-1, values) */
    u64 rinv[MAXN], ninv[MAXN], nn[MAXN] = {0}, oinv[MAXN];
    f_minv(f, rinv, rm);
    nn[0] = (u64)order;
    f_tomont(f, ninv, nn);
    f_minv(f, ninv, ninv);
    rc = ntt_ref_rec(f, rinv, ea, a, order);
    if (!rc) {
      const size_t ql = tl - tr + 1;
      for (size_t i = 0; i < ql; i++) f_mmul(f, a + i * L, a + i * L, ninv);
      f_minv(f, oinv, om);
      poly_scale_m(f, b, a, ql, oinv);               /* scaled_quotient.scale(&offset.inverse()) */
      from_mont_vec(f, out, b, ql);
      *out_len = ql;
    }
  }
  free(a); free(b); free(ea); free(eb); free(lm); free(rhm);
  return rc;
}

/* ------------------------------------------------------------------------------------------- */
/* G2: the same affine group law over Fq2 = Fq[x]/(x^2 + 1)                    */
/*   Fq2 / G2Point            bn128.rs:33-49;  generator bn128.rs:190-206;  b2 = 3/(9+u) :216-222 */
/*   ExtendedFieldElement     efield.rs: mul = polynomial product mod x^2+1 (:351-353), inverse  */
/*                            = extended Euclid over polynomials (:126-151; inverse(0) = 0) --    */
/*                            restated through the norm, which yields the same field element     */
/*   group law / scalar mul   curve.rs:56-191 (generic over the field)                            */
/* Wire format: x = (c0, c1), y = (c0, c1), 4 limbs each, canonical; all-zero = infinity.         */
/* ------------------------------------------------------------------------------------------- */
typedef struct { u64 c0[MAXN], c1[MAXN]; } fq2_t;            /* Montgomery-domain coefficients */
typedef struct { fq2_t x, y; int inf; } pt2_t;
static const fld_t* fq_fld(void) { return fld_of(FID_FQ); }
static void q2_add(fq2_t* r, const fq2_t* a, const fq2_t* b) { const fld_t* f = fq_fld(); f_add(f, r->c0, a->c0, b->c0); f_add(f, r->c1, a->c1, b->c1); }
static void q2_sub(fq2_t* r, const fq2_t* a, const fq2_t* b) { const fld_t* f = fq_fld(); f_sub(f, r->c0, a->c0, b->c0); f_sub(f, r->c1, a->c1, b->c1); }
static void q2_neg(fq2_t* r, const fq2_t* a) { const fld_t* f = fq_fld(); f_neg(f, r->c0, a->c0); f_neg(f, r->c1, a->c1); }
static void q2_mul(fq2_t* r, const fq2_t* a, const fq2_t* b) {   /* (a0 + a1 x)(b0 + b1 x) mod x^2 + 1 */
  const fld_t* f = fq_fld();
  u64 t0[MAXN], t1[MAXN], t2[MAXN], t3[MAXN];
  f_mmul(f, t0, a->c0, b->c0); f_mmul(f, t1, a->c1, b->c1);
  f_mmul(f, t2, a->c0, b->c1); f_mmul(f, t3, a->c1, b->c0);
  f_sub(f, r->c0, t0, t1);
  f_add(f, r->c1, t2, t3);
}
static void q2_inv(fq2_t* r, const fq2_t* a) {                    /* conj(a) / (a0^2 + a1^2); 0 -> 0 */
  const fld_t* f = fq_fld();
  u64 n[MAXN], t[MAXN];
  f_mmul(f, n, a->c0, a->c0); f_mmul(f, t, a->c1, a->c1);
  f_add(f, n, n, t);
  f_minv(f, n, n);
  f_mmul(f, r->c0, a->c0, n);
  f_mmul(f, t, a->c1, n);
  f_neg(f, r->c1, t);
}
static int q2_eq(const fq2_t* a, const fq2_t* b) { const fld_t* f = fq_fld(); return eq_n(a->c0, b->c0, f->n) && eq_n(a->c1, b->c1, f->n); }
static void pt2_set_inf(pt2_t* p) { memset(p, 0, sizeof *p); p->inf = 1; }
static void pt2_slope(fq2_t* s, const pt2_t* p, const pt2_t* q) {   /* curve.rs:56-70, a = 0 */
  fq2_t num, den, t;
  if (q2_eq(&p->x, &q->x)) {
    q2_mul(&t, &p->x, &p->x);
    q2_add(&num, &t, &t); q2_add(&num, &num, &t);
    q2_add(&den, &p->y, &p->y);
  } else {
    q2_sub(&num, &q->y, &p->y);
    q2_sub(&den, &q->x, &p->x);
  }
  q2_inv(&den, &den);
  q2_mul(s, &num, &den);
}
static void pt2_double(pt2_t* r, const pt2_t* p) {                  /* curve.rs:72-101 */
  if (p->inf) { *r = *p; return; }
  fq2_t s, nx, ny, t;
  pt2_slope(&s, p, p);
  q2_mul(&nx, &s, &s); q2_sub(&nx, &nx, &p->x); q2_sub(&nx, &nx, &p->x);
  q2_mul(&t, &s, &nx); q2_neg(&ny, &t);
  q2_mul(&t, &s, &p->x); q2_sub(&t, &t, &p->y);
  q2_add(&ny, &ny, &t);
  r->x = nx; r->y = ny; r->inf = 0;
}
static void pt2_add(pt2_t* r, const pt2_t* p, const pt2_t* q) {      /* curve.rs:103-129 */
  if (p->inf) { *r = *q; return; }
  if (q->inf) { *r = *p; return; }
  if (q2_eq(&p->x, &q->x)) {
    if (q2_eq(&p->y, &q->y)) { pt2_double(r, p); return; }
    pt2_set_inf(r); return;
  }
  fq2_t s, nx, ny, t;
  pt2_slope(&s, p, q);
  q2_mul(&nx, &s, &s); q2_sub(&nx, &nx, &p->x); q2_sub(&nx, &nx, &q->x);
  q2_mul(&t, &s, &nx); q2_neg(&ny, &t);
  q2_mul(&t, &s, &p->x); q2_sub(&t, &t, &p->y);
  q2_add(&ny, &ny, &t);
  r->x = nx; r->y = ny; r->inf = 0;
}
static void pt2_mul(pt2_t* r, const pt2_t* p, const u64* k, int nk) { /* curve.rs:168-191 */
  pt2_t result, cur = *p;
  pt2_set_inf(&result);
  int top = nk * 64 - 1;
  while (top >= 0 && !((k[top / 64] >> (top % 64)) & 1)) top--;
  for (int i = 0; i <= top; i++) {
    if ((k[i / 64] >> (i % 64)) & 1) pt2_add(&result, &result, &cur);
    pt2_double(&cur, &cur);
  }
  *r = result;
}
static void pt2_load(pt2_t* p, const u64* w) {
  const fld_t* f = fq_fld();
  if (is_zero_n(w, 4 * f->n)) { pt2_set_inf(p); return; }
  f_tomont(f, p->x.c0, w); f_tomont(f, p->x.c1, w + f->n); f_tomont(f, p->y.c0, w + 2 * f->n); f_tomont(f, p->y.c1, w + 3 * f->n);
  p->inf = 0;
}
static void pt2_store(u64* w, const pt2_t* p) {
  const fld_t* f = fq_fld();
  if (p->inf) { memset(w, 0, 32 * f->n); return; }
  f_frommont(f, w, p->x.c0); f_frommont(f, w + f->n, p->x.c1); f_frommont(f, w + 2 * f->n, p->y.c0); f_frommont(f, w + 3 * f->n, p->y.c1);
}
int orc_g2_add(const u64* p, const u64* q, u64* out) { pt2_t a, b, r; pt2_load(&a, p); pt2_load(&b, q); pt2_add(&r, &a, &b); pt2_store(out, &r); return 0; }
int orc_g2_double(const u64* p, u64* out) { pt2_t a, r; pt2_load(&a, p); pt2_double(&r, &a); pt2_store(out, &r); return 0; }
int orc_g2_mul(const u64* p, const u64* k, int nk, u64* out) { pt2_t a, r; pt2_load(&a, p); pt2_mul(&r, &a, k, nk); pt2_store(out, &r); return 0; }
/* y^2 - x^3 == 3 / (9 + u)   (bn128.rs:216-222, test_g2 :309-314) */
int orc_g2_on_curve(const u64* w) {
  const fld_t* f = fq_fld();
  pt2_t p; pt2_load(&p, w);
  if (p.inf) return 1;
  fq2_t y2, x3, lhs, three = {{0}, {0}}, nine_u = {{0}, {0}}, b2;
  u64 t[MAXN] = {3, 0, 0, 0}; f_tomont(f, three.c0, t);
  t[0] = 9; f_tomont(f, nine_u.c0, t); t[0] = 1; f_tomont(f, nine_u.c1, t);
  q2_inv(&nine_u, &nine_u); q2_mul(&b2, &three, &nine_u);
  q2_mul(&y2, &p.y, &p.y); q2_mul(&x3, &p.x, &p.x); q2_mul(&x3, &x3, &p.x);
  q2_sub(&lhs, &y2, &x3);
  return q2_eq(&lhs, &b2);
}
/* Polynomial::eval_with_powers_on_curve over G2 (polynomial.rs:156-165; kzg.rs:114), literal */
int orc_g2_msm_ref(const u64* scalars, const u64* points, size_t n, u64* out) {
  pt2_t acc; pt2_set_inf(&acc);
  for (size_t i = 0; i < n; i++) {
    pt2_t p, t;
    pt2_load(&p, points + 16 * i);
    pt2_mul(&t, &p, scalars + 4 * i, 4);
    pt2_add(&acc, &acc, &t);
  }
  pt2_store(out, &acc);
  return 0;
}
/* setup_kzg_with_full_g2's powers_2 (kzg.rs:42-55): [alpha^i] g2, i <= max_d, alpha_power a running product */
int orc_kzg_setup_g2_ref(const u64* g2, const u64* alpha, size_t max_d, u64* powers) {
  const fld_t* fr = fld_of(FID_FR);
  pt2_t g; pt2_load(&g, g2);
  u64 am[MAXN], cur[MAXN], plain[MAXN];
  f_tomont(fr, am, alpha);
  memcpy(cur, fr->one, 8 * fr->n);
  for (size_t i = 0; i <= max_d; i++) {
    pt2_t t;
    f_frommont(fr, plain, cur);
    pt2_mul(&t, &g, plain, 4);
    pt2_store(powers + 16 * i, &t);
    f_mmul(fr, cur, cur, am);
  }
  return 0;
}

/* ---- ntt::fast_zerofier / fast_evaluate / fast_interpolate, algebra/ntt.rs:118-252 -------------------------
 * Literal restatement of the three recursions (half = len / 2, fast_multiply for the zerofier products, schoolbook
 * `%` = div_rem_ref for the remainders, `*` and `+` of reduced polynomials for the final interpolant).  Polynomials
 * are Montgomery-form coefficient arrays with the reference's Vec length (fast_multiply leaves its NTT branch
 * untrimmed).  Return codes: 0, -3 / -4 the two root assertions, -5 an operand longer than the transform order
 * (the reference's inner ntt would panic), -6 mismatching lengths. */
typedef struct { u64* c; size_t len; } poly_t;
static void poly_free(poly_t* p) { free(p->c); p->c = NULL; p->len = 0; }
/* fast_multiply on Montgomery operands (ntt.rs:66-116); rm = Montgomery root */
static int fast_multiply_m(const fld_t* f, const poly_t* a, const poly_t* b, const u64* rm0, size_t root_order, poly_t* out) {
  const int L = f->n;
  u64 rm[MAXN], t[MAXN];
  memcpy(rm, rm0, 8 * L);
  f_mpow_u64(f, t, rm, root_order);
  if (!eq_n(t, f->one, L)) return -3;
  f_mpow_u64(f, t, rm, root_order / 2);
  if (eq_n(t, f->one, L)) return -4;
  out->c = NULL; out->len = 0;
  size_t da = trimmed_len(f, a->c, a->len), db = trimmed_len(f, b->c, b->len);
  if (da == 0 || db == 0) return 0;
  size_t degree = (da - 1) + (db - 1);
  if (degree < 8) {
    out->c = malloc(8 * L * (da + db));
    out->len = poly_mul_school_m(f, a->c, a->len, b->c, b->len, out->c);
    return 0;
  }
  size_t order = root_order;
  while (degree < order / 2) { f_mmul(f, rm, rm, rm); order /= 2; }
  if (a->len > order || b->len > order) return -5;
  u64* x = calloc(order, 8 * L), *y = calloc(order, 8 * L), *X = malloc(8 * L * order), *Y = malloc(8 * L * order);
  memcpy(x, a->c, 8 * L * a->len); memcpy(y, b->c, 8 * L * b->len);
  int rc = ntt_ref_rec(f, rm, x, X, order);
  if (!rc) rc = ntt_ref_rec(f, rm, y, Y, order);
  if (!rc) {
    for (size_t i = 0; i < order; i++) f_mmul(f, X + i * L, X + i * L, Y + i * L);
    u64 rinv[MAXN], nn[MAXN] = {0}, ninv[MAXN];
    f_minv(f, rinv, rm);
    nn[0] = order; f_tomont(f, ninv, nn); f_minv(f, ninv, ninv);
    rc = ntt_ref_rec(f, rinv, X, Y, order);
    if (!rc) {
      for (size_t i = 0; i < order; i++) f_mmul(f, Y + i * L, ninv, Y + i * L);
      out->c = Y; out->len = order; Y = NULL;
    }
  }
  free(x); free(y); free(X); free(Y);
  return rc;
}
/* ntt.rs:118-144 */
static int fast_zerofier_m(const fld_t* f, const u64* dom, size_t n, const u64* rm, size_t root_order, poly_t* out) {
  const int L = f->n;
  u64 t[MAXN];
  f_mpow_u64(f, t, rm, root_order);
  if (!eq_n(t, f->one, L)) return -3;
  f_mpow_u64(f, t, rm, root_order / 2);
  if (eq_n(t, f->one, L)) return -4;
  out->c = NULL; out->len = 0;
  if (n == 0) return 0;
  if (n == 1) {
    out->c = malloc(8 * L * 2); out->len = 2;
    f_neg(f, out->c, dom);                       /* F::zero() - &domain[0] */
    memcpy(out->c + L, f->one, 8 * L);
    return 0;
  }
  size_t half = n / 2;
  poly_t l, r;
  int rc = fast_zerofier_m(f, dom, half, rm, root_order, &l);
  if (rc) return rc;
  rc = fast_zerofier_m(f, dom + half * L, n - half, rm, root_order, &r);
  if (rc) { poly_free(&l); return rc; }
  rc = fast_multiply_m(f, &l, &r, rm, root_order, out);
  poly_free(&l); poly_free(&r);
  return rc;
}
/* Polynomial::eval, polynomial.rs:120-128 (over the whole Vec) */
static void poly_eval_m(const fld_t* f, const poly_t* p, const u64* x, u64* out) {
  const int L = f->n;
  u64 res[MAXN] = {0}, tp[MAXN], t[MAXN];
  memcpy(tp, f->one, 8 * L);
  for (size_t i = 0; i < p->len; i++) {
    f_mmul(f, t, tp, p->c + i * L);
    f_add(f, res, res, t);
    f_mmul(f, tp, tp, x);
  }
  memcpy(out, res, 8 * L);
}
/* `a % b` (polynomial.rs:607-612 -> div_rem_ref :371-405): remainder, trimmed; a zero divisor returns a itself */
static void poly_rem_m(const fld_t* f, const poly_t* a, const poly_t* b, poly_t* out) {
  const int L = f->n;
  out->c = malloc(8 * L * (a->len ? a->len : 1));
  memcpy(out->c, a->c, 8 * L * a->len);
  size_t lb = trimmed_len(f, b->c, b->len), la = trimmed_len(f, a->c, a->len);
  if (lb == 0 || la < lb) { out->len = a->len; return; }       /* (zero, self.clone()) */
  u64* quo = malloc(8 * L * (la - lb + 1));
  size_t rl;
  poly_divrem_m(f, out->c, a->len, b->c, b->len, quo, &rl);
  free(quo);
  out->len = rl;
}
/* ntt.rs:146-189; out: n Montgomery values */
static int fast_evaluate_m(const fld_t* f, const poly_t* p, const u64* dom, size_t n, const u64* rm, size_t root_order, u64* out) {
  const int L = f->n;
  u64 t[MAXN];
  f_mpow_u64(f, t, rm, root_order);
  if (!eq_n(t, f->one, L)) return -3;
  f_mpow_u64(f, t, rm, root_order / 2);
  if (eq_n(t, f->one, L)) return -4;
  if (n == 0) return 0;
  if (n == 1) { poly_eval_m(f, p, dom, out); return 0; }
  size_t half = n / 2;
  poly_t lz, rz, lr, rr;
  int rc = fast_zerofier_m(f, dom, half, rm, root_order, &lz);
  if (rc) return rc;
  rc = fast_zerofier_m(f, dom + half * L, n - half, rm, root_order, &rz);
  if (rc) { poly_free(&lz); return rc; }
  poly_rem_m(f, p, &lz, &lr);
  poly_rem_m(f, p, &rz, &rr);
  rc = fast_evaluate_m(f, &lr, dom, half, rm, root_order, out);
  if (!rc) rc = fast_evaluate_m(f, &rr, dom + half * L, n - half, rm, root_order, out + half * L);
  poly_free(&lz); poly_free(&rz); poly_free(&lr); poly_free(&rr);
  return rc;
}
/* ntt.rs:191-252 */
static int fast_interpolate_m(const fld_t* f, const u64* dom, const u64* val, size_t n, const u64* rm, size_t root_order, poly_t* out) {
  const int L = f->n;
  u64 t[MAXN];
  f_mpow_u64(f, t, rm, root_order);
  if (!eq_n(t, f->one, L)) return -3;
  f_mpow_u64(f, t, rm, root_order / 2);
  if (eq_n(t, f->one, L)) return -4;
  out->c = NULL; out->len = 0;
  if (n == 0) return 0;
  if (n == 1) { out->c = malloc(8 * L); memcpy(out->c, val, 8 * L); out->len = 1; return 0; }
  size_t half = n / 2, rest = n - half;
  poly_t lz = {0}, rz = {0}, li = {0}, ri = {0};
  u64* loff = malloc(8 * L * half), *roff = malloc(8 * L * rest), *ltar = malloc(8 * L * half), *rtar = malloc(8 * L * rest);
  int rc = fast_zerofier_m(f, dom, half, rm, root_order, &lz);
  if (!rc) rc = fast_zerofier_m(f, dom + half * L, rest, rm, root_order, &rz);
  if (!rc) rc = fast_evaluate_m(f, &rz, dom, half, rm, root_order, loff);
  if (!rc) rc = fast_evaluate_m(f, &lz, dom + half * L, rest, rm, root_order, roff);
  if (!rc) {
    u64 inv[MAXN];
    for (size_t i = 0; i < half; i++) { f_minv(f, inv, loff + i * L); f_mmul(f, ltar + i * L, val + i * L, inv); }              /* n.div_ref(d), inverse(0) = 0 */
    for (size_t i = 0; i < rest; i++) { f_minv(f, inv, roff + i * L); f_mmul(f, rtar + i * L, val + (half + i) * L, inv); }
    rc = fast_interpolate_m(f, dom, ltar, half, rm, root_order, &li);
    if (!rc) rc = fast_interpolate_m(f, dom + half * L, rtar, rest, rm, root_order, &ri);
  }
  if (!rc) {
    /* left_interpolant.reduce() * right_zerofier.reduce() + right_interpolant.reduce() * left_zerofier.reduce() */
    u64* p1 = malloc(8 * L * (li.len + rz.len + 1)), *p2 = malloc(8 * L * (ri.len + lz.len + 1));
    size_t l1 = poly_mul_school_m(f, li.c, li.len, rz.c, rz.len, p1), l2 = poly_mul_school_m(f, ri.c, ri.len, lz.c, lz.len, p2);
    size_t lm = l1 > l2 ? l1 : l2;
    out->c = calloc(lm ? lm : 1, 8 * L);
    for (size_t i = 0; i < lm; i++) {
      if (i < l1) f_add(f, out->c + i * L, out->c + i * L, p1 + i * L);
      if (i < l2) f_add(f, out->c + i * L, out->c + i * L, p2 + i * L);
    }
    out->len = trimmed_len(f, out->c, lm);
    free(p1); free(p2);
  }
  poly_free(&lz); poly_free(&rz); poly_free(&li); poly_free(&ri);
  free(loff); free(roff); free(ltar); free(rtar);
  return rc;
}
/* plain-domain wrappers.  out of the zerofier must hold max(n + 1, 2 * next_pow2(n + 1)) elements. */
int orc_fast_zerofier_ref(int fid, const u64* domain, size_t n, const u64* root, size_t root_order, u64* out, size_t* out_len) {
  const fld_t* f = fld_of(fid); if (!f) return -1;
  const int L = f->n;
  u64 rm[MAXN];
  f_tomont(f, rm, root);
  u64* dm = malloc(8 * L * (n ? n : 1));
  to_mont_vec(f, dm, domain, n);
  poly_t z;
  int rc = fast_zerofier_m(f, dm, n, rm, root_order, &z);
  if (!rc) { from_mont_vec(f, out, z.c, z.len); *out_len = z.len; poly_free(&z); }
  free(dm);
  return rc;
}
int orc_fast_evaluate_ref(int fid, const u64* coef, size_t m, const u64* domain, size_t n, const u64* root, size_t root_order, u64* out) {
  const fld_t* f = fld_of(fid); if (!f) return -1;
  const int L = f->n;
  u64 rm[MAXN];
  f_tomont(f, rm, root);
  u64* dm = malloc(8 * L * (n ? n : 1)), *cm = malloc(8 * L * (m ? m : 1)), *om = malloc(8 * L * (n ? n : 1));
  to_mont_vec(f, dm, domain, n); to_mont_vec(f, cm, coef, m);
  poly_t p = {cm, m};
  int rc = fast_evaluate_m(f, &p, dm, n, rm, root_order, om);
  if (!rc) from_mont_vec(f, out, om, n);
  free(dm); free(cm); free(om);
  return rc;
}
int orc_fast_interpolate_ref(int fid, const u64* domain, const u64* values, size_t n, const u64* root, size_t root_order, u64* out, size_t* out_len) {
  const fld_t* f = fld_of(fid); if (!f) return -1;
  const int L = f->n;
  u64 rm[MAXN];
  f_tomont(f, rm, root);
  u64* dm = malloc(8 * L * (n ? n : 1)), *vm = malloc(8 * L * (n ? n : 1));
  to_mont_vec(f, dm, domain, n); to_mont_vec(f, vm, values, n);
  poly_t p;
  int rc = fast_interpolate_m(f, dm, vm, n, rm, root_order, &p);
  if (!rc) { from_mont_vec(f, out, p.c, p.len); *out_len = p.len; poly_free(&p); }
  free(dm); free(vm);
  return rc;
}
