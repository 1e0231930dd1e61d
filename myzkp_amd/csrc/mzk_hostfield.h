// mzk_hostfield.h -- the host arithmetic on field parameters (O(log n) scalar work: roots, n^-1, canonical checks, table entries; never
// on the data path), once for every translation unit: values are canonical, nl little-endian u64 limbs (Fr, Fq: 4; M128: 2), products
// are Montgomery on those limbs.  With it the two decisions built directly on it: the reference's pair of assertions on a root and its
// order (h_root_check) and one Shoup table entry of the transforms (h_shoup_entry).  Host-only C++17 with no HIP include, so that it
// can be compiled and checked on its own against Python integers (tests/test_hostcheck_hostfield.py).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "../../include/mzk.h"

namespace mzk {

// Element shapes per field id.  Goldilocks ids (mzk_gl.h): one or three canonical u64 per element, no Montgomery parameter set -- a
// kernel family of their own
static inline bool field_is_gl(int fid) { return fid == MZK_FIELD_M64 || fid == MZK_FIELD_M64X3; }
static inline int field_gl_comps(int fid) { return fid == MZK_FIELD_M64X3 ? 3 : 1; }
static inline int field_words(int fid) { return field_is_gl(fid) ? 2 * field_gl_comps(fid) : (fid == MZK_FIELD_M128 ? 4 : 8); }   // u32 words per element
static inline int field_limbs64(int fid) { return field_is_gl(fid) ? field_gl_comps(fid) : (fid == MZK_FIELD_M128 ? 2 : 4); }
static inline size_t field_bytes(int fid) { return 8 * (size_t)field_limbs64(fid); }

// 29-bit limbs of the device's elements (FrParams::L, FqParams::L, M128Params::L: mzk_api.hip holds the static_assert)
constexpr int HOST_LIMBS29_FR = 9, HOST_LIMBS29_FQ = 9, HOST_LIMBS29_M128 = 5;

struct HostField {
  int nl;            // u64 limbs
  uint64_t p[4];
  int mont_bits;     // the device's Montgomery radix is R = 2^mont_bits (29 bits per limb: mzk_field.h)
  uint64_t n0;       // the host's own Montgomery constants (64-bit limbs): -p^-1 mod 2^64 ...
  uint64_t r2[4];    // ... and 2^(128 nl) mod p
};

inline int h_cmp(const uint64_t* a, const uint64_t* b, int n) {
  for (int i = n - 1; i >= 0; i--) if (a[i] != b[i]) return a[i] > b[i] ? 1 : -1;
  return 0;
}
// r = a - b over n limbs; the borrow out
inline uint64_t h_sub_limbs(uint64_t* r, const uint64_t* a, const uint64_t* b, int n) {
  uint64_t br = 0;
  for (int i = 0; i < n; i++) {
    const unsigned __int128 d = (unsigned __int128)a[i] - b[i] - br;
    r[i] = (uint64_t)d; br = (uint64_t)(d >> 64) & 1;
  }
  return br;
}
inline bool h_is_canonical(const HostField* f, const uint64_t* a) { return h_cmp(a, f->p, f->nl) < 0; }
inline bool h_is_zero(const HostField* f, const uint64_t* a) {
  for (int i = 0; i < f->nl; i++) if (a[i]) return false;
  return true;
}
inline bool h_is_one(const HostField* f, const uint64_t* a) {
  if (a[0] != 1) return false;
  for (int i = 1; i < f->nl; i++) if (a[i]) return false;
  return true;
}
// a + b, -a (0 -> 0, as the reference's sanitize()), a - b for canonical a, b; r may be an operand
inline void h_addmod(const HostField* f, uint64_t* r, const uint64_t* a, const uint64_t* b) {
  uint64_t t[4] = {0, 0, 0, 0};
  unsigned __int128 c = 0;
  for (int i = 0; i < f->nl; i++) { c += (unsigned __int128)a[i] + b[i]; t[i] = (uint64_t)c; c >>= 64; }
  if (c || h_cmp(t, f->p, f->nl) >= 0) h_sub_limbs(t, t, f->p, f->nl);
  for (int i = 0; i < f->nl; i++) r[i] = t[i];
}
inline void h_negmod(const HostField* f, uint64_t* r, const uint64_t* a) {
  if (h_is_zero(f, a)) { for (int i = 0; i < f->nl; i++) r[i] = 0; return; }
  h_sub_limbs(r, f->p, a, f->nl);
}
inline void h_submod(const HostField* f, uint64_t* r, const uint64_t* a, const uint64_t* b) {
  uint64_t nb[4] = {0, 0, 0, 0};
  h_negmod(f, nb, b);
  h_addmod(f, r, a, nb);
}
// double-and-add product: O(bits) modular additions.  The cross-check of the fast product below (mzk_host_field_op op 3).
inline void h_mulmod_slow(const HostField* f, uint64_t* r, const uint64_t* a, const uint64_t* b) {
  uint64_t acc[4] = {0, 0, 0, 0}, aa[4] = {0, 0, 0, 0}, bb[4] = {0, 0, 0, 0};
  for (int i = 0; i < f->nl; i++) { aa[i] = a[i]; bb[i] = b[i]; }
  for (int bit = 64 * f->nl - 1; bit >= 0; bit--) {
    h_addmod(f, acc, acc, acc);
    if ((bb[bit / 64] >> (bit % 64)) & 1) h_addmod(f, acc, acc, aa);
  }
  for (int i = 0; i < f->nl; i++) r[i] = acc[i];
}

// The three fields, their Montgomery constants derived once per process (a function-local static of an inline function: one
// definition program-wide, filled on the first call, never per product).
inline HostField host_field_make(int nl, uint64_t p0, uint64_t p1, uint64_t p2, uint64_t p3, int limbs29) {
  HostField f = {nl, {p0, p1, p2, p3}, 29 * limbs29, 0, {1, 0, 0, 0}};
  uint64_t inv = p0;                                          // Newton: p0 * p0 == 1 mod 8
  for (int i = 0; i < 6; i++) inv *= 2 - p0 * inv;
  f.n0 = (uint64_t)0 - inv;
  for (int i = 0; i < 128 * nl; i++) h_addmod(&f, f.r2, f.r2, f.r2);      // 2^(128 nl) mod p by 128 nl modular doublings
  return f;
}
inline const HostField* host_field(int fid) {
  static_assert(MZK_FIELD_FR == 0 && MZK_FIELD_M128 == 1 && MZK_FIELD_FQ == 2, "the table below is indexed by field id");
  static const HostField table[3] = {
      host_field_make(4, 0x43e1f593f0000001ULL, 0x2833e84879b97091ULL, 0xb85045b68181585dULL, 0x30644e72e131a029ULL, HOST_LIMBS29_FR),
      host_field_make(2, 1ULL, 407ULL << 55, 0, 0, HOST_LIMBS29_M128),
      host_field_make(4, 0x3c208c16d87cfd47ULL, 0x97816a916871ca8dULL, 0xb85045b68181585dULL, 0x30644e72e131a029ULL, HOST_LIMBS29_FQ)};
  return fid >= 0 && fid < 3 ? &table[fid] : nullptr;
}

// a * b / 2^(64 nl) mod p (CIOS), inputs < p
inline void h_montmul(const HostField* f, uint64_t* r, const uint64_t* a, const uint64_t* b) {
  const int n = f->nl;
  uint64_t t[6] = {0, 0, 0, 0, 0, 0};
  for (int i = 0; i < n; i++) {
    unsigned __int128 c = 0;
    for (int j = 0; j < n; j++) { c += (unsigned __int128)a[j] * b[i] + t[j]; t[j] = (uint64_t)c; c >>= 64; }
    c += t[n]; t[n] = (uint64_t)c; t[n + 1] = (uint64_t)(c >> 64);
    const uint64_t q = t[0] * f->n0;
    c = (unsigned __int128)q * f->p[0] + t[0];
    c >>= 64;
    for (int j = 1; j < n; j++) { c += (unsigned __int128)q * f->p[j] + t[j]; t[j - 1] = (uint64_t)c; c >>= 64; }
    c += t[n]; t[n - 1] = (uint64_t)c;
    t[n] = t[n + 1] + (uint64_t)(c >> 64);
  }
  if (t[n] || h_cmp(t, f->p, n) >= 0) h_sub_limbs(t, t, f->p, n);
  for (int i = 0; i < n; i++) r[i] = t[i];
}
// a * b mod p for canonical a, b: mont(mont(a, b), R^2)
inline void h_mulmod(const HostField* f, uint64_t* r, const uint64_t* a, const uint64_t* b) {
  uint64_t t[4] = {0, 0, 0, 0};
  h_montmul(f, t, a, b);
  h_montmul(f, r, t, f->r2);
}
// a^e for an exponent of ne limbs: square and multiply from the low bit up to the highest one set
inline void h_powmod(const HostField* f, uint64_t* r, const uint64_t* a, const uint64_t* e, int ne) {
  uint64_t res[4] = {1, 0, 0, 0}, base[4] = {0, 0, 0, 0};
  for (int i = 0; i < f->nl; i++) base[i] = a[i];
  int top = 64 * ne;
  while (top > 0 && !((e[(top - 1) / 64] >> ((top - 1) % 64)) & 1)) top--;
  for (int bit = 0; bit < top; bit++) {
    if ((e[bit / 64] >> (bit % 64)) & 1) h_mulmod(f, res, res, base);
    if (bit + 1 < top) h_mulmod(f, base, base, base);
  }
  for (int i = 0; i < f->nl; i++) r[i] = res[i];
}
inline void h_powmod_u64(const HostField* f, uint64_t* r, const uint64_t* a, uint64_t e) { h_powmod(f, r, a, &e, 1); }
// a^(p-2) (0 -> 0)
inline void h_invmod(const HostField* f, uint64_t* r, const uint64_t* a) {
  const uint64_t two[4] = {2, 0, 0, 0};
  uint64_t e[4] = {0, 0, 0, 0};
  h_sub_limbs(e, f->p, two, f->nl);
  h_powmod(f, r, a, e, f->nl);
}
// (2^k)^-1 mod p where n = 2^k divides p - 1:  n * ((p-1)/n) = -1 (mod p)  =>  n^-1 = p - (p-1)/n
inline void h_ninv_pow2(const HostField* f, unsigned k, uint64_t* out) {
  uint64_t q[4] = {0, 0, 0, 0};
  for (int i = 0; i < f->nl; i++) q[i] = f->p[i];
  q[0] -= 1;  // p is odd
  for (unsigned s = 0; s < k; s++) {
    for (int i = 0; i < f->nl; i++) q[i] = (q[i] >> 1) | ((i + 1 < f->nl) ? (q[i + 1] << 63) : 0);
  }
  h_sub_limbs(out, f->p, q, f->nl);
}
// R mod p: x -> x R mod p is one h_mulmod with it
inline void h_rmod(const HostField* f, uint64_t* out) {
  const uint64_t two[4] = {2, 0, 0, 0};
  h_powmod_u64(f, out, two, (uint64_t)f->mont_bits);
}
// One element as a kernel argument (Words8, mzk_elem.h), words [2 nl, 8) zero: limbs -> words, and (v R mod p) -> words
inline void h_words(const uint64_t* v, int nl, uint32_t out8[8]) {
  for (int i = 0; i < 8; i++) out8[i] = i < 2 * nl ? (uint32_t)(v[i / 2] >> (32 * (i & 1))) : 0u;
}
inline void h_mont_words(const HostField* f, const uint64_t* v, uint32_t out8[8]) {
  uint64_t r[4], t[4];
  h_rmod(f, r);
  h_mulmod(f, t, v, r);
  h_words(t, f->nl, out8);
}

// The reference's two assertions on a root and its order (ntt.rs:75-76, :122-123, :282-283 ...) for a canonical root: MZK_OK, or
// the code with the assertion's text in *msg.
inline int h_root_check(const HostField* f, const uint64_t* root, uint64_t root_order, const char** msg) {
  uint64_t t[4] = {0, 0, 0, 0};
  h_powmod_u64(f, t, root, root_order);
  if (!h_is_one(f, t)) { *msg = "assertion failed: primitive_root.pow(root_order).is_one()"; return MZK_E_ROOT_ORDER; }
  h_powmod_u64(f, t, root, root_order / 2);
  if (h_is_one(f, t)) { *msg = "assertion failed: !primitive_root.pow(root_order / 2).is_one()"; return MZK_E_ROOT_PRIM; }
  *msg = "";
  return MZK_OK;
}

// One Shoup table entry of the transforms' in-tile twiddles for a canonical v of a four-limb field (Fr): the nine 29-bit limbs of v
// at words [0, 9), those of floor(v 2^261 / p) at [16, 25) of the 32-word entry; the other words are left as they are.
constexpr int SHOUP_ENTRY_WORDS = 32;
inline void h_limbs29(const uint64_t* v5, uint32_t* dst) {      // 9 limbs of 29 bits from a 5 x 64-bit number
  for (int i = 0; i < 9; i++) {
    const int bit = 29 * i, k = bit >> 6, sft = bit & 63;
    uint64_t x = v5[k] >> sft;
    if (sft > 35 && k + 1 < 5) x |= v5[k + 1] << (64 - sft);
    dst[i] = (uint32_t)(x & 0x1fffffffu);
  }
}
inline void h_shoup_entry(const HostField* f, const uint64_t* v, uint32_t* entry) {
  const uint64_t v5[5] = {v[0], v[1], v[2], v[3], 0};
  h_limbs29(v5, entry);
  // q = floor(v 2^261 / p): restoring division, one quotient bit per step (v < p < 2^254, so the remainder stays below 2^255)
  uint64_t rem[4] = {v[0], v[1], v[2], v[3]}, q[5] = {0, 0, 0, 0, 0};
  for (int step = 0; step < 261; step++) {
    for (int i = 4; i > 0; i--) q[i] = (q[i] << 1) | (q[i - 1] >> 63);
    q[0] <<= 1;
    for (int i = 3; i > 0; i--) rem[i] = (rem[i] << 1) | (rem[i - 1] >> 63);
    rem[0] <<= 1;
    if (h_cmp(rem, f->p, 4) >= 0) { h_sub_limbs(rem, rem, f->p, 4); q[0] |= 1; }
  }
  h_limbs29(q, entry + 16);
}

}  // namespace mzk
