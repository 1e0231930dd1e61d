// mzk_gl.h -- the 64-bit Goldilocks prime field and its cubic extension, for the second instantiation of the reference's FRI
// (zkstark/fri.rs:409-421, test_fri_efield :546-594): M64 = F_p with p = 2^64 - 2^32 + 1, and
// ExtendedFieldElement<M64, Ip3> = F_p[x] / (x^3 - x + 1).
//
// Representation: one canonical uint64_t (< p) per base element, no Montgomery form; an extension element is its three
// coefficients c0 + c1 x + c2 x^2.  Every function takes canonical operands and returns a canonical result.
//
// A product is a 64 x 64 -> 128-bit multiplication (four 32 x 32 multiply-adds on gfx950) and a reduction of shifts and adds:
//   2^64 = 2^32 - 1 (mod p)   and   2^96 = -1 (mod p),
// so  lo + 2^64 hi_lo + 2^96 hi_hi  =  lo - hi_hi + (2^32 - 1) hi_lo.
//
// Plain C++: the same code compiles for the device and, like mzk_field.h, with g++ for the host unit tests (tests/hostcheck).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define MZK_GL_HD __host__ __device__ __forceinline__
#else
#define MZK_GL_HD inline
#endif

namespace mzk {
namespace gl {

constexpr uint64_t P = 0xFFFFFFFF00000001ULL;
constexpr uint64_t EPS = 0xFFFFFFFFULL;                     // 2^64 mod p
constexpr uint64_t ROOT_2_32 = 1753635133440165772ULL;      // of order 2^32: get_nth_root_of_m64, fri.rs:449-473
constexpr unsigned TWO_ADICITY = 32;

MZK_GL_HD bool is_canonical(uint64_t a) { return a < P; }

MZK_GL_HD uint64_t add(uint64_t a, uint64_t b) {
  uint64_t s = a + b;
  if (s < a) return s + EPS;                                // a + b - 2^64 + (2^64 - p) = a + b - p < p
  return s >= P ? s - P : s;
}
MZK_GL_HD uint64_t sub(uint64_t a, uint64_t b) {
  const uint64_t d = a - b;
  return a < b ? d - EPS : d;                               // + p (mod 2^64)
}
MZK_GL_HD uint64_t neg(uint64_t a) { return a ? P - a : 0; }

// (hi, lo) = a 128-bit value  ->  its residue, canonical
MZK_GL_HD uint64_t reduce128(uint64_t lo, uint64_t hi) {
  const uint64_t hi_hi = hi >> 32, hi_lo = hi & EPS;
  uint64_t t0 = lo - hi_hi;
  if (lo < hi_hi) t0 -= EPS;                                // borrowed 2^64: give back 2^64 - p
  const uint64_t t1 = hi_lo * EPS;                          // (2^32 - 1)^2 < 2^64
  uint64_t r = t0 + t1;
  if (r < t1) r += EPS;                                     // carried 2^64 = 2^32 - 1; cannot carry again (t0 + t1 < 2^65 - 2^33)
  return r >= P ? r - P : r;
}
MZK_GL_HD void mul_wide(uint64_t a, uint64_t b, uint64_t* lo, uint64_t* hi) {
#if defined(__HIP_DEVICE_COMPILE__)
  *lo = a * b;
  *hi = __umul64hi(a, b);
#else
  const unsigned __int128 t = (unsigned __int128)a * b;
  *lo = (uint64_t)t;
  *hi = (uint64_t)(t >> 64);
#endif
}
MZK_GL_HD uint64_t mul(uint64_t a, uint64_t b) {
  uint64_t lo, hi;
  mul_wide(a, b, &lo, &hi);
  return reduce128(lo, hi);
}
MZK_GL_HD uint64_t sqr(uint64_t a) { return mul(a, a); }

// a^e by square and multiply: parameters on the host, a lane's starting power on the device
MZK_GL_HD uint64_t pow(uint64_t a, uint64_t e) {
  uint64_t r = 1;
  while (e) {
    if (e & 1) r = mul(r, a);
    a = sqr(a);
    e >>= 1;
  }
  return r;
}
// a^(p-2); inv(0) = 0.  Parameters only (omega^-1, offset^-1, n^-1, 2^-1).
inline uint64_t inv(uint64_t a) { return pow(a, P - 2); }

// ---- F_p[x] / (x^3 - x + 1) ---------------------------------------------------------------------------------------------
struct Ext { uint64_t c[3]; };

MZK_GL_HD Ext ext_make(uint64_t c0, uint64_t c1, uint64_t c2) { Ext r; r.c[0] = c0; r.c[1] = c1; r.c[2] = c2; return r; }
MZK_GL_HD Ext ext_add(const Ext& a, const Ext& b) { return ext_make(add(a.c[0], b.c[0]), add(a.c[1], b.c[1]), add(a.c[2], b.c[2])); }
MZK_GL_HD Ext ext_sub(const Ext& a, const Ext& b) { return ext_make(sub(a.c[0], b.c[0]), sub(a.c[1], b.c[1]), sub(a.c[2], b.c[2])); }
MZK_GL_HD Ext ext_neg(const Ext& a) { return ext_make(neg(a.c[0]), neg(a.c[1]), neg(a.c[2])); }
MZK_GL_HD Ext ext_scale(const Ext& a, uint64_t s) { return ext_make(mul(a.c[0], s), mul(a.c[1], s), mul(a.c[2], s)); }
// schoolbook: d0 .. d4, then x^3 = x - 1 and x^4 = x^2 - x
MZK_GL_HD Ext ext_mul(const Ext& a, const Ext& b) {
  const uint64_t d0 = mul(a.c[0], b.c[0]);
  const uint64_t d1 = add(mul(a.c[0], b.c[1]), mul(a.c[1], b.c[0]));
  const uint64_t d2 = add(add(mul(a.c[0], b.c[2]), mul(a.c[1], b.c[1])), mul(a.c[2], b.c[0]));
  const uint64_t d3 = add(mul(a.c[1], b.c[2]), mul(a.c[2], b.c[1]));
  const uint64_t d4 = mul(a.c[2], b.c[2]);
  return ext_make(sub(d0, d3), sub(add(d1, d3), d4), add(d2, d4));
}

// Elements of NC coefficients (1 = M64, 3 = M64X3) behind one name, for the kernels that serve both ids
template <int NC> struct El { uint64_t c[NC]; };
template <int NC> MZK_GL_HD El<NC> el_add(const El<NC>& a, const El<NC>& b) {
  El<NC> r;
  for (int i = 0; i < NC; i++) r.c[i] = add(a.c[i], b.c[i]);
  return r;
}
template <int NC> MZK_GL_HD El<NC> el_sub(const El<NC>& a, const El<NC>& b) {
  El<NC> r;
  for (int i = 0; i < NC; i++) r.c[i] = sub(a.c[i], b.c[i]);
  return r;
}
template <int NC> MZK_GL_HD El<NC> el_scale(const El<NC>& a, uint64_t s) {
  El<NC> r;
  for (int i = 0; i < NC; i++) r.c[i] = mul(a.c[i], s);
  return r;
}
MZK_GL_HD El<1> el_mul(const El<1>& a, const El<1>& b) { El<1> r; r.c[0] = mul(a.c[0], b.c[0]); return r; }
MZK_GL_HD El<3> el_mul(const El<3>& a, const El<3>& b) {
  const Ext e = ext_mul(ext_make(a.c[0], a.c[1], a.c[2]), ext_make(b.c[0], b.c[1], b.c[2]));
  El<3> r; r.c[0] = e.c[0]; r.c[1] = e.c[1]; r.c[2] = e.c[2];
  return r;
}

// ---- leaf bytes -----------------------------------------------------------------------------------------------------------
// The library's restatement of bincode for the two element types (unpinned against Rust, like the leaves of the other fields):
//   base v      : sign byte (0 for zero, else 1) | u64 LE digit count k | k u32 LE digits          9 .. 17 bytes
//   extension   : u64 LE count of coefficients after trimming trailing zeros (0 .. 3) | that many base leaves      8 .. 59 bytes
// put(pos, byte) receives every byte in order; the return value is the length.
constexpr int LEAF_MAX_BASE = 17, LEAF_MAX_EXT = 59;
template <class Put> MZK_GL_HD int leaf_base(uint64_t v, int pos, Put&& put) {
  const uint32_t d0 = (uint32_t)v, d1 = (uint32_t)(v >> 32);
  const int k = d1 ? 2 : (d0 ? 1 : 0);
  put(pos, k ? 1u : 0u);
  put(pos + 1, (uint32_t)k);
  for (int i = 2; i < 9; i++) put(pos + i, 0u);
  pos += 9;
  if (k >= 1) { for (int i = 0; i < 4; i++) put(pos + i, (d0 >> (8 * i)) & 255u); pos += 4; }
  if (k >= 2) { for (int i = 0; i < 4; i++) put(pos + i, (d1 >> (8 * i)) & 255u); pos += 4; }
  return pos;
}
template <int NC, class Put> MZK_GL_HD int leaf_bytes(const uint64_t* c, int pos, Put&& put) {
  if (NC == 1) return leaf_base(c[0], pos, put);
  int k = 0;
  for (int i = 0; i < NC; i++) if (c[i]) k = i + 1;
  put(pos, (uint32_t)k);
  for (int i = 1; i < 8; i++) put(pos + i, 0u);
  pos += 8;
  for (int i = 0; i < NC; i++) if (i < k) pos = leaf_base(c[i], pos, put);
  return pos;
}

}  // namespace gl
}  // namespace mzk
