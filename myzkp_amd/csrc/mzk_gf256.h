// mzk_gf256.h -- GF(2^8) = GF(2)[x] / (x^8 + x^4 + x^3 + x^2 + 1), the field of algebra/reedsolomon.rs:352-371 (Ip0x11D): a byte is a
// polynomial over GF(2), bit i the coefficient of x^i; addition is XOR.  Plain integer C++ with no HIP include, usable from host and
// device code alike (tests/hostcheck/rs_shim.cpp compiles it with g++), and no table: a product is eight shift-and-xor steps, four
// products at a time when the bytes are packed in a uint32_t.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MZK_GF_FN __host__ __device__ static inline
#else
#define MZK_GF_FN static inline
#endif

namespace mzk {
namespace gf256 {

constexpr uint32_t POLY = 0x11D;

// a * x
MZK_GF_FN uint32_t xtime(uint32_t a) { return ((a << 1) ^ ((a >> 7) * POLY)) & 0xFF; }
// every byte of the packed word times x: the top bits leave as 0x1D into their own byte
MZK_GF_FN uint32_t xtime4(uint32_t a) { return ((a & 0x7F7F7F7Fu) << 1) ^ (((a >> 7) & 0x01010101u) * 0x1Du); }

MZK_GF_FN uint32_t gf_mul(uint32_t a, uint32_t b) {
  uint32_t r = 0;
  for (int i = 0; i < 8; i++) {
    r ^= (0u - ((b >> i) & 1u)) & a;
    a = xtime(a);
  }
  return r;
}

// a^254 = a^-1 (a != 0; 0 -> 0): a^2, a^3, a^6, a^12, a^15, a^30, a^60, a^120, a^127 (a^120 a^6 a), a^254
MZK_GF_FN uint32_t gf_inv(uint32_t a) {
  const uint32_t a2 = gf_mul(a, a), a3 = gf_mul(a2, a), a6 = gf_mul(a3, a3), a12 = gf_mul(a6, a6), a15 = gf_mul(a12, a3);
  const uint32_t a30 = gf_mul(a15, a15), a60 = gf_mul(a30, a30), a120 = gf_mul(a60, a60), a127 = gf_mul(gf_mul(a120, a6), a);
  return gf_mul(a127, a127);
}

MZK_GF_FN uint32_t gf_pow(uint32_t a, uint32_t e) {
  uint32_t r = 1;
  for (; e; e >>= 1) {
    if (e & 1) r = gf_mul(r, a);
    a = gf_mul(a, a);
  }
  return r;
}

// four packed bytes, each times the scalar byte s
MZK_GF_FN uint32_t mul4_scalar(uint32_t v, uint32_t s) {
  uint32_t r = 0;
  for (int i = 0; i < 8; i++) {
    r ^= (0u - ((s >> i) & 1u)) & v;
    v = xtime4(v);
  }
  return r;
}

// A packed constant c and its eight shifted forms c * x^i: shifted8 fills them once, mul4_shifted(forms, s) is then c * s in every byte
// at a bit extract, an and and a xor per bit of s.  The encoder's inner operation: c = four coefficients of the generator polynomial,
// s = the feedback byte (mzk_rs.hip).
MZK_GF_FN void shifted8(uint32_t c, uint32_t forms[8]) {
  for (int i = 0; i < 8; i++) {
    forms[i] = c;
    c = xtime4(c);
  }
}
MZK_GF_FN uint32_t mul4_shifted(const uint32_t forms[8], uint32_t s) {
  uint32_t r = 0;
  for (int i = 0; i < 8; i++) r ^= (0u - ((s >> i) & 1u)) & forms[i];
  return r;
}

}  // namespace gf256
}  // namespace mzk
