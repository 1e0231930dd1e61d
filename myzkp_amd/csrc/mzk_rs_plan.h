// mzk_rs_plan.h -- how a batch of Reed-Solomon codewords over GF(2^8) is encoded and decoded (mzk_rs.hip), decided on the host before
// anything is launched: the kernel form, the lanes per codeword, the parity words per lane, grids, blocks and LDS bytes, a pure function
// of (n, k, batch); and the tables the kernels read, a pure function of (n, k).  Host-only C++17 with no HIP include, so that both can
// be compiled and checked on their own (tests/test_hostcheck_rs.py).  The code is algebra/reedsolomon.rs with g = x = 0x02.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include "../../include/mzk.h"
#include "mzk_gf256.h"

namespace mzk {

constexpr size_t RS_MAX_N = 255;                       // 2 has order 255: from n = 256 on the evaluation points 2^i repeat
constexpr size_t RS_MAX_BATCH = (size_t)1 << 31;
constexpr int RS_LANE_MAX_D = 32;                      // up to here the parity fits 8 packed registers of one lane
constexpr unsigned RS_BLOCK = 256;                     // threads per workgroup of every kernel of the codec
constexpr size_t RS_MAX_GRID = (size_t)1 << 20;        // workgroups of one launch; a larger batch is walked in `iters` rounds
constexpr size_t RS_MAX_LDS = 160 * 1024;

enum RsForm {
  RS_FORM_COPY = 0,      // d = 0: the codeword is the message
  RS_FORM_LANE = 1,      // k_rs_encode_lane<PW>: one codeword per lane, the parity in PW packed registers
  RS_FORM_WAVE = 2       // k_rs_encode_wave: one codeword per wave, lane j owns parity bytes 4j .. 4j + 3
};

// One launch: `per_block` codewords per workgroup, `grid` workgroups, every workgroup walks `iters` rounds `grid * per_block` apart.
struct RsLaunch {
  size_t grid;
  unsigned block;
  unsigned per_block;
  unsigned iters;
  size_t lds;            // bytes of dynamic LDS
};

struct RsPlan {
  int err = MZK_OK;
  char msg[160] = {0};
  int n = 0, k = 0, d = 0, t = 0;
  // encode.  The LFSR holds D = 4 * enc_lanes * enc_pw bytes >= d and divides by g(x) x^(D - d): the remainder then sits in its top d
  // bytes and the feedback byte is always the last one (enc_pad = D - d low bytes stay zero).
  int form = RS_FORM_COPY;
  int enc_lanes = 0, enc_pw = 0, enc_pad = 0;
  RsLaunch enc = {};
  // syndromes and decode: a group of dec_w lanes per codeword (a power of two, 8 .. 64), lane l of a group owns syndromes and
  // coefficients l, l + dec_w, ... (dec_spl of them) and positions l, l + dec_w, ... (dec_ppl)
  int dec_w = 0, dec_spl = 0, dec_ppl = 0;
  int dec_npad = 0, dec_dpad = 0;      // bytes of one LDS array over the positions / over the coefficients
  RsLaunch syn = {}, dec = {};
};

// What the kernels read.  gen_shifted[b][w]: bytes 4w .. 4w + 3 of g(x) x^pad (its monic top coefficient left out) times x^b.
struct RsTables {
  uint8_t gen[256];                 // generator_polynomial (reedsolomon.rs:34-37): d + 1 coefficients from the constant term up
  uint32_t gen_shifted[8][64];
  uint8_t pts[256];                 // 2^i                 (evaluation_points, :40-48)
  uint8_t inv_pts[256];             // (2^i)^-1            (find_error_locations, :193-194)
};

static inline RsLaunch rs_launch(size_t batch, unsigned per_block, size_t lds) {
  RsLaunch L;
  L.block = RS_BLOCK;
  L.per_block = per_block;
  L.lds = lds;
  const size_t blocks = (batch + per_block - 1) / per_block;
  L.grid = blocks < RS_MAX_GRID ? blocks : RS_MAX_GRID;
  L.iters = (unsigned)((blocks + L.grid - 1) / L.grid);
  return L;
}

static inline RsPlan rs_plan(size_t n, size_t k, size_t batch) {
  RsPlan P;
  if (k < 1 || k > n || n > RS_MAX_N) {
    P.err = MZK_E_ARG;
    snprintf(P.msg, sizeof P.msg, "rs: (n, k) = (%zu, %zu) is outside 1 <= k <= n <= 255 (the evaluation points 2^i repeat from n = 256 on)", n, k);
    return P;
  }
  if (batch < 1 || batch > RS_MAX_BATCH) {
    P.err = MZK_E_ARG;
    snprintf(P.msg, sizeof P.msg, "rs: a batch of %zu codewords is outside 1 .. 2^31", batch);
    return P;
  }
  P.n = (int)n; P.k = (int)k; P.d = (int)(n - k); P.t = P.d / 2;
  if (P.d == 0) { P.form = RS_FORM_COPY; P.enc_lanes = 1; P.enc_pw = 0; P.enc = rs_launch(batch, RS_BLOCK, 0); }
  else if (P.d <= RS_LANE_MAX_D) {
    P.form = RS_FORM_LANE;
    P.enc_lanes = 1;
    P.enc_pw = P.d <= 4 ? 1 : (P.d <= 8 ? 2 : (P.d <= 16 ? 4 : 8));
    P.enc = rs_launch(batch, RS_BLOCK, 0);
  } else {
    P.form = RS_FORM_WAVE;
    P.enc_lanes = 64;
    P.enc_pw = 1;
    P.enc = rs_launch(batch, RS_BLOCK / 64, 0);
  }
  P.enc_pad = 4 * P.enc_lanes * P.enc_pw - P.d;
  int w = 8;
  while (w < P.d && w < 64) w <<= 1;
  P.dec_w = w;
  P.dec_spl = (P.d + w - 1) / w;
  if (P.dec_spl < 1) P.dec_spl = 1;
  P.dec_ppl = (P.n + w - 1) / w;
  P.dec_npad = (P.n + 3) & ~3;
  P.dec_dpad = (P.d + 1 + 3) & ~3;
  const unsigned groups = RS_BLOCK / (unsigned)w;
  P.syn = rs_launch(batch, groups, 0);
  P.dec = rs_launch(batch, groups, (size_t)groups * (2 * (size_t)P.dec_npad + 5 * (size_t)P.dec_dpad));
  return P;
}

// n, k as admitted by rs_plan
static inline void rs_tables(size_t n, size_t k, int pad, RsTables* T) {
  memset(T, 0, sizeof *T);
  const int d = (int)(n - k);
  uint32_t x = 1;
  for (int i = 0; i < 256; i++) { T->pts[i] = (uint8_t)x; x = gf256::xtime(x); }
  for (int i = 0; i < 256; i++) T->inv_pts[i] = T->pts[(255 - i % 255) % 255];      // 2^-i = 2^(255 - i)
  // prod_{i < d} (x - 2^i): multiply by one monomial at a time
  T->gen[0] = 1;
  for (int i = 0; i < d; i++) {
    for (int j = i + 1; j >= 0; j--) {
      const uint32_t below = j ? T->gen[j - 1] : 0;
      T->gen[j] = (uint8_t)(below ^ gf256::gf_mul(T->gen[j], T->pts[i]));
    }
  }
  uint8_t padded[256] = {0};
  for (int j = 0; j < d; j++) padded[pad + j] = T->gen[j];
  for (int w = 0; w < 64; w++) {
    const uint32_t c = (uint32_t)padded[4 * w] | (uint32_t)padded[4 * w + 1] << 8 | (uint32_t)padded[4 * w + 2] << 16 | (uint32_t)padded[4 * w + 3] << 24;
    uint32_t f[8];
    gf256::shifted8(c, f);
    for (int b = 0; b < 8; b++) T->gen_shifted[b][w] = f[b];
  }
}

}  // namespace mzk
