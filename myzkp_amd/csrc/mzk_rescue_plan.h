// mzk_rescue_plan.h -- what a batch of Rescue-Prime hash chains (zkstark/rescueprime.rs; mzk_rescue.h, mzk_rescue.hip) runs, decided on the
// host before anything is launched: the straight-line program every S-box exponent becomes, the grid a batch is walked with and the
// words of constants a handle keeps.  Host-only C++17 with no HIP include, so that all of it can be compiled and checked on its own
// (tests/test_hostcheck_rescue.py).
//
// The exponent chain.  x^e is a program over the input x and at most four slots x, x^3, x^5, x^7:
//   RS_OP_TABLE k   build slots 1 .. k: x2 = x^2, slot j = slot (j - 1) * x2             (k + 1 products; absent when only x is used)
//   RS_OP_LOAD j    acc = slot j                                                         (the first window: no product)
//   RS_OP_SQR r     acc = acc^(2^r)                                                      (r products)
//   RS_OP_MUL j     acc = acc * slot j                                                   (1 product)
//   RS_OP_ONE       acc = 1                                                              (exponent 0, 0^0 = 1 included)
// made by a left-to-right sliding window: at a set bit the longest window of at most w bits that ends in a set bit is taken, its odd
// value u selects slot (u - 1) / 2.  The table is built up to the largest slot used.  w = 3 is the form meant; the widths 2 and 1 (the
// binary method) are planned as well and the cheapest is kept (the narrower on a tie), because a lone 111 late in a sparse exponent
// would otherwise pay four products for the table where the binary method pays two: no program costs more than the binary method.
// For the reference's alphainv = 0x87aaaaaaaaaaaaaaaaaaaaaaaaaaaaab: 127 squarings + 32 products + 4 for the table = 163 (binary: 191).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include "../../include/mzk.h"

namespace mzk {

constexpr unsigned RESCUE_BLOCK = 64;                    // one chain per lane, one wave per workgroup: batch / 64 waves spread over all SIMDs
constexpr size_t RESCUE_MAX_GRID = 8192;                 // workgroups of a launch (256 CUs x 4 SIMDs x 8 waves); more work is walked in `iters` rounds
constexpr size_t RESCUE_MAX_BATCH = (size_t)1 << 40;
constexpr int RESCUE_MAX_STEPS = 520;                    // 256 one-bit windows: a LOAD, then 255 (SQR, MUL) pairs, a closing SQR and the TABLE
enum { RS_OP_ONE = 0, RS_OP_TABLE = 1, RS_OP_LOAD = 2, RS_OP_SQR = 3, RS_OP_MUL = 4 };      // a step is op | arg << 8

struct RescueChain {
  int steps = 0;
  uint32_t prog[RESCUE_MAX_STEPS] = {0};
  int window = 0;                                        // width kept (0: exponent 0)
  int slots = 0;                                         // slots read, x included
  int squarings = 0, multiplies = 0, table = 0;
  int products = 0;                                      // squarings + multiplies + table
  int binary = 0;                                        // the binary method's count for the same exponent
};

static inline int rescue_bit(const uint64_t e[4], int i) { return (int)((e[i >> 6] >> (i & 63)) & 1u); }
static inline int rescue_top_bit(const uint64_t e[4]) {
  for (int i = 255; i >= 0; i--) if (rescue_bit(e, i)) return i;
  return -1;
}

static inline void rescue_chain_width(const uint64_t e[4], int w, RescueChain* C) {
  *C = RescueChain();
  const int top = rescue_top_bit(e);
  if (top < 0) { C->prog[C->steps++] = RS_OP_ONE; return; }
  C->window = w;
  uint32_t body[RESCUE_MAX_STEPS];
  int nb = 0, maxu = 1, sq = 0;
  bool first = true;
  for (int i = top; i >= 0;) {
    if (!rescue_bit(e, i)) { sq++; i--; continue; }
    int len = w < i + 1 ? w : i + 1;
    while (!rescue_bit(e, i - len + 1)) len--;
    int u = 0;
    for (int k = 0; k < len; k++) u = 2 * u + rescue_bit(e, i - k);
    if (first) {
      body[nb++] = RS_OP_LOAD | (uint32_t)((u - 1) / 2) << 8;
      first = false;
    } else {
      sq += len;
      body[nb++] = RS_OP_SQR | (uint32_t)sq << 8;
      body[nb++] = RS_OP_MUL | (uint32_t)((u - 1) / 2) << 8;
      C->squarings += sq;
      C->multiplies++;
    }
    sq = 0;
    if (u > maxu) maxu = u;
    i -= len;
  }
  if (sq) { body[nb++] = RS_OP_SQR | (uint32_t)sq << 8; C->squarings += sq; }
  const int k = (maxu - 1) / 2;
  C->slots = k + 1;
  C->table = k ? k + 1 : 0;
  if (k) C->prog[C->steps++] = RS_OP_TABLE | (uint32_t)k << 8;
  for (int s = 0; s < nb; s++) C->prog[C->steps++] = body[s];
  C->products = C->squarings + C->multiplies + C->table;
}

static inline RescueChain rescue_chain(const uint64_t e[4]) {
  RescueChain best, c;
  rescue_chain_width(e, 1, &best);
  const int binary = best.products;
  for (int w = 2; w <= 3; w++) {
    rescue_chain_width(e, w, &c);
    if (c.products < best.products) best = c;
  }
  best.binary = binary;
  return best;
}

struct RescuePlan {
  int err = MZK_OK;
  char msg[160] = {0};
  int fid = 0, limbs = 0;                                // 29-bit limbs of an element: 5 (M128) or 9 (Fr)
  size_t m = 0, n_rounds = 0, batch = 0;
  RescueChain alpha, alphainv;
  size_t rows = 0, min_stride = 0;                       // n_rounds + 1 rows of m: the least trace_stride, in elements
  size_t products_per_hash = 0;                          // n_rounds * (m * (both chains) + 2 m^2) + 2: S-boxes, MDS, and the two changes of form
  unsigned block = RESCUE_BLOCK, iters = 0;
  size_t wgs = 0, grid = 0;
  // the constants of a handle, in 32-bit words: both programs, then the MDS matrix and the round constants as Montgomery-form limbs
  size_t prog_off[2] = {0, 0}, mds_off = 0, rc_off = 0, const_words = 0, const_bytes = 0;
};

// the grid of `batch` chains: one per lane, the capped grid walked in `iters` rounds (0, 0 for an empty batch)
struct RescueGrid { size_t wgs, grid; unsigned iters; };
static inline RescueGrid rescue_grid(size_t batch) {
  RescueGrid G;
  G.wgs = (batch + RESCUE_BLOCK - 1) / RESCUE_BLOCK;
  G.grid = G.wgs < RESCUE_MAX_GRID ? G.wgs : RESCUE_MAX_GRID;
  G.iters = G.grid ? (unsigned)((G.wgs + G.grid - 1) / G.grid) : 0;
  return G;
}

static inline RescuePlan rescue_plan(int fid, size_t m, size_t n_rounds, uint64_t alpha, const uint64_t alphainv[4], size_t batch) {
  RescuePlan P;
  auto refuse = [&](int err, const char* fmt, size_t a) { P.err = err; snprintf(P.msg, sizeof P.msg, fmt, a); return P; };
  if (fid != MZK_FIELD_M128 && fid != MZK_FIELD_FR) return refuse(MZK_E_ARG, "rescue: field id %zu is neither MZK_FIELD_M128 nor MZK_FIELD_FR", (size_t)(unsigned)fid);
  if (m < 1 || m > MZK_RESCUE_MAX_M) return refuse(MZK_E_ARG, "rescue: m = %zu is outside 1 .. 4", m);
  if (n_rounds < 1 || n_rounds > MZK_RESCUE_MAX_ROUNDS) return refuse(MZK_E_ARG, "rescue: n_rounds = %zu is outside 1 .. 64", n_rounds);
  if (batch > RESCUE_MAX_BATCH) return refuse(MZK_E_LENGTH, "rescue: batch = %zu is beyond 2^40", batch);
  P.fid = fid; P.limbs = fid == MZK_FIELD_M128 ? 5 : 9;
  P.m = m; P.n_rounds = n_rounds; P.batch = batch;
  const uint64_t a4[4] = {alpha, 0, 0, 0};
  P.alpha = rescue_chain(a4);
  P.alphainv = rescue_chain(alphainv);
  P.rows = n_rounds + 1;
  P.min_stride = P.rows * m;
  P.products_per_hash = n_rounds * (m * (size_t)(P.alpha.products + P.alphainv.products) + 2 * m * m) + 2;
  const RescueGrid G = rescue_grid(batch);
  P.wgs = G.wgs; P.grid = G.grid; P.iters = G.iters;
  P.prog_off[0] = 0;
  P.prog_off[1] = (size_t)P.alpha.steps;
  P.mds_off = ((size_t)(P.alpha.steps + P.alphainv.steps) + 3) & ~(size_t)3;
  P.rc_off = P.mds_off + m * m * (size_t)P.limbs;
  P.const_words = P.rc_off + 2 * n_rounds * m * (size_t)P.limbs;
  P.const_bytes = 4 * P.const_words;
  return P;
}

// the ABI's view of a plan (include/mzk.h: MZK_RESCUE_PLAN_WORDS values)
static inline void rescue_plan_export(const RescuePlan& P, uint64_t* o) {
  o[MZK_RESCUE_PLAN_FIELD] = (uint64_t)P.fid; o[MZK_RESCUE_PLAN_M] = P.m; o[MZK_RESCUE_PLAN_ROUNDS] = P.n_rounds; o[MZK_RESCUE_PLAN_BATCH] = P.batch;
  const RescueChain* c[2] = {&P.alpha, &P.alphainv};
  for (int h = 0; h < 2; h++) {
    uint64_t* q = o + (h ? MZK_RESCUE_PLAN_ALPHAINV_WINDOW : MZK_RESCUE_PLAN_ALPHA_WINDOW);
    q[0] = (uint64_t)c[h]->window; q[1] = (uint64_t)c[h]->slots; q[2] = (uint64_t)c[h]->steps; q[3] = (uint64_t)c[h]->squarings;
    q[4] = (uint64_t)c[h]->multiplies; q[5] = (uint64_t)c[h]->table; q[6] = (uint64_t)c[h]->products; q[7] = (uint64_t)c[h]->binary;
  }
  o[MZK_RESCUE_PLAN_PRODUCTS_PER_HASH] = P.products_per_hash;
  o[MZK_RESCUE_PLAN_ROWS] = P.rows; o[MZK_RESCUE_PLAN_MIN_STRIDE] = P.min_stride;
  o[MZK_RESCUE_PLAN_BLOCK] = P.block; o[MZK_RESCUE_PLAN_WGS] = P.wgs; o[MZK_RESCUE_PLAN_GRID] = P.grid; o[MZK_RESCUE_PLAN_ITERS] = P.iters;
  o[MZK_RESCUE_PLAN_GRID_CAP] = RESCUE_MAX_GRID; o[MZK_RESCUE_PLAN_CONST_BYTES] = P.const_bytes;
}

}  // namespace mzk
