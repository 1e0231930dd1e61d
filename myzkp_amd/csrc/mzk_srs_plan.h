// mzk_srs_plan.h -- what an SRS handle (mzk_srs.h) decides on the host: the window width for its size, the layouts it may take and in
// which order, how a handle names its points to the MSM, the width of its direct tables, when the grid-batched pass builds the wide
// tables, and whether a dump's stored tables can be used as they are.  Host only and free of HIP: tests/test_srs_plan.py runs every
// function below on a CPU; mzk_srs.h and mzk_srs.hip only execute what they return.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "mzk_msm_plan.h"      // MSM_PTS_*, msm_table_windows, msm_table_rows

namespace mzk {

// Width by SRS size, from the sweep of round 3 (tools/timing/window_sweep.py,
// profiles/r03b_window_sweep.txt; one box, ms per commit at c = 16 / 17 / 19 / 20):
//   2^17  0.54 / 0.57 / 0.89 / 0.80      2^20  1.67 / 1.63 / 2.24 / 1.78      2^22   6.46 /  6.12 /  6.98 / 5.85
//   2^18  0.73 / 0.74 / 1.00 / 0.93      2^21  3.28 / 2.94 / 3.83 / 3.20      2^24  24.38 / 23.00 / 25.01 /  --
//   2^19  1.01 / 0.99 / 1.37 / 1.17
// 17 bits = 15 tables (one accumulation fewer per pair, one table less to hold) with 2^16 buckets wins from 2^19 points on;
// wider windows lose what they save in the accumulation to the sort and to the bucket reduction (2^19 buckets at c = 20:
// reduce 0.42 instead of 0.25 ms) except at exactly 2^22.  Widths whose top window is nearly empty are pathological for the
// merged layout: 254 = 14 * 18 + 2 = 18 * 14 + 2, so at c = 18 (and 14, 21) a quarter of all top-window digits land in each of
// four buckets, 4096 segment partials apiece at 2^20 -- 0.45 ms of heavy-bucket combine at every size.
// Other widths stay selectable through mzk_srs_from_device_ex for tuning and tests (BASELINE configs[2] names 16 bits:
// bench.py reports that width as its own leg).
// Small SRS (the reference's actual sizes: a few thousand powers at most) take the short paths of mzk_msm.hip (two launches:
// k_small_accumulate_scan + the tail); with tables there is no window Horner either (its ~120 serial doublings are the latency
// floor of a small generic MSM), so they get narrow windows: 8 bits = 32 tables x 128 buckets up to 1024 points, 10 bits =
// 26 tables x 512 buckets up to 2^14 (where the sortless path still beats the general pipeline: profiles/r03v_*), then 16 and,
// from 2^19 points on, 17 bits, from 2^22 on 20 bits through the general pipeline (tools/timing/window_sweep.py).
// Round 4 (profiles/round4_window_sweep.txt, tools/timing/window_sweep.py; one box, c = 16 / 17 / 20 / 22):
//   2^22   6.09 /  5.75 /  5.62 / 12.97      2^23  11.97 / 11.27 / 10.89 / 20.26      2^24  23.56 / 22.05 / 20.89 / 30.18
// 20 bits (13 tables, 2^19 buckets) win from 2^22 points on: two accumulations fewer per pair outweigh the wider sort and the
// longer reduction; 22 bits (12 tables) lose everything to the sort (2^21 buckets: 8192 per coarse bin, past the staged fine
// scatter) and their accumulate is no faster (a longer bucket search per segment).
static inline int msm_srs_window_bits(size_t n) {
  return n <= 1024 ? 8 : (n <= ((size_t)1 << 14) ? 10 : (n < ((size_t)1 << 19) ? 16 : (n < ((size_t)1 << 22) ? 17 : 20)));
}
static inline bool msm_srs_default_tables(size_t n) { return n > 0; }

// ---- how a point set is named to the MSM ---------------------------------------------------------------------------------------
// point_kind as msm_plan takes it (mzk_msm_plan.h): window tables carry their width and bucket-set count in the upper bytes.
static inline int srs_point_kind(bool has_tables, int bits, int sets) { return has_tables ? (MSM_PTS_TABLES | (bits << 8) | (sets << 16)) : (int)MSM_PTS_MONT; }
static inline size_t srs_table_rows(bool has_tables, int bits, int sets) { return has_tables ? (size_t)msm_table_rows(bits, sets) : 2; }   // no tables: P_i, then phi(P_i) (GLV layout)
// One argument for a point set: the device pointer, its point_kind and the row stride of its tables (0 for plain points).
struct MsmPoints {
  const void* d;
  int kind;
  size_t stride;
  static MsmPoints plain(const void* d_xy) { return {d_xy, MSM_PTS_PLAIN, 0}; }     // affine canonical, as they cross the ABI
};

// ---- layout of a new handle: what fits -----------------------------------------------------------------------------------------
// commit_kzg(&poly, &pk) never fails for lack of memory, so neither may the seam: the window tables are an accelerator, and a
// handle takes the richest layout that fits the caller's budget (mzk_set_table_budget; 0 = no limit) AND the device --
//   all tables of the wanted width (15 x n points at 17 bits: 0.94 GiB at 2^20, 13 x n at 20 bits: 13 GiB at 2^24)
//   -> every 2nd table with two bucket sets -> every 4th with four (from 2^15 points on; at most 17-bit windows: the bucket
//      sets multiply the bucket count, and beyond 2^19 buckets the sort leaves its staged path)
//   -> the prepared points and their endomorphism images only (the generic GLV layout: 128 bytes per point).
// The last step ignores the budget (it is what the library needs to work at all); only when even that allocation fails is
// the error MZK_E_NOMEM.  mzk_srs_window_bits / mzk_srs_bucket_sets / mzk_srs_table_bytes report what a handle got.
struct SrsRung { bool tables; int bits, sets; size_t rows, bytes; };
struct SrsLadder { SrsRung rung[4]; int count; };
// with_tables: 0 = prepared points, 1 = the default width for n, 8..22 = that width.  The rungs srs_new tries, in order: those over a
// non-zero budget are left out, but for the last.
static inline SrsLadder srs_ladder(size_t n, int with_tables, size_t budget) {
  struct Cand { bool tables; int bits, sets; } cand[4];
  int nc = 0;
  const bool want = with_tables > 1 || (with_tables && msm_srs_default_tables(n));
  const int bits = with_tables > 1 ? with_tables : msm_srs_window_bits(n);
  if (want) {
    cand[nc++] = {true, bits, 1};
    if (n >= ((size_t)1 << 15) && bits >= 14) {
      const int b2 = bits > 17 ? 17 : bits;
      cand[nc++] = {true, b2, 2};
      cand[nc++] = {true, b2, 4};
    }
  }
  cand[nc++] = {false, bits, 1};
  SrsLadder L = {};
  for (int k = 0; k < nc; k++) {
    const size_t rows = srs_table_rows(cand[k].tables, cand[k].bits, cand[k].sets);
    const size_t bytes = n * 64 * rows;
    if (k != nc - 1 && budget && bytes > budget) continue;
    L.rung[L.count++] = {cand[k].tables, cand[k].bits, cand[k].sets, rows, bytes};
  }
  return L;
}

// ---- direct tables (mzk_srs_build_direct) --------------------------------------------------------------------------------------
// D[(w n + i) 2^(c-1) + m] = (m + 1) 2^(c w) P_i: every multiple a signed c-bit digit can ask for, 64 bytes each
static inline size_t msm_direct_bytes(size_t n, int c) { return (size_t)msm_table_windows(c) * n * ((size_t)1 << (c - 1)) * 64; }
enum { SRS_DIRECT_OK = 0, SRS_DIRECT_BAD_WIDTH, SRS_DIRECT_OVER_BUDGET };
struct SrsDirectPlan { int err, bits; size_t bytes; };
// requested: 0 = the widest windows of 12 .. 8 bits (fewest additions per coefficient) that fit the budget, or 8..12 = that width
static inline SrsDirectPlan srs_direct_plan(size_t n, int requested, size_t budget) {
  if (requested != 0 && (requested < 8 || requested > 12)) return {SRS_DIRECT_BAD_WIDTH, 0, 0};
  int c = requested;
  if (c == 0) for (c = 12; c > 8 && msm_direct_bytes(n, c) > budget; c--) {}
  const size_t bytes = msm_direct_bytes(n, c);
  return {bytes > budget ? SRS_DIRECT_OVER_BUDGET : SRS_DIRECT_OK, c, bytes};
}

// ---- wide tables of the grid-batched pass (msm_many_srs) -----------------------------------------------------------------------
// Window width of the bucket pass by polynomial length (same-box sweep, profiles/round5_many_commit_widths.txt: 16 x 2^14 0.884 ms at
// 10 bits, 0.707 at 12; 32 x 2^13 0.842 / 0.713; 64 x 2^12 0.730 / 0.752; 128 x 2^11 0.755 / 1.236): 12 bits from 2^13 coefficients on.
constexpr size_t MANY_WIDE_FROM = (size_t)1 << 13;
constexpr int MANY_WIDE_BITS = 12;
// what a handle remembers of them: a refusal -- budget or device -- is not tried again
enum SrsWideState { SRS_WIDE_UNTRIED = 0, SRS_WIDE_BUILT, SRS_WIDE_REFUSED };
static inline bool srs_wide_wanted(size_t n_poly, bool has_tables, int sets, int bits) {
  return n_poly >= MANY_WIDE_FROM && has_tables && sets == 1 && bits < MANY_WIDE_BITS;
}
static inline size_t srs_wide_bytes(size_t n) { return (size_t)msm_table_windows(MANY_WIDE_BITS) * n * 64; }
// the caller's table budget (mzk_set_table_budget) covers these tables too: `own` = the handle's own and direct tables
static inline bool srs_wide_within_budget(size_t own, size_t bytes, size_t budget) { return budget == 0 || own + bytes <= budget; }
enum SrsWideStep { SRS_WIDE_USE_OWN, SRS_WIDE_USE_WIDE, SRS_WIDE_ALLOCATE, SRS_WIDE_REFUSE };
// one batch of polynomials of n_poly coefficients: which tables it reads, or what has to happen first
static inline SrsWideStep srs_wide_step(size_t n_poly, bool has_tables, int sets, int bits, SrsWideState state, size_t own, size_t n, size_t budget) {
  if (!srs_wide_wanted(n_poly, has_tables, sets, bits) || state == SRS_WIDE_REFUSED) return SRS_WIDE_USE_OWN;
  if (state == SRS_WIDE_BUILT) return SRS_WIDE_USE_WIDE;
  return srs_wide_within_budget(own, srs_wide_bytes(n), budget) ? SRS_WIDE_ALLOCATE : SRS_WIDE_REFUSE;
}

// ---- a dump's stored tables (mzk_srs_load) -------------------------------------------------------------------------------------
// used as they are when the file is of format 2, carries tables of exactly the wanted width and row count, and has points at all
static inline bool srs_use_stored(int with_tables, uint32_t format, uint32_t flags, uint32_t file_bits, uint32_t file_rows, size_t n) {
  const int want_bits = with_tables > 1 ? with_tables : msm_srs_window_bits(n);
  return with_tables && format >= 2 && (flags & 1u) && (int)file_bits == want_bits && file_rows == (uint32_t)(msm_table_windows(want_bits) - 1) && n > 0;
}

}  // namespace mzk
