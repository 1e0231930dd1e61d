// mzk_msm_plan.h -- what one Pippenger MSM call (msm_dev_impl, mzk_msm.hip) does, decided on the host before anything is launched:
// the bucket layout, the sort form, the accumulate's segments and the bytes of every workspace slot.  Host-only C++17 with no HIP
// include, so that the decision can be compiled and checked on its own (tests/test_msm_plan.py).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include "../../include/mzk.h"

namespace mzk {

// point_kind: 0 = affine canonical (ABI form), 1 = affine Montgomery (prepared), 2 = SRS window tables (msm_table_rows(c, sets) x table_stride
// affine Montgomery points: c-bit signed windows, 254 / c + 1 of them), with c in bits 8..15 (0 = 16) and the bucket sets in bits 16..23
// (0 = one).  msm_plan decodes it; nothing else does.
enum { MSM_PTS_PLAIN = 0, MSM_PTS_MONT = 1, MSM_PTS_TABLES = 2 };
static inline int msm_table_windows(int c) { return 254 / c + 1; }
// tables a handle with `sets` bucket sets holds: every sets-th window, ceil(windows / sets) = 254 / (c sets) + 1
static inline int msm_table_rows(int c, int sets) { return 254 / (c * sets) + 1; }

constexpr int SCALAR_BITS = 254;
constexpr int MAX_WINDOWS = 32;
constexpr int GLV_MAG_BITS = 126;      // |k1|, |k2| < 2^126 (mzk_glv.h)
constexpr int SLOT_WORDS = 36;         // a segment partial: 4 x 9 raw limbs (mzk_msm.hip)
constexpr int ACC_RESIDENT_WAVES = 3;  // waves per SIMD the accumulate's grid is sized for (msm_plan); k_seg_accumulate's __launch_bounds__(256, 3) keeps them resident

// Bucket layout.  Generic MSM: bucket = window * 2^(c-1) + |digit| - 1, entry = point index.
// Fixed-base MSM over precomputed tables T[w][i] = 2^(c w) P_i: every window shares ONE bucket set,
// bucket = |digit| - 1, entry = w * table_stride + i.
struct DigitLayout {
  int c, nwin, merged;
  int sets;              // merged layout: bucket sets (mzk_srs::sets); window w goes to set w % sets and reads table row w / sets
  size_t table_stride;
  int glv;               // generic layout only: scalars are GLV-split, the phi images of the points start at phi_offset
  size_t phi_offset;
};

struct MsmShape { int c, nwin, lgB; size_t nbuckets; };     // window bits, windows, log2 buckets per window = c - 1, buckets
// Generic layout after the GLV split: 2n points with scalars below 2^126.  Windows must cover 127 bits plus the
// signed-digit carry; at c = 16 that is exactly 8 windows (2^18 buckets: the two-level sort's power of two).
// force_c (MZK_GLV_C, tuning build): force a width (the sweep).
static MsmShape choose_shape_glv(size_t n, int force_c = 0) {
  int lg = 0;
  while (((size_t)1 << lg) < 2 * n) lg++;
  int c = lg - 3;
  if (c < 8) c = 8;
  if (c > 16) c = 16;
  if (c == 15) c = 16;     // 2^17 pairs: 8 full windows + the two-level sort beat 9 windows with a 6-bit top window
  // From 3 x 2^21 pairs on: 19 bits -- SEVEN windows per half instead of eight (14 mixed additions per pair, not 16: the accumulate is
  // 80 % of the call), 7 x 2^18 buckets.  17 and 18 bits still need eight windows (7 x 18 = 126 leaves the top window nothing but
  // carries), 20 bits also seven but twice the buckets, 22 bits six windows over 6 x 2^21 buckets whose reduction and one-pass sort cost
  // more than the windows save.  The larger bucket set costs ~0.7 ms more to sort, combine and reduce whatever n is, the saved additions
  // 0.145 ms per 2^20 pairs: 2^22 +3.6 %, 2^23 -2 %, 2^24 -6.5 %, 2^26 -7.5 % (profiles/round6_generic_window_sweep.txt).
  if (n >= ((size_t)3 << 21)) c = 19;
  if (force_c > 0) c = force_c;
  // nwin windows must cover the 126 magnitude bits plus the signed-digit carry.  The top window only holds
  // 126 - c (nwin - 1) real bits; if that is (almost) nothing, every scalar whose carry runs into it lands in the
  // same few buckets (c = 14: ONE bucket receives a third of all entries) -- step c down until the top window is
  // reasonably populated.
  for (; c > 8; c--) {
    const int nw = GLV_MAG_BITS / c + 1;
    if (GLV_MAG_BITS - c * (nw - 1) >= 5) break;
  }
  MsmShape s;
  s.c = c;
  s.nwin = GLV_MAG_BITS / c + 1;
  s.lgB = c - 1;
  s.nbuckets = (size_t)s.nwin << s.lgB;
  return s;
}

// ---- the sort's constants --------------------------------------------------------------------------------------------------------
#ifndef MZK_COARSE_LOG
#define MZK_COARSE_LOG 8
#endif
constexpr int COARSE_LOG = MZK_COARSE_LOG;      // 9: A/B build (one more bit for the point reference in the 4-byte sort records)
constexpr int COARSE_PER_WG = 4096;
constexpr int FINE_MAX = 8192;     // buckets per bin: NB / 256 (128 merged c = 16, 2048 generic c = 16, 8192 merged c = 22)
constexpr int STAGE_F_MAX = 2048;  // the most buckets per bin k_fine_scatter stages in LDS
constexpr size_t SMALL_MAX_N = 4097;          // exclusive: 4096 (a blob of das/avail.rs) still takes the three-launch path
constexpr size_t SMALL_MAX_BUCKETS = 8192;
// launch_exclusive_scan (mzk_msm.hip): blocks of SCAN_BLOCK; above SCAN_DIRECT_BLOCKS of them their totals are scanned recursively
constexpr int SCAN_ITEMS = 8;                      // per thread
constexpr int SCAN_BLOCK = 256 * SCAN_ITEMS;       // 2048 per block
constexpr size_t SCAN_DIRECT_BLOCKS = 2048;
static inline size_t scan_scratch_words(size_t n) {
  const size_t sb = (n + SCAN_BLOCK - 1) / SCAN_BLOCK;
  return sb + 2 + (sb > SCAN_DIRECT_BLOCKS ? scan_scratch_words(sb) : 0);
}
// Buckets with more than HEAVY_SLOTS segment partials are summed by a whole workgroup each (k_seg_combine_heavy, mzk_msm.hip).
constexpr uint32_t HEAVY_SLOTS = 32;
// Layout of `heavy`: [0] count, [1] the segment length in force (written by the combine kernel), [2, 2 + HEAVY_GRID) arrival counters of k_seg_combine_heavy's shared buckets (zeroed with
// the count, one memset), then (bucket id, end of its entries as the deferring kernel saw it -- bucket_end) pairs, then HEAVY_GRID
// XYZZ records of scratch for the workgroups that share a bucket.
// Behind the arrival counters, inside the same cleared header: the scan-free sort's per-bin totals and cursors (k_coarse_count /
// k_coarse_scatter*: SORT_CTR_BINS words each) -- one memset per call clears everything that has to start at zero.
constexpr int HEAVY_GRID = 512;
constexpr int SORT_CTR_BINS = 1024;               // the most coarse bins any layout uses (20-bit merged windows)
constexpr int SORT_CTR_AT = 2 + HEAVY_GRID;       // bin totals at heavy[SORT_CTR_AT ..), bin cursors SORT_CTR_BINS words further
constexpr int HEAVY_HDR = SORT_CTR_AT + 2 * SORT_CTR_BINS;
// (a multiple of four words: the scratch records behind the list are read and written as uint4)
constexpr size_t heavy_list_words(size_t max_heavy) { return (HEAVY_HDR + 2 * max_heavy + 2 + 3) & ~(size_t)3; }
constexpr size_t heavy_total_words(size_t max_heavy) { return heavy_list_words(max_heavy) + (size_t)HEAVY_GRID * 32 + 8; }
// One fine kernel per bin (k_fine_sort, mzk_msm.hip): a workgroup of FINE_LANES lanes holds a whole bin in registers, FINE_REGS records
// per lane.  The capacity is sized for the fullest bin of a uniform 2^20-pair commit against 17-bit tables, not for the mean: 512 bins of
// 128 buckets hold 28 672 records of the fourteen full windows, and the bins of the top window's digits (they stop at 49 554: bins
// 0 - 387) another ~2 708 -- 31 380 with a standard deviation of 177.  Eight deviations above that are 32 797: 33 records per lane
// (33 792); 32 (32 768) are 7.8.  33 records and their 17 words of packed places still leave the kernel inside the 64 registers that
// keep two workgroups on a CU (tools/kernel_resources.py: 64 VGPRs, no scratch).
constexpr int FINE_LANES = 1024;
constexpr int FINE_REGS = 33;
constexpr uint32_t FINE_BIN_CAP = (uint32_t)FINE_REGS * FINE_LANES;
constexpr int FINE_SORT_F_MAX = 1024;      // the most buckets per bin k_fine_sort takes: its counters + a 16 Ki-record window, twice per CU
constexpr int FINE_WIN_LOG = 14;           // log2 of the records it stages per round
static_assert(FINE_BIN_CAP + (1u << FINE_WIN_LOG) <= 0xffffu, "a record's position in its bin packs into 16 bits, 0xffff falls into no round");

// code the kernels and the host run alike (the host: tests/hostcheck/*_shim.cpp)
#if defined(__HIPCC__)
#define MZK_HD __host__ __device__ __forceinline__
#else
#define MZK_HD inline
#endif

// ---- the fused fine level: which workgroup of k_fine_sort does what --------------------------------------------------------------------
// The last `bins` workgroups own a bin each, the records [bound[b], bound[b + 1]) of the coarse sort: up to FINE_BIN_CAP of them a
// workgroup sorts alone, from registers.  A fuller bin (skewed scalars: bytes, repeated values, short coefficients) it leaves to SLICES,
// cut as fine_plan cuts them: ceil(len / cap) equal parts, one extra workgroup each.  The extra workgroups stand in front of the bins',
// in bin order -- extra workgroup j is slice j - X_b of the bin b with X_b <= j < X_b + slices(b), X the exclusive prefix of the slice
// counts -- and only count in k_fine_sort; the second launch (k_fine_scatter over the extra workgroups alone) places their records.
// Lane b of an extra workgroup evaluates bin b.
struct FineSlice { int bin, s, Sb; uint32_t lo, hi, start; bool active; };
// register k of lane `lane` of a whole-bin workgroup holds record k FINE_LANES + lane of the bin, if the bin has that many
MZK_HD uint32_t fine_reg_record(int k, uint32_t lane) { return (uint32_t)k * FINE_LANES + lane; }
// workgroup w of a grid of bins + extra: true = extra workgroup *idx, false = the workgroup of bin *idx
MZK_HD bool fine_wg_is_extra(uint32_t w, uint32_t extra, uint32_t* idx) { *idx = w < extra ? w : w - extra; return w < extra; }
MZK_HD uint32_t fine_bin_slices(uint32_t len, uint32_t cap) { return len > FINE_BIN_CAP ? (uint32_t)(((uint64_t)len + cap - 1) / cap) : 0u; }
// records [lo, hi) of slice s of Sb: the slices of a bin tile it exactly
MZK_HD void fine_slice_bounds(uint32_t start, uint32_t len, uint32_t s, uint32_t Sb, uint32_t* lo, uint32_t* hi) {
  *lo = start + (uint32_t)((uint64_t)len * s / Sb);
  *hi = start + (uint32_t)((uint64_t)len * (s + 1) / Sb);
}
// lane `bin`'s answer for extra workgroup j: true, and the slice, when j is one of this bin's (excl = X_bin)
MZK_HD bool fine_slice_of_bin(uint32_t j, int bin, uint32_t start, uint32_t len, uint32_t excl, uint32_t cap, FineSlice* out) {
  const uint32_t Sb = fine_bin_slices(len, cap);
  if (j < excl || j - excl >= Sb) return false;
  out->bin = bin, out->s = (int)(j - excl), out->Sb = (int)Sb, out->start = start, out->active = true;
  fine_slice_bounds(start, len, j - excl, Sb, &out->lo, &out->hi);
  return true;
}
// The most slices the over-full bins of E records in `bins` bins can need -- the extra workgroups the launch provides.  A bin opens at
// FINE_BIN_CAP + 1 records with a = ceil((CAP + 1) / cap) slices, its next slice comes a cap - CAP records later and every further one
// cap records later; with m bins open the rest of the records buys slices at those two prices.  The best m is found by trying all.
static inline size_t fine_max_slices(size_t E, size_t bins, uint32_t cap) {
  const size_t open = (size_t)FINE_BIN_CAP + 1, a = (open + cap - 1) / cap, first = a * cap - FINE_BIN_CAP;
  size_t best = 0;
  for (size_t m = 1; m <= bins && m * open <= E; m++) {
    const size_t rest = E - m * open, cheap = rest / first < m ? rest / first : m;
    const size_t v = m * a + cheap + (rest - cheap * first) / cap;
    if (v > best) best = v;
  }
  return best;
}
// The fullest bin that uniform scalars make, and whether it stays eight standard deviations (of a count: its root) below the capacity.
// Window w spreads its entries evenly over the digit magnitudes it can take -- 2^(c-1), fewer in the top window, whose digits stop at
// the top bits of the modulus (of 2^126 after the GLV split) -- so the bin of the smallest magnitudes is the fullest of its bucket set.
constexpr uint64_t FR_TOP64 = 0x30644e72e131a029ull;      // bits 192 .. 255 of the scalar field's modulus
static inline size_t fine_uniform_max_bin(const DigitLayout& L, size_t n, size_t F) {
  const int nsets = L.merged ? L.sets : L.nwin;
  double best = 0;
  for (int set = 0; set < nsets; set++) {
    double sum = 0;
    for (int w = 0; w < L.nwin; w++) {
      if ((L.merged ? w % L.sets : w) != set) continue;
      double range = (double)((uint64_t)1 << (L.c - 1));
      if (w == L.nwin - 1) {
        const int low = L.c * w, top = (L.glv ? GLV_MAG_BITS : 256) - low;      // bits of the scalar above the window's lowest
        const double r = L.glv ? (double)((uint64_t)1 << (top > 0 ? top : 0)) : (double)(FR_TOP64 >> (64 - top)) + 1;
        if (r < range) range = r;
      }
      sum += (double)(L.glv ? 2 * n : n) * (range > (double)F ? (double)F / range : 1.0);
    }
    if (sum > best) best = sum;
  }
  return (size_t)best + 1;
}
static inline bool fine_bins_fit(size_t fullest) {
  if (fullest >= FINE_BIN_CAP) return false;
  const size_t margin = FINE_BIN_CAP - fullest;
  return margin * margin >= 64 * fullest;
}

// ---- the plan ----------------------------------------------------------------------------------------------------------------------
// The MSM's tuning switches: the shipped values here; the tuning build reads MZK_<NAME> over them, in this order (mzk_msm.hip).
struct MsmKnobs {
  int glv_c = 0;                  // MZK_GLV_C: force the generic layout's width
  int small_scan = 1;             // MZK_SMALL_SCAN: 0 = A/B against the sorted path
  int scan_max_log = 14;          // MZK_SCAN_MAX_LOG
  int acc_seg = 0;                // MZK_ACC_SEG: a fixed segment length (tools/timing/acc_sweep.py sweeps it)
  int coarse_log_20 = 10;         // MZK_COARSE_LOG_20: 8 = the 256-bin form at 20 bits too
  int coarse_log_17 = 9;          // MZK_COARSE_LOG_17: 8 = the 256-bin form with 8-byte records
  int per_fine = 0;               // MZK_PER_FINE: records per fine workgroup (tools/timing/window_sweep.py)
  int sort_scan_free = 3;         // MZK_SORT_SCAN_FREE: bit 0 = coarse level, bit 1 = fine level
  int combine_wide_min_log = 17;  // MZK_COMBINE_WIDE_MIN_LOG
  int combine_form = 0;           // MZK_COMBINE_FORM: 1 = a DPP quad per bucket, 2 = a lane per bucket, whatever the plan would pick
  int combine_lane_tpb = 256;     // MZK_COMBINE_LANE_TPB: lanes per workgroup of the look-ahead lane form (64, 128: the measurement behind 256)
  int fine_fused = -1;            // MZK_FINE_FUSED: 0 = k_fine_count + k_fine_scatter, 1 = k_fine_sort wherever its records and counters fit, however full the bins
  int halve_row = 1;              // MZK_HALVE_ROW: 0 = the late halving steps stay DPP-quad launches (k_halve_multi), no k_halve_multi_row; 1 = row launches unless commits are in flight; 2 = always
};

enum class MsmPath { SmallScan, SmallSort, TwoLevel, LdsOnePass, Atomic };
// Bytes per workspace slot (0: not asked for).  offsets, entries, buckets and slots hold one region per chunk in chunk mode.
struct MsmWsBytes { size_t points, counts, offsets, cursor, entries, buckets, scan, slots, wghist, out; };
struct MsmSizing { size_t E, T, n_coarse, n_fine; };     // what the sized buffers hold: entries, segments, coarse / fine histogram words

struct MsmPlan {
  int err = MZK_OK;
  char msg[192] = {};
  size_t n = 0;                                // pairs of this call
  DigitLayout L{};
  int lgB = 0, red_windows = 0, horner_c = 0;  // log2 buckets per set, bucket sets to reduce, Horner width over them (0: none)
  size_t NB = 0, NBtot = 0;                    // buckets; the two-level sort's power of two >= NB
  bool one_set = false, small_wide = false;    // the tail writes the result itself (no Horner over bucket sets); small sort: a lane per entry
  MsmPath path = MsmPath::SmallSort;
  // two-level sort (log2 coarse bins, buckets per bin, fine key bits, slices per bin); sort workgroups (two-level: coarse, LDS path: one-pass)
  int cl = 0, F = 0, fb = 0, key_shift = 0, S = 0, nwg = 0;
  uint32_t fine_mask = 0, slice_cap = 0;
  unsigned fine_wgs = 0;
  bool fine_fused = false;                     // fine level: k_fine_sort, one workgroup per bin (+ fine_wgs - bins for the slices of over-full bins)
  size_t per_wg = 0;                           // LDS path: pairs per workgroup
  bool compact = false, coarse_free = false, fine_free = false, scatter_staged = false;   // 4-byte records, scan-free levels, staged scatter
  int coarse_c = 0;                            // the compile-time merged width of the coarse count / scatter kernels (0: any layout)
  // accumulate
  uint32_t seg = 0, t_max = 0;
  size_t T = 0, nslots = 0, max_heavy = 0, slot_region_words = 0;    // (one chunk's slots + heavy list)
  bool combine_wide = false, combine_ahead = false;    // segment combine: a lane per bucket (not a DPP quad); ... with the next record on its way
  int combine_tpb = 256;                               // ... in workgroups of so many lanes
  MsmSizing own{}, alloc{};                    // what this call touches; what its buffers are sized for (the largest chunk in chunk mode)
  MsmWsBytes ws{}, ws_used{};                  // requests; the same formula over `own` (no chunk outgrows its region)
  MsmPlan& fail(const char* fmt, size_t a = 0, size_t b = 0, size_t c = 0) { err = MZK_E_ARG; snprintf(msg, sizeof msg, fmt, a, b, c); return *this; }
};

// one chunk's segment partials (T + NB + 1 slots) and heavy-bucket list, rounded to four words
static inline size_t msm_slot_region_words(size_t T, size_t NB) {
  return ((T + NB + 1) * SLOT_WORDS + heavy_total_words((T + NB) / HEAVY_SLOTS + 1) + 3) & ~(size_t)3;
}
// the bytes of the slots that grow with the problem (ws over `alloc`, ws_used over `own`); `regions` copies of the per-chunk ones
static inline MsmPlan& msm_sized(MsmPlan& P, size_t regions) {
  for (int u = 0; u < 2; u++) {
    const MsmSizing& z = u ? P.own : P.alloc;
    MsmWsBytes& w = u ? P.ws_used : P.ws;
    w.points = P.ws.points, w.out = P.ws.out;
    w.offsets = regions * (P.NBtot + 1) * 4;
    w.entries = regions * z.E * 4;
    w.buckets = regions * P.NB * 128;
    if (P.path == MsmPath::SmallScan || P.path == MsmPath::SmallSort) continue;
    const bool two = P.path == MsmPath::TwoLevel;
    w.counts = 2 * P.NBtot * 4;      // (two-level sort, scan-free form: per-bucket totals + cursors)
    w.cursor = z.E * (two ? 8 : 4);
    w.slots = regions * msm_slot_region_words(z.T, P.NB) * 4;
    w.wghist = two ? (z.n_coarse + 1 + z.n_fine + 1 + ((size_t)1 << P.cl) + 1) * 4 : P.path == MsmPath::LdsOnePass ? (size_t)P.nwg * P.NB * 4 : 0;
    w.scan = two ? (scan_scratch_words(z.n_coarse) + scan_scratch_words(z.n_fine) + 4) * 4 : scan_scratch_words(P.NB) * 4;
  }
  return P;
}

// n pairs of a problem of n_shape pairs (the layout follows n_shape), buffers sized for n_alloc pairs.  chunks = 0: one whole call;
// K >= 1: one chunk of an MSM in K chunks (msm_chunked_impl: every chunk's call asks for the same bytes, K regions of the per-chunk
// slots, and stops before the reduction).
static inline MsmPlan msm_plan(size_t n, size_t n_shape, size_t n_alloc, int point_kind, size_t table_stride, int num_cu, int chunks,
                               const MsmKnobs& kn) {
  MsmPlan P;
  P.n = n;
  if (n > ((size_t)1 << 27)) return P.fail("msm: n > 2^27 not supported");
  const int kind = point_kind & 0xff, table_c = (point_kind >> 8) & 0xff, table_sets = (point_kind >> 16) & 0xff;
  DigitLayout& L = P.L;
  L.merged = kind == MSM_PTS_TABLES;
  L.sets = (L.merged && table_sets) ? table_sets : 1;
  L.table_stride = table_stride;
  // generic layout: GLV split (mzk_glv.h) -- 2n points (P_i and phi(P_i) at phi_offset + i), half-length scalars
  L.glv = !L.merged;
  L.phi_offset = kind == MSM_PTS_PLAIN ? n_shape : table_stride;   // prepared by msm_dev_impl / laid out by the SRS handle
  const MsmShape sh = choose_shape_glv(n_shape, kn.glv_c);
  L.c = L.merged ? (table_c ? table_c : 16) : sh.c;
  L.nwin = L.merged ? msm_table_windows(L.c) : sh.nwin;
  P.NB = L.merged ? (size_t)L.sets << (L.c - 1) : sh.nbuckets;
  P.lgB = L.c - 1, P.red_windows = L.merged ? L.sets : L.nwin;
  P.one_set = L.merged && L.sets == 1, P.horner_c = P.one_set ? 0 : L.c;
  const size_t windows_per_pair = L.glv ? 2 * L.nwin : L.nwin, regions = chunks ? chunks : 1;
  const size_t E_max = P.own.E = n * windows_per_pair, E_alloc = P.alloc.E = n_alloc * windows_per_pair;
  P.ws.points = kind == MSM_PTS_PLAIN ? 2 * n_shape * 64 : 0;
  P.ws.out = chunks ? 0 : (size_t)MAX_WINDOWS * 128;
  // The two-level sort wants a power of two: the generic layout's 7 x 2^18 buckets (19-bit windows) sort as if there were an eighth,
  // empty window -- the sort's arrays are sized by NBtot, its offsets beyond NB all equal the entry count, everything after the sort
  // works on the NB real buckets.
  P.NBtot = P.NB;
  if (L.glv && (P.NB & (P.NB - 1)) != 0 && L.c >= 17) { P.NBtot = 1; while (P.NBtot < P.NB) P.NBtot <<= 1; }

  // (the generic layout has twice the entries per pair: measured at 4096 pairs it is 5 % slower on this path, the commit 14 % faster)
  const bool scan_ok = P.one_set && kn.small_scan != 0 && n <= ((size_t)1 << kn.scan_max_log) && (L.c == 8 || (L.c >= 10 && L.c <= 13));
  if (!chunks && (scan_ok || n < (L.merged ? SMALL_MAX_N : SMALL_MAX_N - 1)) && P.NB <= SMALL_MAX_BUCKETS) {
    P.path = scan_ok ? MsmPath::SmallScan : MsmPath::SmallSort;
    P.small_wide = E_max / P.NB > 64;     // ~256 entries per bucket (commits against narrow tables): a lane per entry
    return msm_sized(P, 1);
  }
  // entries pack the point reference into 31 bits (+ sign) and entry positions into 32: reject shapes that overflow
  // (window widths below 16 on a > 2^26-point SRS) instead of gathering a wrong table row
  const size_t ref_max = L.merged ? (size_t)msm_table_rows(L.c, L.sets) * table_stride : L.phi_offset + n;
  if (ref_max > ((size_t)1 << 31) || E_max >= ((size_t)1 << 32))
    return P.fail("msm: %zu pairs x %zu windows (table stride %zu) exceed the 31-bit point references / 32-bit entry offsets", n, (size_t)L.nwin, table_stride);

  // Segment length: one lane per segment, the grid ONE round of the waves that are resident: three per SIMD at the kernel's 159 VGPRs
  // (E / (CUs * 4 * 3 * 64), >= 16).  Until round 7 the grid was sized for four -- three quarters of the workgroups at once, then the
  // last quarter one wave per SIMD -- and measured equal to this form twice: with the loop that exposed a load per iteration
  // (profiles/r03o_accumulate_occupancy_ab.txt) and with the pipelined one (profiles/round7_accumulate_pipeline_ab.txt: 1.3643 against
  // 1.3622 ms per 2^20 commit, 2^24 and the generic MSM equal too).  The accumulate alone is ~10 us faster with the second round (its
  // workgroups fill the first round's ragged end), the segment combine ~10 us faster without it (a quarter fewer partials): of two
  // equal forms the one with the cheaper combine ships.
  const size_t resident_lanes = (size_t)num_cu * 4 * ACC_RESIDENT_WAVES * 64;
  size_t seg = (E_max + resident_lanes - 1) / resident_lanes;
  seg = kn.acc_seg > 0 ? (size_t)kn.acc_seg : seg < 16 ? 16 : seg;
  P.seg = (uint32_t)seg;
  P.T = P.own.T = (E_max + seg - 1) / seg;
  P.t_max = kn.acc_seg > 0 ? 0u : (uint32_t)P.T;       // the kernels shorten the segments when the scalars emit fewer entries (segment_length)
  P.nslots = P.T + P.NB + 1;
  P.max_heavy = (P.T + P.NB) / HEAVY_SLOTS + 1;        // at most (T + NB) / 33 buckets hold more than 32 partials
  // Segment combine: a lane per bucket from 2^17 buckets on, and for the one merged bucket set as soon as a lane per bucket puts a wave
  // on every SIMD (64 lanes x 4 SIMDs x CUs: 2^16 buckets on 256 CUs, the 17-bit commit).  From there on the kernel is bound by the
  // instructions it issues, and the plain addition issues a third of the quad form's per addition; below, lanes would leave SIMDs
  // empty and the quad's shorter chain is what counts (k_seg_combine, mzk_msm.hip).
  const size_t lanes_fill_chip = (size_t)64 * 4 * (size_t)(num_cu > 0 ? num_cu : 1);
  P.combine_wide = kn.combine_form ? kn.combine_form == 2
                                   : P.NB >= ((size_t)1 << kn.combine_wide_min_log) || (P.one_set && P.NB >= lanes_fill_chip);
  // below 2^17 buckets the lanes are a wave or two per SIMD with nothing else to cover a record's latency: they load one record ahead
  P.combine_ahead = P.combine_wide && P.NB < ((size_t)1 << kn.combine_wide_min_log);
  // ... in workgroups of FOUR waves, which the dispatcher spreads over a CU's four SIMDs: 2^16 lanes are then one workgroup per CU and
  // one wave per SIMD.  Workgroups of one or two waves came to lie two waves to a SIMD with half the SIMDs idle (55 - 56 us against
  // 37.6 at the 2^20 commit, profiles/combine_lane_form_ab.txt); an LDS request that admits one workgroup per CU changed nothing.
  P.combine_tpb = (kn.combine_lane_tpb == 64 || kn.combine_lane_tpb == 128) ? kn.combine_lane_tpb : 256;
  // (a chunk never has more segments than resident lanes, nor than entries / 16 -- entries / MZK_ACC_SEG with a fixed length: the
  // slot region of every chunk is sized for that)
  const size_t T_seg = E_alloc / (kn.acc_seg > 0 ? (size_t)kn.acc_seg : 16) + 1;
  P.alloc.T = !chunks ? P.T : kn.acc_seg > 0 ? T_seg : (resident_lanes + 1 < T_seg ? resident_lanes + 1 : T_seg);
  P.slot_region_words = msm_slot_region_words(P.alloc.T, P.NB);

  // two-level sort when the bucket space is a power of two >= 2^12 (merged layout always; generic at c = 16)
  const bool plain_merged = L.merged && L.sets == 1;
  // (small inputs keep the one-pass kernels, except that the merged one-pass histogram must fit the LDS: 2^15 buckets)
  // coarse bins: 256, or 1024 for the 20-bit merged layout (2^19 buckets: 512 per bin instead of 2048; k_coarse_count)
  // (the generic GLV layout stays at 256 bins: its coarse scatter stores records one by one -- the walk is the GLV split, no staging --
  // and 512 bins measured slower at 2^22 and 2^24: sort 3.77 -> 3.91 ms, profiles/round5_sort_1024_bins.txt)
  P.cl = (plain_merged && L.c == 20 && kn.coarse_log_20 == 10) ? 10 : COARSE_LOG;
  // 17-bit merged layout: 512 bins when that one bit is what lets the sort's intermediate records shrink from 8 to 4 bytes (reference
  // 15 n < 2^24, 7-bit fine key, sign: 2^20 pairs exactly) -- the coarse scatter writes and both fine passes read half the bytes
  // (profiles/round6_halving_multi_and_rec4_ab.txt; without that gain 512 bins lost to 256 in round 3: HISTORY)
  if (plain_merged && L.c == 17 && kn.coarse_log_17 == 9 && COARSE_LOG == 8 && ref_max > ((size_t)1 << (31 - 8)) && ref_max <= ((size_t)1 << (31 - 7)))
    P.cl = 9;
  if (L.glv && P.NBtot > ((size_t)STAGE_F_MAX << COARSE_LOG)) P.cl = 10;      // generic layout at 19 bits: 2^21 sorted buckets, 2048 per bin
  const size_t cbins = (size_t)1 << P.cl;
  const bool two_level = (P.NBtot & (P.NBtot - 1)) == 0 && P.NBtot >= 4096 && (P.NBtot / cbins) <= (size_t)FINE_MAX &&
                         (n >= 4096 || (L.merged && P.NBtot > ((size_t)1 << 15)));
  if (chunks && !two_level) return P.fail("msm: chunk mode needs the two-level sort (layout %zu bits, %zu buckets)", (size_t)L.c, P.NB);
  P.path = two_level ? MsmPath::TwoLevel : L.merged ? MsmPath::LdsOnePass : MsmPath::Atomic;
  if (P.path == MsmPath::LdsOnePass) {       // one-pass workgroups: one per 4096 pairs, at most one per CU
    const size_t nwg = (n + 4095) / 4096;
    P.nwg = nwg < 1 ? 1 : nwg > (size_t)num_cu ? num_cu : (int)nwg;
    P.per_wg = (n + P.nwg - 1) / P.nwg;
  }
  if (!two_level) return msm_sized(P, regions);
  while (((size_t)1 << P.key_shift) < P.NBtot) P.key_shift++;
  P.key_shift -= P.cl;
  P.F = (int)(P.NBtot / cbins);
  P.fine_mask = (uint32_t)P.F - 1u;
  while ((1 << P.fb) < P.F) P.fb++;
  P.nwg = (int)((n + COARSE_PER_WG - 1) / COARSE_PER_WG);
  // records per fine workgroup: 32 Ki for the merged layout, 16 Ki for the generic one (measured: generic sort 0.250 -> 0.230 ms
  // at 2^20, merged equal within noise from 16 Ki to 64 Ki: profiles/r04m_*), 128 Ki when a bin has thousands of buckets
  // (the [bucket][sub] histogram that is scanned afterwards has NB * S entries)
  const size_t per_fine = kn.per_fine > 0 ? (size_t)kn.per_fine : (P.F >= 4096 ? 131072 : P.F >= 2048 ? 65536 : (L.glv ? 16384 : 32768));
  const size_t S = (E_max / cbins + per_fine - 1) / per_fine;
  P.S = S < 2 ? 2 : S > 64 ? 64 : (int)S;
  // fine workgroups: S slices for every bin + the extra slices of over-full bins (fine_plan: a slice holds at most 1.5 nominal ones)
  const size_t slice_nom = (E_max + cbins * (size_t)P.S - 1) / (cbins * (size_t)P.S);
  P.slice_cap = (uint32_t)(slice_nom + slice_nom / 2 + 1);
  P.fine_wgs = (unsigned)(cbins * (size_t)P.S + (E_max + P.slice_cap - 1) / P.slice_cap + 1);
  P.own.n_coarse = cbins * P.nwg;
  P.own.n_fine = (size_t)P.F * P.fine_wgs;
  // (chunk mode: sized for the largest chunk, the same request in every chunk's call)
  const size_t slice_nom_a = (E_alloc + cbins * (size_t)64 - 1) / (cbins * (size_t)64);      // (S <= 64: the smallest nominal slice)
  P.alloc.n_coarse = chunks ? cbins * ((n_alloc + COARSE_PER_WG - 1) / COARSE_PER_WG) : P.own.n_coarse;
  P.alloc.n_fine = chunks ? (size_t)P.F * (cbins * 64 + (E_alloc + slice_nom_a) / (slice_nom_a + slice_nom_a / 2 + 1) + 2) : P.own.n_fine;
  P.compact = ref_max <= ((size_t)1 << (31 - P.fb));      // references are < ref_max
  // scan-free sort (k_coarse_count, k_fine_scatter): no global scan at either level, nine launches -> five
  P.coarse_free = (kn.sort_scan_free & 1) != 0 && cbins <= (size_t)SORT_CTR_BINS;
  P.fine_free = (kn.sort_scan_free & 2) != 0 && P.F <= STAGE_F_MAX;
  P.coarse_c = (plain_merged && (L.c == 16 || L.c == 17 || L.c == 20)) ? L.c : 0;     // the default widths by SRS size
  P.scatter_staged = P.coarse_c != 0;
  // Fine level in one kernel per bin (k_fine_sort) where a workgroup holds a bin: 4-byte records, both levels scan-free, counters and a
  // round's window in half a CU's LDS, and the fullest bin of uniform scalars eight deviations inside the capacity.  Bins far above it keep
  // the two launches (2^24 pairs at 20 bits: ~213 000 records per bin), and so does chunk mode, whose buffers are sized once for chunks
  // of several lengths.  The grid: a workgroup per bin and one per slice that over-full bins can need (fine_max_slices).
  // (references strictly below 2^(31 - fb) - 1: the all-ones word is no record, it marks a register that holds none)
  const bool fused_can = !chunks && P.compact && ref_max < ((size_t)1 << (31 - P.fb)) && P.coarse_free && P.fine_free && P.F <= FINE_SORT_F_MAX;
  P.fine_fused = fused_can && kn.fine_fused != 0 && (kn.fine_fused > 0 || fine_bins_fit(fine_uniform_max_bin(L, n, (size_t)P.F)));
  if (P.fine_fused) {
    P.fine_wgs = (unsigned)(cbins + fine_max_slices(E_max, cbins, P.slice_cap));
    P.own.n_fine = P.alloc.n_fine = (size_t)P.F * P.fine_wgs;
  }
  return msm_sized(P, regions);
}

// ---- the segment walk of k_seg_accumulate ------------------------------------------------------------------------------------------
// Which entry a lane adds, which loads it has in flight meanwhile and where it stops -- the index logic of the kernel's loop, templated
// over its loads so that the host runs the same code over arrays of exactly the kernel's sizes (tests/hostcheck/seg_walk_shim.cpp).
constexpr uint32_t MANY_SENTINEL = 0xffffffffu;      // filler behind a polynomial's real entries (k_many_sort1): never a table row

// The segment of lane t: entries [e0, e1) of `total`; false when the lane has none (it must not load anything then).
MZK_HD bool seg_span(uint64_t t, uint32_t seg, uint32_t total, uint32_t* e0, uint32_t* e1) {
  const uint64_t e0w = t * seg;
  if (e0w >= total) return false;
  *e0 = (uint32_t)e0w;
  *e1 = (e0w + seg < total) ? (uint32_t)e0w + seg : total;
  return true;
}

// Bucket of entry e: the b with offsets[b] <= e < offsets[b + 1] (offsets[0] = 0 <= e < offsets[nbuckets]: the caller's contract).
// K-ary: the K - 1 pivots of a level do not depend on one another, so a level costs ONE load latency -- four levels for 2^16 buckets
// and five up to 2^20 with K = 16, five up to 2^25 with K = 32 (seg_first_bucket), where the binary search had 16 to 25 in a row.
// A pivot past hi is clamped to hi, which is above e by the invariant: no branch, and no load outside [lo, hi].
template <int K, class Offset>
MZK_HD size_t seg_bucket_search(Offset offset_at, size_t nbuckets, uint32_t e) {
  size_t lo = 0, hi = nbuckets;      // invariant: offsets[lo] <= e < offsets[hi]
  while (hi - lo > 1) {
    const size_t step = (hi - lo + K - 1) / K;
    uint32_t v[K];
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int j = 1; j < K; j++) v[j] = offset_at(lo + j * step < hi ? lo + j * step : hi);
    size_t below = 0;                // the pivots at or below e are a prefix: offsets is sorted
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int j = 1; j < K; j++) below += v[j] <= e ? 1 : 0;
    lo += below * step;
    if (lo + step < hi) hi = lo + step;
  }
  return lo;
}
template <class Offset>
MZK_HD size_t seg_first_bucket(Offset offset_at, size_t nbuckets, uint32_t e) {
  return nbuckets <= ((size_t)1 << 20) ? seg_bucket_search<16>(offset_at, nbuckets, e) : seg_bucket_search<32>(offset_at, nbuckets, e);
}

// The walk of one lane over entries [e0, e1), e0 < e1 <= offsets[nbuckets], starting in bucket b (seg_first_bucket(e0)), two deep:
// while entry e is added, the table row of entry e + 1 and entries[e + 2] are on their way.  Every load is issued one whole addition
// before its value is needed; the entry goes first because the memory counter retires in order and the next row's address is formed
// from it.  Likewise the end of the NEXT bucket is loaded when a bucket begins, so a bucket change waits for memory only across an
// empty bucket.  There is ONE row buffer and nothing is copied: a step first takes the current row out of the buffer -- the caller
// converts it into the point it adds, which it has to do anyway -- and only then asks for the next row into the same buffer.
// The look-ahead is unconditional -- a branch around a load would make the compiler wait for the memory counter as if the load had
// not been issued, which drains the pipeline -- and clamped instead: near the end of the segment it reads the segment's LAST entry
// and that entry's row again, never an entry at or past e1 and never a bucket end past offsets[nbuckets]; with SENT a MANY_SENTINEL
// entry asks for row 0 in its place, which every table has, and what the buffer then holds is not used.
//   entry_at(e), offset_at(b)    the loads
//   take_row(ent)                the buffer holds the row of the current entry `ent` (unless that is a sentinel): take it out.  This
//                                is the step's only wait for memory, and everything it can wait for was issued an addition ago
//   issue_row(ref)               request the table row of entry word `ref` into the buffer
//   flush(b)                     bucket b is complete as far as this segment goes: store the accumulator, start a new one
//   add(e, ent, b)               entry e (word `ent`, the row just taken) belongs to bucket b
template <bool SENT, class Entry, class Offset, class IssueRow, class TakeRow, class Flush, class Add>
MZK_HD void seg_walk(uint32_t e0, uint32_t e1, size_t b, size_t nbuckets, Entry entry_at, Offset offset_at, IssueRow issue_row, TakeRow take_row,
                     Flush flush, Add add) {
  const auto row_ref = [](uint32_t ent) { return (SENT && ent == MANY_SENTINEL) ? 0u : ent; };
  const auto end_after_next = [&](size_t bb) { return offset_at(bb + 2 <= nbuckets ? bb + 2 : nbuckets); };
  uint32_t ent = entry_at(e0);
  uint32_t ent1 = entry_at(e1 - e0 > 1 ? e0 + 1 : e0);
  issue_row(row_ref(ent));
  uint32_t bend = offset_at(b + 1), bend1 = end_after_next(b);
  for (uint32_t e = e0; e < e1; e++) {
    take_row(ent);
    const uint32_t ent2 = entry_at(e1 - e > 2 ? e + 2 : e1 - 1);      // (e < e1: the difference cannot wrap)
    issue_row(row_ref(ent1));
    if (e >= bend) {
      flush(b);
      b++, bend = bend1;
      while (e >= bend) b++, bend = offset_at(b + 1);     // across empty buckets only: these loads are waited for
      bend1 = end_after_next(b);                          // (one load, outside the loop: nothing in this step waits for it)
    }
    add(e, ent, b);
    ent = ent1, ent1 = ent2;
  }
  flush(b);
}

// ---- the digit walk of the window-table layouts ----------------------------------------------------------------------------------------
// Which bucket and which table row every window of a scalar goes to: the sort's kernels (mzk_msm.hip) and the host
// (tests/hostcheck/digit_walk_shim.cpp) run the same code.  The GLV half of walk_digits stays in mzk_msm.hip (it needs mzk_glv.h).
// (u32 / u64 as in mzk_field.h, which this header must not include: the same typedefs again, a legal redeclaration in the library's
// build and the only declaration in the stand-alone host builds -- keep both)
typedef uint32_t u32;
typedef uint64_t u64;
// digit of window `win` before carry handling: bits [c win, c win + c)
MZK_HD u32 raw_window(const u32* w, int win, int c) {
  const int bit = win * c;
  if (bit >= 256) return 0;
  const int k = bit >> 5, s = bit & 31;
  u64 v = w[k];
  if (k + 1 < 8) v |= (u64)w[k + 1] << 32;
  return (u32)(v >> s) & ((1u << c) - 1u);
}
// walk_digits (mzk_msm.hip) without the GLV split: the windows of the full scalar (canonical words w).  emit(window, key, payload) for
// every non-zero signed digit d: key = |d| - 1 in bucket set window % sets (merged), payload = the point reference -- row window / sets
// of the tables -- with the sign in bit 31.
template <class Emit>
MZK_HD void walk_digits_whole(const u32* w, const DigitLayout& L, size_t i, Emit emit) {
  const int c = L.c;
  const u32 half = 1u << (c - 1);
  u32 carry = 0;
  for (int win = 0; win < L.nwin; win++) {
    u32 raw = raw_window(w, win, c) + carry;
    u32 neg = 0, mag = raw;
    carry = 0;
    if (raw > half) { mag = (1u << c) - raw; neg = 1; carry = 1; }
    if (mag != 0) {
      const u32 key = (L.merged ? ((u32)(win % L.sets) << (c - 1)) : ((u32)win << (c - 1))) + (mag - 1);
      const u32 payload = (L.merged ? (u32)((size_t)(win / L.sets) * L.table_stride + i) : (u32)i) | (neg << 31);
      emit(win, key, payload);
    }
  }
}

// Signed c-bit digits without the serial carry walk: with t = k + sum_w (2^(c-1) - 1) 2^(c w) the digit of window w is
// window_w(t) - (2^(c-1) - 1) (the carries of that ONE long addition are exactly the recoding's carries: window w overflows iff
// raw_w + carry > 2^(c-1)), same digits as walk_digits.  Word k of the constant, C a compile-time width:
constexpr u32 digit_bias_word(int C, int k) {
  const int nwin = 254 / C + 1;
  const unsigned long long hm1 = (1ull << (C - 1)) - 1;
  unsigned long long acc = 0;
  for (int w = 0; w < nwin; w++) {
    const int sh = w * C - 32 * k;
    if (sh >= 0 && sh < 32) acc |= (hm1 << sh) & 0xffffffffull;
    else if (sh < 0 && sh > -32) acc |= hm1 >> (-sh);
  }
  return (u32)acc;
}
// walk_digits for the merged layout with a compile-time window width: the same (window, key, payload) triples in the same order,
// from ONE long addition and NWIN independent extractions with static word indices (walk_digits' runtime window index makes
// every word access a select chain).  Used by the coarse passes of the two-level sort and by the sortless small path.
template <int C, class Emit>
MZK_HD void walk_digits_merged(const u32* w, size_t table_stride, size_t i, Emit emit) {
  constexpr int NWIN = 254 / C + 1;
  constexpr u32 HALF = 1u << (C - 1), MASKC = (1u << C) - 1u;
  u32 t[9];
  u64 cy = 0;
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int k = 0; k < 8; k++) { cy += (u64)w[k] + digit_bias_word(C, k); t[k] = (u32)cy; cy >>= 32; }
  t[8] = (u32)cy + digit_bias_word(C, 8);
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int win = 0; win < NWIN; win++) {
    const int bit = win * C, k = bit >> 5, sft = bit & 31;
    const u64 pair = (u64)t[k] | ((k + 1 < 9) ? ((u64)t[k + 1] << 32) : 0ull);
    const u32 v = (u32)(pair >> sft) & MASKC;            // digit + HALF - 1
    if (v == HALF - 1u) continue;                        // digit 0
    const bool neg = v < HALF - 1u;
    const u32 mag = neg ? (HALF - 1u) - v : v - (HALF - 1u);
    emit(win, mag - 1u, (u32)((size_t)win * table_stride + i) | ((u32)neg << 31));
  }
}

// ---- the halving steps of the bucket reduction: which records a step adds, which launches run the steps ------------------------------------
// (the recursion: mzk_msm.hip, section 5).  Step t of a set of 2^lgB buckets has (t + 1) << (lgB - t - 1) additions; addition `id`
// is buf[*lo] += buf[*hi]: region a = id >> lgh folds its upper half onto its lower half, region 0 at 0, region a >= 1 at 2^(lgB - a).
MZK_HD void halve_indices(int lgB, int t, size_t id, size_t* lo, size_t* hi) {
  const int lgh = lgB - t - 1;
  const size_t a = id >> lgh, j = id & (((size_t)1 << lgh) - 1);
  *lo = ((a == 0) ? 0 : ((size_t)1 << (lgB - a))) + j;
  *hi = *lo + ((size_t)1 << lgh);
}
// SEVERAL steps per launch (k_halve_multi, k_halve_multi_row): steps t0 .. t0 + s - 1 pair no two indices closer than 2^lgs,
// lgs = lgB - t0 - s, so region 0 = [0, 2^(lgB - t0)) and the regions a = 1 .. t0 fall apart into 2^lgs problems of 2^s records
// each, one workgroup per problem: local record k is buf[base + (k << lgs)].  Region 0's problems leave every step's upper half
// behind as a new block (local block aa >= 1 at 2^(s - aa): the global region t0 + aa), the others only fold.
constexpr int HALVE_MULTI_MAX_S = 8;      // k_halve_multi: 2^8 records = 32 KiB of LDS, DPP-quad additions
constexpr int HALVE_ROW_MAX_S = 4;        // k_halve_multi_row: at most 8 additions per step, one per wave
struct HalveWg { int region, lgs; size_t base; };
MZK_HD size_t halve_multi_grid(int lgB, int t0, int s) { return (size_t)(t0 + 1) << (lgB - t0 - s); }      // workgroups per bucket set
MZK_HD HalveWg halve_multi_wg(int lgB, int t0, int s, size_t wg) {
  HalveWg g;
  g.lgs = lgB - t0 - s;
  g.region = (int)(wg >> g.lgs);
  g.base = ((g.region == 0) ? 0 : ((size_t)1 << (lgB - g.region))) + (wg & (((size_t)1 << g.lgs) - 1));
  return g;
}
// additions of local step tl = 0 .. s - 1, and the local records of addition `id`: the single-step rule on 2^s records
MZK_HD int halve_multi_ops(int region, int s, int tl) { return ((region == 0) ? tl + 1 : 1) << (s - tl - 1); }
MZK_HD void halve_multi_pair(int s, int tl, int id, int* lo, int* hi) {
  const int lgh = s - tl - 1, aa = id >> lgh;
  *lo = ((aa == 0) ? 0 : (1 << (s - aa))) + (id & ((1 << lgh) - 1));
  *hi = *lo + (1 << lgh);
}
// what later steps and the tail still read: local 0 and, in region 0, the heads 2^(e - 1) of the blocks the steps left behind
MZK_HD int halve_multi_live(int region, int s) { return (region == 0) ? s + 1 : 1; }
MZK_HD int halve_multi_live_at(int e) { return (e == 0) ? 0 : (1 << (e - 1)); }

// The launches in front of the single-workgroup tail (launch_halving_steps, mzk_msm.hip): one lane per addition while a step is
// throughput-bound (>= 2^16 additions over all sets), then DPP-quad additions -- k_halve_multi, up to eight steps per launch, in the
// latency regime of at most one workgroup per CU, launches of one step above it -- until a step is at most `tail_max` additions wide.
// Once a k_halve_multi launch has left at most eight steps and launches of up to four steps need at most one workgroup per CU, the
// rest runs on row operations (k_halve_multi_row): ceil(steps / 4) launches, four steps each and the remainder last; such a
// workgroup has at most eight additions per step, one per wave, and a row addition is a third of the quad form's chain.
enum { HALVE_STEP_WIDE = 0, HALVE_STEP_QUAD = 1, HALVE_MULTI_QUAD = 2, HALVE_MULTI_ROW = 3 };
struct HalveLaunch { int kind, t, steps; size_t grid; };      // grid: workgroups per bucket set (x sets)
struct HalvePlan {
  int count = 0, t_next = 0;                                  // t_next: the first step left to the tail (lgB: the tail only forms the weighted sum)
  HalveLaunch l[32];                                          // (a launch takes at least one of the lgB < 32 steps)
};
static inline HalvePlan halve_plan(int lgB, int sets, int num_cu, size_t tail_max, int halve_row) {
  HalvePlan H;
  if (lgB < 0 || lgB >= 32) return H;
  auto put = [&H](int kind, int t, int steps, size_t grid) { H.l[H.count++] = HalveLaunch{kind, t, steps, grid}; };
  int t = 0;
  bool multi_ran = false;
  while (t < lgB && ((size_t)(t + 1) << (lgB - t - 1)) > tail_max) {
    const size_t total = (size_t)(t + 1) << (lgB - t - 1);
    if (total * (size_t)sets >= ((size_t)1 << 16)) { put(HALVE_STEP_WIDE, t, 1, (total + 127) / 128); t++; continue; }
    // several steps per launch only with at most one workgroup per CU.  Its workgroups are unequal (region 0 carries t + 1 times the
    // additions of the others) and stay where they were placed, so with more of them than CUs the launches of ONE step, which spread every
    // step's additions over the whole chip, are faster (generic 2^20, 384 workgroups: bucket reduction 0.204 -> 0.222 ms; 256 x 2^10 at
    // 11 bits 0.196 -> 0.270; profiles/round6_halving_multi_and_rec4_ab.txt)
    const int left = lgB - t, st = left < HALVE_MULTI_MAX_S ? left : HALVE_MULTI_MAX_S;
    if (halve_multi_grid(lgB, t, st) * (size_t)sets > (size_t)num_cu) { put(HALVE_STEP_QUAD, t, 1, (4 * total + 127) / 128); t++; continue; }
    bool row = halve_row != 0 && multi_ran && left <= 2 * HALVE_ROW_MAX_S;
    for (int tt = t; row && tt < lgB; tt += HALVE_ROW_MAX_S) {
      const int s = lgB - tt < HALVE_ROW_MAX_S ? lgB - tt : HALVE_ROW_MAX_S;
      row = halve_multi_grid(lgB, tt, s) * (size_t)sets <= (size_t)num_cu;
    }
    if (row) {
      for (; t < lgB; t += HALVE_ROW_MAX_S) {
        const int s = lgB - t < HALVE_ROW_MAX_S ? lgB - t : HALVE_ROW_MAX_S;
        put(HALVE_MULTI_ROW, t, s, halve_multi_grid(lgB, t, s));
      }
      t = lgB;
      break;
    }
    put(HALVE_MULTI_QUAD, t, st, halve_multi_grid(lgB, t, st));
    t += st, multi_ran = true;
  }
  H.t_next = t;
  return H;
}

// Chunk mode (msm_chunked_impl) covers the problems whose every chunk takes the two-level sort with one bucket set: the generic layout
// and window tables of 13 bits and more, from 2^18 pairs on (every chunk must keep the accumulate's lanes busy).  The path does not
// depend on the CU count.
static inline bool msm_chunkable(size_t n_total, int point_kind, size_t table_stride, const MsmKnobs& kn) {
  if (n_total < ((size_t)1 << 18)) return false;
  const MsmPlan P = msm_plan(n_total, n_total, n_total, point_kind, table_stride, 256, 1, kn);
  return P.err == MZK_OK && P.L.sets == 1 && P.path == MsmPath::TwoLevel;
}

}  // namespace mzk
