// mzk_ntt_plan.h -- how one transform call (mzk_ntt.hip over Fr / M128, mzk_gl.hip over Goldilocks) is launched, decided on the host
// before anything is launched: the tile geometry, the split of log2 n into passes and one step per pass with its grid, block, LDS
// bytes and write-through flag.  A pure function of the field id, log2 n, the batch and the tuning switches.  Host-only C++17 with no
// HIP include, so that the schedule can be compiled and checked on its own (tests/test_hostcheck_ntt_plan.py).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include "../../include/mzk.h"

namespace mzk {

#ifndef MZK_NTT_THREADS
#define MZK_NTT_THREADS 256
#endif
#ifndef MZK_NTT_MAX_LEVEL_LOG
#define MZK_NTT_MAX_LEVEL_LOG 8
#endif

// ---- tile geometries ----------------------------------------------------------------------------------------------------------------
// A workgroup of `nt` lanes transforms a tile of 2^tl elements in LDS; a pass's level is at most 2^maxlv points.  twg: the in-tile
// twiddles are NOT staged in LDS but read from global memory; wpe: waves per SIMD the register budget must allow.
// S (1024 elements, 256 lanes, levels of <= 2^8): every size below 2^20.  S1: the one-pass transforms of 2^9 and 2^10 points, whose
// level is wider than S's twiddle rows.  L (4096 elements, 1024 lanes = one workgroup per CU, levels of <= 2^10): where it saves a
// whole pass -- a 2^20 transform is TWO passes of 2^10 levels instead of three (one global round trip and one inter-pass twiddle
// product per element less), each tile still 4+ adjacent columns wide (>= 128-byte runs).  The Fr tile is 144 KiB of limbs, so its
// in-tile twiddles are staged as packed words (16 KiB: 160 KiB exactly) and unpacked at use (ntt_twpack).
// M (M128 large tiles): a 4096-element M128 tile is 80 KiB, so without its 10 KiB of twiddles TWO workgroups of 512 lanes share a CU
// and one's loads / stores run under the other's butterflies (the single 1024-lane workgroup per CU had nothing to overlap its ~22 us
// of global traffic with).  GL: Goldilocks, 4096 base elements = 32 KiB (+ padding + 16 KiB of in-tile twiddles, static LDS: three
// workgroups of four waves per CU).
struct NttGeo { int tl, nt, maxlv; bool twg; int wpe; };
enum NttGeoId { NTT_GEO_S = 0, NTT_GEO_S1 = 1, NTT_GEO_L = 2, NTT_GEO_M = 3, NTT_GEO_GL = 4 };
constexpr NttGeo NTT_GEOS[5] = {{10, MZK_NTT_THREADS, MZK_NTT_MAX_LEVEL_LOG, false, 1},
                                {10, MZK_NTT_THREADS, 10, false, 1},
                                {12, 1024, 10, false, 1},
                                {12, 512, 10, true, 4},
                                {12, 256, 8, false, 3}};
constexpr size_t NTT_LDS_DEFAULT_MAX = 64 * 1024, NTT_LDS_MAX = 160 * 1024;      // above the first a kernel needs the dynamic-LDS attribute

// Fr / M128 element: `limbs` 29-bit limbs in LDS, `words` packed u32 words in memory (mzk_field.h: P::L, P::NW)
constexpr int ntt_limbs(int fid) { return fid == MZK_FIELD_M128 ? 5 : 9; }
constexpr int ntt_words(int fid) { return fid == MZK_FIELD_M128 ? 4 : 8; }
constexpr bool ntt_twpack(NttGeo g, int limbs) { return !g.twg && (size_t)4 * limbs * ((1 << g.tl) + (1 << (g.maxlv - 1))) > NTT_LDS_MAX; }
// dynamic LDS of the Fr / M128 pass kernels: the tile limb-major, then the rows of the widest level's n/2 in-tile twiddles
constexpr size_t ntt_lds_bytes(NttGeo g, int limbs, int words) {
  return 4 * ((size_t)limbs << g.tl) + (g.twg ? 0 : 4 * ((size_t)(ntt_twpack(g, limbs) ? words : limbs) << (g.maxlv - 1)));
}

// log2 of every pass's level, in launch order; a kernel argument of the last-pass kernels
struct NttLevels { int nlev; int lg[4]; };

// The transforms' launch-shape switches: the shipped values here; the tuning build reads MZK_NTT_<NAME> over them (ntt_knobs, mzk_ntt.hip).
struct NttKnobs {
  int large_fr = -1, large_m128 = -1;      // MZK_NTT_LARGE_FR / MZK_NTT_LARGE_M128: smallest log2 size forced onto the large geometry (99 = never)
  int m128_two_wg = 21;                    // MZK_NTT_M128_TWO_WG: smallest log2 size of a large-geometry M128 transform on M (99 = never)
  int wt_lo = 21;                          // MZK_NTT_WT_LO
  int wt_hi_fr = 24, wt_hi_m128 = 26;      // MZK_NTT_WT_HI
  int wt_mask = 3;                         // MZK_NTT_WT_MASK: bit 0 = the strided passes, bit 1 = the last pass
};

// One launch.  Strided (every pass but the last): in place on the 2^lgn strided columns of a block of 2^(lgn + lgM) elements, 2^lgc
// adjacent columns per tile.  Last: contiguous rows of 2^lgn, scattered transposed, 2^lgr of the total_rows = batch << lg_rows per tile.
enum { NTT_STEP_STRIDED = 0, NTT_STEP_LAST = 1 };
struct NttStep {
  int kind, lgn;
  int lgM, lgc;                        // strided
  int lgr, lg_rows; size_t total_rows; // last
  unsigned grid, block;
  size_t lds;                          // dynamic LDS bytes (Goldilocks: 0, its tile is static)
  bool wt;                             // stores go out write-through (stream_store16, mzk_ntt.hip)
};

struct NttSchedule {
  int err = MZK_OK;
  char msg[64] = {};
  int fid = 0; unsigned logn = 0; size_t batch = 0;      // what was asked
  int geo = NTT_GEO_S;
  bool large = false;        // Fr / M128: the large geometry's level split; a key of the plan cache (the tables follow the split)
  NttLevels li{};
  size_t tmp_bytes = 0;      // WS_NTT_TMP: what the strided passes write and the next pass reads (0: single pass)
  bool lds_attr = false;     // the kernels of `geo` need hipFuncAttributeMaxDynamicSharedMemorySize = NTT_LDS_MAX
  int nsteps = 0;
  NttStep steps[4];
};

// fid: MZK_FIELD_FR, MZK_FIELD_M128, MZK_FIELD_M64 or MZK_FIELD_M64X3; 1 <= logn <= 32, batch << logn <= 2^40 (the entry points check)
static inline NttSchedule ntt_plan(int fid, unsigned logn, size_t batch, const NttKnobs& k) {
  NttSchedule S;
  S.fid = fid; S.logn = logn; S.batch = batch;
  const bool gl = fid == MZK_FIELD_M64 || fid == MZK_FIELD_M64X3, m128 = fid == MZK_FIELD_M128;
  const size_t nc = fid == MZK_FIELD_M64X3 ? 3 : 1;      // Goldilocks: one workgroup per tile and coefficient
  const size_t bytes = (batch << logn) * (gl ? 8 * nc : 4 * (size_t)ntt_words(fid));
  const int small_lv = NTT_GEOS[NTT_GEO_S].maxlv, large_lv = NTT_GEOS[NTT_GEO_L].maxlv;
  // The large geometry is used exactly where it saves a whole pass: 2^20 (two passes of 2^10 instead of 7/7/6: measured
  // Fr 0.147 -> 0.137 ms, M128 0.063 -> 0.056 ms) and 2^25 .. 2^30.  Where both geometries need three passes the small
  // tiles win (2^21 .. 2^24: Fr +8 %, M128 +16 % with large tiles; tools/timing/time_ntt.py with MZK_NTT_LARGE_FR / MZK_NTT_LARGE_M128).
  // A BATCH of transforms gives the small tiles what a single 2^20 transform lacks: several rounds of workgroups per CU,
  // so the loads and stores of one tile run under the butterflies of its neighbours (four small-tile workgroups share a
  // CU; the large tile owns it) -- from three Fr / two M128 transforms of 2^20 on, three overlapped passes beat two
  // exposed ones (tools/timing/ntt_batch.py: Fr 0.1045 vs 0.1131 ms per transform at batch 16, M128 0.041 vs 0.048).
  if (!gl) {
    const int force = m128 ? k.large_m128 : k.large_fr;
    if (force >= 0) S.large = logn >= (unsigned)force && logn >= 14;
    else S.large = logn >= 20 && batch <= (m128 ? 1u : 2u) && (logn + large_lv - 1) / large_lv < (logn + small_lv - 1) / small_lv;
  }
  // levels: one pass up to a small (Goldilocks: the) tile, else the fewest passes of at most the widest level, as equal as possible
  const int one_pass = NTT_GEOS[gl ? NTT_GEO_GL : NTT_GEO_S].tl, maxlv = gl ? NTT_GEOS[NTT_GEO_GL].maxlv : S.large ? large_lv : small_lv;
  NttLevels& li = S.li;
  if (logn <= (unsigned)one_pass) {
    li.nlev = 1;
    li.lg[0] = (int)logn;
  } else {
    const int n = (int)((logn + maxlv - 1) / maxlv), base = (int)logn / n, extra = (int)logn % n;
    li.nlev = n;
    // Goldilocks, the wider levels last: a strided pass works on whole tiles, so the block it splits -- at the second to last pass the
    // last two levels together -- must hold at least one (2^13 = 6 + 7, 2^17 = 5 + 6 + 6); Fr / M128: the wider ones first, and the
    // same holds (both checked below, and for every admitted size by the host test)
    for (int i = 0; i < n; i++) li.lg[i] = base + ((gl ? i >= n - extra : i < extra) ? 1 : 0);
  }
  // M128 large tiles: two 512-lane workgroups per CU (M) once there are at least two tiles per CU -- 2^25 and up: 1.69 instead of
  // 1.83 - 1.85 ms at 2^25 (same box A/B, profiles/round4_ntt_m128_two_workgroups_ab.txt).  A 2^20 transform is exactly 256 tiles, ONE per CU
  // whatever the workgroup size, and the 512-lane form only halves the lanes working on it (0.057 against 0.047 ms): it keeps the
  // single 1024-lane workgroup.
  if (gl) S.geo = NTT_GEO_GL;
  else if (S.large) S.geo = m128 && (int)logn >= k.m128_two_wg ? NTT_GEO_M : NTT_GEO_L;
  else S.geo = li.nlev == 1 && li.lg[0] > small_lv ? NTT_GEO_S1 : NTT_GEO_S;
  const NttGeo g = NTT_GEOS[S.geo];
  const size_t lds = gl ? 0 : ntt_lds_bytes(g, ntt_limbs(fid), ntt_words(fid));
  S.lds_attr = lds > NTT_LDS_DEFAULT_MAX;
  S.tmp_bytes = li.nlev > 1 ? bytes : 0;
  // write-through stores for multi-pass Fr / M128 transforms whose data is between 2^wt_lo and 2^wt_hi bytes
  // (same-box map, profiles/round5_ntt_write_through_ab.txt: Fr 2^17..2^19 -1..-13 %, M128 2^17..2^22 -2..-16 %; below 2 MiB and
  // from 32 MiB (Fr) / 128 MiB (M128) up it gains nothing or costs 3-9 %: the working set no longer sits in the Infinity Cache)
  const bool wt = !gl && li.nlev > 1 && bytes >= ((size_t)1 << k.wt_lo) && bytes <= ((size_t)1 << (m128 ? k.wt_hi_m128 : k.wt_hi_fr));
  auto fail = [&](const char* what) { S.err = MZK_E_ARG; snprintf(S.msg, sizeof S.msg, "%s", what); return S; };
  auto push = [&](NttStep st, size_t grid) {
    st.grid = (unsigned)grid; st.block = (unsigned)g.nt; st.lds = lds;
    S.steps[S.nsteps++] = st;
  };
  int lg_after = (int)logn;      // log2 of the block the pass splits
  for (int t = 0; t < li.nlev - 1; t++) {
    const int lgn = li.lg[t], lgM = lg_after - lgn, lgc = g.tl - lgn;
    const size_t grid = (batch << (logn - g.tl)) * nc;      // a tile per workgroup; the kernel's block index runs over the batch too
    if (grid > 0x7fffffffu) return fail("ntt: too many tiles for one launch");
    if (lgM < lgc) return fail("ntt: level split leaves a block smaller than a tile");
    push(NttStep{NTT_STEP_STRIDED, lgn, lgM, lgc, 0, 0, 0, 0, 0, 0, wt && (k.wt_mask & 1)}, grid);
    lg_after = lgM;
  }
  const int lgn = li.lg[li.nlev - 1], lg_rows = (int)logn - lgn;
  const size_t total_rows = batch << lg_rows;
  int lgr = g.tl - lgn;
  while (lgr > 0 && ((size_t)1 << lgr) > total_rows) lgr--;
  const size_t grid = ((total_rows + ((size_t)1 << lgr) - 1) >> lgr) * nc;
  if (grid > 0x7fffffffu) return fail("ntt: too many tiles for one launch");
  push(NttStep{NTT_STEP_LAST, lgn, 0, 0, lgr, lg_rows, total_rows, 0, 0, 0, wt && (k.wt_mask & 2)}, grid);
  return S;
}

}  // namespace mzk
