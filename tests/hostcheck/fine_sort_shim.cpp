// The fused fine level of the MSM's sort (k_fine_sort and the k_fine_scatter launch behind it, myzkp_amd/csrc/mzk_msm.hip) run on the
// host for tests/test_hostcheck_fine_sort.py: which workgroup takes which bin or slice, the whole-bin capacity, the slice bounds and the
// grid size are the kernels' own code (mzk_msm_plan.h: fine_reg_record, fine_bin_slices, fine_slice_of_bin, fine_slice_bounds,
// fine_max_slices); the counting, the prefix and the staging window around them are restated lane by lane.  Every array has EXACTLY the
// size the kernels' arrays have (bin bounds bins + 1, records and entries `total`, offsets buckets + 1, the window 2^FINE_WIN_LOG, the
// slice histograms F x workgroups), so that an index past any of them is an AddressSanitizer report.
// A stand-alone program: no arguments: the checks, exit status 0 and "ok <cases> <workgroups>";
// "plan <window bits> <table stride>": the smallest n at which msm_plan sorts in two levels at that width, and what it chooses there.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <string>
#include <vector>
#include "../../myzkp_amd/csrc/mzk_msm_plan.h"

using namespace mzk;

static int g_fail = 0;
#define CHECK(c, ...) do { if (!(c)) { if (g_fail++ < 20) { printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #c); printf(__VA_ARGS__); printf("\n"); } } } while (0)

struct Case {
  std::string name;
  int F;
  uint32_t cap;                      // records per slice of an over-full bin (MsmPlan::slice_cap)
  std::vector<uint32_t> lens;        // records per bin
};

template <class T>
struct Heap {      // exactly n elements
  T* p;
  size_t n;
  explicit Heap(size_t n_, T fill) : p((T*)malloc(n_ ? n_ * sizeof(T) : 1)), n(n_) { for (size_t i = 0; i < n; i++) p[i] = fill; }
  ~Heap() { free(p); }
  Heap(const Heap&) = delete;
  T& operator[](size_t i) { return p[i]; }
};

// the 4-byte record of the sort (Rec4, mzk_msm.hip): reference << (fb + 1) | bucket in the bin << 1 | sign
static uint32_t rec_make(uint32_t payload, uint32_t fine, int fb) { return ((payload & 0x7fffffffu) << (fb + 1)) | (fine << 1) | (payload >> 31); }
static uint32_t rec_fine(uint32_t r, uint32_t fmask) { return (r >> 1) & fmask; }
static uint32_t rec_payload(uint32_t r, int fb) { return (r >> (fb + 1)) | ((r & 1u) << 31); }

static size_t run_case(const Case& c, uint32_t seed) {
  const int bins = (int)c.lens.size(), F = c.F;
  int fb = 0;
  while ((1 << fb) < F) fb++;
  const uint32_t fmask = (uint32_t)F - 1u;
  const size_t NB = (size_t)bins * F;
  Heap<uint32_t> bound(bins + 1, 0);
  uint64_t run = 0;
  for (int b = 0; b < bins; b++) { bound[b] = (uint32_t)run; run += c.lens[b]; }
  CHECK(run < ((uint64_t)1 << 31 >> fb), "%s: the case itself: %llu records do not fit the 4-byte form", c.name.c_str(), (unsigned long long)run);
  const uint32_t total = (uint32_t)run;
  bound[bins] = total;
  // the host's grid: it knows the entry count's bound, here exactly the count (the tightest bound it can have)
  const size_t max_slices = fine_max_slices(total, bins, c.cap), fine_wgs = bins + max_slices;
  Heap<uint32_t> tmp(total, 0), entries(total, 0xffffffffu), covered(total, 0), offsets(NB + 1, 0xdeadbeefu), finehist((size_t)F * fine_wgs, 0xdeadbeefu),
      bucket_tot(NB, 0), win((size_t)1 << FINE_WIN_LOG, 0), cnt(F, 0);
  uint32_t x = seed * 2654435761u + 99u;
  for (uint32_t e = 0; e < total; e++) {      // record e: reference e (unique), a bucket that is skewed in some bins, a sign
    x = x * 1664525u + 1013904223u;
    const uint32_t fine = (e % 7 == 0) ? fmask : (e % 5 == 0) ? 0u : (x >> 9) & fmask;
    tmp[e] = rec_make(e | (x & 0x80000000u), fine, fb);
  }
  // X_b: exclusive prefix of the slice counts (the kernels: block_excl_scan over one lane per bin)
  std::vector<uint32_t> X(bins + 1, 0);
  for (int b = 0; b < bins; b++) X[b + 1] = X[b] + fine_bin_slices(c.lens[b], c.cap);
  CHECK(X[bins] <= max_slices, "%s: %u slices, the grid has %zu extra workgroups", c.name.c_str(), X[bins], max_slices);
  size_t last_used = 0;
  std::vector<FineSlice> slices;
  constexpr int NPOS = (FINE_REGS + 1) / 2;
  constexpr uint32_t WIN = 1u << FINE_WIN_LOG, NOWHERE = 0xffffu, NO_RECORD = 0xffffffffu;
  std::vector<uint32_t> r((size_t)FINE_LANES * FINE_REGS), pos((size_t)FINE_LANES * NPOS);
  for (size_t wg = 0; wg < fine_wgs; wg++) {
    uint32_t idx;
    const bool is_extra = fine_wg_is_extra((uint32_t)wg, (uint32_t)max_slices, &idx);
    CHECK(is_extra ? idx < max_slices : idx < (uint32_t)bins, "%s: workgroup %zu is %s %u", c.name.c_str(), wg, is_extra ? "slice" : "bin", idx);
    const size_t w = idx;         // the bin, or the extra workgroup
    if (is_extra) {               // lane b asks whether it is one of bin b's slices
      const uint32_t j = idx;
      int hits = 0;
      FineSlice p{};
      for (int b = 0; b < bins; b++) {
        FineSlice q{};
        if (fine_slice_of_bin(j, b, bound[b], bound[b + 1] - bound[b], X[b], c.cap, &q)) { hits++; p = q; }
      }
      CHECK(hits == (j < X[bins] ? 1 : 0), "%s: extra workgroup %u belongs to %d bins", c.name.c_str(), j, hits);
      if (!hits) continue;
      last_used = j;
      CHECK(p.active && p.s >= 0 && p.s < p.Sb && c.lens[p.bin] > FINE_BIN_CAP, "%s: slice %d of %d of bin %d (%u records)", c.name.c_str(), p.s, p.Sb, p.bin, c.lens[p.bin]);
      CHECK(p.lo >= bound[p.bin] && p.lo <= p.hi && p.hi <= bound[p.bin + 1] && p.hi - p.lo <= c.cap, "%s: slice [%u, %u) of bin %d [%u, %u)", c.name.c_str(), p.lo, p.hi,
            p.bin, bound[p.bin], bound[p.bin + 1]);
      CHECK(p.start == bound[p.bin], "%s: start of bin %d", c.name.c_str(), p.bin);
      for (int f = 0; f < F; f++) cnt[f] = 0;
      for (uint32_t e = p.lo; e < p.hi; e++) { covered[e]++; cnt[rec_fine(tmp[e], fmask)]++; }
      const size_t hbase = (size_t)F * (w - (size_t)p.s);
      for (int f = 0; f < F; f++) {
        finehist[hbase + (size_t)f * p.Sb + p.s] = cnt[f];
        bucket_tot[(size_t)p.bin * F + f] += cnt[f];
      }
      slices.push_back(p);
      continue;
    }
    const uint32_t start = bound[w], len = bound[w + 1] - start;
    if (w == 0) offsets[NB] = bound[bins];
    if (len > FINE_BIN_CAP) continue;
    // (registers k >= rows hold no record in any lane: set once here, the loops below walk the rows that hold some)
    const int rows = (int)((len + FINE_LANES - 1) / FINE_LANES), prows = (rows + 1) / 2;
    CHECK(rows <= FINE_REGS, "%s: %u records need %d registers", c.name.c_str(), len, rows);
    std::fill(r.begin(), r.end(), NO_RECORD);
    std::fill(pos.begin(), pos.end(), NOWHERE | (NOWHERE << 16));
    for (uint32_t lane = 0; lane < (uint32_t)FINE_LANES; lane++)
      for (int k = 0; k < rows; k++) {
        uint32_t v = NO_RECORD;
        if (fine_reg_record(k, lane) < len) { v = tmp[start + fine_reg_record(k, lane)]; covered[start + fine_reg_record(k, lane)]++; }
        CHECK(v != NO_RECORD || fine_reg_record(k, lane) >= len, "%s: a record of all ones", c.name.c_str());
        r[(size_t)lane * FINE_REGS + k] = v;
      }
    for (int f = 0; f < F; f++) cnt[f] = 0;
    for (uint32_t lane = 0; lane < (uint32_t)FINE_LANES; lane++)
      for (int h = 0; h < prows; h++) {
        uint32_t half[2] = {NOWHERE, NOWHERE};
        for (int o = 0; o < 2 && 2 * h + o < FINE_REGS; o++) {
          const uint32_t v = r[(size_t)lane * FINE_REGS + 2 * h + o];
          if (v != NO_RECORD) half[o] = cnt[rec_fine(v, fmask)]++;
          CHECK(half[o] <= NOWHERE, "%s: rank %u", c.name.c_str(), half[o]);
        }
        pos[(size_t)lane * NPOS + h] = half[0] | (half[1] << 16);
      }
    uint32_t pre = 0;
    for (int f = 0; f < F; f++) { const uint32_t v = cnt[f]; cnt[f] = pre; offsets[w * F + f] = start + pre; pre += v; }
    CHECK(pre == len, "%s: bin %zu counted %u of %u", c.name.c_str(), w, pre, len);
    for (uint32_t lane = 0; lane < (uint32_t)FINE_LANES; lane++)
      for (int h = 0; h < prows; h++) {
        uint32_t half[2] = {pos[(size_t)lane * NPOS + h] & 0xffffu, pos[(size_t)lane * NPOS + h] >> 16};
        for (int o = 0; o < 2 && 2 * h + o < FINE_REGS; o++) {
          const uint32_t first = cnt[rec_fine(r[(size_t)lane * FINE_REGS + 2 * h + o], fmask)];
          half[o] = half[o] == NOWHERE ? NOWHERE : first + half[o];
          CHECK(half[o] == NOWHERE || half[o] < len, "%s: place %u in a bin of %u", c.name.c_str(), half[o], len);
        }
        pos[(size_t)lane * NPOS + h] = half[0] | (half[1] << 16);
      }
    for (uint32_t w0 = 0; w0 < len; w0 += WIN) {
      const uint32_t q = w0 >> FINE_WIN_LOG;
      CHECK(q < (NOWHERE >> FINE_WIN_LOG), "%s: round %u takes the empty registers", c.name.c_str(), q);
      for (uint32_t lane = 0; lane < (uint32_t)FINE_LANES; lane++)
        for (int k = 0; k < rows; k++) {
          const uint32_t both = pos[(size_t)lane * NPOS + (k >> 1)], at = (k & 1) ? both >> 16 : both & 0xffffu;
          if ((at >> FINE_WIN_LOG) == q) win[at & (WIN - 1u)] = rec_payload(r[(size_t)lane * FINE_REGS + k], fb);
        }
      const uint32_t m = (len - w0 < WIN) ? len - w0 : WIN;
      for (uint32_t j = 0; j < m; j++) entries[start + w0 + j] = win[j];
    }
  }
  CHECK(slices.empty() || last_used < max_slices, "%s: extra workgroup %zu of %zu", c.name.c_str(), last_used, max_slices);
  // the second launch over the slices (k_fine_scatter's scan-free form, restated): bucket offsets from the bin's totals, runs claimed per slice
  {
    Heap<uint32_t> cur(NB, 0);
    for (const FineSlice& p : slices) {
      uint32_t pre = p.start;
      std::vector<uint32_t> gbase(F);
      for (int f = 0; f < F; f++) {
        const size_t bkt = (size_t)p.bin * F + f;
        gbase[f] = pre + cur[bkt];
        cur[bkt] += finehist[(size_t)F * X[p.bin] + (size_t)f * p.Sb + p.s];
        if (p.s == 0) offsets[bkt] = pre;
        pre += bucket_tot[bkt];
      }
      for (uint32_t e = p.lo; e < p.hi; e++) entries[gbase[rec_fine(tmp[e], fmask)]++] = rec_payload(tmp[e], fb);
    }
  }
  // every record taken exactly once; offsets monotone from 0 to total; every bucket's run holds its own records, each record once
  for (uint32_t e = 0; e < total; e++) CHECK(covered[e] == 1, "%s: record %u taken %u times", c.name.c_str(), e, covered[e]);
  CHECK(offsets[0] == 0 && offsets[NB] == total, "%s: offsets run from %u to %u of %u", c.name.c_str(), offsets[0], offsets[NB], total);
  for (size_t b = 0; b < NB; b++) CHECK(offsets[b] <= offsets[b + 1], "%s: offsets fall at bucket %zu", c.name.c_str(), b);
  Heap<uint32_t> seen(total, 0);
  for (size_t b = 0; b < NB && !g_fail; b++)
    for (uint32_t e = offsets[b]; e < offsets[b + 1]; e++) {
      const uint32_t ref = entries[e] & 0x7fffffffu;
      CHECK(ref < total, "%s: entry %u is %08x", c.name.c_str(), e, entries[e]);
      if (ref >= total) continue;
      seen[ref]++;
      CHECK(rec_payload(tmp[ref], fb) == entries[e], "%s: entry %u lost its sign", c.name.c_str(), e);
      CHECK(ref >= bound[b / F] && ref < bound[b / F + 1] && rec_fine(tmp[ref], fmask) == b % F, "%s: record %u in bucket %zu", c.name.c_str(), ref, b);
    }
  for (uint32_t e = 0; e < total && !g_fail; e++) CHECK(seen[e] == 1, "%s: record %u written %u times", c.name.c_str(), e, seen[e]);
  return fine_wgs;
}

// lengths whose slices are exactly the grid's extra workgroups: the optimum fine_max_slices finds, built bin by bin
static std::vector<uint32_t> fullest(size_t E, size_t bins, uint32_t cap) {
  const size_t open = (size_t)FINE_BIN_CAP + 1, a = (open + cap - 1) / cap, first = a * cap - FINE_BIN_CAP, want = fine_max_slices(E, bins, cap);
  for (size_t m = 1; m <= bins && m * open <= E; m++) {
    const size_t rest = E - m * open, cheap = rest / first < m ? rest / first : m, more = (rest - cheap * first) / cap;
    if (m * a + cheap + more != want) continue;
    std::vector<uint32_t> v(bins, 0);
    for (size_t b = 0; b < m; b++) v[b] = (uint32_t)(open + (b < cheap ? first : 0));
    v[0] += (uint32_t)(more * cap);
    return v;
  }
  return std::vector<uint32_t>(bins, 0);
}

static int plan_mode(int c, size_t stride) {
  const int kind = MSM_PTS_TABLES | (c << 8) | (1 << 16);
  for (size_t n = 1; n <= stride; n++) {
    const MsmPlan P = msm_plan(n, n, n, kind, stride, 256, 0, MsmKnobs());
    if (P.err != MZK_OK || P.path != MsmPath::TwoLevel) continue;
    const MsmPlan Q = msm_plan(n + 3 <= stride ? n + 3 : n, n + 3 <= stride ? n + 3 : n, n + 3 <= stride ? n + 3 : n, kind, stride, 256, 0, MsmKnobs());
    const MsmPlan Pfull = msm_plan(stride, stride, stride, kind, stride, 256, 0, MsmKnobs());
    printf("n %zu fused %d fused_plus3 %d fused_at_stride %d F %d bins %d cap %u fine_wgs %u\n", n, (int)P.fine_fused, (int)Q.fine_fused, (int)Pfull.fine_fused, P.F, 1 << P.cl,
           FINE_BIN_CAP, P.fine_wgs);
    return 0;
  }
  printf("none\n");
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 4 && !strcmp(argv[1], "plan")) return plan_mode(atoi(argv[2]), (size_t)atoll(argv[3]));
  const uint32_t CAP = FINE_BIN_CAP;
  std::vector<Case> cases;
  const struct { int bins, F; uint32_t cap; } shapes[] = {{512, 128, 23041}, {256, 16, 1486}, {32, 1024, 33792}, {8, 256, 50000}};
  for (const auto& s : shapes) {
    const auto tag = [&](const char* what) { return std::string(what) + " (" + std::to_string(s.bins) + " bins of " + std::to_string(s.F) + ", slices of " + std::to_string(s.cap) + ")"; };
    const std::vector<uint32_t> none(s.bins, 0);
    cases.push_back({tag("all empty"), s.F, s.cap, none});
    cases.push_back({tag("all equal, 700"), s.F, s.cap, std::vector<uint32_t>(s.bins, 700)});
    if (s.bins <= 64) cases.push_back({tag("all at capacity"), s.F, s.cap, std::vector<uint32_t>(s.bins, CAP)});
    for (uint32_t len : {CAP - 1, CAP, CAP + 1}) {
      std::vector<uint32_t> v(s.bins, 300);
      v[s.bins / 3] = len;
      cases.push_back({tag("one bin at capacity - 1 / capacity / capacity + 1"), s.F, s.cap, v});
      std::vector<uint32_t> lone(none);
      lone[s.bins - 1] = len;      // the last bin, nothing around it
      cases.push_back({tag("only the last bin, at capacity - 1 / capacity / capacity + 1"), s.F, s.cap, lone});
    }
    for (int at : {0, s.bins / 2, s.bins - 1}) {
      std::vector<uint32_t> v(none);
      v[at] = 300007;
      cases.push_back({tag("one bin holds everything"), s.F, s.cap, v});
    }
    {      // whole bins, sliced bins and empty ones side by side
      std::vector<uint32_t> v(s.bins, 0);
      for (int b = 0; b < s.bins; b++) v[b] = (b % 5 == 0) ? 0u : (b % 7 == 0) ? CAP + 1 + 977u * (b % 11) : 100u + 13u * b;
      cases.push_back({tag("mixed"), s.F, s.cap, v});
    }
    for (size_t E : {(size_t)CAP + 1, (size_t)3 * CAP + 5, (size_t)400000, (size_t)(s.bins < 64 ? s.bins : 64) * (CAP + 1) + 3 * s.cap + 17}) {
      const std::vector<uint32_t> v = fullest(E, s.bins, s.cap);
      size_t sum = 0, sl = 0;
      for (uint32_t l : v) { sum += l; sl += fine_bin_slices(l, s.cap); }
      CHECK(sum <= E && sum > CAP && sl == fine_max_slices(E, s.bins, s.cap) && sl == fine_max_slices(sum, s.bins, s.cap), "%s: %zu slices from %zu of %zu records, the bound says %zu / %zu",
            tag("fullest").c_str(), sl, sum, E, fine_max_slices(E, s.bins, s.cap), fine_max_slices(sum, s.bins, s.cap));
      cases.push_back({tag("as many slices as the grid has workgroups"), s.F, s.cap, v});
    }
  }
  // the bound itself: no lengths need more slices than fine_max_slices says (lengths on and around every step of the slice count)
  {
    uint32_t x = 12345;
    for (int t = 0; t < 20000; t++) {
      const auto rnd = [&]() { x = x * 1664525u + 1013904223u; return x >> 8; };
      const size_t bins = 1 + rnd() % 16;
      static const uint32_t caps[] = {1486, 23041, 33792, 33793, 40000, 7};
      const uint32_t cap = caps[rnd() % 6];
      size_t sum = 0, sl = 0;
      for (size_t b = 0; b < bins; b++) {
        const uint32_t kind = rnd() % 4;
        const uint32_t len = kind == 0 ? rnd() % (CAP + 1) : kind == 1 ? CAP + 1 + rnd() % 3 : kind == 2 ? ((CAP / cap) + 1 + rnd() % 4) * cap + rnd() % 3 : CAP + rnd() % 100000;
        sum += len, sl += fine_bin_slices(len, cap);
      }
      CHECK(sl <= fine_max_slices(sum, bins, cap), "bound: %zu slices from %zu records in %zu bins, slices of %u: the bound says %zu", sl, sum, bins, cap, fine_max_slices(sum, bins, cap));
    }
  }
  size_t wgs = 0;
  for (size_t i = 0; i < cases.size(); i++) wgs += run_case(cases[i], (uint32_t)i);
  if (g_fail) { printf("%d checks failed\n", g_fail); return 1; }
  printf("ok %zu %zu\n", cases.size(), wgs);
  return 0;
}
