// The segment walk of k_seg_accumulate (seg_span / seg_first_bucket / seg_walk, myzkp_amd/csrc/mzk_msm_plan.h) run on the host for
// tests/test_hostcheck_seg_walk.py: the same templates the kernel instantiates, over entry and offset arrays allocated at EXACTLY their
// size, so that a look-ahead past either end is an AddressSanitizer report.  For every lane of every case the (entry, bucket) pairs it
// adds and the buckets it flushes must be those of a plain loop without look-ahead, every row request must name a real table row and
// the row buffer must hold the row of the entry that is added.  A stand-alone program: exit status 0 and "ok <cases> <lanes>".
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <utility>
#include <vector>
#include "../../myzkp_amd/csrc/mzk_msm_plan.h"

using namespace mzk;

static int g_fail = 0;
#define CHECK(c, ...) do { if (!(c)) { if (g_fail++ < 20) { printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #c); printf(__VA_ARGS__); printf("\n"); } } } while (0)

constexpr uint32_t TABLE_ROWS = 1000;
typedef std::vector<std::pair<uint32_t, size_t>> Trace;

struct Case {
  const char* name;
  std::vector<uint32_t> counts;      // entries per bucket
  uint32_t sentinels;                // behind the last bucket's real entries, counted into that bucket (k_many_sort1)
  uint32_t seg;
};

// heap arrays of exactly the kernel's sizes: offsets[nbuckets + 1], entries[total]
struct Arrays {
  size_t nbuckets;
  uint32_t total, *offsets, *entries;
  explicit Arrays(const Case& c, uint32_t seed) : nbuckets(c.counts.size()) {
    offsets = (uint32_t*)malloc((nbuckets + 1) * sizeof(uint32_t));
    uint32_t run = 0;
    for (size_t b = 0; b < nbuckets; b++) { offsets[b] = run; run += c.counts[b] + (b + 1 == nbuckets ? c.sentinels : 0); }
    offsets[nbuckets] = total = run;
    entries = (uint32_t*)malloc(total ? total * sizeof(uint32_t) : 1);
    uint32_t x = seed * 2654435761u + 12345u;
    for (uint32_t e = 0; e < total; e++) {
      x = x * 1664525u + 1013904223u;
      entries[e] = e + c.sentinels >= total ? MANY_SENTINEL : ((x >> 8) % TABLE_ROWS) | (x & 0x80000000u);
    }
  }
  ~Arrays() { free(offsets); free(entries); }
  Arrays(const Arrays&) = delete;
};

// what the loop did before it had any look-ahead
static void plain_lane(const Arrays& A, uint32_t e0, uint32_t e1, Trace* adds, std::vector<size_t>* flushes) {
  size_t lo = 0, hi = A.nbuckets;
  while (hi - lo > 1) { const size_t mid = (lo + hi) >> 1; if (A.offsets[mid] <= e0) lo = mid; else hi = mid; }
  size_t b = lo;
  uint32_t bend = A.offsets[b + 1];
  for (uint32_t e = e0; e < e1; e++) {
    if (e >= bend) { flushes->push_back(b); do { b++; bend = A.offsets[b + 1]; } while (e >= bend); }
    adds->push_back({A.entries[e], b});
  }
  flushes->push_back(b);
}

template <bool SENT>
static void walk_lane(const Arrays& A, uint32_t e0, uint32_t e1, Trace* adds, std::vector<size_t>* flushes, const char* name) {
  uint32_t in_row = MANY_SENTINEL, taken = MANY_SENTINEL, expect_e = e0;      // the reference the row buffer was last asked for
  const auto entry_at = [&](uint32_t e) { CHECK(e >= e0 && e < e1, "%s: entry %u outside the segment [%u, %u)", name, e, e0, e1); return A.entries[e]; };
  const auto offset_at = [&](size_t b) { return A.offsets[b]; };
  const size_t b0 = seg_first_bucket(offset_at, A.nbuckets, e0);
  CHECK(A.offsets[b0] <= e0 && e0 < A.offsets[b0 + 1], "%s: first bucket %zu of entry %u", name, b0, e0);
  CHECK(b0 == seg_bucket_search<32>(offset_at, A.nbuckets, e0), "%s: the 32-ary search disagrees at entry %u", name, e0);
  seg_walk<SENT>(
      e0, e1, b0, A.nbuckets, entry_at, offset_at,
      [&](uint32_t ref) {
        CHECK(ref != MANY_SENTINEL && (ref & 0x7fffffffu) < TABLE_ROWS, "%s: row request %08x", name, ref);
        in_row = ref;
      },
      [&](uint32_t ent) {
        if (!(SENT && ent == MANY_SENTINEL)) CHECK(in_row == ent, "%s: the buffer holds %08x, the entry is %08x", name, in_row, ent);
        taken = ent;
      },
      [&](size_t b) { flushes->push_back(b); },
      [&](uint32_t e, uint32_t ent, size_t b) {
        CHECK(e == expect_e && ent == A.entries[e] && taken == ent, "%s: entry %u (expected %u)", name, e, expect_e);
        expect_e = e + 1;
        adds->push_back({ent, b});
      });
  CHECK(expect_e == e1, "%s: the lane stopped at %u, its segment ends at %u", name, expect_e, e1);
}

static size_t run_case(const Case& c, uint32_t seed) {
  const Arrays A(c, seed);
  size_t lanes = 0;
  // lanes past the data too: they must return before they load anything
  for (uint64_t t = 0; t < (uint64_t)A.total / c.seg + 3; t++) {
    uint32_t e0 = 0, e1 = 0;
    const bool has = seg_span(t, c.seg, A.total, &e0, &e1);
    CHECK(has == (t * c.seg < A.total), "%s: lane %llu", c.name, (unsigned long long)t);
    if (!has) continue;
    CHECK(e0 == t * c.seg && e1 > e0 && e1 <= A.total && e1 - e0 <= c.seg && (e1 == A.total || e1 - e0 == c.seg), "%s: span of lane %llu", c.name, (unsigned long long)t);
    Trace want, got;
    std::vector<size_t> want_f, got_f;
    plain_lane(A, e0, e1, &want, &want_f);
    if (c.sentinels) walk_lane<true>(A, e0, e1, &got, &got_f, c.name);
    else walk_lane<false>(A, e0, e1, &got, &got_f, c.name);
    CHECK(want == got, "%s: lane %llu adds differ (%zu against %zu)", c.name, (unsigned long long)t, got.size(), want.size());
    CHECK(want_f == got_f, "%s: lane %llu flushes differ", c.name, (unsigned long long)t);
    lanes++;
  }
  return lanes;
}

int main() {
  std::vector<Case> cases;
  const uint32_t segs[] = {1, 2, 3, 8};
  for (uint32_t seg : segs) {
    // totals 0, 1, seg - 1, seg, seg + 1 and k seg + 1, in one bucket and spread over several
    const uint32_t totals[] = {0, 1, seg - 1, seg, seg + 1, 5 * seg + 1};
    for (uint32_t total : totals) {
      cases.push_back({"one bucket", {total}, 0, seg});
      cases.push_back({"spread", {total / 3, total - total / 3 - total / 4, total / 4}, 0, seg});
      cases.push_back({"spread, empty buckets around", {0, 0, total / 2, 0, 0, 0, total - total / 2, 0, 0}, 0, seg});
    }
    // a bucket boundary on the first entry of a segment (bucket sizes that are multiples of seg) and on the last (one less / one more)
    cases.push_back({"boundary on a segment's first entry", {seg, 2 * seg, seg, 3 * seg}, 0, seg});
    cases.push_back({"boundary on a segment's last entry", {seg - 1 + seg, seg, 1, 2 * seg - 1, 1}, 0, seg});
    cases.push_back({"boundary on first and last", {seg, seg - 1 + seg, 1, seg}, 0, seg});
    cases.push_back({"one entry per bucket", std::vector<uint32_t>(4 * seg + 1, 1), 0, seg});
    cases.push_back({"runs of empty buckets", {0, 0, 0, 1, 0, 0, 0, 0, seg, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 2 * seg + 1, 0, 0, 0}, 0, seg});
    cases.push_back({"many buckets, few entries", [] { std::vector<uint32_t> v(300, 0); v[0] = 1; v[17] = 2; v[255] = 1; v[256] = 3; v[299] = 1; return v; }(), 0, seg});
    // sentinel tails: shorter than, equal to and longer than a segment, a region of nothing but sentinels, a tail that starts a segment
    const uint32_t tails[] = {1, seg, seg + 1, 3 * seg + 2};
    for (uint32_t tail : tails) {
      cases.push_back({"sentinel tail", {seg + 1, 0, 2, seg}, tail, seg});
      cases.push_back({"sentinel tail from a segment's first entry", {seg, seg}, tail, seg});
      cases.push_back({"only sentinels", {0, 0}, tail, seg});
    }
  }
  // more buckets than one level of either search holds, uneven
  {
    std::vector<uint32_t> v(5000);
    uint32_t x = 7;
    for (auto& c : v) { x = x * 1103515245u + 12345u; c = (x >> 16) % 7 == 0 ? 0 : (x >> 20) % 5; }
    cases.push_back({"5000 buckets", v, 0, 8});
    cases.push_back({"5000 buckets", v, 0, 3});
    cases.push_back({"5000 buckets, sentinel tail", v, 11, 8});
  }
  size_t lanes = 0;
  for (size_t i = 0; i < cases.size(); i++) lanes += run_case(cases[i], (uint32_t)i);
  if (g_fail) { printf("%d checks failed\n", g_fail); return 1; }
  printf("ok %zu %zu\n", cases.size(), lanes);
  return 0;
}
