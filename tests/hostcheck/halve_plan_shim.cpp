// The halving steps of the bucket reduction on the host (tests/test_hostcheck_halve_plan.py): the index templates k_halve_multi_row
// runs (myzkp_amd/csrc/mzk_msm_plan.h: halve_multi_wg / _ops / _pair / _live) against the single-step rule halve_indices, and the
// launch list halve_plan makes of a layout.  Stand-alone: g++ -fsanitize=address,undefined, arrays of exactly 2^lgB records.
//   halve_plan_shim                       every check; prints "ok <launches> <splits>"
//   halve_plan_shim list LGB SETS CUS TAIL_MAX ROW      the launch list: "kind t steps grid" per launch, then "tail t_next"
//   halve_plan_shim layout C N CUS        lgB and bucket sets msm_plan gives C-bit window tables (C = 0: arbitrary points) at N pairs
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <stdint.h>
#include <vector>
#include "../../myzkp_amd/csrc/mzk_msm_plan.h"

using namespace mzk;

static int g_fail = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (g_fail < 20) { printf("FAIL: " __VA_ARGS__); printf("\n"); } g_fail++; } } while (0)

static size_t step_ops(int lgB, int t) { return (size_t)(t + 1) << (lgB - t - 1); }
static uint64_t mix(uint64_t& s) {
  uint64_t z = (s += 0x9e3779b97f4a7c15ull);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}

// One launch of steps t0 .. t0 + s - 1 over a set of 2^lgB records:
//  * the workgroups' records lie inside the set and no two workgroups share one;
//  * every step's (lo, hi) pairs are the single-step rule's, each exactly once, and inside a workgroup no addition of a step reads a
//    record that an addition of the same step writes: with the barrier between steps, every read follows the write it depends on;
//  * what a workgroup writes back is exactly what it holds of the records that later steps or the tail's weighted sum read.
struct Scratch { std::vector<int32_t> owner; std::vector<int64_t> want_hi; std::vector<uint8_t> seen, needed; };
static void check_launch(int lgB, int t0, int s, Scratch& S) {
  const size_t B = (size_t)1 << lgB, grid = halve_multi_grid(lgB, t0, s);
  // (the arrays have exactly B entries and are wiped entry by entry behind every use: a launch touches a small part of a large set)
  if (S.owner.size() != B) { S.owner.assign(B, -1); S.want_hi.assign(B, -1); S.seen.assign(B, 0); S.needed.assign(B, 0); }
  for (size_t wg = 0; wg < grid; wg++) {
    const HalveWg g = halve_multi_wg(lgB, t0, s, wg);
    CHECK(g.region >= 0 && g.region <= t0 && g.lgs == lgB - t0 - s, "lgB %d t0 %d s %d wg %zu: region %d lgs %d", lgB, t0, s, wg, g.region, g.lgs);
    for (int k = 0; k < (1 << s); k++) {
      const size_t r = g.base + ((size_t)k << g.lgs);
      CHECK(r < B, "lgB %d t0 %d s %d wg %zu: record %zu outside the set", lgB, t0, s, wg, r);
      if (r >= B) return;
      CHECK(S.owner[r] < 0, "lgB %d t0 %d s %d: record %zu in workgroups %d and %zu", lgB, t0, s, r, S.owner[r], wg);
      S.owner[r] = (int32_t)wg;
    }
  }
  for (int tl = 0; tl < s; tl++) {
    const int t = t0 + tl;
    for (size_t id = 0; id < step_ops(lgB, t); id++) {
      size_t lo, hi;
      halve_indices(lgB, t, id, &lo, &hi);
      CHECK(lo < hi && hi < B && S.want_hi[lo] < 0, "halve_indices(%d, %d, %zu) = (%zu, %zu)", lgB, t, id, lo, hi);
      if (hi >= B) return;
      S.want_hi[lo] = (int64_t)hi;
    }
    size_t ops = 0;
    for (size_t wg = 0; wg < grid; wg++) {
      const HalveWg g = halve_multi_wg(lgB, t0, s, wg);
      const int n = halve_multi_ops(g.region, s, tl);
      uint8_t written[1 << HALVE_MULTI_MAX_S] = {}, read[1 << HALVE_MULTI_MAX_S] = {};
      for (int id = 0; id < n; id++) {
        int lo = -1, hi = -1;
        halve_multi_pair(s, tl, id, &lo, &hi);
        CHECK(lo >= 0 && lo < hi && hi < (1 << s), "lgB %d t0 %d s %d step %d op %d: local (%d, %d)", lgB, t0, s, tl, id, lo, hi);
        if (lo < 0 || hi >= (1 << s)) return;
        written[lo]++, read[hi]++;
        const size_t glo = g.base + ((size_t)lo << g.lgs), ghi = g.base + ((size_t)hi << g.lgs);
        CHECK(S.want_hi[glo] == (int64_t)ghi && !S.seen[glo], "lgB %d t0 %d s %d step %d wg %zu op %d: (%zu, %zu) is not the step's, or twice", lgB, t0, s, tl, wg,
              id, glo, ghi);
        S.seen[glo] = 1, ops++;
      }
      for (int k = 0; k < (1 << s); k++)
        CHECK(written[k] <= 1 && !(written[k] && read[k]), "lgB %d t0 %d s %d step %d wg %zu: local %d written %d read %d", lgB, t0, s, tl, wg, k, written[k], read[k]);
    }
    CHECK(ops == step_ops(lgB, t), "lgB %d t0 %d s %d step %d: %zu additions, the step has %zu", lgB, t0, s, tl, ops, step_ops(lgB, t));
    for (size_t id = 0; id < step_ops(lgB, t); id++) {
      size_t lo, hi;
      halve_indices(lgB, t, id, &lo, &hi);
      S.want_hi[lo] = -1, S.seen[lo] = 0;
    }
  }
  for (int t = t0 + s; t < lgB; t++)
    for (size_t id = 0; id < step_ops(lgB, t); id++) {
      size_t lo, hi;
      halve_indices(lgB, t, id, &lo, &hi);
      S.needed[lo] = S.needed[hi] = 1;
    }
  S.needed[0] = 1;
  for (int q = 0; q < lgB; q++) S.needed[(size_t)1 << q] = 1;      // the tail: buf[0] + sum_q 2^q buf[2^q]
  for (size_t wg = 0; wg < grid; wg++) {
    const HalveWg g = halve_multi_wg(lgB, t0, s, wg);
    for (int e = 0; e < halve_multi_live(g.region, s); e++) {
      const int k = halve_multi_live_at(e);
      CHECK(k >= 0 && k < (1 << s), "live record %d of region %d: local %d", e, g.region, k);
      if (k < 0 || k >= (1 << s)) return;
      const size_t r = g.base + ((size_t)k << g.lgs);
      CHECK(S.needed[r] && !S.seen[r], "lgB %d t0 %d s %d wg %zu: writes back record %zu, which nothing reads (or twice)", lgB, t0, s, wg, r);
      S.seen[r] = 1;
    }
  }
  for (size_t wg = 0; wg < grid; wg++) {
    const HalveWg g = halve_multi_wg(lgB, t0, s, wg);
    for (int k = 0; k < (1 << s); k++) {
      const size_t r = g.base + ((size_t)k << g.lgs);
      CHECK(!S.needed[r] || S.seen[r], "lgB %d t0 %d s %d: record %zu of workgroup %zu is read later and not written back", lgB, t0, s, r, wg);
      S.owner[r] = -1, S.seen[r] = 0;
    }
  }
  for (int t = t0 + s; t < lgB; t++)
    for (size_t id = 0; id < step_ops(lgB, t); id++) {
      size_t lo, hi;
      halve_indices(lgB, t, id, &lo, &hi);
      S.needed[lo] = S.needed[hi] = 0;
    }
  S.needed[0] = 0;
  for (int q = 0; q < lgB; q++) S.needed[(size_t)1 << q] = 0;
}

// A whole split on values: steps 0 .. t_begin - 1 by the single-step rule, then launches of parts[0], parts[1], ... steps as the
// kernel runs them -- a local copy per workgroup, the steps on it, the live records back, everything else left stale -- against the
// single-step rule all the way, at the records the tail reads.  Addition is + mod 2^64 on random values.
static void run_launch(std::vector<uint64_t>& buf, int lgB, int t0, int s) {
  const size_t grid = halve_multi_grid(lgB, t0, s);
  std::vector<uint64_t> local((size_t)1 << s);        // exactly the kernel's records: the sanitizer sees an index past them
  for (size_t wg = 0; wg < grid; wg++) {
    const HalveWg g = halve_multi_wg(lgB, t0, s, wg);
    for (int k = 0; k < (1 << s); k++) local[k] = buf[g.base + ((size_t)k << g.lgs)];
    for (int tl = 0; tl < s; tl++)
      for (int id = 0; id < halve_multi_ops(g.region, s, tl); id++) {
        int lo, hi;
        halve_multi_pair(s, tl, id, &lo, &hi);
        local[lo] += local[hi];
      }
    for (int e = 0; e < halve_multi_live(g.region, s); e++) {
      const int k = halve_multi_live_at(e);
      buf[g.base + ((size_t)k << g.lgs)] = local[k];
    }
  }
}
static size_t check_splits(int lgB, int max_part) {
  const size_t B = (size_t)1 << lgB;
  uint64_t seed = 0x5eed0000ull + (uint64_t)lgB;
  std::vector<uint64_t> ref(B);
  for (auto& v : ref) v = mix(seed);
  std::vector<std::vector<uint64_t>> at(lgB + 1);      // the set after t single steps, kept for the last 2 max_part steps
  const int first = lgB > 2 * max_part ? lgB - 2 * max_part : 0;
  for (int t = 0; t < lgB; t++) {
    if (t >= first) at[t] = ref;
    for (size_t id = 0; id < step_ops(lgB, t); id++) {
      size_t lo, hi;
      halve_indices(lgB, t, id, &lo, &hi);
      ref[lo] += ref[hi];
    }
  }
  size_t splits = 0;
  for (int t_begin = first; t_begin < lgB; t_begin++) {
    const int left = lgB - t_begin;
    std::vector<uint64_t> buf;
    // every composition of `left` into parts of 1 .. max_part: the bits of `cut` say where a launch ends
    for (uint32_t cut = 0; cut < (1u << (left - 1)); cut++) {
      int parts[32], np = 0, len = 1;
      bool ok = true;
      for (int i = 0; i < left - 1; i++) {
        if (cut >> i & 1) { parts[np++] = len; ok = ok && len <= max_part; len = 1; } else len++;
      }
      parts[np++] = len;
      if (!ok || len > max_part) continue;
      // only the live records differ between splits (region a: its first 2^(lgB - t_begin) records): put those back, not the whole set
      if (buf.empty()) buf = at[t_begin];
      for (int a = 0; a <= t_begin; a++) {
        const size_t start = a ? (size_t)1 << (lgB - a) : 0;
        for (size_t j = 0; j < ((size_t)1 << left); j++) buf[start + j] = at[t_begin][start + j];
      }
      int t = t_begin;
      for (int i = 0; i < np; i++) { run_launch(buf, lgB, t, parts[i]); t += parts[i]; }
      bool same = buf[0] == ref[0];
      for (int q = 0; q < lgB; q++) same = same && buf[(size_t)1 << q] == ref[(size_t)1 << q];
      CHECK(same, "lgB %d from step %d, split %#x: the tail's records differ from the single-step rule's", lgB, t_begin, cut);
      splits++;
    }
  }
  return splits;
}

static void print_list(const HalvePlan& H) {
  for (int i = 0; i < H.count; i++) printf("%d %d %d %zu\n", H.l[i].kind, H.l[i].t, H.l[i].steps, H.l[i].grid);
  printf("tail %d\n", H.t_next);
}
// what every list must satisfy, whatever the layout
static void check_list(int lgB, int sets, int cus, size_t tail_max, int row) {
  const HalvePlan H = halve_plan(lgB, sets, cus, tail_max, row);
  int t = 0;
  bool multi = false;
  for (int i = 0; i < H.count; i++) {
    const HalveLaunch& l = H.l[i];
    CHECK(l.t == t && l.steps >= 1 && t + l.steps <= lgB, "lgB %d sets %d cus %d: launch %d starts at %d, expected %d", lgB, sets, cus, i, l.t, t);
    if (l.kind == HALVE_STEP_WIDE) CHECK(l.steps == 1 && l.grid == (step_ops(lgB, t) + 127) / 128, "wide step grid");
    if (l.kind == HALVE_STEP_QUAD) CHECK(l.steps == 1 && l.grid == (4 * step_ops(lgB, t) + 127) / 128, "quad step grid");
    if (l.kind == HALVE_MULTI_QUAD || l.kind == HALVE_MULTI_ROW)
      CHECK(l.grid == halve_multi_grid(lgB, t, l.steps) && l.grid * (size_t)sets <= (size_t)cus, "lgB %d sets %d cus %d: multi launch %d grid %zu", lgB, sets, cus, i, l.grid);
    if (l.kind == HALVE_MULTI_QUAD) CHECK(l.steps <= HALVE_MULTI_MAX_S, "quad launch of %d steps", l.steps);
    if (l.kind == HALVE_MULTI_ROW) CHECK(row && multi && l.steps <= HALVE_ROW_MAX_S && lgB - l.t <= 2 * HALVE_ROW_MAX_S, "lgB %d sets %d: row launch at %d, %d steps", lgB, sets, l.t, l.steps);
    multi = multi || l.kind == HALVE_MULTI_QUAD;
    t += l.steps;
  }
  CHECK(H.t_next == t && t <= lgB && (t == lgB || step_ops(lgB, t) <= tail_max), "lgB %d sets %d cus %d: the tail starts at %d", lgB, sets, cus, H.t_next);
  if (!row) return;
  // the switch changes nothing but the kind and the cut of the last launches
  const HalvePlan Q = halve_plan(lgB, sets, cus, tail_max, 0);
  int i = 0;
  while (i < H.count && H.l[i].kind != HALVE_MULTI_ROW) {
    CHECK(i < Q.count && Q.l[i].kind == H.l[i].kind && Q.l[i].t == H.l[i].t && Q.l[i].steps == H.l[i].steps && Q.l[i].grid == H.l[i].grid, "lgB %d sets %d: launch %d differs without the row form", lgB, sets, i);
    i++;
  }
  if (i < H.count) {
    CHECK(Q.count == i + 1 && Q.l[i].kind == HALVE_MULTI_QUAD && Q.l[i].t == H.l[i].t && Q.l[i].steps == lgB - H.l[i].t && Q.t_next == lgB && H.t_next == lgB &&
              H.count - i == (lgB - H.l[i].t + HALVE_ROW_MAX_S - 1) / HALVE_ROW_MAX_S,
          "lgB %d sets %d cus %d: the row launches do not replace ONE quad launch of the rest", lgB, sets, cus);
  } else {
    CHECK(Q.count == H.count && Q.t_next == H.t_next, "lgB %d sets %d: lists differ", lgB, sets);
  }
}

int main(int argc, char** argv) {
  if (argc == 7 && !strcmp(argv[1], "list")) {
    print_list(halve_plan(atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), (size_t)atoll(argv[5]), atoi(argv[6])));
    return 0;
  }
  if (argc == 5 && !strcmp(argv[1], "layout")) {
    const int c = atoi(argv[2]);
    const size_t n = (size_t)atoll(argv[3]);
    const MsmPlan P = msm_plan(n, n, n, c ? (MSM_PTS_TABLES | (c << 8) | (1 << 16)) : MSM_PTS_MONT, n, atoi(argv[4]), 0, MsmKnobs());
    printf("err %d lgB %d sets %d halve_row %d\n", P.err, P.lgB, P.red_windows, MsmKnobs().halve_row);
    return 0;
  }
  Scratch S;
  size_t launches = 0, splits = 0;
  for (int lgB = 4; lgB <= 20; lgB++) {
    // every launch a list can hold: up to eight steps (the quad form's records), at most 1024 workgroups (four times the CUs of any part)
    for (int t0 = 0; t0 < lgB; t0++)
      for (int s = 1; s <= HALVE_MULTI_MAX_S && t0 + s <= lgB; s++) {
        if (halve_multi_grid(lgB, t0, s) > 1024) continue;
        check_launch(lgB, t0, s, S);
        launches++;
      }
    splits += check_splits(lgB, HALVE_ROW_MAX_S);
    if (lgB <= 10) splits += check_splits(lgB, HALVE_MULTI_MAX_S);
    for (int sets : {1, 2, 4, 8, 16, 32})
      for (int cus : {64, 256, 304})
        for (size_t tail_max : {(size_t)1, (size_t)64, (size_t)256})
          for (int row : {0, 1}) check_list(lgB, sets, cus, tail_max, row);
  }
  if (g_fail) { printf("%d checks failed\n", g_fail); return 1; }
  printf("ok %zu %zu\n", launches, splits);
  return 0;
}
