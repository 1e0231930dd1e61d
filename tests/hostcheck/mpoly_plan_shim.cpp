// The host decisions of mzk_mpoly_compose* (myzkp_amd/csrc/mzk_mpoly_plan.h: mp_plan, mp_compile), tests/test_hostcheck_mpoly_plan.py.
// Stand-alone: g++ -fsanitize=address,undefined.  Every compiled term program is interpreted the way k_mp_terms runs it -- the tables
// x, x^2, x^3 per variable in `slots` slots, LOADC / ADDC / MULT / HORNER / POW (square-and-multiply from the top bit down), the flush
// bit -- in 64-bit arithmetic modulo 2^31 - 1 and compared with the naive sum over the terms at random x (an empty point polynomial
// is x = 0 with 0^0 = 1), and the structure the kernel relies on is checked op by op.  Every plan is compared with a restatement in
// 128-bit integers.
//   mpoly_plan_shim                                  every check; prints "ok <exhaustive> <random> <plans> ratio <largest ops / terms>"
//   mpoly_plan_shim plan MAXLOG NV NT LEN.. EXP..    one constraint of NT terms: "err n stride_min bound"
//   mpoly_plan_shim prog NV NT LEN.. EXP..           its program: "slots depth.. | op.slot.arg[!] .." (! = flush)
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <stdint.h>
#include <vector>
#include "../../myzkp_amd/csrc/mzk_mpoly_plan.h"

using namespace mzk;

static int g_fail = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (g_fail < 20) { printf("FAIL: " __VA_ARGS__); printf("\n"); } g_fail++; } } while (0)
// a failed check on an address: a slot, a coefficient index, the LDS bound.  Counted apart: such a program must not run on a device.
static int g_fail_address = 0;
#define CHECK_ADDRESS(cond, ...) do { if (!(cond)) g_fail_address++; CHECK(cond, __VA_ARGS__); } while (0)

static const uint64_t Q = 2147483647u;      // 2^31 - 1
static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() { g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17; return g_rng; }
static uint64_t rnd_below(uint64_t n) { return rnd() % n; }
static uint64_t powmod(uint64_t x, uint64_t e) {
  uint64_t r = 1;
  for (x %= Q; e; e >>= 1, x = x * x % Q) if (e & 1) r = r * x % Q;
  return r;
}

struct Call {
  size_t nv = 0;
  std::vector<size_t> toff, poff;          // nc + 1, nv + 1
  std::vector<uint32_t> exps;              // term_offsets.back() rows of nv (the rows in front of toff[0] are filler)
  size_t nc() const { return toff.size() - 1; }
  bool empty_var(size_t i) const { return poff[i + 1] == poff[i]; }
  bool vanishes(size_t t) const {
    for (size_t i = 0; i < nv; i++) if (exps[t * nv + i] && empty_var(i)) return true;
    return false;
  }
};

static double g_ratio = 0;

// structure and value of every constraint's program; returns the number of constraints checked
static size_t check_programs(const Call& C, const char* what) {
  const size_t nc = C.nc(), nv = C.nv, t0 = C.toff[0], nt = C.toff[nc] - t0;
  static MpProgram pg;                       // the buffers of this function are kept between calls: millions of them
  static std::vector<int> owner, power, used;
  static std::vector<uint64_t> x, tab, coef;
  pg.ops.clear();
  owner.clear();
  power.clear();
  mp_compile(C.exps.data(), C.toff.data(), nc, nv, C.poff.data(), &pg);
  // the variables' slots: depth = min(largest exponent of the call, MP_TABLE), back to back, inside the LDS of the widest field
  uint32_t next = 0;
  for (size_t i = 0; i < (size_t)MP_MAX_VARS; i++) {
    uint32_t maxe = 0;
    if (i < nv) for (size_t t = t0; t < t0 + nt; t++) maxe = std::max(maxe, C.exps[t * nv + i]);
    const uint32_t depth = maxe > (uint32_t)MP_TABLE ? (uint32_t)MP_TABLE : maxe;
    CHECK_ADDRESS(pg.vars.depth[i] == depth && pg.vars.first_slot[i] == next, "%s: variable %zu depth %u first slot %u, expected %u %u", what, i, pg.vars.depth[i],
          pg.vars.first_slot[i], depth, next);
    for (uint32_t d = 0; d < pg.vars.depth[i] && d < (uint32_t)MP_TABLE; d++) { owner.push_back((int)i); power.push_back((int)d + 1); }
    next += depth;
  }
  CHECK_ADDRESS(pg.slots == next && pg.slots == owner.size(), "%s: %u slots, expected %u", what, pg.slots, next);
  CHECK_ADDRESS((size_t)pg.slots * MP_MAX_LIMBS * MP_LANES * 4 <= 65536, "%s: %u slots are above 64 KiB of LDS", what, pg.slots);
  CHECK(pg.off.size() == nc + 1 && pg.off[0] == 0 && pg.off.back() == pg.ops.size(), "%s: offsets %zu, last %u, ops %zu", what, pg.off.size(),
        pg.off.empty() ? 0u : pg.off.back(), pg.ops.size());
  if (pg.off.size() != nc + 1 || pg.slots != owner.size()) return 0;
  // the tables as k_mp_terms fills them, and the coefficients
  x.assign(nv, 0);
  tab.assign(pg.slots, 0);
  coef.assign(nt, 0);
  for (size_t i = 0; i < nv; i++) x[i] = C.empty_var(i) ? 0 : 1 + rnd_below(Q - 1);
  for (size_t s = 0; s < tab.size(); s++) tab[s] = powmod(x[owner[s]], (uint64_t)power[s]);
  for (size_t t = 0; t < nt; t++) coef[t] = 1 + rnd_below(Q - 1);
  used.assign(nt, 0);
  size_t live_total = 0;
  for (size_t a = 0; a < nc; a++) {
    CHECK(pg.off[a] <= pg.off[a + 1] && pg.off[a + 1] <= pg.ops.size(), "%s: constraint %zu: offsets %u %u of %zu ops", what, a, pg.off[a], pg.off[a + 1], pg.ops.size());
    if (pg.off[a] > pg.off[a + 1] || pg.off[a + 1] > pg.ops.size()) return 0;
    size_t live = 0;
    uint64_t want = 0;
    for (size_t t = C.toff[a]; t < C.toff[a + 1]; t++) {
      if (!C.vanishes(t)) live++;
      uint64_t m = coef[t - t0];
      for (size_t i = 0; i < nv; i++) m = m * powmod(x[i], C.exps[t * nv + i]) % Q;
      want = (want + m) % Q;
    }
    live_total += live;
    if (live == 0) CHECK(pg.off[a] == pg.off[a + 1], "%s: constraint %zu has no term left and %u ops", what, a, pg.off[a + 1] - pg.off[a]);
    uint64_t acc = 0, sum = 0;
    bool run_open = false;      // between a LOADC and the flush that ends its run
    bool ok = true;
    for (uint32_t pc = pg.off[a]; pc < pg.off[a + 1] && ok; pc++) {
      const uint32_t w = pg.ops[pc].op, arg = pg.ops[pc].arg, op = w & 0xffu, slot = (w >> 8) & 0xffffu;
      CHECK((w & ~(MP_FLUSH | 0xffffffu)) == 0, "%s: op word %08x has bits the kernel does not read", what, w);
      CHECK((op == MP_LOADC) == !run_open, "%s: constraint %zu pc %u: op %u %s", what, a, pc, op, run_open ? "inside a run" : "where a run must begin");
      run_open = true;
      if (op == MP_LOADC || op == MP_ADDC || op == MP_HORNER) {
        CHECK_ADDRESS(arg < nt, "%s: coefficient index %u of %zu", what, arg, nt);
        if (arg >= nt) { ok = false; break; }
        used[arg]++;
        CHECK(arg + t0 >= C.toff[a] && arg + t0 < C.toff[a + 1] && !C.vanishes(arg + t0), "%s: constraint %zu reads the coefficient of term %zu", what, a, arg + t0);
      }
      if (op == MP_MULT || op == MP_HORNER || op == MP_POW) {
        CHECK_ADDRESS(slot < pg.slots, "%s: slot %u of %u", what, slot, pg.slots);
        if (slot >= pg.slots) { ok = false; break; }
      } else CHECK(slot == 0, "%s: slot %u on op %u", what, slot, op);
      if (op == MP_LOADC) acc = coef[arg];
      else if (op == MP_ADDC) acc = (acc + coef[arg]) % Q;
      else if (op == MP_MULT) { CHECK(arg == 0, "%s: MULT with arg %u", what, arg); acc = acc * tab[slot] % Q; }
      else if (op == MP_HORNER) acc = (acc * tab[slot] + coef[arg]) % Q;
      else if (op == MP_POW) {
        CHECK_ADDRESS(arg > 2u * MP_TABLE && power[slot] == 1, "%s: POW %u on slot %u (power %d of variable %d)", what, arg, slot, power[slot], owner[slot]);
        if (arg < 2) { ok = false; break; }
        uint64_t y = tab[slot];
        for (int bit = 30 - __builtin_clz(arg); bit >= 0; bit--) {
          y = y * y % Q;
          if ((arg >> bit) & 1u) y = y * tab[slot] % Q;
        }
        acc = acc * y % Q;
      } else { CHECK(false, "%s: op %u", what, op); ok = false; break; }
      if (w & MP_FLUSH) { sum = (sum + acc) % Q; run_open = false; }
    }
    CHECK(!run_open, "%s: constraint %zu: the last run is not flushed", what, a);
    if (ok) CHECK(sum == want, "%s: constraint %zu of %zu (%zu variables, %zu terms): program %llu, naive sum %llu", what, a, nc, nv, C.toff[a + 1] - C.toff[a],
                  (unsigned long long)sum, (unsigned long long)want);
  }
  for (size_t t = 0; t < nt; t++) CHECK(used[t] == (C.vanishes(t + t0) ? 0 : 1), "%s: the coefficient of term %zu is read %d times", what, t + t0, used[t]);
  if (live_total) g_ratio = std::max(g_ratio, (double)pg.ops.size() / (double)live_total);
  return nc;
}

// ---- the plan, restated ----------------------------------------------------------------------------------------------------------------
typedef unsigned __int128 u128;
struct RefPlan { int err; size_t n, smin; std::vector<size_t> bounds; };
static RefPlan ref_plan(unsigned max_log, const Call& C) {
  RefPlan R = {MZK_OK, 0, 0, {}};
  const size_t nc = C.nc();
  if (C.nv > (size_t)MZK_MPOLY_MAX_VARS) { R.err = MZK_E_ARG; return R; }
  if (nc == 0) return R;
  u128 smin = 0;
  for (size_t a = 0; a < nc; a++) {
    u128 b = 0;
    for (size_t t = C.toff[a]; t < C.toff[a + 1]; t++) {
      if (C.vanishes(t)) continue;
      u128 d = 1;
      for (size_t i = 0; i < C.nv; i++) if (C.exps[t * C.nv + i]) d += (u128)C.exps[t * C.nv + i] * (C.poff[i + 1] - C.poff[i] - 1);
      if (d > b) b = d;
    }
    if (b > (u128)SIZE_MAX) { R.err = MZK_E_LENGTH; return R; }        // D + 1 does not fit 64 bits
    R.bounds.push_back((size_t)b);
    if (b > smin) smin = b;
  }
  u128 n = 1;
  unsigned lg = 0;
  while (n < smin) { n <<= 1; lg++; }
  if (lg > max_log) { R.err = MZK_E_LENGTH; return R; }
  R.n = (size_t)n;
  R.smin = (size_t)smin;
  return R;
}
static void check_plan(unsigned max_log, const Call& C, const char* what) {
  MpPlan pl;
  const int rc = mp_plan(max_log, C.exps.data(), C.toff.data(), C.nc(), C.nv, C.poff.data(), &pl);
  const RefPlan R = ref_plan(max_log, C);
  CHECK(rc == R.err, "%s: plan returns %d (%s), expected %d", what, rc, pl.msg, R.err);
  CHECK((rc != MZK_OK) == (pl.msg[0] != 0) && strlen(pl.msg) < sizeof pl.msg - 1, "%s: plan returns %d with the message '%s'", what, rc, pl.msg);
  if (rc != MZK_OK || R.err != MZK_OK || C.nc() == 0) return;
  CHECK(pl.n == R.n && pl.stride_min == R.smin && pl.bounds == R.bounds, "%s: plan n %zu stride_min %zu, expected %zu %zu (or the bounds differ)", what, pl.n,
        pl.stride_min, R.n, R.smin);
  CHECK(pl.n >= 1 && (pl.n & (pl.n - 1)) == 0 && pl.n >= pl.stride_min && (pl.n == 1 || pl.n / 2 < pl.stride_min), "%s: n %zu for stride_min %zu", what, pl.n, pl.stride_min);
}

// ---- enumeration -------------------------------------------------------------------------------------------------------------------------
static const uint32_t ALPHABET[10] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 13};

// every constraint of 1 .. max_terms terms over nv variables with exponents of the alphabet, alone and in front of a fixed constraint
// that takes every depth to 3 and has the last variable as its Horner variable
static size_t exhaustive(size_t nv, size_t max_terms) {
  size_t monos = 1, count = 0;
  for (size_t i = 0; i < nv; i++) monos *= 10;
  std::vector<uint32_t> fixed;
  for (uint32_t last : {5u, 2u}) { for (size_t i = 0; i + 1 < nv; i++) fixed.push_back(3); fixed.push_back(last); }
  for (size_t i = 0; i < nv; i++) fixed.push_back(i == 0 && nv > 1 ? 1 : 0);
  Call alone, both;
  alone.nv = both.nv = nv;
  alone.poff.resize(nv + 1);
  for (size_t i = 0; i <= nv; i++) alone.poff[i] = 2 * i;
  both.poff = alone.poff;
  for (size_t nt = 1; nt <= max_terms; nt++) {
    size_t total = 1;
    for (size_t k = 0; k < nt; k++) total *= monos;
    alone.toff = {0, nt};
    both.toff = {0, nt, nt + 3};
    alone.exps.assign(nt * nv, 0);
    for (size_t code = 0; code < total; code++) {
      size_t c = code;
      for (size_t k = 0; k < nt * nv; k++) { alone.exps[k] = ALPHABET[c % 10]; c /= 10; }
      count += check_programs(alone, "exhaustive, alone");
      both.exps = alone.exps;
      both.exps.insert(both.exps.end(), fixed.begin(), fixed.end());
      count += check_programs(both, "exhaustive, beside the fixed constraint") / 2;
      if ((code & 1023) == 0) { check_plan(32, alone, "exhaustive"); check_plan(28, both, "exhaustive"); }
    }
  }
  return count;
}

static uint32_t random_exponent(int mode) {
  const uint64_t r = rnd_below(100);
  if (mode == 0) return r < 45 ? 0 : ALPHABET[rnd_below(10)];
  if (mode == 1) return r < 60 ? 0 : (uint32_t)rnd_below(4);                          // table depths 0 .. 3 only
  if (r < 50) return 0;
  if (r < 80) return ALPHABET[rnd_below(10)];
  if (r < 90) return (uint32_t)(rnd() >> (32 + rnd_below(32)));                       // any width up to 32 bits
  static const uint32_t EDGE[8] = {0xffffffffu, 0x80000000u, 0x7fffffffu, 0xfffffffeu, 9, 64, 65, 100};
  return EDGE[rnd_below(8)];
}
static size_t random_length(bool wide) {
  const uint64_t r = rnd_below(100);
  if (r < 10) return 0;
  if (!wide || r < 70) return 1 + rnd_below(40);
  const size_t p2 = (size_t)1 << rnd_below(64);
  return r < 80 ? p2 : r < 90 ? p2 + 1 : p2 - 1 + (p2 == 1);
}
// returns constraints checked; *plans counts the plans compared
static size_t random_call(size_t* plans) {
  Call C;
  C.nv = rnd_below(9);
  const size_t nc = 1 + rnd_below(4), front = rnd_below(4) == 0 ? rnd_below(5) : 0;
  const int mode = (int)rnd_below(3);
  const bool wide = rnd_below(4) == 0;
  C.poff.assign(1, rnd_below(3) == 0 ? rnd_below(1000) : 0);
  for (size_t i = 0; i < C.nv; i++) C.poff.push_back(C.poff.back() + random_length(wide) % ((size_t)1 << 60));
  C.toff.assign(1, front);
  for (size_t a = 0; a < nc; a++) C.toff.push_back(C.toff.back() + (rnd_below(8) == 0 ? rnd_below(41) : rnd_below(8)));
  const size_t rows = C.toff.back();
  C.exps.resize(rows * C.nv + 1);           // + 1: data() of an empty vector may be null, which the plan refuses by design
  for (size_t t = 0; t < rows; t++) {
    if (t > front && rnd_below(100) < 15) {                                             // a duplicate of an earlier row of the call
      const size_t src = front + rnd_below(t - front);
      for (size_t i = 0; i < C.nv; i++) C.exps[t * C.nv + i] = C.exps[src * C.nv + i];
    } else if (t > front && rnd_below(100) < 40) {                                      // an earlier row with another power of one variable: a run
      const size_t src = front + rnd_below(t - front);
      for (size_t i = 0; i < C.nv; i++) C.exps[t * C.nv + i] = C.exps[src * C.nv + i];
      if (C.nv) C.exps[t * C.nv + rnd_below(C.nv)] = random_exponent(mode);
    } else
      for (size_t i = 0; i < C.nv; i++) C.exps[t * C.nv + i] = random_exponent(mode);
  }
  check_plan(28, C, "random");
  check_plan(32, C, "random");
  *plans += 2;
  return check_programs(C, "random");
}

static Call one_term(size_t nv, const size_t* lens, const uint32_t* exps) {
  Call C;
  C.nv = nv;
  C.toff = {0, 1};
  C.poff.assign(1, 0);
  for (size_t i = 0; i < nv; i++) C.poff.push_back(C.poff.back() + lens[i]);
  C.exps.assign(exps, exps + nv);
  return C;
}
static int plan_rc(unsigned max_log, const Call& C, MpPlan* pl) { return mp_plan(max_log, C.exps.data(), C.toff.data(), C.nc(), C.nv, C.poff.data(), pl); }

static size_t plan_edges() {
  size_t count = 0;
  // the refusal one step past the field's largest transform, by the length and by the exponent
  for (unsigned max_log : {28u, 32u}) {
    const size_t top = (size_t)1 << max_log;
    for (int by_exponent = 0; by_exponent < 2; by_exponent++)
      for (size_t smin : {top - 1, top, top + 1}) {
        const size_t lens[1] = {by_exponent ? 2 : smin};
        const uint32_t exps[1] = {by_exponent ? (uint32_t)(smin - 1) : 1u};
        if (by_exponent && smin - 1 > 0xffffffffu) continue;
        const Call C = one_term(1, lens, exps);
        MpPlan pl;
        const int rc = plan_rc(max_log, C, &pl);
        if (smin <= top) CHECK(rc == MZK_OK && pl.stride_min == smin && pl.n == top, "max_log %u stride_min %zu: rc %d n %zu", max_log, smin, rc, pl.n);
        else CHECK(rc == MZK_E_LENGTH && strstr(pl.msg, "needs a transform of 2^"), "max_log %u stride_min %zu: rc %d '%s'", max_log, smin, rc, pl.msg);
        check_plan(max_log, C, "edge of the field");
        count++;
      }
  }
  // products and sums that leave 64 bits: refused, no wrap-around
  {
    const size_t big = (size_t)1 << 60;
    const size_t lens[3][2] = {{big, 2}, {((size_t)1 << 33) + 2, ((size_t)1 << 33) + 2}, {((size_t)1 << 32) + 2, 2}};
    const uint32_t exps[3][2] = {{0xffffffffu, 1}, {0x80000000u, 0x80000000u}, {0xffffffffu, 0xffffffffu}};
    for (int k = 0; k < 3; k++) {
      const Call C = one_term(2, lens[k], exps[k]);
      MpPlan pl;
      CHECK(plan_rc(32, C, &pl) == MZK_E_LENGTH && strstr(pl.msg, "overflows 64 bits"), "overflow case %d: '%s'", k, pl.msg);
      check_plan(32, C, "overflow");
      count++;
    }
    // D + 1 = 2^64 exactly: (2^32 - 1) (2^32 + 1) = 2^64 - 1
    const size_t l1[1] = {((size_t)1 << 32) + 2};
    const uint32_t e1[1] = {0xffffffffu};
    const Call C = one_term(1, l1, e1);
    MpPlan pl;
    CHECK(plan_rc(32, C, &pl) == MZK_E_LENGTH && strstr(pl.msg, "overflows 64 bits"), "D = 2^64 - 1: '%s'", pl.msg);
    check_plan(32, C, "D = 2^64 - 1");
    // a term that vanishes has no degree: an empty polynomial behind a product that would overflow
    const size_t l2[2] = {big, 0};
    const uint32_t e2[2] = {0xffffffffu, 1};
    const Call V = one_term(2, l2, e2);
    MpPlan pv;
    CHECK(plan_rc(32, V, &pv) == MZK_OK && pv.stride_min == 0 && pv.n == 1 && pv.bounds == std::vector<size_t>(1, 0), "vanishing term with a huge factor: '%s'", pv.msg);
    check_plan(32, V, "vanishing overflow");
    count += 2;
  }
  // everything vanishes: stride_min 0, N 1, no ops
  {
    Call C;
    C.nv = 2;
    C.toff = {0, 2, 2, 3};
    C.poff = {0, 0, 5};
    C.exps = {1, 0, 3, 2, 13, 1};
    MpPlan pl;
    CHECK(plan_rc(28, C, &pl) == MZK_OK && pl.stride_min == 0 && pl.n == 1, "all terms vanish: stride_min %zu n %zu", pl.stride_min, pl.n);
    check_plan(28, C, "all vanish");
    check_programs(C, "all vanish");
    count++;
  }
  // refusals that come before the sizes
  {
    Call C;
    C.nv = 9;
    C.toff = {0, 1};
    C.poff.assign(10, 0);
    C.exps.assign(9, 0);
    MpPlan pl;
    CHECK(plan_rc(32, C, &pl) == MZK_E_ARG && !strcmp(pl.msg, "mpoly_compose: 9 variables (at most 8)"), "nine variables: '%s'", pl.msg);
    C.nv = 1;
    C.toff = {2, 1};
    C.poff = {0, 1};
    MpPlan p2;
    CHECK(plan_rc(32, C, &p2) == MZK_E_LENGTH && !strcmp(p2.msg, "mpoly_compose: term_offsets[1] = 1 is below term_offsets[0] = 2"), "'%s'", p2.msg);
    C.toff = {0, 1};
    C.poff = {3, 1};
    MpPlan p3;
    CHECK(plan_rc(32, C, &p3) == MZK_E_LENGTH && !strcmp(p3.msg, "mpoly_compose: point_offsets[1] = 1 is below point_offsets[0] = 3"), "'%s'", p3.msg);
    MpPlan p4;
    CHECK(mp_plan(32, nullptr, C.toff.data(), 1, 1, nullptr, &p4) == MZK_E_ARG && !strcmp(p4.msg, "mpoly_compose: null pointer"), "'%s'", p4.msg);
    MpPlan p5;
    CHECK(mp_plan(32, nullptr, nullptr, 0, 1, nullptr, &p5) == MZK_OK && p5.n == 0 && p5.stride_min == 0, "no constraints");
    count += 5;
  }
  return count;
}

static Call call_of_args(int argc, char** argv, int at) {
  Call C;
  C.nv = (size_t)atoll(argv[at]);
  const size_t nt = (size_t)atoll(argv[at + 1]);
  if ((size_t)argc != (size_t)at + 2 + C.nv + nt * C.nv) { fprintf(stderr, "expected %zu lengths and %zu exponents\n", C.nv, nt * C.nv); exit(2); }
  C.toff = {0, nt};
  C.poff.assign(1, 0);
  for (size_t i = 0; i < C.nv; i++) C.poff.push_back(C.poff.back() + (size_t)strtoull(argv[at + 2 + i], nullptr, 10));
  for (size_t k = 0; k < nt * C.nv; k++) C.exps.push_back((uint32_t)strtoull(argv[at + 2 + C.nv + k], nullptr, 10));
  C.exps.push_back(0);
  return C;
}

int main(int argc, char** argv) {
  if (argc >= 5 && !strcmp(argv[1], "plan")) {
    const Call C = call_of_args(argc, argv, 3);
    MpPlan pl;
    const int rc = plan_rc((unsigned)atoi(argv[2]), C, &pl);
    printf("%d %zu %zu %zu\n", rc, pl.n, pl.stride_min, pl.bounds.empty() ? (size_t)0 : pl.bounds[0]);
    return 0;
  }
  if (argc >= 4 && !strcmp(argv[1], "prog")) {
    const Call C = call_of_args(argc, argv, 2);
    MpProgram pg;
    mp_compile(C.exps.data(), C.toff.data(), 1, C.nv, C.poff.data(), &pg);
    static const char* NAME[6] = {"?", "LOADC", "ADDC", "MULT", "HORNER", "POW"};
    printf("%u", pg.slots);
    for (size_t i = 0; i < C.nv; i++) printf(" %u", pg.vars.depth[i]);
    printf(" |");
    for (const MpOp& o : pg.ops) printf(" %s.%u.%u%s", NAME[(o.op & 0xffu) < 6 ? (o.op & 0xffu) : 0], (o.op >> 8) & 0xffffu, o.arg, (o.op & MP_FLUSH) ? "!" : "");
    printf("\n");
    return 0;
  }
  size_t n_exh = 0, n_rand = 0, n_plans = 0;
  n_exh += exhaustive(1, 3);
  n_exh += exhaustive(2, 3);
  n_exh += exhaustive(3, 2);
  while (n_rand < 1000000) n_rand += random_call(&n_plans);
  n_plans += plan_edges();
  if (g_fail) { printf("%d checks failed, %d of them on an address\n", g_fail, g_fail_address); return 1; }
  printf("ok %zu %zu %zu ratio %.3f\n", n_exh, n_rand, n_plans, g_ratio);
  return 0;
}
