// The Rescue-Prime plan (myzkp_amd/csrc/mzk_rescue_plan.h) and the per-lane code (myzkp_amd/csrc/mzk_rescue.h, with the portable products)
// run on the host for tests/test_hostcheck_rescue.py.  Stand-alone; one argument, the file the test writes:
//   <count> then one exponent per line (hex);  <count> then one batch per line (decimal);  the case table (rescue_cases.dump).
// Prints
//   X exponent window slots steps squarings multiplies table products binary reached  steps...      per exponent: `reached` is the exponent the
//                                                  program raises to, found by running it on integers (a step as op:arg)
//   G batch wgs grid iters block cap                                                                per batch
//   R fid m n batch err <message>                                                                   per refused parameter set
//   P <the exported plan words of the reference's parameters at batch 4099>
//   H case input link <output>            the hash form,  O case input link <output>  the trace form's outputs
//   T case input link row <m elements>    the trace form
// then "ok".  Built once plain and once with -fsanitize=address,undefined, both with -DMZK_CHECK_BOUNDS (the products assert their limb bounds).
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include "../../myzkp_amd/csrc/mzk_rescue.h"

using namespace mzk;

// ---- a small unsigned integer, enough for exponents below 2^256 and one carry word ------------------------------------------------------
struct Big {
  uint32_t w[10] = {0};
  void shl1() {
    uint32_t c = 0;
    for (int i = 0; i < 10; i++) { const uint32_t n = w[i] >> 31; w[i] = (w[i] << 1) | c; c = n; }
  }
  void add(uint32_t v) {
    uint64_t c = v;
    for (int i = 0; i < 10 && c; i++) { c += w[i]; w[i] = (uint32_t)c; c >>= 32; }
  }
  std::string hex() const {
    char buf[16];
    std::string s;
    int i = 9;
    while (i > 0 && w[i] == 0) i--;
    snprintf(buf, sizeof buf, "%x", w[i]);
    s = buf;
    for (i--; i >= 0; i--) { snprintf(buf, sizeof buf, "%08x", w[i]); s += buf; }
    return s;
  }
};

// hex -> n 32-bit words, little-endian; false when it does not fit
static bool parse_hex(const char* s, uint32_t* w, int n) {
  for (int i = 0; i < n; i++) w[i] = 0;
  const int len = (int)strlen(s);
  for (int k = 0; k < len; k++) {
    const char ch = s[len - 1 - k];
    const int d = ch >= '0' && ch <= '9' ? ch - '0' : ch >= 'a' && ch <= 'f' ? ch - 'a' + 10 : -1;
    if (d < 0) return false;
    if (k / 8 >= n) { if (d) return false; continue; }
    w[k / 8] |= (uint32_t)d << (4 * (k % 8));
  }
  return true;
}
static void words_to_u64(const uint32_t* w, uint64_t e[4]) {
  for (int i = 0; i < 4; i++) e[i] = (uint64_t)w[2 * i] | (uint64_t)w[2 * i + 1] << 32;
}

// the program on integers: the exponent it raises x to; false when it reads a slot it has not built, or more than four
static bool interpret(const RescueChain& C, Big* out) {
  Big acc;
  int built = 0;            // highest slot built (slot 0 = x is there from the start)
  bool have = false;
  for (int s = 0; s < C.steps; s++) {
    const uint32_t op = C.prog[s] & 0xffu, arg = C.prog[s] >> 8;
    if (op == RS_OP_ONE) { acc = Big(); have = true; }
    else if (op == RS_OP_TABLE) { if (arg < 1 || arg > 3 || s != 0) return false; built = (int)arg; }
    else if (op == RS_OP_LOAD) { if ((int)arg > built) return false; acc = Big(); acc.add(2 * arg + 1); have = true; }
    else if (op == RS_OP_SQR) { if (!have) return false; for (uint32_t k = 0; k < arg; k++) acc.shl1(); }
    else if (op == RS_OP_MUL) { if (!have || (int)arg > built) return false; acc.add(2 * arg + 1); }
    else return false;
  }
  if (!have || built + 1 != (C.slots ? C.slots : 1) || built + 1 > 4) return false;
  *out = acc;
  return true;
}

template <class P> struct HostOut {
  std::vector<Fe<P>> rows, outs;
  int m, nrows;
  void row(size_t l, u32 r, u32 i, const Fe<P>& v) { rows[(l * (size_t)nrows + r) * (size_t)m + i] = v; }
  void output(size_t l, const Fe<P>& v) { outs[l] = v; }
};
template <class P> static std::string fe_hex(const Fe<P>& v) {
  u32 w[P::NW];
  fe_pack<P>(v, w);
  Big b;
  for (int i = 0; i < P::NW; i++) b.w[i] = w[i];
  return b.hex();
}
template <class P> static bool read_fe(FILE* f, Fe<P>* out) {
  char tok[80];
  u32 w[P::NW];
  if (fscanf(f, "%79s", tok) != 1 || !parse_hex(tok, w, P::NW)) return false;
  *out = fe_unpack<P>(w);
  return true;
}

template <class P, int M> static int run_case_m(const char* name, const RescueConsts& c, const std::vector<Fe<P>>& inputs, size_t links) {
  const int nrows = (int)c.n_rounds + 1;
  for (size_t k = 0; k < inputs.size(); k++) {
    HostOut<P> h{{}, std::vector<Fe<P>>(links), M, nrows}, t{std::vector<Fe<P>>(links * (size_t)nrows * M), std::vector<Fe<P>>(links), M, nrows};
    rs_chain<P, M, false>(c, inputs[k], links, h);
    rs_chain<P, M, true>(c, inputs[k], links, t);
    for (size_t l = 0; l < links; l++) {
      printf("H %s %zu %zu %s\n", name, k, l, fe_hex<P>(h.outs[l]).c_str());
      printf("O %s %zu %zu %s\n", name, k, l, fe_hex<P>(t.outs[l]).c_str());
      for (int r = 0; r < nrows; r++) {
        printf("T %s %zu %zu %d", name, k, l, r);
        for (int i = 0; i < M; i++) printf(" %s", fe_hex<P>(t.rows[(l * (size_t)nrows + (size_t)r) * M + (size_t)i]).c_str());
        printf("\n");
      }
    }
  }
  return 0;
}

template <class P> static int run_case(FILE* f, const char* name, int fid, size_t m, size_t n, uint64_t alpha, const uint64_t ai[4], size_t n_inputs, size_t links) {
  const RescuePlan pl = rescue_plan(fid, m, n, alpha, ai, 0);
  if (pl.err != MZK_OK) { fprintf(stderr, "%s refused: %s\n", name, pl.msg); return 1; }
  std::vector<u32> words(pl.const_words, 0);
  for (int k = 0; k < pl.alpha.steps; k++) words[pl.prog_off[0] + (size_t)k] = pl.alpha.prog[k];
  for (int k = 0; k < pl.alphainv.steps; k++) words[pl.prog_off[1] + (size_t)k] = pl.alphainv.prog[k];
  for (size_t i = 0; i < m * m + 2 * n * m; i++) {
    Fe<P> v;
    if (!read_fe<P>(f, &v)) { fprintf(stderr, "%s: bad constant %zu\n", name, i); return 1; }
    const Fe<P> mont = fe_reduce<P>(fe_to_mont<P>(v));
    const size_t at = i < m * m ? pl.mds_off + i * (size_t)P::L : pl.rc_off + (i - m * m) * (size_t)P::L;
    for (int j = 0; j < P::L; j++) words[at + (size_t)j] = mont.l[j];
  }
  std::vector<Fe<P>> inputs(n_inputs);
  for (size_t i = 0; i < n_inputs; i++) if (!read_fe<P>(f, &inputs[i])) { fprintf(stderr, "%s: bad input %zu\n", name, i); return 1; }
  RescueConsts c;
  c.words = words.data();
  c.prog[0] = (u32)pl.prog_off[0]; c.prog[1] = (u32)pl.prog_off[1];
  c.steps[0] = (u32)pl.alpha.steps; c.steps[1] = (u32)pl.alphainv.steps;
  c.mds = (u32)pl.mds_off; c.rc = (u32)pl.rc_off; c.n_rounds = (u32)n;
  switch (m) {
    case 1: return run_case_m<P, 1>(name, c, inputs, links);
    case 2: return run_case_m<P, 2>(name, c, inputs, links);
    case 3: return run_case_m<P, 3>(name, c, inputs, links);
    default: return run_case_m<P, 4>(name, c, inputs, links);
  }
}

int main(int argc, char** argv) {
  if (argc != 2) { fprintf(stderr, "usage: rescue_shim <input file>\n"); return 2; }
  FILE* f = fopen(argv[1], "r");
  if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
  size_t count = 0;
  char tok[80];
  // (a) the exponents
  if (fscanf(f, "%zu", &count) != 1) return 2;
  for (size_t k = 0; k < count; k++) {
    uint32_t w[8];
    uint64_t e[4];
    if (fscanf(f, "%79s", tok) != 1 || !parse_hex(tok, w, 8)) { fprintf(stderr, "bad exponent %zu\n", k); return 1; }
    words_to_u64(w, e);
    const RescueChain C = rescue_chain(e);
    Big reached;
    if (!interpret(C, &reached)) { fprintf(stderr, "exponent %s: the program reads a slot it has not built, or is malformed\n", tok); return 1; }
    if (C.steps > RESCUE_MAX_STEPS) { fprintf(stderr, "exponent %s: %d steps\n", tok, C.steps); return 1; }
    printf("X %s %d %d %d %d %d %d %d %d %s ", tok, C.window, C.slots, C.steps, C.squarings, C.multiplies, C.table, C.products, C.binary, reached.hex().c_str());
    for (int s = 0; s < C.steps; s++) printf(" %u:%u", C.prog[s] & 0xffu, C.prog[s] >> 8);
    printf("\n");
  }
  // the grid
  const uint64_t three[4] = {3, 0, 0, 0};
  if (fscanf(f, "%zu", &count) != 1) return 2;
  for (size_t k = 0; k < count; k++) {
    size_t batch;
    if (fscanf(f, "%zu", &batch) != 1) return 2;
    const RescuePlan P = rescue_plan(MZK_FIELD_M128, 2, 27, 3, three, batch);
    if (P.err != MZK_OK) { fprintf(stderr, "batch %zu refused: %s\n", batch, P.msg); return 1; }
    printf("G %zu %zu %zu %u %u %zu\n", batch, P.wgs, P.grid, P.iters, P.block, RESCUE_MAX_GRID);
  }
  const size_t refused[][4] = {{2, 2, 27, 1}, {3, 2, 27, 1}, {4, 2, 27, 1}, {99, 2, 27, 1}, {1, 0, 27, 1}, {1, 5, 27, 1}, {0, 2, 0, 1}, {0, 2, 65, 1}, {1, 4, 64, ((size_t)1 << 40) + 1}};
  for (const auto& r : refused) {
    const RescuePlan P = rescue_plan((int)r[0], r[1], r[2], 3, three, r[3]);
    printf("R %zu %zu %zu %zu %d %s\n", r[0], r[1], r[2], r[3], P.err, P.msg);
  }
  if (rescue_plan(MZK_FIELD_FR, 4, 64, ~(uint64_t)0, three, (size_t)1 << 40).err != MZK_OK || rescue_plan(MZK_FIELD_M128, 1, 1, 0, three, 0).err != MZK_OK) {
    fprintf(stderr, "an admitted boundary parameter set was refused\n");
    return 1;
  }
  {
    const uint64_t ai[4] = {0xaaaaaaaaaaaaaaabULL, 0x87aaaaaaaaaaaaaaULL, 0, 0};
    uint64_t E[MZK_RESCUE_PLAN_WORDS];
    rescue_plan_export(rescue_plan(MZK_FIELD_M128, 2, 27, 3, ai, 4099), E);
    printf("P");
    for (int i = 0; i < MZK_RESCUE_PLAN_WORDS; i++) printf(" %" PRIu64, E[i]);
    printf("\n");
  }
  // (b) the per-lane code on every case
  if (fscanf(f, "%zu", &count) != 1) return 2;
  for (size_t k = 0; k < count; k++) {
    char name[80], a_hex[80], ai_hex[80];
    int fid;
    size_t m, n, n_inputs, links;
    if (fscanf(f, "%79s %d %zu %zu %79s %79s %zu %zu", name, &fid, &m, &n, a_hex, ai_hex, &n_inputs, &links) != 8) { fprintf(stderr, "bad case header %zu\n", k); return 1; }
    uint32_t w[8] = {0};
    uint64_t a[4], ai[4];
    if (!parse_hex(a_hex, w, 2)) return 1;
    words_to_u64(w, a);
    if (!parse_hex(ai_hex, w, 8)) return 1;
    words_to_u64(w, ai);
    const int rc = fid == MZK_FIELD_M128 ? run_case<M128Params>(f, name, fid, m, n, a[0], ai, n_inputs, links) : run_case<FrParams>(f, name, fid, m, n, a[0], ai, n_inputs, links);
    if (rc) return rc;
  }
  fclose(f);
  printf("ok\n");
  return 0;
}
