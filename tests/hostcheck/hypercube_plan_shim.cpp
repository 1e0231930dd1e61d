// Stand-alone host program over myzkp_amd/csrc/mzk_hypercube_plan.h: reads term tables from a text file, runs hc_plan and
// hc_merge_coefs on each and prints every field of the plan; tests/test_hostcheck_hypercube_plan.py compares the output with
// tests/hypercube_model.py.  Built once plain and once with -fsanitize=address,undefined.
//
// Input:  count, then per table:  el k form n_offsets n_rows | the offsets | per row: a 64-hex-digit coefficient and el exponents.
//         (n_offsets is k + 1 except in tables written to be refused; rows are indexed by the offsets as the ABI indexes them)
// Output: per table "T rc"; on a refusal the message; else the scalar fields, then per factor "F masks groups", "M" the masks,
//         per mask "S" its source terms, "G" the groups as (high part, count), "C" the merged coefficients in hex.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include "../../myzkp_amd/csrc/mzk_hypercube_plan.h"

using namespace mzk;

static bool read_hex256(FILE* f, uint64_t out[4]) {
  char buf[80];
  if (fscanf(f, "%79s", buf) != 1 || strlen(buf) != 64) return false;
  for (int i = 0; i < 4; i++) {
    char part[17];
    memcpy(part, buf + 16 * (3 - i), 16);
    part[16] = 0;
    out[i] = strtoull(part, nullptr, 16);
  }
  return true;
}

int main(int argc, char** argv) {
  if (argc != 2) { fprintf(stderr, "usage: %s INPUT\n", argv[0]); return 2; }
  FILE* f = fopen(argv[1], "r");
  if (!f) { perror(argv[1]); return 2; }
  size_t count;
  if (fscanf(f, "%zu", &count) != 1) return 2;
  for (size_t c = 0; c < count; c++) {
    size_t el, k, n_off, n_rows;
    int form;
    if (fscanf(f, "%zu %zu %d %zu %zu", &el, &k, &form, &n_off, &n_rows) != 5) return 2;
    std::vector<size_t> off(n_off);
    for (auto& o : off) if (fscanf(f, "%zu", &o) != 1) return 2;
    std::vector<uint64_t> coefs(4 * n_rows);
    std::vector<uint32_t> exps(el * n_rows);
    for (size_t t = 0; t < n_rows; t++) {
      if (!read_hex256(f, &coefs[4 * t])) return 2;
      for (size_t i = 0; i < el; i++) if (fscanf(f, "%u", &exps[t * el + i]) != 1) return 2;
    }
    HcPlan pl;
    const int rc = hc_plan(exps.empty() ? nullptr : exps.data(), off.empty() ? nullptr : off.data(), k, el, form, &pl);
    printf("T %d\n", rc);
    if (rc != MZK_OK) { printf("%s\n", pl.msg); continue; }
    printf("%d %d %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", pl.form, pl.g, pl.terms, pl.mask.size(), pl.grp_hi.size(), pl.max_masks, pl.max_groups,
           pl.launches, pl.memsets, pl.grid_x, pl.grid_y, pl.mle_passes, pl.upload_bytes, pl.workspace_bytes, pl.table_bytes);
    // what the kernels rely on: the arrays close, every mask is below 2^el, every source term is used once
    if (pl.ent_off.size() != k + 1 || pl.grp_off.size() != k + 1 || pl.seg.size() != pl.mask.size() + 1 || pl.grp_begin.size() != pl.grp_hi.size() + 1 ||
        pl.order.size() != pl.terms || pl.seg.back() != pl.terms || pl.grp_begin.back() != pl.mask.size()) { printf("BROKEN sizes\n"); return 1; }
    for (uint32_t m : pl.mask) if ((uint64_t)m >> el) { printf("BROKEN mask\n"); return 1; }
    std::vector<uint32_t> merged(8 * pl.mask.size() + 1);
    hc_merge_coefs(pl, coefs.data(), k ? off[0] : 0, merged.data());
    for (size_t fi = 0; fi < k; fi++) {
      printf("F %u %u\nM", pl.ent_off[fi + 1] - pl.ent_off[fi], pl.grp_off[fi + 1] - pl.grp_off[fi]);
      for (uint32_t e = pl.ent_off[fi]; e < pl.ent_off[fi + 1]; e++) printf(" %u", pl.mask[e]);
      printf("\n");
      for (uint32_t e = pl.ent_off[fi]; e < pl.ent_off[fi + 1]; e++) {
        printf("S");
        for (uint32_t q = pl.seg[e]; q < pl.seg[e + 1]; q++) printf(" %u", pl.order[q]);
        printf("\n");
      }
      printf("G");
      for (uint32_t j = pl.grp_off[fi]; j < pl.grp_off[fi + 1]; j++) printf(" %u %u", pl.grp_hi[j], pl.grp_begin[j + 1] - pl.grp_begin[j]);
      printf("\nC");
      for (uint32_t e = pl.ent_off[fi]; e < pl.ent_off[fi + 1]; e++) {
        printf(" ");
        for (int w = 7; w >= 0; w--) printf("%08x", merged[8 * e + w]);
      }
      printf("\n");
    }
  }
  fclose(f);
  return 0;
}
