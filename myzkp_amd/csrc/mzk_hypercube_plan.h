// mzk_hypercube_plan.h -- what mzk_mpoly_hypercube_evals* and mzk_sumcheck_product_prove_terms* (mzk_sumcheck.hip) decide on the host
// before they touch the device: the evaluation table over {0,1}^el of a sparse multivariate factor depends on the SUPPORT of every
// term alone (0^0 = 1, b^e = b for e > 0), so a term is its mask (variable i <-> bit el-1-i, BitCombinationsDictOrder) and
//   evals[b] = sum over the terms whose mask is a subset of b of their coefficients.
// hc_plan turns the flat term table of mzk_mpoly_compose into, per factor, the distinct masks in ascending order, for each the segment
// of source terms that carry it (their coefficients are added ON THE HOST, mzk_hostfield.h, by the caller of this plan), and the
// groups of masks that share their high part mask >> g, g = min(el, HC_TILE_LOG); it chooses the device form and states the launches,
// grids and bytes.  Pure functions of the exponent table, the offsets, el and the form asked for.  Host-only C++17 with no HIP
// include: tests/hostcheck/hypercube_plan_shim.cpp checks every field against Python integers.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <algorithm>
#include <vector>
#include "../../include/mzk.h"
#include "mzk_hostfield.h"

namespace mzk {

constexpr int HC_TILE_LOG = 10;          // a tile of 2^10 elements of 32 bytes: the 32 KiB of LDS k_mle_pass uses
constexpr int HC_MAX_VARS = 30;
constexpr int HC_THREADS = 256;
constexpr size_t HC_MAX_TERMS = (size_t)1 << 28;
// MZK_HYPER_AUTO: the tile form while no factor has more groups or more distinct masks than these.  Every workgroup of the tile form
// tests every group of its factor once (2^(el-g) * groups uniform tests) and the last tile takes every mask of its factor, a barrier per
// group; the scatter form's cost depends on neither.  Set from profiles/hypercube_time.txt (DESIGN.md 9f has the crossovers).
constexpr size_t HC_TILE_MAX_GROUPS = 256;
constexpr size_t HC_TILE_MAX_MASKS = 4096;

struct HcPlan {
  int form = 0;                          // MZK_HYPER_TILE or MZK_HYPER_SCATTER: the form that runs
  int el = 0, g = 0;
  size_t k = 0, terms = 0;
  // the merged table, factor by factor.  Entry e is the mask mask[e]; its coefficient is the sum of term_coefs[t0 + order[q]] for q in
  // [seg[e], seg[e + 1]), t0 = term_offsets[0].  Factor f owns the entries [ent_off[f], ent_off[f + 1]), masks ascending.
  std::vector<uint32_t> mask, seg, order, ent_off;
  // group j: the entries [grp_begin[j], grp_begin[j + 1]) share grp_hi[j] = mask >> g.  Factor f owns the groups [grp_off[f], grp_off[f + 1]).
  std::vector<uint32_t> grp_hi, grp_begin, grp_off;
  size_t max_masks = 0, max_groups = 0;  // the largest count of one factor
  // what runs: kernel launches (the memset apart), the grid of the form's own kernel, the passes of the butterfly per factor
  size_t launches = 0, memsets = 0, grid_x = 0, grid_y = 0, mle_passes = 0;
  size_t upload_words_head = 0;          // fac_off | grp_hi | grp_begin | mask, padded to a multiple of 4 words; the coefficients follow
  size_t upload_bytes = 0, workspace_bytes = 0, table_bytes = 0;
  char msg[192] = {0};                   // what set_error gets when the return value is not MZK_OK
};

// the passes of mle_dev_impl over el index bits: the first takes HC_TILE_LOG bits, every later one HC_TILE_LOG - 2
static inline size_t hc_mle_passes(size_t el) {
  size_t n = 0;
  for (size_t lo = 0; lo < el; n++) {
    const size_t cb = lo < 2 ? lo : 2, g = el - lo < HC_TILE_LOG - cb ? el - lo : HC_TILE_LOG - cb;
    lo += g;
  }
  return n;
}
// the rule of MZK_HYPER_AUTO: a function of (el, distinct masks, groups) of the largest factor.  At el <= HC_TILE_LOG a factor is one
// tile and has at most one group and 2^el <= 1024 masks, so the tile form always runs there.
static inline int hc_auto_form(size_t el, size_t max_masks, size_t max_groups) {
  (void)el;
  return max_groups <= HC_TILE_MAX_GROUPS && max_masks <= HC_TILE_MAX_MASKS ? MZK_HYPER_TILE : MZK_HYPER_SCATTER;
}

static inline int hc_plan(const uint32_t* term_exps, const size_t* term_offsets, size_t k, size_t el, int form, HcPlan* pl) {
  if (form != MZK_HYPER_AUTO && form != MZK_HYPER_TILE && form != MZK_HYPER_SCATTER) {
    snprintf(pl->msg, sizeof pl->msg, "mpoly_hypercube: form %d (MZK_HYPER_AUTO, _TILE or _SCATTER)", form);
    return MZK_E_ARG;
  }
  if (k && !term_offsets) { snprintf(pl->msg, sizeof pl->msg, "mpoly_hypercube: null pointer"); return MZK_E_ARG; }
  if (el > (size_t)HC_MAX_VARS) { snprintf(pl->msg, sizeof pl->msg, "mpoly_hypercube: %zu variables (at most %d)", el, HC_MAX_VARS); return MZK_E_LENGTH; }
  for (size_t f = 0; f < k; f++)
    if (term_offsets[f + 1] < term_offsets[f]) {
      snprintf(pl->msg, sizeof pl->msg, "mpoly_hypercube: term_offsets[%zu] = %zu is below term_offsets[%zu] = %zu", f + 1, term_offsets[f + 1], f, term_offsets[f]);
      return MZK_E_LENGTH;
    }
  const size_t t0 = k ? term_offsets[0] : 0, nt = k ? term_offsets[k] - t0 : 0;
  if (nt >= HC_MAX_TERMS) { snprintf(pl->msg, sizeof pl->msg, "mpoly_hypercube: %zu terms (at most 2^28 - 1)", nt); return MZK_E_LENGTH; }
  if (nt && el && !term_exps) { snprintf(pl->msg, sizeof pl->msg, "mpoly_hypercube: null pointer"); return MZK_E_ARG; }
  if (k >= ((size_t)1 << 16)) { snprintf(pl->msg, sizeof pl->msg, "mpoly_hypercube: %zu factors (the factor is a grid dimension: at most 65535)", k); return MZK_E_LENGTH; }
  pl->el = (int)el;
  pl->g = (int)(el < (size_t)HC_TILE_LOG ? el : (size_t)HC_TILE_LOG);
  pl->k = k;
  pl->terms = nt;
  pl->mask.clear(); pl->seg.assign(1, 0); pl->order.clear(); pl->ent_off.assign(1, 0);
  pl->grp_hi.clear(); pl->grp_begin.assign(1, 0); pl->grp_off.assign(1, 0);
  pl->order.reserve(nt);
  pl->max_masks = pl->max_groups = 0;
  std::vector<uint64_t> keys;              // mask << 32 | term index relative to t0: sorting orders by mask, then by source order
  for (size_t f = 0; f < k; f++) {
    keys.clear();
    for (size_t t = term_offsets[f]; t < term_offsets[f + 1]; t++) {
      uint32_t m = 0;
      for (size_t i = 0; i < el; i++) m |= (uint32_t)(term_exps[t * el + i] != 0) << (el - 1 - i);
      keys.push_back((uint64_t)m << 32 | (uint64_t)(t - t0));
    }
    std::sort(keys.begin(), keys.end());
    const size_t e0 = pl->mask.size(), g0 = pl->grp_hi.size();
    for (size_t q = 0; q < keys.size(); q++) {
      const uint32_t m = (uint32_t)(keys[q] >> 32);
      if (q == 0 || m != pl->mask.back()) {
        if (q) pl->seg.push_back((uint32_t)pl->order.size());
        if (q == 0 || (m >> pl->g) != pl->grp_hi.back()) {
          if (pl->grp_hi.size() > g0) pl->grp_begin.push_back((uint32_t)pl->mask.size());
          pl->grp_hi.push_back(m >> pl->g);
        }
        pl->mask.push_back(m);
      }
      pl->order.push_back((uint32_t)keys[q]);
    }
    if (!keys.empty()) {
      pl->seg.push_back((uint32_t)pl->order.size());
      pl->grp_begin.push_back((uint32_t)pl->mask.size());
    }
    pl->ent_off.push_back((uint32_t)pl->mask.size());
    pl->grp_off.push_back((uint32_t)pl->grp_hi.size());
    pl->max_masks = std::max(pl->max_masks, pl->mask.size() - e0);
    pl->max_groups = std::max(pl->max_groups, pl->grp_hi.size() - g0);
  }
  pl->form = form == MZK_HYPER_AUTO ? hc_auto_form(el, pl->max_masks, pl->max_groups) : form;
  const size_t E = pl->mask.size(), G = pl->grp_hi.size(), n = (size_t)1 << el;
  pl->table_bytes = k * n * 32;
  pl->mle_passes = hc_mle_passes(el);
  if (k == 0) {
    pl->launches = pl->memsets = pl->grid_x = pl->grid_y = pl->upload_words_head = pl->upload_bytes = pl->workspace_bytes = 0;
    return MZK_OK;
  }
  size_t head;
  if (pl->form == MZK_HYPER_TILE) {
    pl->launches = 1; pl->memsets = 0;
    pl->grid_x = n >> pl->g; pl->grid_y = k;
    head = (k + 1) + G + (G + 1) + E;
  } else {
    const bool scatter = E > 0;
    pl->memsets = 1;
    pl->grid_x = scatter ? (pl->max_masks + HC_THREADS - 1) / HC_THREADS : 0;
    pl->grid_y = scatter ? k : 0;
    pl->launches = scatter ? 1 + k * pl->mle_passes : 0;       // without a term the zero-filled tables are the result
    head = (k + 1) + E;
  }
  pl->upload_words_head = (head + 3) & ~(size_t)3;
  pl->upload_bytes = 4 * (pl->upload_words_head + 8 * E);
  pl->workspace_bytes = (pl->upload_bytes + 255) & ~(size_t)255;
  return MZK_OK;
}

// The host merge: entry e's coefficient = the sum of its segment's coefficients, as 8 words (standard form, canonical).
// coefs: the caller's term_coefs (4 limbs per term, canonical); t0 = term_offsets[0].
static inline void hc_merge_coefs(const HcPlan& pl, const uint64_t* coefs, size_t t0, uint32_t* out) {
  const HostField* fr = host_field(MZK_FIELD_FR);
  for (size_t e = 0; e < pl.mask.size(); e++) {
    uint64_t acc[4];
    for (int i = 0; i < 4; i++) acc[i] = coefs[4 * (t0 + pl.order[pl.seg[e]]) + i];
    for (uint32_t q = pl.seg[e] + 1; q < pl.seg[e + 1]; q++) h_addmod(fr, acc, acc, coefs + 4 * (t0 + pl.order[q]));
    h_words(acc, 4, out + 8 * e);
  }
}

}  // namespace mzk
