// mzk_mpoly_plan.h -- what mzk_mpoly_compose* (mzk_mpoly.hip) decides on the host before it touches the device: the size plan
// (mp_plan: the degree bound of every constraint, out_stride_min, the transform size N, every refusal with its message) and the
// term programs k_mp_terms runs (mp_compile: the Horner variable and the runs of every constraint, the op of every exponent and gap,
// the LDS slots of every variable, the flush bits).  Pure functions of the exponent table, the offsets and the field's largest
// transform.  Host-only C++17 with no HIP include, so that it can be compiled and checked on its own: tests/hostcheck/
// mpoly_plan_shim.cpp interprets every program in integers against the naive sum (tests/test_hostcheck_mpoly_plan.py).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <algorithm>
#include <vector>
#include "../../include/mzk.h"

namespace mzk {

constexpr int MP_MAX_VARS = MZK_MPOLY_MAX_VARS;
constexpr int MP_TABLE = 3;              // deepest power kept per variable
constexpr int MP_LANES = 64;
constexpr int MP_MAX_LIMBS = 9;          // 29-bit limbs of the widest field (Fr: L = 9; M128: 5)
// the power tables of one wave, every variable at full depth over the widest field, fit the LDS a launch gets without an attribute
static_assert(MZK_MPOLY_MAX_VARS * MP_TABLE * MP_MAX_LIMBS * MP_LANES * 4 <= 65536, "k_mp_terms: power tables above 64 KiB of LDS");
enum { MP_LOADC = 1, MP_ADDC = 2, MP_MULT = 3, MP_HORNER = 4, MP_POW = 5 };
constexpr uint32_t MP_FLUSH = 1u << 31;  // after the op: sum += acc
// op word: op | slot << 8 | flush; arg word: coefficient index (LOADC, ADDC, HORNER) or exponent (POW; slot = the variable's first slot)
struct MpOp { uint32_t op, arg; };
struct MpVars { uint32_t first_slot[MP_MAX_VARS]; uint32_t depth[MP_MAX_VARS]; };

// ---- size plan -----------------------------------------------------------------------------------------------------------------------
// msg: what set_error gets when the return value is not MZK_OK
struct MpPlan { size_t n = 0, stride_min = 0; std::vector<size_t> bounds; char msg[192] = {0}; };

static inline int mp_monotone(const size_t* off, size_t count, const char* what, MpPlan* pl) {
  for (size_t i = 0; i < count; i++)
    if (off[i + 1] < off[i]) {
      snprintf(pl->msg, sizeof pl->msg, "mpoly_compose: %s[%zu] = %zu is below %s[%zu] = %zu", what, i + 1, off[i + 1], what, i, off[i]);
      return MZK_E_LENGTH;
    }
  return MZK_OK;
}
// term t vanishes (a positive exponent on an empty polynomial) ?  *deg = sum_i k_i (len_i - 1).  A term that vanishes has no degree:
// it is recognised before any product is formed, so that it cannot be refused for an overflow in front of its empty polynomial.
static inline int mp_term_degree(const uint32_t* k, size_t nv, const size_t* point_offsets, bool* vanishes, size_t* deg, MpPlan* pl) {
  size_t d = 0;
  *vanishes = false;
  for (size_t i = 0; i < nv; i++)
    if (k[i] && point_offsets[i + 1] == point_offsets[i]) { *vanishes = true; return MZK_OK; }
  for (size_t i = 0; i < nv; i++) {
    if (k[i] == 0) continue;
    const size_t len = point_offsets[i + 1] - point_offsets[i];
    size_t m;
    if (__builtin_mul_overflow((size_t)k[i], len - 1, &m) || __builtin_add_overflow(d, m, &d)) {
      snprintf(pl->msg, sizeof pl->msg, "mpoly_compose: the degree bound of a term overflows 64 bits");
      return MZK_E_LENGTH;
    }
  }
  *deg = d;
  return MZK_OK;
}
// max_log: the field's largest transform is 2^max_log points (the caller has checked the field id)
static inline int mp_plan(unsigned max_log, const uint32_t* term_exps, const size_t* term_offsets, size_t nc, size_t nv, const size_t* point_offsets, MpPlan* pl) {
  if (nv > (size_t)MP_MAX_VARS) { snprintf(pl->msg, sizeof pl->msg, "mpoly_compose: %zu variables (at most %d)", nv, MP_MAX_VARS); return MZK_E_ARG; }
  if (nc == 0) return MZK_OK;
  if (!term_offsets || (nv && !point_offsets)) { snprintf(pl->msg, sizeof pl->msg, "mpoly_compose: null pointer"); return MZK_E_ARG; }
  if (int rc = mp_monotone(term_offsets, nc, "term_offsets", pl)) return rc;
  if (nv) if (int rc = mp_monotone(point_offsets, nv, "point_offsets", pl)) return rc;
  if (term_offsets[nc] > term_offsets[0] && nv && !term_exps) { snprintf(pl->msg, sizeof pl->msg, "mpoly_compose: null pointer"); return MZK_E_ARG; }
  pl->bounds.assign(nc, 0);
  for (size_t a = 0; a < nc; a++)
    for (size_t t = term_offsets[a]; t < term_offsets[a + 1]; t++) {
      bool vanishes;
      size_t d = 0;
      if (int rc = mp_term_degree(nv ? term_exps + t * nv : nullptr, nv, point_offsets, &vanishes, &d, pl)) return rc;
      if (vanishes) continue;
      if (d == SIZE_MAX) { snprintf(pl->msg, sizeof pl->msg, "mpoly_compose: the degree bound of a term overflows 64 bits"); return MZK_E_LENGTH; }
      pl->bounds[a] = std::max(pl->bounds[a], d + 1);
    }
  pl->stride_min = *std::max_element(pl->bounds.begin(), pl->bounds.end());
  unsigned lg = 0;
  while (lg < 64 && ((size_t)1 << lg) < pl->stride_min) lg++;
  if (lg > max_log) {
    snprintf(pl->msg, sizeof pl->msg, "mpoly_compose: degree bound %zu needs a transform of 2^%u points (at most 2^%u over this field)", pl->stride_min - 1, lg, max_log);
    return MZK_E_LENGTH;
  }
  pl->n = (size_t)1 << lg;
  return MZK_OK;
}

// ---- term programs -------------------------------------------------------------------------------------------------------------------
struct MpProgram { std::vector<MpOp> ops; std::vector<uint32_t> off; MpVars vars; uint32_t slots = 0; };

static inline void mp_emit_pow(std::vector<MpOp>& ops, const MpVars& v, uint32_t var, uint32_t e) {
  const uint32_t s0 = v.first_slot[var];
  if (e == 0) return;
  if (e <= (uint32_t)MP_TABLE) ops.push_back({MP_MULT | (s0 + e - 1) << 8, 0});
  else if (e <= 2u * MP_TABLE) { ops.push_back({MP_MULT | (s0 + MP_TABLE - 1) << 8, 0}); ops.push_back({MP_MULT | (s0 + e - MP_TABLE - 1) << 8, 0}); }
  else ops.push_back({MP_POW | s0 << 8, e});
}
// term_exps / term_offsets as at the ABI; coefficient index = term index - term_offsets[0]
static inline void mp_compile(const uint32_t* term_exps, const size_t* term_offsets, size_t nc, size_t nv, const size_t* point_offsets, MpProgram* pg) {
  // table depth per variable: the largest exponent any term asks for, at most MP_TABLE (gaps and tails of a Horner run are no larger)
  uint32_t maxe[MP_MAX_VARS] = {};
  for (size_t t = term_offsets[0]; t < term_offsets[nc]; t++)
    for (size_t i = 0; i < nv; i++) maxe[i] = std::max(maxe[i], term_exps[t * nv + i]);
  pg->slots = 0;
  for (size_t i = 0; i < (size_t)MP_MAX_VARS; i++) {
    const uint32_t e = i < nv ? maxe[i] : 0;
    pg->vars.depth[i] = e > (uint32_t)MP_TABLE ? (uint32_t)MP_TABLE : e;
    pg->vars.first_slot[i] = pg->slots;
    pg->slots += pg->vars.depth[i];
  }
  pg->off.assign(1, 0);
  for (size_t a = 0; a < nc; a++) {
    std::vector<size_t> terms;
    uint32_t cmax[MP_MAX_VARS] = {};
    for (size_t t = term_offsets[a]; t < term_offsets[a + 1]; t++) {
      bool vanishes = false;
      for (size_t i = 0; i < nv; i++) {
        const uint32_t e = term_exps[t * nv + i];
        if (e && point_offsets[i + 1] == point_offsets[i]) vanishes = true;
        cmax[i] = std::max(cmax[i], e);
      }
      if (!vanishes) terms.push_back(t);
    }
    size_t h = 0;                                        // the Horner variable
    for (size_t i = 1; i < nv; i++) if (cmax[i] > cmax[h]) h = i;
    auto rest_less = [&](size_t x, size_t y) {           // by the monomial of the other variables, then by falling exponent of h
      for (size_t i = 0; i < nv; i++) {
        if (i == h) continue;
        const uint32_t ex = term_exps[x * nv + i], ey = term_exps[y * nv + i];
        if (ex != ey) return ex < ey;
      }
      if (nv && term_exps[x * nv + h] != term_exps[y * nv + h]) return term_exps[x * nv + h] > term_exps[y * nv + h];
      return x < y;
    };
    std::sort(terms.begin(), terms.end(), rest_less);
    auto same_rest = [&](size_t x, size_t y) {
      for (size_t i = 0; i < nv; i++) if (i != h && term_exps[x * nv + i] != term_exps[y * nv + i]) return false;
      return true;
    };
    for (size_t r0 = 0; r0 < terms.size();) {
      size_t r1 = r0 + 1;
      while (r1 < terms.size() && same_rest(terms[r0], terms[r1])) r1++;
      pg->ops.push_back({MP_LOADC, (uint32_t)(terms[r0] - term_offsets[0])});
      for (size_t q = r0 + 1; q < r1; q++) {
        const uint32_t gap = nv ? term_exps[terms[q - 1] * nv + h] - term_exps[terms[q] * nv + h] : 0u;
        const uint32_t ci = (uint32_t)(terms[q] - term_offsets[0]);
        if (gap == 0) pg->ops.push_back({MP_ADDC, ci});
        else if (gap <= (uint32_t)MP_TABLE) pg->ops.push_back({MP_HORNER | (pg->vars.first_slot[h] + gap - 1) << 8, ci});
        else {
          mp_emit_pow(pg->ops, pg->vars, (uint32_t)h, gap);
          // the product is below p + 1: the sum with a canonical coefficient is what HORNER leaves, one reduction more is harmless
          pg->ops.push_back({MP_ADDC, ci});
        }
      }
      if (nv) mp_emit_pow(pg->ops, pg->vars, (uint32_t)h, term_exps[terms[r1 - 1] * nv + h]);
      for (size_t i = 0; i < nv; i++) if (i != h) mp_emit_pow(pg->ops, pg->vars, (uint32_t)i, term_exps[terms[r0] * nv + i]);
      pg->ops.back().op |= MP_FLUSH;
      r0 = r1;
    }
    pg->off.push_back((uint32_t)pg->ops.size());
  }
}

}  // namespace mzk
