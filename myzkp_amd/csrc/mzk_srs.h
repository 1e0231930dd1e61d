// mzk_srs.h -- the KZG SRS handle: device-resident PublicKeyKZG.powers_1 (kzg.rs:8-11) in the layout mzk_srs_plan.h picked for it,
// with the optional direct and wide tables of the grid-batched passes.  Host only and free of HIP, as mzk_ws.h is: srs_new and the
// table sets run on a CPU with malloc-backed hooks (tests/hostcheck/srs_handle_main.cpp); what fills the tables is mzk_srs.hip.
#pragma once
#include <memory>
#include <utility>
#include "mzk_srs_plan.h"
#include "mzk_ws.h"

namespace mzk {
void clear_error();                            // a refused allocation that the call then does without leaves no message behind
inline size_t g_table_budget = 0;              // mzk_set_table_budget: bytes of tables a handle may hold (0 = no limit)

// One set of device tables and what it was built as: window bits and bytes (0, 0 while there is none).
struct SrsTables {
  DevMem mem;
  int bits = 0;
  size_t bytes = 0;
  void attach(DevMem&& m, int bits_, size_t bytes_) { mem = std::move(m); bits = bits_; bytes = bytes_; }      // the tables held before are freed
  void drop() { mem.reset(); bits = 0; bytes = 0; }
};
}  // namespace mzk

struct mzk_srs {       // made by srs_new alone
  // own.mem: msm_table_rows(own.bits, sets) x n window tables when has_tables, else n prepared points + their n phi images
  mzk::SrsTables own;
  size_t n = 0;
  bool has_tables = false;
  // Bucket sets of the table layout (1 = every window shares one set: the default).  With k sets the handle holds only every
  // k-th window table, T[q][i] = 2^(c k q) P_i: window w = k q + r adds T[q][i] into bucket set r, and the result is
  // sum_r 2^(c r) B_r (k - 1 times c doublings at the very end).  1/k of the table memory for the same additions -- what a
  // handle degrades to when the full tables do not fit the budget / the device (srs_ladder).
  int sets = 1;
  int ctx_index = 0;     // the context (device) that owns the tables
  // optional (mzk_srs_build_direct): every multiple a window digit can ask for, D[(w n + i) 2^(direct.bits-1) + m] = (m + 1) 2^(direct.bits w) P_i,
  // affine Montgomery -- commitments of many short polynomials then need no buckets at all (msm_many_srs)
  mzk::SrsTables direct;
  // optional, built by the first grid-batched pass that wants them (msm_many_srs, which has the handle as the commit calls do: const):
  // a SECOND set of window tables, wider than the handle's own.  A handle of <= 2^14 points keeps 8- / 10-bit tables for the sortless
  // single commit; a batch of LONG polynomials (>= 2^13 coefficients) is 20 % faster over 12-bit ones (shorter accumulate, and a
  // bucket's partials are a chain a quarter as long in the segment combine: profiles/round5_many_commit_widths.txt).  22 x n points:
  // 22 MiB at 2^14.
  struct Wide : mzk::SrsTables { mzk::SrsWideState state = mzk::SRS_WIDE_UNTRIED; };
  mutable Wide wide;

  int kind() const { return mzk::srs_point_kind(has_tables, own.bits, sets); }
  size_t table_rows() const { return mzk::srs_table_rows(has_tables, own.bits, sets); }
  size_t table_bytes() const { return own.bytes + direct.bytes + wide.bytes; }
  // the handle's points [shift, n) as the MSM takes them: every layout keeps point i of a table at row offset i, so the tables are
  // entered `shift` rows further on with the row stride unchanged
  mzk::MsmPoints points(size_t shift = 0) const { return {own.mem.as<char>() + shift * 64, kind(), n}; }
};

namespace mzk {

typedef std::unique_ptr<mzk_srs> SrsOwner;
// A handle of n points on the current context, its tables allocated in the richest layout of srs_ladder that the device grants and
// not yet filled.  Every rung goes through dev_alloc: a refused allocation is tried again after the idle workspace has been released
// -- BEFORE the layout degrades.  n == 0: the first rung, no memory.
inline int srs_new(size_t n, int with_tables, SrsOwner* out) {
  const SrsLadder L = srs_ladder(n, with_tables, g_table_budget);
  SrsOwner h(new mzk_srs);
  h->n = n;
  h->ctx_index = ws_current_ctx();
  for (int k = 0; k < L.count; k++) {
    const SrsRung& r = L.rung[k];
    if (n == 0 || h->own.mem.alloc(r.bytes, "SRS handle") == MZK_OK) {
      h->own.bits = r.bits; h->own.bytes = r.bytes; h->has_tables = r.tables; h->sets = r.sets;
      *out = std::move(h);
      return MZK_OK;
    }
  }
  set_error("SRS handle: the device has no %zu bytes left for the prepared points alone (idle workspace already released)", n * 128);
  return MZK_E_NOMEM;
}

// The wide tables for one batch of polynomials of n_poly coefficients.  SRS_WIDE_USE_OWN / SRS_WIDE_USE_WIDE: which tables the batch
// reads.  SRS_WIDE_ALLOCATE: this batch builds them, *mem is allocated -- the caller fills it and attaches it with srs_wide_built.
// A refusal -- budget or device -- is remembered on the handle, so that later batches do not repeat a failing allocation and the
// idle-workspace release it triggers, and the message of the refused allocation does not stay behind on a call that returns MZK_OK.
inline SrsWideStep srs_wide_reserve(const mzk_srs* h, size_t n_poly, DevMem* mem) {
  const SrsWideStep step = srs_wide_step(n_poly, h->has_tables, h->sets, h->own.bits, h->wide.state, h->own.bytes + h->direct.bytes, h->n, g_table_budget);
  if (step == SRS_WIDE_USE_OWN || step == SRS_WIDE_USE_WIDE) return step;
  if (step == SRS_WIDE_ALLOCATE) {
    if (mem->alloc(srs_wide_bytes(h->n), "wide window tables of the grid-batched pass") == MZK_OK) return step;
    clear_error();
  }
  h->wide.state = SRS_WIDE_REFUSED;         // no memory (or no budget) for them: the handle's own tables serve (slower, same points)
  return SRS_WIDE_USE_OWN;
}
inline void srs_wide_built(const mzk_srs* h, DevMem&& mem) {
  h->wide.attach(std::move(mem), MANY_WIDE_BITS, srs_wide_bytes(h->n));
  h->wide.state = SRS_WIDE_BUILT;
}

// MZK_OK when the current context may use the handle: any context on the handle's device (a handle is plain device memory), or --
// same_context, the save and download calls -- the handle's own context alone.  mzk_srs.hip.
int srs_check_ctx(const mzk_srs* srs, bool same_context = false);
// a grid-batched pass exists for the handle: direct tables, or narrow window tables with one bucket set
bool srs_many_capable(const mzk_srs* srs);

}  // namespace mzk
