// mzk_srs.hip -- everything that touches the tables of an SRS handle (mzk_srs.h): filling a new handle, the direct and wide tables, the
// grid-batched pass against them, and what a handle reports of itself.  The decisions are mzk_srs_plan.h's.
//
// Every SRS handle gets window tables of the width msm_srs_window_bits picks for its size, unless the caller asks for
// plain prepared points (mzk_srs_from_device_ex(with_tables = 0): the one-shot pipelines).
// A handle is plain device memory: any context on the SAME GPU may commit against it (two contexts on one device
// keep two commits in flight: the latency-bound tail of one overlaps the sort / accumulate of the next).
#include "mzk_common.h"
#include "mzk_srs.h"

namespace mzk {

int srs_check_ctx(const mzk_srs* srs, bool same_context) {
  if (same_context) {
    if (srs->ctx_index != ctx().index) { set_error("SRS handle lives on context %d, the current context is %d", srs->ctx_index, ctx().index); return MZK_E_ARG; }
    return MZK_OK;
  }
  if (srs->ctx_index != ctx().index && mzk_ctx_device(srs->ctx_index) != ctx().device) {
    set_error("SRS handle lives on context %d (device %d), the current context %d drives device %d (mzk_ctx_select)", srs->ctx_index,
              mzk_ctx_device(srs->ctx_index), ctx().index, ctx().device);
    return MZK_E_ARG;
  }
  return MZK_OK;
}

// fills a freshly laid-out handle from n affine canonical points in device memory
static int srs_fill(mzk_srs* h, const void* d_plain, hipStream_t s) {
  WsFrame ws("srs_fill");
  const size_t n = h->n;
  if (n == 0) return MZK_OK;
  void* const d_own = h->own.mem.get();
  if (!h->has_tables) return msm_prepare_points(d_plain, n, d_own, (uint8_t*)d_own + n * 64, s);
  void* d_mont;
  MZK_TRY(ws.get(WS_MSM_POINTS, n * 64, &d_mont));
  MZK_TRY(msm_prepare_points(d_plain, n, d_mont, nullptr, s));
  return msm_build_tables(d_mont, n, d_own, h->own.bits * h->sets, s);     // every sets-th window: rows 2^(c sets q) P_i
}
int srs_from_points(const uint64_t* host_xy, const void* d_xy, size_t n, int with_tables, mzk_srs** out, hipStream_t s) {
  WsFrame ws("srs_from_points");
  SrsOwner h;
  MZK_TRY(srs_new(n, with_tables, &h));
  if (n) {
    if (host_xy) {
      void* d_staged;
      MZK_TRY(ws.get(WS_MISC_A, n * 64, &d_staged));
      MZK_HIP(hipMemcpyAsync(d_staged, host_xy, n * 64, hipMemcpyHostToDevice, s));
      d_xy = d_staged;
    }
    MZK_TRY(srs_fill(h.get(), d_xy, s));
    if (hipStreamSynchronize(s) != hipSuccess) return MZK_E_HIP;
  }
  *out = h.release();
  return MZK_OK;
}

bool srs_many_capable(const mzk_srs* srs) { return srs->direct.mem || (srs->has_tables && srs->sets == 1 && msm_many_supported(srs->own.bits)); }
int msm_many_srs(const mzk_srs* srs, const void* d_scalars, size_t n, size_t stride_elems, size_t count, void* d_out, hipStream_t s,
                 size_t shift) {
  if (shift && shift + n > srs->n) { set_error("msm_many: points [%zu, %zu) past the handle's %zu", shift, shift + n, srs->n); return MZK_E_LENGTH; }
  if (srs->direct.mem)      // D[(w n + i) 2^(c-1) + m]: point i's multiples are 2^(c-1) records of 64 bytes
    return msm_direct_many_dev_impl(d_scalars, n, stride_elems, count, srs->direct.mem.as<char>() + shift * ((size_t)1 << (srs->direct.bits - 1)) * 64,
                                    srs->direct.bits, srs->n, d_out, s);
  DevMem fresh;
  SrsWideStep step = srs_wide_reserve(srs, n, &fresh);
  if (step == SRS_WIDE_ALLOCATE) {       // once per handle: row 0 of its own tables are the prepared points
    MZK_TRY(msm_build_tables(srs->own.mem.get(), srs->n, fresh.get(), MANY_WIDE_BITS, s));
    srs_wide_built(srs, std::move(fresh));
    step = SRS_WIDE_USE_WIDE;
  }
  const SrsTables& t = step == SRS_WIDE_USE_WIDE ? srs->wide : srs->own;
  return msm_many_dev_impl(d_scalars, n, stride_elems, count, t.mem.as<char>() + shift * 64, t.bits, srs->n, d_out, s);
}

}  // namespace mzk

using namespace mzk;

extern "C" {

int mzk_set_table_budget(size_t bytes) { g_table_budget = bytes; return MZK_OK; }

int mzk_srs_upload(const uint64_t* powers_xy, size_t n, mzk_srs** out) {
  MZK_ENTER();
  if (!out || (!powers_xy && n)) { set_error("srs_upload: null pointer"); return MZK_E_ARG; }
  hipStream_t s = ctx().stream;
  WsGuard wsg(s);
  return srs_from_points(powers_xy, nullptr, n, 1, out, s);
}
int mzk_srs_from_device(const void* d_powers_xy, size_t n, mzk_srs** out, void* stream) {
  return mzk_srs_from_device_ex(d_powers_xy, n, 1, out, stream);
}
int mzk_srs_from_device_ex(const void* d_powers_xy, size_t n, int with_tables, mzk_srs** out, void* stream) {
  MZK_ENTER();
  WsGuard wsg((hipStream_t)stream);
  if (!out || (!d_powers_xy && n)) { set_error("srs_from_device: null pointer"); return MZK_E_ARG; }
  if (with_tables < 0 || (with_tables > 1 && (with_tables < 8 || with_tables > 22))) { set_error("srs_from_device: with_tables must be 0, 1 or a window width 8..22"); return MZK_E_ARG; }
  return srs_from_points(nullptr, d_powers_xy, n, with_tables, out, (hipStream_t)stream);
}
void mzk_srs_free(mzk_srs* srs) { delete srs; }

// Direct tables (every multiple of every window-table row) for the grid-batched commitments of short polynomials.
int mzk_srs_build_direct(mzk_srs* srs, int window_bits, size_t max_bytes, void* stream) {
  MZK_ENTER();
  WsGuard wsg((hipStream_t)stream);
  if (!srs) { set_error("srs_build_direct: null handle"); return MZK_E_ARG; }
  MZK_TRY(srs_check_ctx(srs));
  if (srs->n == 0) return MZK_OK;
  if (srs->n > MSM_DIRECT_MAX_N) { set_error("srs_build_direct: direct tables are for SRS of at most %zu points (this one has %zu)", MSM_DIRECT_MAX_N, srs->n); return MZK_E_ARG; }
  if (srs_direct_plan(srs->n, window_bits, 0).err == SRS_DIRECT_BAD_WIDTH) { set_error("srs_build_direct: window_bits must be 0 (by budget) or 8..12"); return MZK_E_ARG; }
  size_t budget = max_bytes;
  if (budget == 0) {                       // default: a quarter of what is free now, at most 4 GiB
    size_t free_b = 0, total_b = 0;
    MZK_HIP(hipMemGetInfo(&free_b, &total_b));
    budget = free_b / 4;
    if (budget > ((size_t)4 << 30)) budget = (size_t)4 << 30;
  }
  const SrsDirectPlan D = srs_direct_plan(srs->n, window_bits, budget);
  if (D.err) { set_error("srs_build_direct: %d-bit direct tables of %zu points take %zu bytes, the budget is %zu", D.bits, srs->n, D.bytes, budget); return MZK_E_ARG; }
  if (srs->direct.mem && srs->direct.bits == D.bits) return MZK_OK;
  DevMem d;
  MZK_TRY(d.alloc(D.bytes, "srs_build_direct: direct tables"));
  MZK_TRY(msm_build_direct(srs->own.mem.get(), srs->n, D.bits, d.get(), (hipStream_t)stream));
  if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess) return MZK_E_HIP;
  // the old tables may still be read by work enqueued on OTHER streams of the handle's device (the in-flight lanes of the batch
  // entry points, a caller's second stream): wait for the whole device -- srs_check_ctx above made it the current one -- before freeing
  if (srs->direct.mem) (void)hipDeviceSynchronize();
  srs->direct.attach(std::move(d), D.bits, D.bytes);
  return MZK_OK;
}
void mzk_srs_drop_direct(mzk_srs* srs) {
  mzk::EntryGuard entry;
  if (!entry.ok) return;          // another thread is inside a call that may be reading the tables
  if (!srs || !srs->direct.mem) return;
  CtxScope sc(srs->ctx_index);    // the handle's own context and device, whatever is current: synchronise THAT device
  if (!sc.ok) return;
  (void)hipDeviceSynchronize();
  srs->direct.drop();
}
int mzk_srs_window_bits(const mzk_srs* srs) { return (srs && srs->has_tables) ? srs->own.bits : 0; }
int mzk_srs_direct_bits(const mzk_srs* srs) { return (srs && srs->direct.mem) ? srs->direct.bits : 0; }
int mzk_srs_bucket_sets(const mzk_srs* srs) { return (srs && srs->has_tables) ? srs->sets : 0; }
size_t mzk_srs_table_bytes(const mzk_srs* srs) { return srs ? srs->table_bytes() : 0; }

}  // extern "C"
