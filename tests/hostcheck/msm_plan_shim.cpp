// C entry points over myzkp_amd/csrc/mzk_msm_plan.h for tests/test_msm_plan.py: the MSM's host-side plan, compiled for the host alone.
#include "../../myzkp_amd/csrc/mzk_msm_plan.h"

using namespace mzk;

#define PLAN_FIELDS(X)                                                                                                           \
  X(err, P.err) X(path, (int)P.path) X(c, P.L.c) X(nwin, P.L.nwin) X(sets, P.L.sets) X(NB, P.NB) X(NBtot, P.NBtot)                \
  X(one_set, P.one_set) X(red_windows, P.red_windows) X(horner_c, P.horner_c) X(cl, P.cl) X(F, P.F) X(S, P.S) X(compact, P.compact) \
  X(coarse_c, P.coarse_c) X(staged, P.scatter_staged) X(seg, P.seg) X(T, P.T)                                                     \
  X(own_E, P.own.E) X(own_T, P.own.T) X(own_n_coarse, P.own.n_coarse) X(own_n_fine, P.own.n_fine)                                 \
  X(alloc_E, P.alloc.E) X(alloc_T, P.alloc.T) X(alloc_n_coarse, P.alloc.n_coarse) X(alloc_n_fine, P.alloc.n_fine)                \
  X(ws_points, P.ws.points) X(ws_counts, P.ws.counts) X(ws_offsets, P.ws.offsets) X(ws_cursor, P.ws.cursor)                      \
  X(ws_entries, P.ws.entries) X(ws_buckets, P.ws.buckets) X(ws_scan, P.ws.scan) X(ws_slots, P.ws.slots)                           \
  X(ws_wghist, P.ws.wghist) X(ws_out, P.ws.out)                                                                                   \
  X(used_points, P.ws_used.points) X(used_counts, P.ws_used.counts) X(used_offsets, P.ws_used.offsets)                             \
  X(used_cursor, P.ws_used.cursor) X(used_entries, P.ws_used.entries) X(used_buckets, P.ws_used.buckets)                          \
  X(used_scan, P.ws_used.scan) X(used_slots, P.ws_used.slots) X(used_wghist, P.ws_used.wghist) X(used_out, P.ws_used.out)

extern "C" {
const char* plan_fields() {
#define NAME(f, e) #f " "
  return PLAN_FIELDS(NAME);
#undef NAME
}
// the default knobs (the shipped library's)
int plan(uint64_t n, uint64_t n_shape, uint64_t n_alloc, int point_kind, uint64_t table_stride, int num_cu, int chunks, uint64_t* out) {
  const MsmPlan P = msm_plan(n, n_shape, n_alloc, point_kind, table_stride, num_cu, chunks, MsmKnobs());
  int i = 0;
#define PUT(f, e) out[i++] = (uint64_t)(e);
  PLAN_FIELDS(PUT)
#undef PUT
  return i;
}
int chunkable(uint64_t n_total, int point_kind, uint64_t table_stride) { return msm_chunkable(n_total, point_kind, table_stride, MsmKnobs()); }
}
