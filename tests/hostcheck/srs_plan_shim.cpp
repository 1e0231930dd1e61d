// myzkp_amd/csrc/mzk_srs_plan.h compiled for the host, for tests/test_srs_plan.py: every decision an SRS handle takes on the host,
// behind plain C entry points.
#include "../../myzkp_amd/csrc/mzk_srs_plan.h"

using namespace mzk;

extern "C" {

int window_bits(uint64_t n) { return msm_srs_window_bits((size_t)n); }
// the rungs srs_new tries: out[5 k ..] = tables, bits, sets, rows, bytes of rung k; returns their number
int ladder(uint64_t n, int with_tables, uint64_t budget, uint64_t* out) {
  const SrsLadder L = srs_ladder((size_t)n, with_tables, (size_t)budget);
  for (int k = 0; k < L.count; k++) {
    const SrsRung& r = L.rung[k];
    const uint64_t v[5] = {r.tables, (uint64_t)r.bits, (uint64_t)r.sets, r.rows, r.bytes};
    for (int j = 0; j < 5; j++) out[5 * k + j] = v[j];
  }
  return L.count;
}
int point_kind(int has_tables, int bits, int sets) { return srs_point_kind(has_tables != 0, bits, sets); }
uint64_t table_rows(int has_tables, int bits, int sets) { return srs_table_rows(has_tables != 0, bits, sets); }
uint64_t direct_bytes(uint64_t n, int c) { return msm_direct_bytes((size_t)n, c); }
// out = err, bits, bytes
void direct_plan(uint64_t n, int requested, uint64_t budget, uint64_t* out) {
  const SrsDirectPlan D = srs_direct_plan((size_t)n, requested, (size_t)budget);
  out[0] = (uint64_t)D.err; out[1] = (uint64_t)D.bits; out[2] = D.bytes;
}
uint64_t wide_from() { return MANY_WIDE_FROM; }
int wide_bits() { return MANY_WIDE_BITS; }
uint64_t wide_bytes(uint64_t n) { return srs_wide_bytes((size_t)n); }
int wide_step(uint64_t n_poly, int has_tables, int sets, int bits, int state, uint64_t own, uint64_t n, uint64_t budget) {
  return srs_wide_step((size_t)n_poly, has_tables != 0, sets, bits, (SrsWideState)state, (size_t)own, (size_t)n, (size_t)budget);
}
int use_stored(int with_tables, uint32_t format, uint32_t flags, uint32_t file_bits, uint32_t file_rows, uint64_t n) {
  return srs_use_stored(with_tables, format, flags, file_bits, file_rows, (size_t)n);
}

}  // extern "C"
