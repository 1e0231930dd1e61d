// Host build of myzkp_amd/csrc/mzk_sumcheck_tx.h (TEST INFRASTRUCTURE, never shipped): the record writer, the header parser and the
// packed-proof layout of the product sum-check, checked against tests/sumcheck_product_model.py by tests/test_sumcheck_product_model.py.
#include <string.h>
#include "../../myzkp_amd/csrc/mzk_sumcheck_tx.h"
using namespace mzk_tx;

extern "C" {
// the object vec![bincode(v)] of the canonical value in 8 u32 words; out has room for SCP_RECORD_MAX bytes
size_t sctx_write_record(const uint32_t* words, u8* out) { return scp_write_record(out, words); }
int sctx_record_max(void) { return SCP_RECORD_MAX; }
int sctx_header_ok(const u8* h, size_t len, size_t objects) { return scp_header_ok(h, len, objects) ? 1 : 0; }
// off[7], size[7], total
void sctx_layout(u64 el, u64 k, u64 d, u64 header_len, u64* out) {
  ScpLayout L;
  scp_layout(el, k, d, header_len, &L);
  for (int s = 0; s < SCP_COUNT; s++) { out[s] = L.off[s]; out[SCP_COUNT + s] = L.size[s]; }
  out[2 * SCP_COUNT] = L.total;
}
}
