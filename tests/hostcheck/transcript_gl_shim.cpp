// Host build of the Goldilocks pieces of myzkp_amd/csrc/mzk_transcript.h (TEST INFRASTRUCTURE, never shipped): F::sample mod p, the
// packed-proof layout of mzk_fri_prove_gl, the transcript capacity and the last-codeword writer that k_fri_tx_last places its
// records with, checked against tests/goldilocks_model.py and tests/fri_prove_model.py by tests/test_fri_prove_gl_model.py.
#include "../../myzkp_amd/csrc/mzk_transcript.h"
using namespace mzk_tx;

extern "C" {
u64 txg_sample_gl(u64 w3) { return sample_gl(w3); }
// rounds, then off[8], size[8], total
void txg_layout(u64 n, u64 e, u64 t, int nc, u64* out) {
  FriLayout L;
  fri_layout_gl(n, e, t, nc, &L);
  out[0] = (u64)L.rounds;
  for (int k = 0; k < SEC_COUNT; k++) { out[1 + k] = L.off[k]; out[9 + k] = L.size[k]; }
  out[17] = L.total;
}
u64 txg_transcript_cap(u64 n, u64 e, u64 t, int nc) {
  FriLayout L;
  fri_layout_gl(n, e, t, nc, &L);
  return fri_transcript_cap_gl(L, nc);
}
u64 txg_record_len(int nc, const u64* c) { return nc == 1 ? fri_gl_record_len<1>(c) : fri_gl_record_len<3>(c); }
// tx holds the `rounds` root records already; returns the stream's length
u64 txg_push_last(int nc, u8* tx, int rounds, const u64* cw, u64 m) {
  return nc == 1 ? fri_gl_push_last<1>(tx, rounds, cw, m) : fri_gl_push_last<3>(tx, rounds, cw, m);
}
}
