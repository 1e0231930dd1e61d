// mzk_sumcheck_tx.h -- the byte-level pieces of the product sum-check's proof stream (examples/sumcheck/src/prover.rs:98-247,
// algebra/fiat_shamir.rs), written once for the kernels of mzk_sumcheck.hip and for the host (mzk_sumcheck_product_layout, the header
// check of mzk_sumcheck_product_prove, and tests/hostcheck/sumcheck_tx_shim.cpp, which checks them against the Python model without a
// GPU).
//
//   header     the objects pushed before round 0 (max_degree, num_factors, num_variables, bincode of each factor), handed over by the
//              caller in stream form: per object u64 LE string count | per string u64 LE length, the bytes.
//   round j    d + 1 objects vec![bincode(s_j(c))], c = 0..=d: u64 1 | u64 length | bincode(FiniteFieldElement).
//   bincode(FiniteFieldElement) of a canonical value: sign byte (0 for zero, 1 otherwise) | u64 LE digit count | u32 LE digits with
//              no leading zero digit -- the library's restatement (tests/fri_prove_model.py: leaf), as everywhere else in the library
//              NOT pinned against a Rust vector.
#pragma once
#include "mzk_transcript.h"

namespace mzk_tx {

constexpr int SCP_MAX_FACTORS = 8, SCP_MAX_DEGREE = 8, SCP_MAX_VARS = 30;
constexpr int SCP_RECORD_MAX = 16 + 9 + 32;      // one pushed Fr value: string count, length, sign, digit count, 8 digits
enum { SCP_STATUS = 0, SCP_SUM, SCP_EVALS, SCP_CHALLENGES, SCP_FINALS, SCP_TRANSCRIPT_LEN, SCP_TRANSCRIPT, SCP_COUNT };
struct ScpLayout { u64 off[SCP_COUNT], size[SCP_COUNT], total; };

// bytes of the proof stream after the last round at most: the object count, the header, el (d + 1) records
MZK_TX_HD u64 scp_transcript_cap(u64 el, u64 d, u64 header_len) { return 8 + header_len + el * (d + 1) * (u64)SCP_RECORD_MAX; }
MZK_TX_HD void scp_layout(u64 el, u64 k, u64 d, u64 header_len, ScpLayout* L) {
  L->size[SCP_STATUS] = 8;
  L->size[SCP_SUM] = 32;
  L->size[SCP_EVALS] = 32 * el * (d + 1);
  L->size[SCP_CHALLENGES] = 32 * el;
  L->size[SCP_FINALS] = 32 * k;
  L->size[SCP_TRANSCRIPT_LEN] = 8;
  L->size[SCP_TRANSCRIPT] = scp_transcript_cap(el, d, header_len);
  u64 at = 0;
  for (int s = 0; s < SCP_COUNT; s++) {
    L->off[s] = at;
    at += (L->size[s] + 7) & ~(u64)7;
  }
  L->total = at;
}

// One pushed value: the object vec![bincode(v)] of the canonical v = w[0 .. 8) (u32 words, little-endian) at p; returns its length,
// 16 + 9 + 4 * digits.  p need not be aligned.
MZK_TX_HD int scp_digits(const uint32_t* w) {
  int k = 0;
  for (int q = 0; q < 8; q++)
    if (w[q]) k = q + 1;
  return k;
}
MZK_TX_HD size_t scp_write_record(u8* p, const uint32_t* w) {
  const int k = scp_digits(w);
  const u64 len = 9 + 4 * (u64)k;
  for (int b = 0; b < 8; b++) p[b] = b == 0 ? 1 : 0;
  for (int b = 0; b < 8; b++) p[8 + b] = (u8)(len >> (8 * b));
  p[16] = k ? 1 : 0;                                    // Sign::Plus / NoSign
  for (int b = 0; b < 8; b++) p[17 + b] = b == 0 ? (u8)k : 0;
  for (int q = 0; q < k; q++)
    for (int b = 0; b < 4; b++) p[25 + 4 * q + b] = (u8)(w[q] >> (8 * b));
  return 16 + (size_t)len;
}

// The caller's header: exactly `objects` objects over exactly `len` bytes?
MZK_TX_HD u64 scp_read_u64(const u8* p) {
  u64 v = 0;
  for (int b = 0; b < 8; b++) v |= (u64)p[b] << (8 * b);
  return v;
}
MZK_TX_HD bool scp_header_ok(const u8* h, size_t len, size_t objects) {
  size_t at = 0;
  for (size_t o = 0; o < objects; o++) {
    if (len - at < 8) return false;
    const u64 strings = scp_read_u64(h + at);
    at += 8;
    for (u64 s = 0; s < strings; s++) {
      if (len - at < 8) return false;
      const u64 bytes = scp_read_u64(h + at);
      at += 8;
      if (bytes > len - at) return false;
      at += (size_t)bytes;
    }
  }
  return at == len;
}

}  // namespace mzk_tx
