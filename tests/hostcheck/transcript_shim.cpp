// Host build of myzkp_amd/csrc/mzk_transcript.h (TEST INFRASTRUCTURE, never shipped): the SHAKE256 framing, Blake2b-256,
// F::sample, the packed-proof layout and the leaf records of M128 and Fr that the FRI prove kernels run, checked against hashlib and
// tests/fri_prove_model.py by tests/test_fri_transcript_model.py.
#include <string.h>
#include <vector>
#include "../../myzkp_amd/csrc/mzk_transcript.h"
using namespace mzk_tx;

// Keccak-f[1600] (FIPS 202), plain 64-bit lanes: the kernels use mzk_keccak_pair.h's lane-pair form of the same permutation
static void keccak_f(u64 (&a)[25]) {
  static const u64 RC[24] = {0x0000000000000001ULL, 0x0000000000008082ULL, 0x800000000000808aULL, 0x8000000080008000ULL, 0x000000000000808bULL,
                             0x0000000080000001ULL, 0x8000000080008081ULL, 0x8000000000008009ULL, 0x000000000000008aULL, 0x0000000000000088ULL,
                             0x0000000080008009ULL, 0x000000008000000aULL, 0x000000008000808bULL, 0x800000000000008bULL, 0x8000000000008089ULL,
                             0x8000000000008003ULL, 0x8000000000008002ULL, 0x8000000000000080ULL, 0x000000000000800aULL, 0x800000008000000aULL,
                             0x8000000080008081ULL, 0x8000000000008080ULL, 0x0000000080000001ULL, 0x8000000080008008ULL};
  static const int ROT[24] = {1, 3, 6, 10, 15, 21, 28, 36, 45, 55, 2, 14, 27, 41, 56, 8, 25, 43, 62, 18, 39, 61, 20, 44};
  static const int PI[24] = {10, 7, 11, 17, 18, 3, 5, 16, 8, 21, 24, 4, 15, 23, 19, 13, 12, 2, 20, 14, 22, 9, 6, 1};
  auto rotl = [](u64 x, int r) { return (x << r) | (x >> (64 - r)); };
  for (int r = 0; r < 24; r++) {
    u64 bc[5];
    for (int i = 0; i < 5; i++) bc[i] = a[i] ^ a[i + 5] ^ a[i + 10] ^ a[i + 15] ^ a[i + 20];
    for (int i = 0; i < 5; i++) {
      const u64 t = bc[(i + 4) % 5] ^ rotl(bc[(i + 1) % 5], 1);
      for (int j = 0; j < 25; j += 5) a[j + i] ^= t;
    }
    u64 t = a[1];
    for (int i = 0; i < 24; i++) { const int j = PI[i]; const u64 b = a[j]; a[j] = rotl(t, ROT[i]); t = b; }
    for (int j = 0; j < 25; j += 5) {
      for (int i = 0; i < 5; i++) bc[i] = a[j + i];
      for (int i = 0; i < 5; i++) a[j + i] ^= (~bc[(i + 1) % 5]) & bc[(i + 2) % 5];
    }
    a[0] ^= RC[r];
  }
}

extern "C" {
// SHAKE256(msg)[0..32) with the kernels' framing (shake_word over an 8-byte aligned copy)
void tx_shake256_32(const u8* msg, size_t len, u8* out) {
  std::vector<u64> buf(len / 8 + 2, 0);
  memcpy(buf.data(), msg, len);
  u64 a[25] = {};
  const u8* m = reinterpret_cast<const u8*>(buf.data());
  for (size_t b = 0; b < shake_blocks(len); b++) {
    for (int w = 0; w < SHAKE_RATE / 8; w++) a[w] ^= shake_word(m, len, b, w);
    keccak_f(a);
  }
  memcpy(out, a, 32);
}
void tx_blake2b256(const u8* msg, size_t len, u8* out) {
  u64 h[4];
  blake2b256(msg, len, h);
  memcpy(out, h, 32);
}
void tx_blake2b256_seed_counter(const u8* seed, u64 counter, u8* out) {
  u64 s[4], h[4];
  memcpy(s, seed, 32);
  blake2b256_seed_counter(s, counter, h);
  memcpy(out, h, 32);
}
u64 tx_sample_bytes(const u8* b, size_t len) { return sample_bytes(b, len); }
u64 tx_sample_digest_word3(u64 w3) { return sample_digest_word3(w3); }
int tx_num_rounds(u64 n, u64 e, u64 t) { return fri_num_rounds(n, e, t); }
// rounds, then off[8], size[8], total
void tx_layout(u64 n, u64 e, u64 t, int limbs, u64* out) {
  FriLayout L;
  fri_layout(n, e, t, limbs, &L);
  out[0] = (u64)L.rounds;
  for (int k = 0; k < SEC_COUNT; k++) { out[1 + k] = L.off[k]; out[9 + k] = L.size[k]; }
  out[17] = L.total;
}
// the leaf form of M128 (nw = 4) and of Fr and Fq (nw = 8): one element's record, and the whole last-codeword push
u64 tx_transcript_cap(u64 n, u64 e, u64 t, int nw) {
  FriLayout L;
  fri_layout(n, e, t, nw / 2, &L);
  return nw == 4 ? fri_transcript_cap<FriLeafLimbs<4>>(L) : fri_transcript_cap<FriLeafLimbs<8>>(L);
}
u64 tx_record_len(int nw, const uint32_t* w) { return nw == 4 ? fri_record_len<4>(w) : fri_record_len<8>(w); }
u64 tx_record_put(int nw, const uint32_t* w, int negative, u8* dst) {
  return nw == 4 ? fri_record_put<4>(w, negative != 0, dst) : fri_record_put<8>(w, negative != 0, dst);
}
// tx holds the `rounds` root records already; returns the stream's length
u64 tx_push_last(int nw, u8* tx, int rounds, const uint32_t* cw, u64 m) {
  return nw == 4 ? fri_push_last<FriLeafLimbs<4>>(tx, rounds, cw, m) : fri_push_last<FriLeafLimbs<8>>(tx, rounds, cw, m);
}
}

// The stand-alone form (built with -fsanitize=address,undefined): every record and every stream is written into a heap block of exactly
// its length, so a byte too many is a report.  Input: lines "nw rounds m <m * nw words in hex>"; per line the output is one
// "R <plus record> <minus record>" per element, then "S <stream>" with all-zero roots, in hex; then "ok <lines>".
#include <stdio.h>
static void hex(const u8* p, size_t n) { for (size_t i = 0; i < n; i++) printf("%02x", p[i]); }
int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = fopen(argv[1], "r");
  if (!f) return 2;
  int nw, rounds, lines = 0;
  unsigned long long m;
  while (fscanf(f, "%d %d %llu", &nw, &rounds, &m) == 3) {
    std::vector<uint32_t> cw(m * (size_t)nw);
    for (uint32_t& w : cw) if (fscanf(f, "%x", &w) != 1) return 3;
    u64 sum = 0;
    for (u64 j = 0; j < m; j++) {
      const uint32_t* w = cw.data() + j * nw;
      const u64 len = tx_record_len(nw, w);
      std::vector<u8> plus(len), minus(len);
      if (tx_record_put(nw, w, 0, plus.data()) != len || tx_record_put(nw, w, 1, minus.data()) != len) return 4;
      printf("R "); hex(plus.data(), len); printf(" "); hex(minus.data(), len); printf("\n");
      sum += len;
    }
    const u64 head = 8 + 48 * (u64)rounds, total = head + 8 + sum;
    std::vector<u8> tx(total, 0);
    for (int r = 0; r < rounds; r++) { tx[8 + 48 * r] = 1; tx[16 + 48 * r] = 32; }
    if (tx_push_last(nw, tx.data(), rounds, cw.data(), m) != total) return 5;
    printf("S "); hex(tx.data(), total); printf("\n");
    lines++;
  }
  fclose(f);
  printf("ok %d\n", lines);
  return 0;
}
