// Host build of myzkp_amd/csrc/mzk_transcript.h (TEST INFRASTRUCTURE, never shipped): the SHAKE256 framing, Blake2b-256,
// F::sample and the packed-proof layout that the FRI prove kernels run, checked against hashlib by tests/test_fri_transcript_model.py.
#include <string.h>
#include <vector>
#include "../../myzkp_amd/csrc/mzk_transcript.h"
using namespace mzk_tx;

// Keccak-f[1600] (FIPS 202), plain 64-bit lanes: the kernels use mzk_merkle.hip's lane-pair form of the same permutation
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
}
