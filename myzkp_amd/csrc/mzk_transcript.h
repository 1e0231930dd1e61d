// mzk_transcript.h -- the byte-level pieces of FRI::prove's transcript and query sampling (zkstark/fri.rs:19-62, 86-143;
// algebra/fiat_shamir.rs), written once for the device kernels of mzk_fri.hip and for the host (mzk_fri_proof_layout, and
// tests/hostcheck/transcript_shim.cpp, which checks them against hashlib without a GPU).
//
//   proof stream      Vec<Vec<Vec<u8>>> in bincode 1.x default form: u64 LE object count | per object: u64 LE count of byte
//                     strings | per string: u64 LE length, the bytes.  Round r pushes vec![root_r] (48 bytes: 1 | 32 | root).
//   prover_fiat_shamir(32)  SHAKE256 of the whole serialization, first 32 output bytes (domain pad 0x1F, rate 136).
//   F::sample / sample_index  acc = (acc << 8) ^ b over the bytes with a wrapping usize: the LAST 8 bytes read big-endian.
//   sample_indices    Blake2b-256 (unkeyed, 12 rounds) of seed || counter as u64 LE.
//
// The Keccak permutation is not here: the kernels use the lane-pair permutation of mzk_keccak_pair.h, the host tests a plain one.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "mzk_gl.h"

#if defined(__HIPCC__)
#define MZK_TX_HD __host__ __device__ __forceinline__
#else
#define MZK_TX_HD inline
#endif

namespace mzk_tx {

typedef uint64_t u64;
typedef uint8_t u8;

constexpr int SHAKE_RATE = 136;
constexpr int PATH_STRIDE = 48;          // bytes per authentication-path entry in a packed proof (a leaf is at most 41 bytes)
constexpr int PATH_STRIDE_GL = 64;       // the same in a packed proof of mzk_fri_prove_gl (an M64X3 leaf is up to 59 bytes)
constexpr u64 SAMPLE_COUNTER_LIMIT = (u64)1 << 20;      // sample_indices gives up (status word 1) after this many counters

// ---- SHAKE256 framing ---------------------------------------------------------------------------------------------
MZK_TX_HD size_t shake_blocks(size_t len) { return len / SHAKE_RATE + 1; }
// Rate word w (0..16) of block blk of the padded message msg[0 .. len): pad10*1 with the SHAKE domain bits (0x1F ... 0x80).
// msg must be 8-byte aligned and readable up to the next multiple of 8 past len.
MZK_TX_HD u64 shake_word(const u8* msg, size_t len, size_t blk, int w) {
  const size_t off = blk * SHAKE_RATE + 8 * (size_t)w;
  u64 v = 0;
  if (off < len) {
    v = *reinterpret_cast<const u64*>(msg + off);
    if (len - off < 8) v &= ((u64)1 << (8 * (len - off))) - 1;
  }
  if (len >= off && len < off + 8) v |= (u64)0x1F << (8 * (len - off));
  if (w == SHAKE_RATE / 8 - 1 && blk + 1 == shake_blocks(len)) v |= (u64)0x80 << 56;
  return v;
}

// ---- F::sample / sample_index (field.rs:272-278, fri.rs:19-25) ---------------------------------------------------------
MZK_TX_HD u64 sample_bytes(const u8* b, size_t len) {
  u64 acc = 0;
  for (size_t i = 0; i < len; i++) acc = (acc << 8) ^ (u64)b[i];
  return acc;
}
// the same for a 32-byte digest whose last 8 bytes are the little-endian word `w3`: only they survive the shifts
MZK_TX_HD u64 sample_digest_word3(u64 w3) {
  u64 r = 0;
  for (int i = 0; i < 8; i++) r = (r << 8) | ((w3 >> (8 * i)) & 0xFF);
  return r;
}
// F::sample over Goldilocks: that accumulator taken mod p = 2^64 - 2^32 + 1 (the base value; id 4 embeds it as (v, 0, 0),
// efield.rs:180-186).  The accumulator can be >= p -- with probability 2^-32 -- and is below 2 p: one conditional subtraction.
MZK_TX_HD u64 sample_gl(u64 w3) {
  const u64 acc = sample_digest_word3(w3);
  return acc >= mzk::gl::P ? acc - mzk::gl::P : acc;
}

// ---- Blake2b-256 (RFC 7693; no key, digest length 32) -----------------------------------------------------------------
MZK_TX_HD u64 b2_rotr(u64 x, int r) { return (x >> r) | (x << (64 - r)); }
#define MZK_B2_G(a, b, c, d, x, y)   \
  a = a + b + (x); d = b2_rotr(d ^ a, 32); c = c + d; b = b2_rotr(b ^ c, 24); \
  a = a + b + (y); d = b2_rotr(d ^ a, 16); c = c + d; b = b2_rotr(b ^ c, 63);
MZK_TX_HD void blake2b_compress(u64 (&h)[8], const u64 (&m)[16], u64 t, bool last) {
  constexpr u64 IV[8] = {0x6a09e667f3bcc908ULL, 0xbb67ae8584caa73bULL, 0x3c6ef372fe94f82bULL, 0xa54ff53a5f1d36f1ULL,
                         0x510e527fade682d1ULL, 0x9b05688c2b3e6c1fULL, 0x1f83d9abfb41bd6bULL, 0x5be0cd19137e2179ULL};
  constexpr u8 S[10][16] = {{0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15}, {14, 10, 4, 8, 9, 15, 13, 6, 1, 12, 0, 2, 11, 7, 5, 3},
                            {11, 8, 12, 0, 5, 2, 15, 13, 10, 14, 3, 6, 7, 1, 9, 4}, {7, 9, 3, 1, 13, 12, 11, 14, 2, 6, 5, 10, 4, 0, 15, 8},
                            {9, 0, 5, 7, 2, 4, 10, 15, 14, 1, 11, 12, 6, 8, 3, 13}, {2, 12, 6, 10, 0, 11, 8, 3, 4, 13, 7, 5, 15, 14, 1, 9},
                            {12, 5, 1, 15, 14, 13, 4, 10, 0, 7, 6, 3, 9, 2, 8, 11}, {13, 11, 7, 14, 12, 1, 3, 9, 5, 0, 15, 4, 8, 6, 2, 10},
                            {6, 15, 14, 9, 11, 3, 0, 8, 12, 2, 13, 7, 1, 4, 10, 5}, {10, 2, 8, 4, 7, 6, 1, 5, 15, 11, 9, 14, 3, 12, 13, 0}};
  u64 v[16];
  for (int i = 0; i < 8; i++) { v[i] = h[i]; v[i + 8] = IV[i]; }
  v[12] ^= t;                     // byte counter (messages here are far below 2^64 bytes: the high word stays 0)
  if (last) v[14] = ~v[14];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int r = 0; r < 12; r++) {
    const u8* s = S[r % 10];
    MZK_B2_G(v[0], v[4], v[8], v[12], m[s[0]], m[s[1]]);
    MZK_B2_G(v[1], v[5], v[9], v[13], m[s[2]], m[s[3]]);
    MZK_B2_G(v[2], v[6], v[10], v[14], m[s[4]], m[s[5]]);
    MZK_B2_G(v[3], v[7], v[11], v[15], m[s[6]], m[s[7]]);
    MZK_B2_G(v[0], v[5], v[10], v[15], m[s[8]], m[s[9]]);
    MZK_B2_G(v[1], v[6], v[11], v[12], m[s[10]], m[s[11]]);
    MZK_B2_G(v[2], v[7], v[8], v[13], m[s[12]], m[s[13]]);
    MZK_B2_G(v[3], v[4], v[9], v[14], m[s[14]], m[s[15]]);
  }
  for (int i = 0; i < 8; i++) h[i] ^= v[i] ^ v[i + 8];
}
#undef MZK_B2_G
MZK_TX_HD void blake2b_init256(u64 (&h)[8]) {
  constexpr u64 IV[8] = {0x6a09e667f3bcc908ULL, 0xbb67ae8584caa73bULL, 0x3c6ef372fe94f82bULL, 0xa54ff53a5f1d36f1ULL,
                         0x510e527fade682d1ULL, 0x9b05688c2b3e6c1fULL, 0x1f83d9abfb41bd6bULL, 0x5be0cd19137e2179ULL};
  for (int i = 0; i < 8; i++) h[i] = IV[i];
  h[0] ^= 0x01010000ULL ^ 32;     // parameter block: digest length 32, key length 0, fanout 1, depth 1
}
// digest words 0..3 (little-endian: byte 8i + j of the digest is byte j of out[i]) of Blake2b-256(msg[0 .. len))
MZK_TX_HD void blake2b256(const u8* msg, size_t len, u64 (&out)[4]) {
  u64 h[8];
  blake2b_init256(h);
  const size_t blocks = len ? (len + 127) / 128 : 1;
  for (size_t b = 0; b < blocks; b++) {
    u64 m[16];
    for (int w = 0; w < 16; w++) {
      u64 v = 0;
      for (int j = 0; j < 8; j++) {
        const size_t i = b * 128 + 8 * (size_t)w + j;
        if (i < len) v |= (u64)msg[i] << (8 * j);
      }
      m[w] = v;
    }
    const bool last = b + 1 == blocks;
    blake2b_compress(h, m, last ? (u64)len : (u64)(b + 1) * 128, last);
  }
  for (int i = 0; i < 4; i++) out[i] = h[i];
}
// the sampler's message: seed (32 bytes, words s[0..3]) || counter as u64 LE -- one block of 40 bytes
MZK_TX_HD void blake2b256_seed_counter(const u64 (&s)[4], u64 counter, u64 (&out)[4]) {
  u64 h[8], m[16];
  blake2b_init256(h);
  for (int w = 0; w < 16; w++) m[w] = w < 4 ? s[w] : (w == 4 ? counter : 0);
  blake2b_compress(h, m, 40, true);
  for (int i = 0; i < 4; i++) out[i] = h[i];
}

// ---- FRI::num_rounds (fri.rs:86-97) and the packed proof of mzk_fri_prove ---------------------------------------------
MZK_TX_HD int fri_num_rounds(u64 n, u64 expansion_factor, u64 tests) {
  int r = 0;
  while (n > expansion_factor && tests <= (n - 1) / 4) {     // 4 * tests < n, without the overflow
    n /= 2;
    r++;
  }
  return r;
}
enum { SEC_STATUS = 0, SEC_TOP_INDICES, SEC_ROOTS, SEC_LAST_CODEWORD, SEC_VALUES, SEC_SIGNS, SEC_PATHS, SEC_PATH_LENS, SEC_COUNT };
struct FriLayout {
  int rounds;
  u64 tests, last_len, entries;       // entries: authentication-path entries of all layers
  u64 off[SEC_COUNT], size[SEC_COUNT], total;
};
MZK_TX_HD int log2_pow2(u64 n) {
  int d = 0;
  while (((u64)1 << d) < n) d++;
  return d;
}
// first path entry of (layer i, kind 0/1/2 = a/b/c) in the paths section: layer i holds T paths of depth d_i for a, as many for b,
// then T paths of depth d_(i+1) for c (d_r = log2 of round r's codeword length)
MZK_TX_HD u64 fri_entry_base(u64 n, u64 tests, int layer, int kind) {
  u64 e = 0;
  for (int i = 0; i < layer; i++) e += tests * (2 * (u64)log2_pow2(n >> i) + (u64)log2_pow2(n >> (i + 1)));
  const u64 di = (u64)log2_pow2(n >> layer);
  return e + (u64)kind * tests * di;
}
// n a power of two, rounds >= 2 and tests <= the last codeword's length (the caller checks); limbs = 2 (M128) or 4 (Fr) with
// PATH_STRIDE, 1 (M64) or 3 (M64X3) with PATH_STRIDE_GL
MZK_TX_HD void fri_layout_stride(u64 n, u64 expansion_factor, u64 tests, int limbs, int stride, FriLayout* L) {
  L->rounds = fri_num_rounds(n, expansion_factor, tests);
  L->tests = tests;
  L->last_len = L->rounds > 0 ? n >> (L->rounds - 1) : n;
  const u64 layers = L->rounds > 0 ? (u64)(L->rounds - 1) : 0;
  L->entries = layers ? fri_entry_base(n, tests, (int)layers, 0) : 0;
  L->size[SEC_STATUS] = 8;
  L->size[SEC_TOP_INDICES] = 8 * tests;
  L->size[SEC_ROOTS] = 32 * (u64)L->rounds;
  L->size[SEC_LAST_CODEWORD] = 8 * (u64)limbs * L->last_len;
  L->size[SEC_VALUES] = 8 * (u64)limbs * 3 * tests * layers;
  L->size[SEC_SIGNS] = 3 * tests * layers;
  L->size[SEC_PATHS] = (u64)stride * L->entries;
  L->size[SEC_PATH_LENS] = 8 * L->entries;
  u64 at = 0;
  for (int s = 0; s < SEC_COUNT; s++) {
    L->off[s] = at;
    at += (L->size[s] + 7) & ~(u64)7;
  }
  L->total = at;
}
MZK_TX_HD void fri_layout(u64 n, u64 expansion_factor, u64 tests, int limbs, FriLayout* L) { fri_layout_stride(n, expansion_factor, tests, limbs, PATH_STRIDE, L); }
// the packed proof of mzk_fri_prove_gl: the same sections, nc = 1 or 3 words per element, 64-byte path entries, signs all zero
MZK_TX_HD void fri_layout_gl(u64 n, u64 expansion_factor, u64 tests, int nc, FriLayout* L) { fri_layout_stride(n, expansion_factor, tests, nc, PATH_STRIDE_GL, L); }

// ---- the leaf of one codeword element: bincode(FiniteFieldElement) ----------------------------------------------------------
// The proof stream holds a leaf as a record (u64 LE length | leaf), an authentication path holds the sibling's leaf bare.
// Fr, Fq (NW = 8) and M128 (NW = 4): a magnitude of NW 32-bit words w and its Sign::Minus flag.  The leaf is the sign byte | u64 LE k |
// the first k words, k = the index past the last non-zero word; the sign byte is 0 (NoSign) when k = 0, else 0xff if negative, else 1.
template <int NW> MZK_TX_HD int fri_leaf_digits(const uint32_t* w) {
  int k = 0;
  for (int q = 0; q < NW; q++) if (w[q]) k = q + 1;
  return k;
}
// writes the leaf at dst (any alignment) and returns its length, 9 .. 9 + 4 NW
template <int NW> MZK_TX_HD u64 fri_leaf_put(const uint32_t* w, bool negative, u8* dst) {
  const int k = fri_leaf_digits<NW>(w);
  dst[0] = k ? (negative ? 0xff : 1) : 0;
  for (int b = 0; b < 8; b++) dst[1 + b] = b == 0 ? (u8)k : 0;
  for (int q = 0; q < NW; q++)
    if (q < k)
      for (int b = 0; b < 4; b++) dst[9 + 4 * q + b] = (u8)(w[q] >> (8 * b));
  return 9 + 4 * (u64)k;
}
// bytes of the element's record (length word included), and the record itself at dst (any alignment; returns its length)
template <int NW> MZK_TX_HD u64 fri_record_len(const uint32_t* w) { return 8 + 9 + 4 * (u64)fri_leaf_digits<NW>(w); }
template <int NW> MZK_TX_HD u64 fri_record_put(const uint32_t* w, bool negative, u8* dst) {
  const u64 len = fri_leaf_put<NW>(w, negative, dst + 8);
  for (int b = 0; b < 8; b++) dst[b] = (u8)(len >> (8 * b));
  return 8 + len;
}
// M64 (NC = 1) and M64X3 (NC = 3): gl::leaf_bytes<NC> of NC canonical words, 9 .. 17 bytes for M64, 8 .. 59 (nested) for M64X3; no signs.
template <int NC> MZK_TX_HD u64 fri_gl_record_len(const u64* c) { return 8 + (u64)mzk::gl::leaf_bytes<NC>(c, 0, [](int, uint32_t) {}); }
template <int NC> MZK_TX_HD u64 fri_gl_record_put(const u64* c, u8* dst) {
  const u64 len = (u64)mzk::gl::leaf_bytes<NC>(c, 8, [&](int pos, uint32_t byte) { dst[pos] = (u8)byte; }) - 8;
  for (int b = 0; b < 8; b++) dst[b] = (u8)(len >> (8 * b));
  return 8 + len;
}

// The two families under one set of names, for the kernels of mzk_fri.hip and their host checks: an element is WORDS words of type
// `word`, a path entry a zero-padded slot of STRIDE bytes, RECORD_MAX the longest record, and GL says that F::sample reduces mod
// the Goldilocks prime (sample_gl).  `negative` is ignored by the Goldilocks form.
template <int NW> struct FriLeafLimbs {
  typedef uint32_t word;
  static constexpr int WORDS = NW, STRIDE = PATH_STRIDE, RECORD_MAX = 8 + 9 + 4 * NW;
  static constexpr bool GL = false;
  static MZK_TX_HD u64 record_len(const word* w) { return fri_record_len<NW>(w); }
  static MZK_TX_HD u64 record_put(const word* w, bool negative, u8* dst) { return fri_record_put<NW>(w, negative, dst); }
  static MZK_TX_HD u64 leaf_put(const word* w, bool negative, u8* dst) { return fri_leaf_put<NW>(w, negative, dst); }
};
template <int NC> struct FriLeafGl {
  typedef u64 word;
  static constexpr int WORDS = NC, STRIDE = PATH_STRIDE_GL, RECORD_MAX = 8 + (NC == 1 ? mzk::gl::LEAF_MAX_BASE : mzk::gl::LEAF_MAX_EXT);
  static constexpr bool GL = true;
  static MZK_TX_HD u64 record_len(const word* c) { return fri_gl_record_len<NC>(c); }
  static MZK_TX_HD u64 record_put(const word* c, bool, u8* dst) { return fri_gl_record_put<NC>(c, dst); }
  static MZK_TX_HD u64 leaf_put(const word* c, bool, u8* dst) {
    return (u64)mzk::gl::leaf_bytes<NC>(c, 0, [&](int pos, uint32_t byte) { dst[pos] = (u8)byte; });
  }
};

// bytes of the proof stream after the last push: count | one record per root | the last codeword as one object of `last_len` records
template <class LEAF> MZK_TX_HD u64 fri_transcript_cap(const FriLayout& L) { return 8 + 48 * (u64)L.rounds + 8 + L.last_len * (u64)LEAF::RECORD_MAX; }
// The whole push, one record after the other: behind the `rounds` root records of tx the object's string count m, then the records
// of the (canonical, unsigned) elements; the object count becomes rounds + 1.  Returns the stream's length.  (k_fri_tx_last places
// the same records by a prefix sum over record_len, a workgroup's worth at a time; this serial form is the host's, and the check of
// both record functions.)
template <class LEAF> MZK_TX_HD u64 fri_push_last(u8* tx, int rounds, const typename LEAF::word* cw, u64 m) {
  u64 at = 8 + 48 * (u64)rounds;
  for (int b = 0; b < 8; b++) { tx[b] = (u8)(((u64)rounds + 1) >> (8 * b)); tx[at + b] = (u8)(m >> (8 * b)); }
  at += 8;
  for (u64 j = 0; j < m; j++) at += LEAF::record_put(cw + j * LEAF::WORDS, false, tx + at);
  return at;
}
// the two above by a coefficient count, as the host check of the Goldilocks ids (tests/hostcheck/transcript_gl_shim.cpp) names them
MZK_TX_HD u64 fri_transcript_cap_gl(const FriLayout& L, int nc) { return nc == 1 ? fri_transcript_cap<FriLeafGl<1>>(L) : fri_transcript_cap<FriLeafGl<3>>(L); }
template <int NC> MZK_TX_HD u64 fri_gl_push_last(u8* tx, int rounds, const u64* cw, u64 m) { return fri_push_last<FriLeafGl<NC>>(tx, rounds, cw, m); }

}  // namespace mzk_tx
