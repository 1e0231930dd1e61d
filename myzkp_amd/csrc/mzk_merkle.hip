// mzk_merkle.hip -- SHA3-256 Merkle trees over FRI / STARK codewords, device-resident.
//
// Replaces Merkle::commit / Merkle::open (merkle.rs:15-46) as the provers call them: leaves are
// bincode(FiniteFieldElement) of each codeword element (fri.rs:160-166, fast_stark.rs:64-68) and are NOT hashed
// themselves -- a one-leaf tree commits to the leaf bytes (merkle.rs:17-19), so a level-1 node is
// SHA3(leaf_2i || leaf_2i+1) and every node above is SHA3(left32 || right32).  The leaf bytes are produced on
// the fly from the canonical element (layout: see oracle/mzk_oracle_merkle.c header; unpinned third-party format).
//
// Work shape: n/2 + n/4 + ... one-block Keccak-f[1600] permutations (each message fits the 136-byte rate), pure
// 64-bit logic ops -- ALU-bound, ~5k VALU ops per hash; algorithmic HBM traffic is S*n bytes in, 32*(n-1) out.
#include <algorithm>
#include <atomic>
#include "mzk_common.h"
#include "mzk_keccak_pair.h"
#include "mzk_gl.h"
#include "mzk_merkle_plan.h"      // the level schedule and its thresholds (LEAF_PAIR_MAX, LEVEL_PAIR_MAX, TAIL_NODES)

namespace mzk {

typedef uint64_t u64;
typedef uint8_t u8;

template <int R> __device__ __forceinline__ u64 rotl64(u64 x) {
  if constexpr (R == 0) return x;
  else return (x << R) | (x >> (64 - R));
}
__constant__ u64 KECCAK_RC[24] = {
    0x0000000000000001ULL, 0x0000000000008082ULL, 0x800000000000808aULL, 0x8000000080008000ULL, 0x000000000000808bULL,
    0x0000000080000001ULL, 0x8000000080008081ULL, 0x8000000000008009ULL, 0x000000000000008aULL, 0x0000000000000088ULL,
    0x0000000080008009ULL, 0x000000008000000aULL, 0x000000008000808bULL, 0x800000000000008bULL, 0x8000000000008089ULL,
    0x8000000000008003ULL, 0x8000000000008002ULL, 0x8000000000000080ULL, 0x000000000000800aULL, 0x800000008000000aULL,
    0x8000000080008081ULL, 0x8000000000008080ULL, 0x0000000080000001ULL, 0x8000000080008008ULL};

// Keccak-f[1600], FIPS 202 section 3.2/3.3: theta, rho+pi (fused with the theta xor), chi, iota; lane (x, y) = a[x + 5y].
// The 64-bit lanes are handled as explicit 32-bit halves: a rotation is then two v_alignbit_b32 (hipcc turns a 64-bit
// rotate into two 64-bit shifts and an or) and chi's a ^ (~b & c) one v_bitop3_b32 per half (instead of v_bfi + v_xor):
// with the column parities as two three-input xors (v_bitop3_b32 again) 190 instructions per round instead of ~330 -- the tree's upper levels are one hash per lane on a nearly empty GPU,
// i.e. pure instruction latency.
struct KW { u32 lo, hi; };
__device__ __forceinline__ KW kw_xor(KW a, KW b) { return KW{a.lo ^ b.lo, a.hi ^ b.hi}; }
template <int R> __device__ __forceinline__ KW kw_rot(KW x) {
  if constexpr (R == 0) return x;
  else if constexpr (R == 32) return KW{x.hi, x.lo};
  else if constexpr (R < 32) return KW{__builtin_amdgcn_alignbit(x.lo, x.hi, 32 - R), __builtin_amdgcn_alignbit(x.hi, x.lo, 32 - R)};
  else return KW{__builtin_amdgcn_alignbit(x.hi, x.lo, 64 - R), __builtin_amdgcn_alignbit(x.lo, x.hi, 64 - R)};
}
__device__ __forceinline__ KW kw_chi(KW a, KW b, KW c) { return KW{a.lo ^ (~b.lo & c.lo), a.hi ^ (~b.hi & c.hi)}; }
// a ^ b ^ c as one v_bitop3_b32 (truth table 0x96) per half: the five-lane column parities of theta in two steps
__device__ __forceinline__ KW kw_xor3(KW a, KW b, KW c) {
  return KW{(u32)__builtin_amdgcn_bitop3_b32((int)a.lo, (int)b.lo, (int)c.lo, 0x96), (u32)__builtin_amdgcn_bitop3_b32((int)a.hi, (int)b.hi, (int)c.hi, 0x96)};
}
__device__ __forceinline__ void keccak_f(u64 (&st)[25]) {
  KW a[25];
#pragma unroll
  for (int i = 0; i < 25; i++) a[i] = KW{(u32)st[i], (u32)(st[i] >> 32)};
#pragma unroll 1
  for (int rnd = 0; rnd < 24; rnd++) {
    const KW c0 = kw_xor3(kw_xor3(a[0], a[5], a[10]), a[15], a[20]);
    const KW c1 = kw_xor3(kw_xor3(a[1], a[6], a[11]), a[16], a[21]);
    const KW c2 = kw_xor3(kw_xor3(a[2], a[7], a[12]), a[17], a[22]);
    const KW c3 = kw_xor3(kw_xor3(a[3], a[8], a[13]), a[18], a[23]);
    const KW c4 = kw_xor3(kw_xor3(a[4], a[9], a[14]), a[19], a[24]);
    const KW d0 = kw_xor(c4, kw_rot<1>(c1)), d1 = kw_xor(c0, kw_rot<1>(c2)), d2 = kw_xor(c1, kw_rot<1>(c3));
    const KW d3 = kw_xor(c2, kw_rot<1>(c4)), d4 = kw_xor(c3, kw_rot<1>(c0));
    const KW b0 = kw_rot<0>(kw_xor(a[0], d0)), b16 = kw_rot<36>(kw_xor(a[5], d0)), b7 = kw_rot<3>(kw_xor(a[10], d0));
    const KW b23 = kw_rot<41>(kw_xor(a[15], d0)), b14 = kw_rot<18>(kw_xor(a[20], d0));
    const KW b10 = kw_rot<1>(kw_xor(a[1], d1)), b1 = kw_rot<44>(kw_xor(a[6], d1)), b17 = kw_rot<10>(kw_xor(a[11], d1));
    const KW b8 = kw_rot<45>(kw_xor(a[16], d1)), b24 = kw_rot<2>(kw_xor(a[21], d1));
    const KW b20 = kw_rot<62>(kw_xor(a[2], d2)), b11 = kw_rot<6>(kw_xor(a[7], d2)), b2 = kw_rot<43>(kw_xor(a[12], d2));
    const KW b18 = kw_rot<15>(kw_xor(a[17], d2)), b9 = kw_rot<61>(kw_xor(a[22], d2));
    const KW b5 = kw_rot<28>(kw_xor(a[3], d3)), b21 = kw_rot<55>(kw_xor(a[8], d3)), b12 = kw_rot<25>(kw_xor(a[13], d3));
    const KW b3 = kw_rot<21>(kw_xor(a[18], d3)), b19 = kw_rot<56>(kw_xor(a[23], d3));
    const KW b15 = kw_rot<27>(kw_xor(a[4], d4)), b6 = kw_rot<20>(kw_xor(a[9], d4)), b22 = kw_rot<39>(kw_xor(a[14], d4));
    const KW b13 = kw_rot<8>(kw_xor(a[19], d4)), b4 = kw_rot<14>(kw_xor(a[24], d4));
    a[0] = kw_chi(b0, b1, b2); a[1] = kw_chi(b1, b2, b3); a[2] = kw_chi(b2, b3, b4); a[3] = kw_chi(b3, b4, b0); a[4] = kw_chi(b4, b0, b1);
    a[5] = kw_chi(b5, b6, b7); a[6] = kw_chi(b6, b7, b8); a[7] = kw_chi(b7, b8, b9); a[8] = kw_chi(b8, b9, b5); a[9] = kw_chi(b9, b5, b6);
    a[10] = kw_chi(b10, b11, b12); a[11] = kw_chi(b11, b12, b13); a[12] = kw_chi(b12, b13, b14); a[13] = kw_chi(b13, b14, b10); a[14] = kw_chi(b14, b10, b11);
    a[15] = kw_chi(b15, b16, b17); a[16] = kw_chi(b16, b17, b18); a[17] = kw_chi(b17, b18, b19); a[18] = kw_chi(b18, b19, b15); a[19] = kw_chi(b19, b15, b16);
    a[20] = kw_chi(b20, b21, b22); a[21] = kw_chi(b21, b22, b23); a[22] = kw_chi(b22, b23, b24); a[23] = kw_chi(b23, b24, b20); a[24] = kw_chi(b24, b20, b21);
    const u64 rc = KECCAK_RC[rnd];
    a[0].lo ^= (u32)rc;
    a[0].hi ^= (u32)(rc >> 32);
  }
#pragma unroll
  for (int i = 0; i < 25; i++) st[i] = ((u64)a[i].hi << 32) | a[i].lo;
}

// hash of two child digests by a lane pair: lane `parity` reads and writes its halves of the 64-bit words
__device__ __forceinline__ void sha3_of_two_digests_pair(const u64* __restrict__ children, u64* __restrict__ out, int parity) {
  u32 a[25];
  const u32* c32 = reinterpret_cast<const u32*>(children);
#pragma unroll
  for (int i = 0; i < 8; i++) a[i] = c32[2 * i + parity];
  a[8] = parity ? 0u : 0x06u;
#pragma unroll
  for (int i = 9; i < 25; i++) a[i] = 0;
  a[16] = parity ? 0x80000000u : 0u;
  keccak_f_pair(a, parity);
  u32* o32 = reinterpret_cast<u32*>(out);
#pragma unroll
  for (int i = 0; i < 4; i++) o32[2 * i + parity] = a[i];
}

constexpr int SHA3_RATE = 136;

// hash of one 64-byte message (two child digests): a[0..7] = data, pad 0x06 at byte 64, 0x80 at byte 135
__device__ __forceinline__ void sha3_of_two_digests(const u64* __restrict__ children, u64* __restrict__ out) {
  u64 a[25];
  const ulonglong2* c2 = reinterpret_cast<const ulonglong2*>(children);
#pragma unroll
  for (int i = 0; i < 4; i++) { ulonglong2 v = c2[i]; a[2 * i] = v.x; a[2 * i + 1] = v.y; }
  a[8] = 0x06ULL;
#pragma unroll
  for (int i = 9; i < 25; i++) a[i] = 0;
  a[16] = 0x8000000000000000ULL;
  keccak_f(a);
  ulonglong2* o2 = reinterpret_cast<ulonglong2*>(out);
  o2[0] = make_ulonglong2(a[0], a[1]);
  o2[1] = make_ulonglong2(a[2], a[3]);
}

// ---- level 1 from field elements -----------------------------------------------------------------------
// One lane per leaf pair.  The pair's message (<= 2 * (9 + 4 NW) <= 82 bytes) is serialised bytewise into a
// word-major LDS block buffer, padded, and absorbed as 17 lanes.
template <int NW>
__global__ __launch_bounds__(LEAF_THREADS) void k_merkle_leaf_pairs(const u32* __restrict__ elems, size_t pairs, u64* __restrict__ nodes,
                                                                     const u8* __restrict__ neg) {
  __shared__ u32 blk[SHA3_RATE / 4][LEAF_THREADS];
  const int tid = threadIdx.x;
  const size_t i = (size_t)blockIdx.x * LEAF_THREADS + tid;
  if (i >= pairs) return;
#pragma unroll
  for (int w = 0; w < SHA3_RATE / 4; w++) blk[w][tid] = 0;
  auto put = [&](int pos, u32 byte) { reinterpret_cast<u8*>(&blk[pos >> 2][tid])[pos & 3] = (u8)byte; };
  int pos = 0;
#pragma unroll
  for (int e = 0; e < 2; e++) {
    u32 w[NW];
    const uint4* p4 = reinterpret_cast<const uint4*>(elems + (2 * i + e) * NW);
#pragma unroll
    for (int q = 0; q < NW / 4; q++) { uint4 v = p4[q]; w[4 * q] = v.x; w[4 * q + 1] = v.y; w[4 * q + 2] = v.z; w[4 * q + 3] = v.w; }
    int k = 0;                                    // significant u32 digits (BigUint keeps no leading zero digit)
#pragma unroll
    for (int j = 0; j < NW; j++) if (w[j]) k = j + 1;
    // Sign as i8: Plus = 1, NoSign = 0, Minus = -1 (elements whose BigInt the reference left negative, field.rs:98-110;
    // `neg` is null for canonical codewords)
    put(pos, k ? ((neg && neg[2 * i + e]) ? 0xffu : 1u) : 0u);
    put(pos + 1, (u32)k);                          // sequence length as u64 LE (k <= 8: one non-zero byte)
    pos += 9;
#pragma unroll
    for (int j = 0; j < NW; j++) {
      if (j < k) {
        put(pos, w[j] & 255u); put(pos + 1, (w[j] >> 8) & 255u); put(pos + 2, (w[j] >> 16) & 255u); put(pos + 3, w[j] >> 24);
        pos += 4;
      }
    }
  }
  put(pos, 0x06u);
  reinterpret_cast<u8*>(&blk[(SHA3_RATE - 1) >> 2][tid])[3] |= 0x80u;
  u64 a[25];
#pragma unroll
  for (int l = 0; l < SHA3_RATE / 8; l++) a[l] = (u64)blk[2 * l][tid] | ((u64)blk[2 * l + 1][tid] << 32);
#pragma unroll
  for (int l = SHA3_RATE / 8; l < 25; l++) a[l] = 0;
  keccak_f(a);
  ulonglong2* o2 = reinterpret_cast<ulonglong2*>(nodes + 4 * i);
  o2[0] = make_ulonglong2(a[0], a[1]);
  o2[1] = make_ulonglong2(a[2], a[3]);
}

// The same level by lane PAIRS, for trees whose leaf level is itself latency-bound (a FRI round's codeword: at most 2^15 pairs are one
// wave per SIMD at two lanes each): lane e of a pair serialises element e of its message -- the odd lane starts behind the even lane's
// element, whose digit count it recounts --, the halves of the 17 rate words come back from LDS and the permutation is the lane-pair one
// (~127 instructions per round and lane instead of 190).  Same bytes, same digests as k_merkle_leaf_pairs.
template <int NW>
__global__ __launch_bounds__(LEAF_THREADS) void k_merkle_leaf_pairs_lp(const u32* __restrict__ elems, size_t pairs, u64* __restrict__ nodes,
                                                                        const u8* __restrict__ neg) {
  __shared__ u32 blk[SHA3_RATE / 4][LEAF_THREADS / 2];
  const int tid = threadIdx.x, col = tid >> 1, parity = tid & 1;
  const size_t i = (size_t)blockIdx.x * (LEAF_THREADS / 2) + col;
  const bool live = i < pairs;                    // pair-uniform; every lane reaches the barriers
#pragma unroll
  for (int w = parity; w < SHA3_RATE / 4; w += 2) blk[w][col] = 0;
  __syncthreads();
  if (live) {
    auto put = [&](int pos, u32 byte) { atomicOr(&blk[pos >> 2][col], (byte & 255u) << (8 * (pos & 3))); };     // the two lanes may meet in one word
    u32 w0[NW], w[NW];
    {
      const uint4* p4 = reinterpret_cast<const uint4*>(elems + (2 * i) * NW);
#pragma unroll
      for (int q = 0; q < NW / 4; q++) { uint4 v = p4[q]; w0[4 * q] = v.x; w0[4 * q + 1] = v.y; w0[4 * q + 2] = v.z; w0[4 * q + 3] = v.w; }
    }
    int k0 = 0;
#pragma unroll
    for (int j = 0; j < NW; j++) if (w0[j]) k0 = j + 1;
    if (parity) {
      const uint4* p4 = reinterpret_cast<const uint4*>(elems + (2 * i + 1) * NW);
#pragma unroll
      for (int q = 0; q < NW / 4; q++) { uint4 v = p4[q]; w[4 * q] = v.x; w[4 * q + 1] = v.y; w[4 * q + 2] = v.z; w[4 * q + 3] = v.w; }
    } else {
#pragma unroll
      for (int j = 0; j < NW; j++) w[j] = w0[j];
    }
    int k = 0;
#pragma unroll
    for (int j = 0; j < NW; j++) if (w[j]) k = j + 1;
    int pos = parity ? 9 + 4 * k0 : 0;
    put(pos, k ? ((neg && neg[2 * i + parity]) ? 0xffu : 1u) : 0u);
    put(pos + 1, (u32)k);
    pos += 9;
#pragma unroll
    for (int j = 0; j < NW; j++) {
      if (j < k) {
        put(pos, w[j] & 255u); put(pos + 1, (w[j] >> 8) & 255u); put(pos + 2, (w[j] >> 16) & 255u); put(pos + 3, w[j] >> 24);
        pos += 4;
      }
    }
    if (parity) {
      put(pos, 0x06u);
      put(SHA3_RATE - 1, 0x80u);
    }
  }
  __syncthreads();
  if (!live) return;
  u32 a[25];
#pragma unroll
  for (int l = 0; l < SHA3_RATE / 8; l++) a[l] = blk[2 * l + parity][col];
#pragma unroll
  for (int l = SHA3_RATE / 8; l < 25; l++) a[l] = 0;
  keccak_f_pair(a, parity);
  u32* o32 = reinterpret_cast<u32*>(nodes + 4 * i);
#pragma unroll
  for (int l = 0; l < 4; l++) o32[2 * l + parity] = a[l];
}

// The same level over Goldilocks elements (NC = 1: M64, 3: M64X3; leaf bytes: mzk_gl.h leaf_bytes).  A pair is at most 2 * 59 = 118 bytes:
// still one block.  One lane per leaf pair at every size.
template <int NC>
__global__ __launch_bounds__(LEAF_THREADS) void k_merkle_leaf_pairs_gl(const u64* __restrict__ elems, size_t pairs, u64* __restrict__ nodes) {
  __shared__ u32 blk[SHA3_RATE / 4][LEAF_THREADS];
  const int tid = threadIdx.x;
  const size_t i = (size_t)blockIdx.x * LEAF_THREADS + tid;
  if (i >= pairs) return;
#pragma unroll
  for (int w = 0; w < SHA3_RATE / 4; w++) blk[w][tid] = 0;
  auto put = [&](int pos, u32 byte) { reinterpret_cast<u8*>(&blk[pos >> 2][tid])[pos & 3] = (u8)byte; };
  int pos = 0;
#pragma unroll
  for (int e = 0; e < 2; e++) {
    u64 c[NC];
#pragma unroll
    for (int q = 0; q < NC; q++) c[q] = elems[(2 * i + e) * NC + q];
    pos = gl::leaf_bytes<NC>(c, pos, put);
  }
  put(pos, 0x06u);
  reinterpret_cast<u8*>(&blk[(SHA3_RATE - 1) >> 2][tid])[3] |= 0x80u;
  u64 a[25];
#pragma unroll
  for (int l = 0; l < SHA3_RATE / 8; l++) a[l] = (u64)blk[2 * l][tid] | ((u64)blk[2 * l + 1][tid] << 32);
#pragma unroll
  for (int l = SHA3_RATE / 8; l < 25; l++) a[l] = 0;
  keccak_f(a);
  ulonglong2* o2 = reinterpret_cast<ulonglong2*>(nodes + 4 * i);
  o2[0] = make_ulonglong2(a[0], a[1]);
  o2[1] = make_ulonglong2(a[2], a[3]);
}

// ---- level 1 from arbitrary byte leaves: leaf 2i || leaf 2i+1 is the contiguous range off[2i] .. off[2i+2) ---
__global__ __launch_bounds__(128) void k_merkle_leaf_pairs_bytes(const u8* __restrict__ leaves, const u64* __restrict__ off, size_t pairs,
                                                                 u64* __restrict__ nodes) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= pairs) return;
  const u8* msg = leaves + off[2 * i];
  const size_t len = (size_t)(off[2 * i + 2] - off[2 * i]);
  u64 a[25];
#pragma unroll
  for (int l = 0; l < 25; l++) a[l] = 0;
  size_t base = 0;
  for (;;) {
    const bool last = (len - base) < (size_t)SHA3_RATE;      // the padded final block
#pragma unroll
    for (int l = 0; l < SHA3_RATE / 8; l++) {
      u64 wv = 0;
#pragma unroll
      for (int t = 0; t < 8; t++) {
        const size_t idx = base + 8 * l + t;
        u64 b = idx < len ? (u64)msg[idx] : (idx == len ? 0x06ULL : 0ULL);
        wv |= b << (8 * t);
      }
      a[l] ^= wv;
    }
    if (last) a[SHA3_RATE / 8 - 1] ^= 0x8000000000000000ULL;
    keccak_f(a);
    if (last) break;
    base += SHA3_RATE;
  }
  ulonglong2* o2 = reinterpret_cast<ulonglong2*>(nodes + 4 * i);
  o2[0] = make_ulonglong2(a[0], a[1]);
  o2[1] = make_ulonglong2(a[2], a[3]);
}

// (magnitude, Sign::Minus) -> canonical representative p - magnitude, in place (magnitude 0 stays 0: BigInt has no -0)
template <int NW>
__global__ __launch_bounds__(256) void k_canonicalize_signed(u32* __restrict__ elems, const u8* __restrict__ neg, size_t n, int fid) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || !neg[i]) return;
  u32 w[NW], any = 0;
#pragma unroll
  for (int j = 0; j < NW; j++) { w[j] = elems[i * NW + j]; any |= w[j]; }
  if (!any) return;
  u32 pw[8];
  if (NW == 4) { Fe<M128Params> pm; for (int k = 0; k < M128Params::L; k++) pm.l[k] = M128Params::P[k]; fe_pack<M128Params>(pm, pw); }
  else { Fe<FrParams> pm; for (int k = 0; k < FrParams::L; k++) pm.l[k] = FrParams::P[k]; fe_pack<FrParams>(pm, pw); }
  u32 borrow = 0;
#pragma unroll
  for (int j = 0; j < NW; j++) {
    const u64 d = (u64)pw[j] - w[j] - borrow;
    elems[i * NW + j] = (u32)d;
    borrow = (u32)(d >> 32) & 1u;
  }
}
static int canonicalize_signed(int fid, void* d_elems, const void* d_neg, size_t n, hipStream_t s) {
  MZK_TRY(MZK_FIELD_LAUNCH(fid, k_canonicalize_signed<P::NW>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, (u32*)d_elems, (const u8*)d_neg, n, fid));
  MZK_HIP(hipGetLastError());
  return MZK_OK;
}

// ---- ragged leaf counts (merkle.rs:15-25 accepts any non-empty slice: mid = len / 2) ----------------------------
// The recursion splits k leaves into floor(k/2) | ceil(k/2), so at depth D = floor(log2 n) there are M = 2^D subtrees
// of one or two leaves.  Define item p = the commitment of subtree p: the leaf ITSELF (one leaf, merkle.rs:17-19) or
// hash(leaf || leaf).  Everything above depth D is a full binary tree, hence
//     Merkle::commit(n ragged leaves) == Merkle::commit(M power-of-two items),
// and the kernel below only has to produce the items (bytes, at host-computed offsets); the power-of-two byte-leaf
// path does the rest.  node_start[p] = first leaf of subtree p (node_start[M] = n).
__global__ __launch_bounds__(128) void k_merkle_ragged_items(const u8* __restrict__ leaves, const u64* __restrict__ off, const u32* __restrict__ node_start,
                                                             size_t m, const u64* __restrict__ item_off, u8* __restrict__ items) {
  const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= m) return;
  const u32 first = node_start[p], cnt = node_start[p + 1] - first;
  const u8* msg = leaves + off[first];
  const size_t len = (size_t)(off[first + cnt] - off[first]);
  u8* dst = items + item_off[p];
  if (cnt == 1) {
    for (size_t i = 0; i < len; i++) dst[i] = msg[i];
    return;
  }
  u64 a[25];
#pragma unroll
  for (int l = 0; l < 25; l++) a[l] = 0;
  size_t base = 0;
  for (;;) {
    const bool last = (len - base) < (size_t)SHA3_RATE;
#pragma unroll
    for (int l = 0; l < SHA3_RATE / 8; l++) {
      u64 wv = 0;
#pragma unroll
      for (int t = 0; t < 8; t++) {
        const size_t idx = base + 8 * l + t;
        u64 b = idx < len ? (u64)msg[idx] : (idx == len ? 0x06ULL : 0ULL);
        wv |= b << (8 * t);
      }
      a[l] ^= wv;
    }
    if (last) a[SHA3_RATE / 8 - 1] ^= 0x8000000000000000ULL;
    keccak_f(a);
    if (last) break;
    base += SHA3_RATE;
  }
  for (int q = 0; q < 4; q++)
    for (int t = 0; t < 8; t++) dst[8 * q + t] = (u8)(a[q] >> (8 * t));
}

// ---- inner levels -------------------------------------------------------------------------------------------
__global__ __launch_bounds__(128) void k_merkle_level(const u64* __restrict__ below, size_t count, u64* __restrict__ above) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  sha3_of_two_digests(below + 8 * i, above + 4 * i);
}
// small levels (latency-bound: fewer hashes than the GPU has lanes to spare): one lane PAIR per hash
__global__ __launch_bounds__(128) void k_merkle_level_pair(const u64* __restrict__ below, size_t count, u64* __restrict__ above) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t i = t >> 1;
  if (i >= count) return;                    // pair-uniform
  sha3_of_two_digests_pair(below + 8 * i, above + 4 * i, (int)(t & 1));
}
// LV consecutive small levels in one launch (round 5): a workgroup hashes 32 << LV parents from global children, then their parents from
// the digests it just left in LDS, and so on -- each level after the first costs one hash (~5 us) instead of a launch of its own (8.7 us:
// the same hash plus the dependent kernel boundary).  Every digest still goes to global memory for the authentication paths.
template <int LV>
__global__ __launch_bounds__(64 << LV) void k_merkle_level_pair_multi(const u64* __restrict__ below, size_t parents, u64* __restrict__ above) {
  constexpr int H0 = 32 << LV;
  __shared__ u32 sh[2][H0 * 8];
  const int h = threadIdx.x >> 1, parity = threadIdx.x & 1;
  size_t cnt = parents, base = (size_t)blockIdx.x * H0;
  u64* dst = above;
  int width = H0;
#pragma unroll 1
  for (int lv = 0; lv < LV; lv++) {
    if (h < width && base + h < cnt) {                 // pair-uniform
      u32 a[25];
      const u32* c32 = lv == 0 ? reinterpret_cast<const u32*>(below + 8 * (base + h)) : sh[(lv - 1) & 1] + 16 * h;
#pragma unroll
      for (int i = 0; i < 8; i++) a[i] = c32[2 * i + parity];
      a[8] = parity ? 0u : 0x06u;
#pragma unroll
      for (int i = 9; i < 25; i++) a[i] = 0;
      a[16] = parity ? 0x80000000u : 0u;
      keccak_f_pair(a, parity);
      u32* o32 = reinterpret_cast<u32*>(dst + 4 * (base + h));
      u32* l32 = sh[lv & 1] + 8 * h;
#pragma unroll
      for (int i = 0; i < 4; i++) { o32[2 * i + parity] = a[i]; l32[2 * i + parity] = a[i]; }
    }
    __syncthreads();
    dst += 4 * cnt;
    cnt >>= 1; base >>= 1; width >>= 1;
  }
}
// the last levels (<= TAIL_NODES nodes each) in one workgroup: no launch per level; one lane pair per hash
__global__ __launch_bounds__(TAIL_NODES) void k_merkle_tail(u64* __restrict__ level, size_t count, size_t stop, u32* __restrict__ mailbox, u32 seq) {
  // `level` holds `count` nodes; the levels above follow contiguously (count/2, count/4, ... stop); stop = 1 for one tree,
  // the number of trees for a batch (their roots are the last level).
  // The digests travel from level to level through LDS (ping-pong): every level is one dependent hash on an almost empty CU, and
  // reading the children back from global memory behind a fence was a ~1.5-us round trip per level on top of the ~7 us of the hash.
  // Global memory still receives every digest (the authentication paths are gathered from there) but nobody waits for it.
  __shared__ u32 sh[2][TAIL_NODES * 8];
  const int tid = threadIdx.x;
  {
    const u32* g = reinterpret_cast<const u32*>(level);
    for (size_t i = tid; i < count * 8; i += TAIL_NODES) sh[0][i] = g[i];
  }
  __syncthreads();
  u64* below = level;
  int cur = 0;
  while (count > stop) {
    const size_t up = count / 2;
    u64* above = below + 4 * count;
    const int h = tid >> 1, parity = tid & 1;
    if ((size_t)h < up) {
      u32 a[25];
      const u32* c32 = sh[cur] + 16 * h;
#pragma unroll
      for (int i = 0; i < 8; i++) a[i] = c32[2 * i + parity];
      a[8] = parity ? 0u : 0x06u;
#pragma unroll
      for (int i = 9; i < 25; i++) a[i] = 0;
      a[16] = parity ? 0x80000000u : 0u;
      keccak_f_pair(a, parity);
      u32* o32 = reinterpret_cast<u32*>(above + 4 * h);
      u32* l32 = sh[cur ^ 1] + 8 * h;
#pragma unroll
      for (int i = 0; i < 4; i++) { o32[2 * i + parity] = a[i]; l32[2 * i + parity] = a[i]; }
    }
    __syncthreads();
    below = above;
    count = up;
    cur ^= 1;
  }
  // one tree whose root the host is waiting for (a FRI round's transcript, Merkle::commit): the root goes straight into the caller's mapped
  // host buffer, then a fence, then the sequence number the host spins on -- no copy engine, no stream synchronize (merkle_root_to_host)
  if (mailbox != nullptr && tid == 0) {
#pragma unroll
    for (int i = 0; i < 8; i++) __builtin_nontemporal_store(sh[cur][i], mailbox + i);
    __threadfence_system();
    __hip_atomic_store(mailbox + 8, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}
// authentication path: node (index >> l) ^ 1 of level l, l = 1 .. depth-1; level l starts at node n - n / 2^(l-1)
__global__ void k_merkle_gather(const u64* __restrict__ nodes, size_t n, size_t index, int depth, u64* __restrict__ out) {
  const int l = 1 + blockIdx.x * blockDim.x + threadIdx.x;
  if (l >= depth) return;
  const size_t start = n - (n >> (l - 1));
  const u64* src = nodes + 4 * (start + ((index >> l) ^ 1));
#pragma unroll
  for (int q = 0; q < 4; q++) out[4 * (l - 1) + q] = src[q];
}

// many authentication paths at once (the FRI query phase opens three indices per colinearity test and round): block q
// gathers the digests of path q and the limbs of its sibling leaf
__global__ __launch_bounds__(64) void k_merkle_gather_batch(const u64* __restrict__ nodes, const u32* __restrict__ leaves, int leaf_words, size_t n,
                                                            const u64* __restrict__ indices, int depth, u64* __restrict__ out_nodes,
                                                            u32* __restrict__ out_leaves) {
  const size_t q = blockIdx.x;
  const size_t index = indices[q];
  const int l = 1 + threadIdx.x;
  if (l < depth) {
    const size_t start = n - (n >> (l - 1));
    const u64* src = nodes + 4 * (start + ((index >> l) ^ 1));
#pragma unroll
    for (int k = 0; k < 4; k++) out_nodes[(q * (size_t)(depth - 1) + (l - 1)) * 4 + k] = src[k];
  }
  if ((int)threadIdx.x < leaf_words) out_leaves[q * leaf_words + threadIdx.x] = leaves[(index ^ 1) * leaf_words + threadIdx.x];
}

// out[q] = leaves[indices[q]] (whole elements of leaf_words 32-bit words)
__global__ void k_gather_leaves(const u32* __restrict__ leaves, int leaf_words, const u64* __restrict__ indices, size_t count, u32* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count * (size_t)leaf_words) return;
  const size_t q = i / (size_t)leaf_words, w = i - q * (size_t)leaf_words;
  out[i] = leaves[indices[q] * (size_t)leaf_words + w];
}

}  // namespace mzk

using namespace mzk;

struct mzk_merkle {
  int kind;              // 0 = field elements, 1 = byte leaves
  int field;
  size_t n;
  int depth;             // log2 n
  u64* d_nodes;          // n - 1 digests: level 1 (n/2), level 2 (n/4), ..., root
  void* d_leaves;        // copy of the elements / the leaf bytes (needed by open and by n == 1)
  DevMem own_nodes, own_leaves, own_items;     // what d_nodes, d_leaves and d_items point to, where the handle owns it alone
  std::vector<uint64_t> offsets;   // byte leaves only
  std::vector<uint8_t> neg;        // field leaves given as (magnitude, sign): 1 = Sign::Minus; empty = all non-negative
  hipStream_t stream;    // the stream the tree was BUILT on (a caller stream for the *_dev builders); never used again
  // Owner: the context (and its device) whose memory holds the tree.  Every later operation enters that context, runs on
  // ITS stream and workspace (MerkleScope) behind `built`, whatever context is current and whatever became of `stream`.
  int ctx_index = 0;
  int device = -1;
  hipEvent_t built = nullptr;    // recorded behind the last kernel of the build
  // ragged leaf counts: the tree is built over m = 2^floor(log2 n) items (see k_merkle_ragged_items); d_nodes, depth
  // and the gather kernel then refer to the item tree
  // FRI::commit with the trees kept: the codewords and digests of ALL rounds live in one device allocation shared by the rounds'
  // handles (one allocation per commit instead of two per round, and no copies: a round hashes and folds in place there);
  // d_leaves / d_nodes then point into it -- but for signed round-0 leaves, a copy in own_leaves -- and the last handle freed
  // releases it.
  std::shared_ptr<DevMem> shared;
  bool ragged = false;
  size_t m = 0;
  void* d_items = nullptr;
  std::vector<uint64_t> item_off;
  std::vector<uint32_t> node_start;
};

namespace mzk {
static bool is_pow2(size_t n) { return n && !(n & (n - 1)); }

// end of a successful build on stream s of the current context
// complete_on_return: the caller synchronizes the stream before it hands the tree out (mzk_fri_commit does once, after its last round --
// since round 6 a round's root reaches the transcript through the mailbox without a synchronize; an error return frees the trees, and
// hipFree waits for the device), so there is nothing to order later calls behind: no event (one marker packet per round less)
static int merkle_stamp(mzk_merkle* t, hipStream_t s, bool complete_on_return = false) {
  t->ctx_index = ctx().index;
  t->device = ctx().device;
  if (complete_on_return) return MZK_OK;
  if (!t->built) MZK_HIP(hipEventCreateWithFlags(&t->built, hipEventDisableTiming));
  MZK_HIP(hipEventRecord(t->built, s));
  return MZK_OK;
}
// Enter the owning context of a tree for the scope of one entry point.  rc != MZK_OK: the context is gone or drives another
// device now (mzk_init_devices since the build) -- MZK_E_ARG, as srs_check_ctx reports a foreign SRS handle.
struct MerkleScope {
  CtxScope sc;
  int rc;
  hipStream_t s;
  explicit MerkleScope(const mzk_merkle* t) : sc(t->ctx_index), rc(MZK_OK), s(nullptr) {
    if (!sc.ok || ctx().device != t->device) {
      set_error("Merkle tree handle was built on context %d (device %d); that context %s", t->ctx_index, t->device,
                sc.ok ? "drives another device now" : "no longer exists");
      rc = MZK_E_ARG;
      return;
    }
    s = ctx().stream;
    if (t->built && hipStreamWaitEvent(s, t->built, 0) != hipSuccess) { (void)hipGetLastError(); rc = MZK_E_HIP; set_error("merkle: cannot order behind the build"); }
  }
};

// hashes level 1 .. root into d_nodes; d_leaves / d_off already on the device
// `trees` > 1: n = trees * (leaves per tree), all trees of one power-of-two size, leaves back to back.  Level l of the whole
// array is then level l of every tree side by side (pairs never straddle trees), so a batch is the bottom of one big tree,
// hashed down to `trees` nodes: the roots, at d_nodes + 4 * (n - 2 * trees).
// mailbox / seq: see merkle_root_to_host; *mailed = the tail ran and will post the root there
static int merkle_hash_levels(int kind, int fid, const void* d_leaves, const u64* d_off, size_t n, u64* d_nodes, hipStream_t s,
                              const u8* d_neg = nullptr, size_t trees = 1, u32* mailbox = nullptr, u32 seq = 0, bool* mailed = nullptr) {
  if (mailed) *mailed = false;
  if (n < 2) return MZK_OK;
  ProfScope ps(s, MZK_PH_MERKLE);
  static const int lp_on = tune_int("MZK_LEAF_LANE_PAIRS", 1);      // tuning build: 0 = one lane per leaf pair at every size (A/B)
  const int leaf_kind = kind == 1 ? MERKLE_LEAVES_BYTES : field_is_gl(fid) ? MERKLE_LEAVES_GL : lp_on ? MERKLE_LEAVES_FIELD : MERKLE_LEAVES_FIELD_PLAIN;
  const MerklePlan plan = merkle_plan(n, trees, leaf_kind);
  for (int i = 0; i < plan.nsteps; i++) {
    const MerkleStep& st = plan.steps[i];
    const dim3 grid((unsigned)st.grid), block(st.block);
    u64* above = d_nodes + 4 * st.out_offset;
    // inner steps: the level below ends where this step's output begins (a leaf step reads the leaves: no digests below it)
    u64* below = st.kernel >= MK_LEVEL ? above - 4 * st.nodes_in : nullptr;
    switch (st.kernel) {
      case MK_LEAF_BYTES:
        hipLaunchKernelGGL(k_merkle_leaf_pairs_bytes, grid, block, 0, s, (const u8*)d_leaves, d_off, st.parents, above);
        break;
      case MK_LEAF_GL:
        MZK_TRY(with_gl(fid, [&](auto tag) {
          hipLaunchKernelGGL((k_merkle_leaf_pairs_gl<decltype(tag)::NC>), grid, block, 0, s, (const u64*)d_leaves, st.parents, above);
          return MZK_OK;
        }));
        break;
      case MK_LEAF_LP:
        MZK_TRY(MZK_FIELD_LAUNCH(fid, k_merkle_leaf_pairs_lp<P::NW>, grid, block, 0, s, (const u32*)d_leaves, st.parents, above, d_neg));
        break;
      case MK_LEAF_PLAIN:
        MZK_TRY(MZK_FIELD_LAUNCH(fid, k_merkle_leaf_pairs<P::NW>, grid, block, 0, s, (const u32*)d_leaves, st.parents, above, d_neg));
        break;
      case MK_LEVEL:
        hipLaunchKernelGGL(k_merkle_level, grid, block, 0, s, (const u64*)below, st.parents, above);
        break;
      case MK_LEVEL_PAIR:
        hipLaunchKernelGGL(k_merkle_level_pair, grid, block, 0, s, (const u64*)below, st.parents, above);
        break;
      case MK_MULTI2:
        hipLaunchKernelGGL((k_merkle_level_pair_multi<2>), grid, block, 0, s, (const u64*)below, st.parents, above);
        break;
      case MK_MULTI3:
        hipLaunchKernelGGL((k_merkle_level_pair_multi<3>), grid, block, 0, s, (const u64*)below, st.parents, above);
        break;
      case MK_TAIL: {
        const bool mail = mailbox != nullptr && trees == 1;
        hipLaunchKernelGGL(k_merkle_tail, grid, block, 0, s, below, st.nodes_in, trees, mail ? mailbox : (u32*)nullptr, seq);
        if (mail && mailed) *mailed = true;
        break;
      }
    }
  }
  MZK_HIP(hipGetLastError());
  return MZK_OK;
}
// The root of ONE tree to the host.  The copy engine and the stream synchronize behind it cost ~15 us per FRI round; the tail kernel instead
// writes the 32 bytes and a sequence number into the context's pinned landing zone (mapped into the device's address space) and the host spins on
// the number.  Stream errors still surface: every 1024 spins the stream is queried, and when it has drained without the number showing up
// (or the tail was not part of this tree: two leaves) the root is fetched the ordinary way.  The stream is NOT synchronized on return.
struct RootMailbox { u32* p; u32 seq; };
static u32 g_mailbox_seq[MZK_MAX_CTX];        // per context: the number of the last root a tail kernel was asked to post
static int merkle_mailbox(RootMailbox* mb) {
  Context& c = ctx();
  if (!c.bounce) MZK_HIP(hipHostMalloc(&c.bounce, SMALL_D2H_MAX, hipHostMallocPortable));
  static const int enabled = tune_int("MZK_ROOT_MAILBOX", 1);     // tuning build: 0 = copy + synchronize (A/B)
  mb->p = enabled ? (u32*)c.bounce + 512 : nullptr;                 // the second half of the landing zone: d2h_sync uses the first bytes
  mb->seq = ++g_mailbox_seq[c.index];
  if (mb->seq == 0) mb->seq = ++g_mailbox_seq[c.index];
  if (mb->p) ((volatile u32*)mb->p)[8] = 0;                         // (a larger d2h_sync may have run over this half since the last root)
  return MZK_OK;
}
static int merkle_root_to_host(uint8_t* root, const u64* d_root, const RootMailbox& mb, bool mailed, hipStream_t s) {
  if (mailed && mb.p) {
    volatile u32* flag = mb.p + 8;
    for (unsigned spins = 1;; spins++) {
      if (*flag == mb.seq) { std::atomic_thread_fence(std::memory_order_acquire); memcpy(root, (const void*)mb.p, 32); return MZK_OK; }
      if ((spins & 1023) == 0) {
        const hipError_t q = hipStreamQuery(s);
        if (q == hipSuccess) { if (*flag == mb.seq) continue; break; }       // drained: the number is there or never comes
        if (q != hipErrorNotReady) return hip_fail(q, "hipStreamQuery", __FILE__, __LINE__);
      }
    }
  }
  return d2h_sync(root, d_root, 32, s);
}

// bincode(FiniteFieldElement) of ONE canonical element on the host: used for the n == 1 root and for the
// sibling leaf of an authentication path (both are a copy of input bytes, not computation).
static size_t host_bincode_field(const uint64_t* limbs, int nl, uint8_t* out, bool negative = false) {
  int k = 2 * nl;
  while (k > 0 && (uint32_t)(limbs[(k - 1) / 2] >> (32 * ((k - 1) & 1))) == 0) k--;
  out[0] = k ? (negative ? 0xff : 1) : 0;
  uint64_t len = (uint64_t)k;
  memcpy(out + 1, &len, 8);
  for (int i = 0; i < k; i++) { uint32_t d = (uint32_t)(limbs[i / 2] >> (32 * (i & 1))); memcpy(out + 9 + 4 * i, &d, 4); }
  return 9 + 4 * (size_t)k;
}

// The leaf bytes of one element of field `fid` on the host (at most HOST_LEAF_MAX: a 59-byte M64X3 leaf is the longest)
constexpr size_t HOST_LEAF_MAX = 64;
static size_t host_leaf(int fid, const uint64_t* limbs, uint8_t* out, bool negative = false) {
  if (!field_is_gl(fid)) return host_bincode_field(limbs, field_limbs64(fid), out, negative);
  auto put = [&](int pos, uint32_t byte) { out[pos] = (uint8_t)byte; };
  return (size_t)(fid == MZK_FIELD_M64X3 ? gl::leaf_bytes<3>(limbs, 0, put) : gl::leaf_bytes<1>(limbs, 0, put));
}
// canonical elements of a host array: every limb group below the modulus (Goldilocks: every word below p)
static int host_elems_canonical(int fid, const uint64_t* elems, size_t n) {
  if (field_is_gl(fid)) {
    const size_t words = n * (size_t)field_gl_comps(fid);
    for (size_t i = 0; i < words; i++)
      if (!gl::is_canonical(elems[i])) { set_error("merkle: element %zu not canonical", i / (size_t)field_gl_comps(fid)); return MZK_E_RANGE; }
    return MZK_OK;
  }
  const HostField* hf = host_field(fid);
  for (size_t i = 0; i < n; i++)
    if (!h_is_canonical(hf, elems + (size_t)hf->nl * i)) { set_error("merkle: element %zu not canonical", i); return MZK_E_RANGE; }
  return MZK_OK;
}

static int merkle_build(int kind, int fid, const void* src, bool src_on_device, size_t leaf_bytes, const uint64_t* offsets, size_t n,
                        mzk_merkle** out, hipStream_t s, const uint8_t* neg_host = nullptr);

// Any leaf count that is not a power of two (never produced by the provers, but accepted by merkle.rs:15-25).
static int merkle_build_ragged(const uint8_t* leaves, const uint64_t* offsets, size_t n, mzk_merkle** out, hipStream_t s) {
  WsFrame ws("merkle_build_ragged");
  if (n > ((size_t)1 << 31)) { set_error("merkle: ragged trees support up to 2^31 leaves"); return MZK_E_ARG; }
  mzk_merkle* t = new mzk_merkle();
  t->kind = 1; t->field = -1; t->n = n; t->stream = s; t->d_nodes = nullptr; t->d_leaves = nullptr; t->ragged = true;
  int D = 0;
  while (((size_t)2 << D) <= n) D++;
  const size_t m = (size_t)1 << D;
  t->m = m; t->depth = D;
  t->offsets.assign(offsets, offsets + n + 1);
  // subtree p at depth D: walk the bits of p from the root (0 = left = floor half, 1 = right = ceil half)
  t->node_start.resize(m + 1);
  t->item_off.resize(m + 1);
  for (size_t p = 0; p < m; p++) {
    size_t start = 0, size = n;
    for (int b = D - 1; b >= 0; b--) {
      const size_t l = size / 2;
      if ((p >> b) & 1) { start += l; size -= l; } else size = l;
    }
    t->node_start[p] = (uint32_t)start;
  }
  t->node_start[m] = (uint32_t)n;
  uint64_t io = 0;
  for (size_t p = 0; p < m; p++) {
    t->item_off[p] = io;
    const uint32_t first = t->node_start[p], cnt = t->node_start[p + 1] - first;
    io += cnt == 1 ? offsets[first + 1] - offsets[first] : 32;
  }
  t->item_off[m] = io;
  const size_t leaf_bytes = (size_t)(offsets[n] - offsets[0]);
  u64 *d_off = nullptr, *d_ioff = nullptr;
  u32* d_ns = nullptr;
  int rc = MZK_OK;
  do {
    if ((rc = t->own_leaves.alloc(leaf_bytes ? leaf_bytes : 16, "merkle: leaves")) != MZK_OK) break;
    if ((rc = t->own_items.alloc(io ? io : 16, "merkle: items")) != MZK_OK) break;
    if ((rc = t->own_nodes.alloc((m - 1) * 32, "merkle: digests")) != MZK_OK) break;
    t->d_leaves = t->own_leaves.get(); t->d_items = t->own_items.get(); t->d_nodes = t->own_nodes.as<u64>();
    if ((rc = ws.get(WS_MISC_D, (n + 1) * 8, (void**)&d_off)) != MZK_OK) break;
    if ((rc = ws.get(WS_MISC_E, (m + 1) * 8, (void**)&d_ioff)) != MZK_OK) break;
    if ((rc = ws.get(WS_MISC_F, (m + 1) * 4, (void**)&d_ns)) != MZK_OK) break;
    if ((leaf_bytes && hipMemcpyAsync(t->d_leaves, leaves, leaf_bytes, hipMemcpyHostToDevice, s) != hipSuccess) ||
        hipMemcpyAsync(d_off, offsets, (n + 1) * 8, hipMemcpyHostToDevice, s) != hipSuccess ||
        hipMemcpyAsync(d_ioff, t->item_off.data(), (m + 1) * 8, hipMemcpyHostToDevice, s) != hipSuccess ||
        hipMemcpyAsync(d_ns, t->node_start.data(), (m + 1) * 4, hipMemcpyHostToDevice, s) != hipSuccess) { set_error("merkle: copy failed"); rc = MZK_E_HIP; break; }
    hipLaunchKernelGGL(k_merkle_ragged_items, dim3((unsigned)((m + 127) / 128)), dim3(128), 0, s, (const u8*)t->d_leaves, (const u64*)d_off, (const u32*)d_ns, m,
                       (const u64*)d_ioff, (u8*)t->d_items);
    rc = merkle_hash_levels(1, -1, t->d_items, d_ioff, m, t->d_nodes, s);
    if (rc == MZK_OK && hipStreamSynchronize(s) != hipSuccess) { set_error("merkle: sync failed"); rc = MZK_E_HIP; }
    if (rc == MZK_OK) rc = merkle_stamp(t, s);
  } while (0);
  if (rc != MZK_OK) { mzk_merkle_free(t); return rc; }
  *out = t;
  return MZK_OK;
}

static int merkle_build(int kind, int fid, const void* src, bool src_on_device, size_t leaf_bytes, const uint64_t* offsets, size_t n,
                        mzk_merkle** out, hipStream_t s, const uint8_t* neg_host) {
  WsFrame ws("merkle_build");
  if (!out) { set_error("merkle: null output handle"); return MZK_E_ARG; }
  *out = nullptr;
  if (n == 0) { set_error("merkle: empty leaf set (Merkle::commit recurses forever on it, merkle.rs:20-22)"); return MZK_E_LENGTH; }
  if (!src) { set_error("merkle: null pointer"); return MZK_E_ARG; }
  if (!is_pow2(n)) {
    if (kind == 1) return merkle_build_ragged((const uint8_t*)src, offsets, n, out, s);
    // field elements: serialise bincode(FiniteFieldElement) on the host and take the byte-leaf path (not a prover path:
    // every codeword the reference commits to has a power-of-two length)
    const int nl = field_limbs64(fid);
    std::vector<uint64_t> host(n * (size_t)nl);
    if (src_on_device) {
      MZK_TRY(d2h_sync(host.data(), src, leaf_bytes, s));
    } else {
      memcpy(host.data(), src, leaf_bytes);
    }
    std::vector<uint8_t> blob(n * HOST_LEAF_MAX);
    std::vector<uint64_t> off(n + 1);
    uint64_t o = 0;
    for (size_t i = 0; i < n; i++) { off[i] = o; o += host_leaf(fid, host.data() + i * nl, blob.data() + o, neg_host && neg_host[i]); }
    off[n] = o;
    return merkle_build_ragged(blob.data(), off.data(), n, out, s);
  }
  mzk_merkle* t = new mzk_merkle();
  t->kind = kind; t->field = fid; t->n = n; t->stream = s; t->d_nodes = nullptr; t->d_leaves = nullptr;
  t->depth = 0;
  while (((size_t)1 << t->depth) < n) t->depth++;
  u64* d_off = nullptr;
  int rc = MZK_OK;
  do {
    if ((rc = t->own_leaves.alloc(leaf_bytes ? leaf_bytes : 16, "merkle: leaves")) != MZK_OK) break;
    t->d_leaves = t->own_leaves.get();
    if (leaf_bytes && hipMemcpyAsync(t->d_leaves, src, leaf_bytes, src_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s) != hipSuccess) {
      set_error("merkle: leaf copy failed"); rc = MZK_E_HIP; break;
    }
    if (n > 1 && (rc = t->own_nodes.alloc((n - 1) * 32, "merkle: digests")) != MZK_OK) break;
    t->d_nodes = t->own_nodes.as<u64>();
    if (kind == 1) {
      t->offsets.assign(offsets, offsets + n + 1);
      if ((rc = ws.get(WS_MISC_D, (n + 1) * 8, (void**)&d_off)) != MZK_OK) break;
      if (hipMemcpyAsync(d_off, offsets, (n + 1) * 8, hipMemcpyHostToDevice, s) != hipSuccess) { set_error("merkle: offset copy failed"); rc = MZK_E_HIP; break; }
    }
    u8* d_neg = nullptr;
    if (kind == 0 && neg_host) {
      t->neg.assign(neg_host, neg_host + n);
      if ((rc = ws.get(WS_MISC_E, n, (void**)&d_neg)) != MZK_OK) break;
      if (hipMemcpyAsync(d_neg, neg_host, n, hipMemcpyHostToDevice, s) != hipSuccess) { set_error("merkle: sign copy failed"); rc = MZK_E_HIP; break; }
    }
    rc = merkle_hash_levels(kind, fid, t->d_leaves, d_off, n, t->d_nodes, s, d_neg);
    if (rc == MZK_OK && kind == 1 && hipStreamSynchronize(s) != hipSuccess) { set_error("merkle: sync failed"); rc = MZK_E_HIP; }
    if (rc == MZK_OK) rc = merkle_stamp(t, s);
  } while (0);
  if (rc != MZK_OK) { mzk_merkle_free(t); return rc; }
  *out = t;
  return MZK_OK;
}
}  // namespace mzk

extern "C" {

int mzk_merkle_build_field_dev(int field_id, const void* d_elems, size_t n, mzk_merkle** out, void* stream) {
  MZK_ENTER();
  WsGuard wsg((hipStream_t)stream);
  MZK_TRY(field_check_gl(field_id, "merkle"));
  return merkle_build(0, field_id, d_elems, true, n * field_bytes(field_id), nullptr, n, out, (hipStream_t)stream);
}
// signed_form: the (magnitude, sign) calls serve Fr and M128 only
static int build_field_host(int field_id, const uint64_t* elems, const uint8_t* negative, size_t n, mzk_merkle** out, bool signed_form) {
  MZK_ENTER();
  MZK_TRY(signed_form ? field_check(field_id, "merkle") : field_check_gl(field_id, "merkle"));
  if (elems) MZK_TRY(host_elems_canonical(field_id, elems, n));
  WsGuard wsg(ctx().stream);
  MZK_TRY(merkle_build(0, field_id, elems, false, n * field_bytes(field_id), nullptr, n, out, ctx().stream, negative));
  MZK_HIP(hipStreamSynchronize(ctx().stream));
  return MZK_OK;
}
int mzk_merkle_build_field(int field_id, const uint64_t* elems, size_t n, mzk_merkle** out) { return build_field_host(field_id, elems, nullptr, n, out, false); }
int mzk_merkle_build_field_signed(int field_id, const uint64_t* magnitudes, const uint8_t* negative, size_t n, mzk_merkle** out) {
  return build_field_host(field_id, magnitudes, negative, n, out, true);
}
int mzk_merkle_commit_field_signed(int field_id, const uint64_t* magnitudes, const uint8_t* negative, size_t n, uint8_t* root, size_t cap,
                                   size_t* root_len) {
  mzk_merkle* t = nullptr;
  MZK_TRY(build_field_host(field_id, magnitudes, negative, n, &t, true));
  const int rc = mzk_merkle_root(t, root, cap, root_len);
  mzk_merkle_free(t);
  return rc;
}
int mzk_merkle_build_bytes(const uint8_t* leaves, const uint64_t* offsets, size_t n, mzk_merkle** out) {
  MZK_ENTER();
  if (!offsets) { set_error("merkle: null offsets"); return MZK_E_ARG; }
  for (size_t i = 0; i < n; i++)
    if (offsets[i + 1] < offsets[i]) { set_error("merkle: offsets must be non-decreasing"); return MZK_E_ARG; }
  const size_t total = n ? (size_t)(offsets[n] - offsets[0]) : 0;
  uint8_t dummy = 0;
  if (!leaves) { if (total) { set_error("merkle: null pointer"); return MZK_E_ARG; } leaves = &dummy; }
  // offsets are rebased to the copied range
  std::vector<uint64_t> off(n + 1);
  for (size_t i = 0; i <= n; i++) off[i] = offsets[i] - offsets[0];
  WsGuard wsg(ctx().stream);
  return merkle_build(1, -1, leaves + offsets[0], false, total, off.data(), n, out, ctx().stream);
}

int mzk_merkle_root(const mzk_merkle* t, uint8_t* root, size_t cap, size_t* root_len) {
  if (!t || !root || !root_len) { set_error("merkle_root: null pointer"); return MZK_E_ARG; }
  MZK_ENTER();
  MerkleScope ms(t);
  MZK_TRY(ms.rc);
  if (t->n == 1) {   // merkle.rs:17-19: the single leaf itself
    uint8_t buf[HOST_LEAF_MAX];
    size_t len;
    if (t->kind == 0) {
      uint64_t limbs[4];
      MZK_TRY(d2h_sync(limbs, t->d_leaves, field_bytes(t->field), ms.s));
      len = host_leaf(t->field, limbs, buf, !t->neg.empty() && t->neg[0]);
      if (cap < len) { set_error("merkle_root: buffer too small (%zu < %zu)", cap, len); return MZK_E_LENGTH; }
      memcpy(root, buf, len);
    } else {
      len = (size_t)(t->offsets[1] - t->offsets[0]);
      if (cap < len) { set_error("merkle_root: buffer too small (%zu < %zu)", cap, len); return MZK_E_LENGTH; }
      MZK_TRY(d2h_sync(root, t->d_leaves, len, ms.s));
    }
    *root_len = len;
    return MZK_OK;
  }
  if (cap < 32) { set_error("merkle_root: buffer too small"); return MZK_E_LENGTH; }
  MZK_TRY(d2h_sync(root, t->d_nodes + 4 * ((t->ragged ? t->m : t->n) - 2), 32, ms.s));
  *root_len = 32;
  return MZK_OK;
}

int mzk_merkle_open_batch(const mzk_merkle* t, const uint64_t* indices, size_t count, uint8_t* paths, size_t stride, uint64_t* path_lens,
                          size_t* depth);
int mzk_merkle_open(const mzk_merkle* t, size_t index, uint8_t* path, size_t stride, uint64_t* path_len, size_t* depth) {
  if (!t || !path || !path_len || !depth) { set_error("merkle_open: null pointer"); return MZK_E_ARG; }
  if (t->n < 2) { set_error("merkle_open: needs at least two leaves (merkle.rs:32)"); return MZK_E_LENGTH; }
  if (index >= t->n) { set_error("merkle_open: index %zu out of range", index); return MZK_E_LENGTH; }
  if (stride < 32) { set_error("merkle_open: stride < 32"); return MZK_E_LENGTH; }
  if (t->kind == 0 && !t->ragged) {        // field-element tree: sibling leaf and digests in one gather and one synchronisation
    const uint64_t idx64 = (uint64_t)index;
    return mzk_merkle_open_batch(t, &idx64, 1, path, stride, path_len, depth);
  }
  MZK_ENTER();
  WsFrame ws("mzk_merkle_open");
  MerkleScope ms(t);
  MZK_TRY(ms.rc);
  hipStream_t s = ms.s;
  WsGuard wsg(s);          // WS_MISC_C below is shared with every other entry point of the context
  if (t->ragged) {
    // subtree p (depth D) that holds the leaf.  Merkle::open only terminates when its descent ends in a TWO-leaf
    // slice (merkle.rs:32-34); a one-leaf slice recurses forever (mid = 0), so those indices are an error here.
    size_t p = (size_t)(std::upper_bound(t->node_start.begin(), t->node_start.end(), (uint32_t)index) - t->node_start.begin()) - 1;
    const uint32_t first = t->node_start[p], cnt = t->node_start[p + 1] - first;
    const size_t sibp = p ^ 1;
    const uint32_t sib_cnt = t->node_start[sibp + 1] - t->node_start[sibp];
    if (cnt == 1 && sib_cnt != 1) {
      set_error("merkle_open: leaf %zu is the one-leaf half of a three-leaf slice; Merkle::open recurses forever there (merkle.rs:36-45)", index);
      return MZK_E_LENGTH;
    }
    // cnt == 2: the recursion ends inside subtree p (entry 0 = the other leaf), then climbs the item tree;
    // cnt == 1 with a one-leaf sibling: it ends one level higher, on the two-leaf slice {p, p ^ 1} -- the item path itself.
    int k = 0;
    if (cnt == 2) {
      const size_t other = first + (1 - (index - first));
      const size_t l0 = (size_t)(t->offsets[other + 1] - t->offsets[other]);
      if (stride < l0) { set_error("merkle_open: stride %zu < entry length %zu", stride, l0); return MZK_E_LENGTH; }
      if (l0) MZK_HIP(hipMemcpyAsync(path, (const uint8_t*)t->d_leaves + t->offsets[other], l0, hipMemcpyDeviceToHost, s));
      path_len[0] = l0;
      k = 1;
    }
    const size_t l1 = (size_t)(t->item_off[sibp + 1] - t->item_off[sibp]);
    if (stride < l1) { set_error("merkle_open: stride %zu < entry length %zu", stride, l1); return MZK_E_LENGTH; }
    if (l1) MZK_HIP(hipMemcpyAsync(path + (size_t)k * stride, (const uint8_t*)t->d_items + t->item_off[sibp], l1, hipMemcpyDeviceToHost, s));   // sibling item: a leaf or a digest
    path_len[k] = l1;
    if (t->depth > 1) {
      u64* d_out;
      MZK_TRY(ws.get(WS_MISC_C, (size_t)t->depth * 32, (void**)&d_out));
      hipLaunchKernelGGL(k_merkle_gather, dim3(1), dim3(64), 0, s, (const u64*)t->d_nodes, t->m, p, t->depth, d_out);
      MZK_HIP(hipGetLastError());
      uint8_t tmp[64 * 32];
      MZK_TRY(d2h_sync(tmp, d_out, (size_t)(t->depth - 1) * 32, s));
      for (int l = 1; l < t->depth; l++) { memcpy(path + (size_t)(l + k) * stride, tmp + 32 * (l - 1), 32); path_len[l + k] = 32; }
    } else {
      MZK_HIP(hipStreamSynchronize(s));
    }
    *depth = (size_t)t->depth + k;
    return MZK_OK;
  }
  const size_t sib = index ^ 1;
  // byte leaves: entry 0 is the sibling LEAF, verbatim
  {
    const size_t len = (size_t)(t->offsets[sib + 1] - t->offsets[sib]);
    if (stride < len) { set_error("merkle_open: stride %zu < leaf length %zu", stride, len); return MZK_E_LENGTH; }
    if (len) MZK_HIP(hipMemcpyAsync(path, (const uint8_t*)t->d_leaves + t->offsets[sib], len, hipMemcpyDeviceToHost, s));
    path_len[0] = len;
  }
  if (t->depth > 1) {
    u64* d_out;
    MZK_TRY(ws.get(WS_MISC_C, (size_t)t->depth * 32, (void**)&d_out));
    hipLaunchKernelGGL(k_merkle_gather, dim3(1), dim3(64), 0, s, (const u64*)t->d_nodes, t->n, index, t->depth, d_out);
    MZK_HIP(hipGetLastError());
    uint8_t tmp[64 * 32];
    MZK_TRY(d2h_sync(tmp, d_out, (size_t)(t->depth - 1) * 32, s));
    for (int l = 1; l < t->depth; l++) { memcpy(path + (size_t)l * stride, tmp + 32 * (l - 1), 32); path_len[l] = 32; }
  } else {
    MZK_HIP(hipStreamSynchronize(s));
  }
  *depth = (size_t)t->depth;
  return MZK_OK;
}

// `count` openings of one tree: paths[(q * depth + l) * stride ..] / path_lens[q * depth + l] as mzk_merkle_open writes them
// for index indices[q]; *depth entries per path.  Field-element trees with a power-of-two leaf count (every codeword of
// the provers): ONE gather launch and ONE copy for all paths.  Byte-leaf and ragged trees: MZK_E_ARG (open one by one).
int mzk_merkle_open_batch(const mzk_merkle* t, const uint64_t* indices, size_t count, uint8_t* paths, size_t stride, uint64_t* path_lens,
                          size_t* depth) {
  if (!t || !depth || ((!indices || !paths || !path_lens) && count)) { set_error("merkle_open_batch: null pointer"); return MZK_E_ARG; }
  if (t->n < 2) { set_error("merkle_open: needs at least two leaves (merkle.rs:32)"); return MZK_E_LENGTH; }
  if (t->ragged || t->kind != 0) {
    set_error("merkle_open_batch: field-element trees with a power-of-two leaf count only (this one: %s); open its paths one by one",
              t->kind != 0 ? "byte leaves" : "ragged");
    return MZK_E_ARG;
  }
  *depth = (size_t)t->depth;
  if (count == 0) return MZK_OK;
  if (stride < 32) { set_error("merkle_open: stride < 32"); return MZK_E_LENGTH; }
  for (size_t q = 0; q < count; q++)
    if (indices[q] >= t->n) { set_error("merkle_open: index %llu out of range", (unsigned long long)indices[q]); return MZK_E_LENGTH; }
  MZK_ENTER();
  WsFrame ws("mzk_merkle_open_batch");
  MerkleScope ms(t);
  MZK_TRY(ms.rc);
  hipStream_t s = ms.s;
  WsGuard wsg(s);
  const int lw = (int)field_words(t->field);
  const size_t node_words64 = count * (size_t)(t->depth - 1) * 4;
  u64 *d_idx, *d_on;
  u32* d_ol;
  MZK_TRY(ws.get(WS_MISC_C, count * 8 + node_words64 * 8 + count * (size_t)lw * 4 + 64, (void**)&d_idx));
  d_on = d_idx + count;
  d_ol = (u32*)(d_on + node_words64);
  MZK_HIP(hipMemcpyAsync(d_idx, indices, count * 8, hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(k_merkle_gather_batch, dim3((unsigned)count), dim3(64), 0, s, (const u64*)t->d_nodes, (const u32*)t->d_leaves, lw, t->n,
                     (const u64*)d_idx, t->depth, d_on, d_ol);
  MZK_HIP(hipGetLastError());
  std::vector<uint64_t> hn(node_words64 + 1);
  std::vector<uint32_t> hl(count * (size_t)lw);
  if (node_words64) MZK_HIP(hipMemcpyAsync(hn.data(), d_on, node_words64 * 8, hipMemcpyDeviceToHost, s));
  MZK_TRY(d2h_sync(hl.data(), d_ol, count * (size_t)lw * 4, s));
  for (size_t q = 0; q < count; q++) {
    uint64_t limbs[4] = {0, 0, 0, 0};
    memcpy(limbs, hl.data() + q * lw, (size_t)lw * 4);
    uint8_t buf[HOST_LEAF_MAX];
    const size_t sib = (size_t)indices[q] ^ 1;
    const size_t len = host_leaf(t->field, limbs, buf, !t->neg.empty() && t->neg[sib]);
    if (stride < len) { set_error("merkle_open: stride %zu < leaf length %zu", stride, len); return MZK_E_LENGTH; }
    uint8_t* pq = paths + q * (size_t)t->depth * stride;
    memcpy(pq, buf, len);
    path_lens[q * (size_t)t->depth] = len;
    for (int l = 1; l < t->depth; l++) {
      memcpy(pq + (size_t)l * stride, hn.data() + (q * (size_t)(t->depth - 1) + (l - 1)) * 4, 32);
      path_lens[q * (size_t)t->depth + l] = 32;
    }
  }
  return MZK_OK;
}

// Openings of SEVERAL trees in one call: the query phase of FRI::prove (fri.rs:127-137, reveal :211-260) opens the a / b indices
// in round i's tree and the c indices in round i+1's, for every round -- with the trees of mzk_fri_commit_keep_trees that is one
// call, one copy back and one synchronisation instead of two of each per round (48 us per call measured).  Tree t takes the
// next counts[t] entries of `indices`; its paths follow tree t-1's in paths / path_lens, laid out as mzk_merkle_open_batch
// lays them out with depths[t] entries per path.  counts[t] == 0 skips tree t (which may then be NULL).
int mzk_merkle_open_multi(const mzk_merkle* const* trees, size_t n_trees, const uint64_t* indices, const size_t* counts, uint8_t* paths,
                          size_t stride, uint64_t* path_lens, size_t* depths) {
  if (!trees || !counts || !depths) { set_error("merkle_open_multi: null pointer"); return MZK_E_ARG; }
  size_t total = 0, total_nodes = 0, total_leaf_words = 0;
  const mzk_merkle* first = nullptr;
  for (size_t t = 0; t < n_trees; t++) {
    depths[t] = trees[t] ? (size_t)trees[t]->depth : 0;
    if (counts[t] == 0) continue;
    const mzk_merkle* tr = trees[t];
    if (!tr || !indices || !paths || !path_lens) { set_error("merkle_open_multi: null pointer"); return MZK_E_ARG; }
    if (tr->n < 2) { set_error("merkle_open: needs at least two leaves (merkle.rs:32)"); return MZK_E_LENGTH; }
    if (tr->ragged || tr->kind != 0) {
      set_error("merkle_open_multi: field-element trees with a power-of-two leaf count only (tree %zu: %s)", t, tr->kind != 0 ? "byte leaves" : "ragged");
      return MZK_E_ARG;
    }
    for (size_t q = 0; q < counts[t]; q++)
      if (indices[total + q] >= tr->n) { set_error("merkle_open: index %llu out of range (tree %zu)", (unsigned long long)indices[total + q], t); return MZK_E_LENGTH; }
    if (!first) first = tr;
    if (tr->ctx_index != first->ctx_index || tr->device != first->device) {
      set_error("merkle_open_multi: tree %zu lives on context %d, the first opened tree on context %d; one call opens trees of one context", t,
                tr->ctx_index, first->ctx_index);
      return MZK_E_ARG;
    }
    total += counts[t];
    total_nodes += counts[t] * (size_t)(tr->depth - 1) * 4;
    total_leaf_words += counts[t] * field_words(tr->field);
  }
  if (total == 0) return MZK_OK;
  if (stride < 32) { set_error("merkle_open: stride < 32"); return MZK_E_LENGTH; }
  MZK_ENTER();
  WsFrame ws("mzk_merkle_open_multi");
  MerkleScope ms(first);
  MZK_TRY(ms.rc);
  hipStream_t s = ms.s;
  for (size_t t = 0; t < n_trees; t++)      // every opened tree's build, not only the first one's
    if (counts[t] && trees[t]->built) MZK_HIP(hipStreamWaitEvent(s, trees[t]->built, 0));
  WsGuard wsg(s);
  u64 *d_idx, *d_on;
  u32* d_ol;
  MZK_TRY(ws.get(WS_MISC_C, total * 8 + total_nodes * 8 + total_leaf_words * 4 + 64, (void**)&d_idx));
  d_on = d_idx + total;
  d_ol = (u32*)(d_on + total_nodes);
  MZK_HIP(hipMemcpyAsync(d_idx, indices, total * 8, hipMemcpyHostToDevice, s));
  {
    size_t at = 0, at_nodes = 0, at_leaf = 0;
    for (size_t t = 0; t < n_trees; t++) {
      if (counts[t] == 0) continue;
      const mzk_merkle* tr = trees[t];
      const int lw = (int)field_words(tr->field);
      hipLaunchKernelGGL(k_merkle_gather_batch, dim3((unsigned)counts[t]), dim3(64), 0, s, (const u64*)tr->d_nodes, (const u32*)tr->d_leaves, lw, tr->n,
                         (const u64*)(d_idx + at), tr->depth, d_on + at_nodes, d_ol + at_leaf);
      at += counts[t];
      at_nodes += counts[t] * (size_t)(tr->depth - 1) * 4;
      at_leaf += counts[t] * (size_t)lw;
    }
  }
  MZK_HIP(hipGetLastError());
  std::vector<uint64_t> hn(total_nodes + 1);
  std::vector<uint32_t> hl(total_leaf_words + 1);
  if (total_nodes) MZK_HIP(hipMemcpyAsync(hn.data(), d_on, total_nodes * 8, hipMemcpyDeviceToHost, s));
  MZK_TRY(d2h_sync(hl.data(), d_ol, total_leaf_words * 4, s));
  size_t at = 0, at_nodes = 0, at_leaf = 0, at_entry = 0;
  for (size_t t = 0; t < n_trees; t++) {
    if (counts[t] == 0) continue;
    const mzk_merkle* tr = trees[t];
    const int lw = (int)field_words(tr->field);
    for (size_t q = 0; q < counts[t]; q++) {
      uint64_t limbs[4] = {0, 0, 0, 0};
      memcpy(limbs, hl.data() + at_leaf + q * lw, (size_t)lw * 4);
      uint8_t buf[HOST_LEAF_MAX];
      const size_t sib = (size_t)indices[at + q] ^ 1;
      const size_t len = host_leaf(tr->field, limbs, buf, !tr->neg.empty() && tr->neg[sib]);
      if (stride < len) { set_error("merkle_open: stride %zu < leaf length %zu", stride, len); return MZK_E_LENGTH; }
      uint8_t* pq = paths + (at_entry + q * (size_t)tr->depth) * stride;
      memcpy(pq, buf, len);
      path_lens[at_entry + q * (size_t)tr->depth] = len;
      for (int l = 1; l < tr->depth; l++) {
        memcpy(pq + (size_t)l * stride, hn.data() + at_nodes + (q * (size_t)(tr->depth - 1) + (l - 1)) * 4, 32);
        path_lens[at_entry + q * (size_t)tr->depth + l] = 32;
      }
    }
    at += counts[t];
    at_nodes += counts[t] * (size_t)(tr->depth - 1) * 4;
    at_leaf += counts[t] * (size_t)lw;
    at_entry += counts[t] * (size_t)tr->depth;
  }
  return MZK_OK;
}

void mzk_merkle_free(mzk_merkle* t) {
  if (!t) return;
  if (t->built) (void)hipEventDestroy(t->built);
  delete t;
}

// One-shot commit of a device-resident codeword (the FRI round: root -> transcript -> alpha -> fold); nothing is
// retained, the node levels live in workspace.  root: 32 bytes (n >= 2) or the leaf bytes (n == 1; cap >= 41).
int mzk_merkle_commit_field_dev(int field_id, const void* d_elems, size_t n, uint8_t* root, size_t cap, size_t* root_len, void* stream) {
  MZK_ENTER();
  WsFrame ws("mzk_merkle_commit_field_dev");
  WsGuard wsg((hipStream_t)stream);
  MZK_TRY(field_check_gl(field_id, "merkle"));
  if (n == 0) { set_error("merkle: empty leaf set (Merkle::commit recurses forever on it, merkle.rs:20-22)"); return MZK_E_LENGTH; }
  if (!d_elems || !root || !root_len) { set_error("merkle: null pointer"); return MZK_E_ARG; }
  if (!is_pow2(n)) {      // ragged (merkle.rs:15-25 accepts it; no prover call site produces it): handle path
    mzk_merkle* t = nullptr;
    MZK_TRY(merkle_build(0, field_id, d_elems, true, n * field_bytes(field_id), nullptr, n, &t, (hipStream_t)stream));
    const int rc = mzk_merkle_root(t, root, cap, root_len);
    mzk_merkle_free(t);
    return rc;
  }
  hipStream_t s = (hipStream_t)stream;
  if (n == 1) {
    uint64_t limbs[4];
    uint8_t buf[HOST_LEAF_MAX];
    MZK_TRY(d2h_sync(limbs, d_elems, field_bytes(field_id), s));
    const size_t len = host_leaf(field_id, limbs, buf);
    if (cap < len) { set_error("merkle: root buffer too small"); return MZK_E_LENGTH; }
    memcpy(root, buf, len);
    *root_len = len;
    return MZK_OK;
  }
  if (cap < 32) { set_error("merkle: root buffer too small"); return MZK_E_LENGTH; }
  u64* d_nodes;
  MZK_TRY(ws.get(WS_MERKLE_NODES, (n - 1) * 32, (void**)&d_nodes));
  RootMailbox mb;
  bool mailed = false;
  MZK_TRY(merkle_mailbox(&mb));
  MZK_TRY(merkle_hash_levels(0, field_id, d_elems, nullptr, n, d_nodes, s, nullptr, 1, mb.p, mb.seq, &mailed));
  MZK_TRY(merkle_root_to_host(root, d_nodes + 4 * (n - 2), mb, mailed, s));
  *root_len = 32;
  return MZK_OK;
}
// Merkle::commit of `batch` codewords of n elements each (n a power of two >= 2), roots only: one set of launches for all
// trees, so the latency-bound upper levels of the trees run side by side.
int mzk_merkle_commit_field_batch_dev(int field_id, const void* d_elems, size_t n, size_t batch, uint8_t* roots, void* stream) {
  MZK_ENTER();
  WsFrame ws("mzk_merkle_commit_field_batch_dev");
  WsGuard wsg((hipStream_t)stream);
  MZK_TRY(field_check(field_id, "merkle"));
  if (batch == 0) return MZK_OK;
  if (n == 0) { set_error("merkle: empty leaf set (Merkle::commit recurses forever on it, merkle.rs:20-22)"); return MZK_E_LENGTH; }
  if (!d_elems || !roots) { set_error("merkle: null pointer"); return MZK_E_ARG; }
  if (!is_pow2(n) || n < 2) { set_error("merkle batch: codewords of %zu elements (need a power of two >= 2; use the single-tree calls)", n); return MZK_E_NOT_POW2; }
  if (batch > ((size_t)1 << 36) / n) { set_error("merkle batch: too many leaves"); return MZK_E_ARG; }
  hipStream_t s = (hipStream_t)stream;
  const size_t total = n * batch;
  u64* d_nodes;
  MZK_TRY(ws.get(WS_MERKLE_NODES, (total - batch) * 32, (void**)&d_nodes));
  MZK_TRY(merkle_hash_levels(0, field_id, d_elems, nullptr, total, d_nodes, s, nullptr, batch));
  MZK_TRY(d2h_sync(roots, d_nodes + 4 * (total - 2 * batch), batch * 32, s));
  return MZK_OK;
}
int mzk_merkle_commit_field_batch(int field_id, const uint64_t* elems, size_t n, size_t batch, uint8_t* roots) {
  MZK_ENTER();
  WsFrame ws("mzk_merkle_commit_field_batch");
  MZK_TRY(field_check(field_id, "merkle"));
  if (batch == 0) return MZK_OK;
  if (!elems) { set_error("merkle: null pointer"); return MZK_E_ARG; }
  hipStream_t s = ctx().stream;
  void* d;
  {
    WsGuard wsg(s);
    MZK_TRY(ws.get(WS_MISC_D, n * batch * field_bytes(field_id) + 16, &d));
    MZK_HIP(hipMemcpyAsync(d, elems, n * batch * field_bytes(field_id), hipMemcpyHostToDevice, s));
  }
  return mzk_merkle_commit_field_batch_dev(field_id, d, n, batch, roots, s);
}
int mzk_merkle_commit_field(int field_id, const uint64_t* elems, size_t n, uint8_t* root, size_t cap, size_t* root_len) {
  mzk_merkle* t = nullptr;
  MZK_TRY(mzk_merkle_build_field(field_id, elems, n, &t));
  const int rc = mzk_merkle_root(t, root, cap, root_len);
  mzk_merkle_free(t);
  return rc;
}
int mzk_merkle_commit_bytes(const uint8_t* leaves, const uint64_t* offsets, size_t n, uint8_t* root, size_t cap, size_t* root_len) {
  mzk_merkle* t = nullptr;
  MZK_TRY(mzk_merkle_build_bytes(leaves, offsets, n, &t));
  const int rc = mzk_merkle_root(t, root, cap, root_len);
  mzk_merkle_free(t);
  return rc;
}

// FRI::commit (zkstark/fri.rs:144-209) with the codewords resident in HBM for the whole loop.  Per round r:
//   root_r = Merkle::commit(codeword_r as bincode leaves)              fri.rs:160-168
//   challenge(user, r, last, root_r, len, alpha)  -- the host pushes the root to its proof stream and, unless
//                                                    `last`, samples alpha from it                 fri.rs:168-176
//   codeword_{r+1} = split-and-fold(codeword_r, alpha, offset, omega); omega, offset squared      fri.rs:182-195
// Outputs: roots (num_rounds entries of 48 bytes, lengths in root_len: 32, or the leaf bytes once a codeword has
// shrunk to one element) and all num_rounds codewords concatenated (n + n/2 + ... elements) -- the reference's
// return value `(codewords, roots)`; sending the last codeword (fri.rs:198-206) is the caller's transcript work.
static int fri_commit_rounds(int field_id, const uint64_t* codeword, const uint8_t* negative, size_t n, const uint64_t* omega, const uint64_t* offset,
                             int num_rounds, mzk_fri_challenge_fn challenge, void* user, uint8_t* roots, uint64_t* root_len, uint64_t* codewords_out,
                             mzk_merkle** trees_out, bool on_device, bool signed_form);
// trees_out (optional, num_rounds entries): the Merkle tree of every round's codeword stays on the device as a handle for the
// query phase (mzk_merkle_open_batch; fri.rs:211-260 opens from exactly these codewords); a one-element round gets NULL.
// On failure every handle made so far is released.
static int fri_commit_impl(int field_id, const uint64_t* codeword, const uint8_t* negative, size_t n, const uint64_t* omega, const uint64_t* offset,
                           int num_rounds, mzk_fri_challenge_fn challenge, void* user, uint8_t* roots, uint64_t* root_len, uint64_t* codewords_out,
                           mzk_merkle** trees_out = nullptr, bool on_device = false, bool signed_form = false) {
  if (trees_out) for (int r = 0; r < num_rounds; r++) trees_out[r] = nullptr;
  const int rc = fri_commit_rounds(field_id, codeword, negative, n, omega, offset, num_rounds, challenge, user, roots, root_len, codewords_out, trees_out, on_device,
                                   signed_form);
  if (rc != MZK_OK && trees_out)
    for (int r = 0; r < num_rounds; r++) { if (trees_out[r]) mzk_merkle_free(trees_out[r]); trees_out[r] = nullptr; }
  return rc;
}
static int fri_commit_rounds(int field_id, const uint64_t* codeword, const uint8_t* negative, size_t n, const uint64_t* omega, const uint64_t* offset,
                             int num_rounds, mzk_fri_challenge_fn challenge, void* user, uint8_t* roots, uint64_t* root_len, uint64_t* codewords_out,
                             mzk_merkle** trees_out, bool on_device, bool signed_form) {
  MZK_ENTER();
  WsFrame ws("fri_commit_rounds");
  // the Goldilocks ids: every form but mzk_fri_commit_signed, and without signs (an extension element's coefficients carry their own
  // signs in the reference; parity is defined on canonical coefficients only -- DESIGN.md section 9e)
  MZK_TRY(signed_form ? field_check(field_id, "fri_commit") : field_check_gl(field_id, "fri_commit"));
  const bool is_gl = field_is_gl(field_id);
  if (is_gl && negative) { set_error("fri_commit: field id %d takes canonical elements only (negative must be NULL)", field_id); return MZK_E_ARG; }
  if (num_rounds <= 0) return MZK_OK;
  if (!codeword || !omega || !offset || !challenge || !roots || !root_len) { set_error("fri_commit: null pointer"); return MZK_E_ARG; }
  if (!codewords_out && !trees_out) { set_error("fri_commit: no codeword output and no trees kept"); return MZK_E_ARG; }
  if (n == 0) { set_error("fri_commit: empty codeword"); return MZK_E_LENGTH; }
  if (!is_pow2(n)) { set_error("fri_commit: codeword length must be a power of two"); return MZK_E_NOT_POW2; }
  if ((n >> (num_rounds - 1)) == 0) { set_error("fri_commit: %d rounds halve a length-%zu codeword away", num_rounds, n); return MZK_E_LENGTH; }
  const HostField* hf = host_field(field_id);      // null for the Goldilocks ids
  if (is_gl) {
    MZK_TRY(gl_param_check(field_id, omega, "fri_commit", "parameter", true));
    MZK_TRY(gl_param_check(field_id, offset, "fri_commit", "parameter", true));
    // a one-element round's "root" is the leaf itself: up to 59 bytes for M64X3, and a root slot holds 48
    if (field_id == MZK_FIELD_M64X3 && (n >> (num_rounds - 1)) == 1) { set_error("fri_commit: a one-element round of field id %d does not fit the 48-byte root slot", field_id); return MZK_E_LENGTH; }
  } else if (!h_is_canonical(hf, omega) || !h_is_canonical(hf, offset)) { set_error("fri_commit: parameter not canonical"); return MZK_E_RANGE; }
  hipStream_t s = ctx().stream;
  WsGuard wsg(s);
  const size_t esz = field_bytes(field_id);
  const int nl = field_limbs64(field_id);
  size_t total = 0;
  for (int r = 0; r < num_rounds; r++) total += n >> r;
  uint8_t* d_all;
  u64* d_nodes;
  std::shared_ptr<DevMem> shared;      // this function's own reference: the handles already handed out keep the block alive on every exit path
  if (trees_out) {
    // trees kept: codewords and digests of every round in ONE allocation that the rounds' handles share (two allocations and two
    // device copies per round before: ~25 us of a ~155-us round at 2^14); layout: [codewords of all rounds | digests of round 0 | 1 | ...]
    for (int r = 0; r < num_rounds; r++) trees_out[r] = nullptr;
    size_t node_bytes = 0;
    for (int r = 0; r < num_rounds; r++) if ((n >> r) >= 2) node_bytes += ((n >> r) - 1) * 32;
    const size_t cw_bytes = (total * esz + 255) & ~(size_t)255;
    shared = std::make_shared<DevMem>();
    MZK_TRY(shared->alloc(cw_bytes + node_bytes + 256, "fri_commit: kept trees"));
    d_all = shared->as<uint8_t>();
    d_nodes = (u64*)(d_all + cw_bytes);
  } else {
    MZK_TRY(ws.get(WS_NTT_IO_A, total * esz, (void**)&d_all));
    MZK_TRY(ws.get(WS_MERKLE_NODES, n * 32, (void**)&d_nodes));
  }
  MZK_HIP(hipMemcpyAsync(d_all, codeword, n * esz, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s));
  u8* d_neg = nullptr;
  if (negative) {     // round 0 hashes bincode of the UNSANITIZED elements (fri.rs:160-166); the fold sanitizes (fri.rs:190)
    MZK_TRY(ws.get(WS_MISC_E, n, (void**)&d_neg));
    MZK_HIP(hipMemcpyAsync(d_neg, negative, n, hipMemcpyHostToDevice, s));
  }
  uint64_t alpha[4];
  // the fold's constants 2^-1, offset^-1, omega^-1: inverted ONCE here and squared along with omega and offset (three host
  // inversions per round before)
  FriFoldConsts fc;
  MZK_TRY(fri_fold_consts(field_id, offset, omega, &fc));
  uint8_t* cur = d_all;
  size_t len = n;
  for (int r = 0; r < num_rounds; r++) {
    uint8_t* root = roots + 48 * (size_t)r;
    if (len == 1) {
      uint64_t limbs[4];
      MZK_TRY(d2h_sync(limbs, cur, esz, s));
      root_len[r] = host_leaf(field_id, limbs, root, r == 0 && negative && negative[0]);
    } else {
      RootMailbox mb;
      bool mailed = false;
      MZK_TRY(merkle_mailbox(&mb));
      MZK_TRY(merkle_hash_levels(0, field_id, cur, nullptr, len, d_nodes, s, r == 0 ? d_neg : nullptr, 1, mb.p, mb.seq, &mailed));
      if (trees_out) {      // keep this round's tree: its leaves and digests stay where they were computed, in the shared block
        mzk_merkle* t = new mzk_merkle();
        t->kind = 0; t->field = field_id; t->n = len; t->stream = s;
        t->d_nodes = d_nodes; t->d_leaves = cur;
        t->shared = shared;
        t->depth = 0;
        while (((size_t)1 << t->depth) < len) t->depth++;
        trees_out[r] = t;
        if (r == 0 && negative) {
          // round 0 commits to the UNSANITIZED elements and the fold below canonicalises the codeword in place: the tree keeps
          // the magnitudes as they were given, in a copy of its own
          MZK_TRY(t->own_leaves.alloc(len * esz, "fri_commit: round-0 leaves"));
          MZK_HIP(hipMemcpyAsync(t->own_leaves.get(), cur, len * esz, hipMemcpyDeviceToDevice, s));
          t->d_leaves = t->own_leaves.get();
          t->neg.assign(negative, negative + n);
        }
        MZK_TRY(merkle_stamp(t, s, true));
      }
      MZK_TRY(merkle_root_to_host(root, d_nodes + 4 * (len - 2), mb, mailed, s));      // the transcript needs the root now
      root_len[r] = 32;
    }
    if (r == 0 && d_neg) {      // from here on the codeword is its canonical representative: v -> p - |v| where Sign::Minus
      MZK_TRY(canonicalize_signed(field_id, cur, d_neg, n, s));
    }
    const int last = (r == num_rounds - 1);
    memset(alpha, 0xff, sizeof alpha);     // a callback that forgets alpha leaves a non-canonical value, never a silent 0
    const int crc = challenge(user, r, last, root, (size_t)root_len[r], alpha);
    if (crc != 0) { set_error("fri_commit: challenge callback failed in round %d (status %d)", r, crc); return MZK_E_CALLBACK; }
    if (last) break;
    bool alpha_ok = true;
    if (is_gl) { for (int i = 0; i < nl; i++) alpha_ok = alpha_ok && gl::is_canonical(alpha[i]); } else alpha_ok = h_is_canonical(hf, alpha);
    if (!alpha_ok) { set_error("fri_commit: challenge of round %d not canonical", r); return MZK_E_RANGE; }
    uint8_t* next = cur + len * esz;
    MZK_TRY(fri_fold_dev_consts(field_id, cur, len, alpha, fc, next, s));
    fri_fold_consts_square(field_id, &fc);
    if (trees_out && len >= 2) d_nodes += 4 * (len - 1);        // the next round's digests follow this round's
    cur = next;
    len /= 2;
  }
  MZK_TRY(d2h_sync(codewords_out, d_all, codewords_out ? total * esz : 0, s));
  return MZK_OK;
}
int mzk_fri_commit(int field_id, const uint64_t* codeword, size_t n, const uint64_t* omega, const uint64_t* offset, int num_rounds,
                   mzk_fri_challenge_fn challenge, void* user, uint8_t* roots, uint64_t* root_len, uint64_t* codewords_out) {
  return fri_commit_impl(field_id, codeword, nullptr, n, omega, offset, num_rounds, challenge, user, roots, root_len, codewords_out);
}
int mzk_fri_commit_signed(int field_id, const uint64_t* magnitudes, const uint8_t* negative, size_t n, const uint64_t* omega, const uint64_t* offset,
                          int num_rounds, mzk_fri_challenge_fn challenge, void* user, uint8_t* roots, uint64_t* root_len, uint64_t* codewords_out) {
  return fri_commit_impl(field_id, magnitudes, negative, n, omega, offset, num_rounds, challenge, user, roots, root_len, codewords_out, nullptr, false, true);
}
int mzk_fri_commit_keep_trees(int field_id, const uint64_t* magnitudes, const uint8_t* negative, size_t n, const uint64_t* omega, const uint64_t* offset,
                              int num_rounds, mzk_fri_challenge_fn challenge, void* user, uint8_t* roots, uint64_t* root_len, uint64_t* codewords_out,
                              mzk_merkle** trees_out) {
  if (!trees_out && num_rounds > 0) { set_error("fri_commit_keep_trees: null handle array"); return MZK_E_ARG; }
  return fri_commit_impl(field_id, magnitudes, negative, n, omega, offset, num_rounds, challenge, user, roots, root_len, codewords_out, trees_out);
}
// the same with the initial codeword already in HBM (the output of mzk_coset_lde_dev: fast_stark.rs commits to what it has just
// extended); d_codeword must be complete before the call.  negative (host, optional) as in mzk_fri_commit_signed.
int mzk_fri_commit_keep_trees_dev(int field_id, const void* d_magnitudes, const uint8_t* negative, size_t n, const uint64_t* omega, const uint64_t* offset,
                                  int num_rounds, mzk_fri_challenge_fn challenge, void* user, uint8_t* roots, uint64_t* root_len, uint64_t* codewords_out,
                                  mzk_merkle** trees_out) {
  if (!trees_out && num_rounds > 0) { set_error("fri_commit_keep_trees: null handle array"); return MZK_E_ARG; }
  return fri_commit_impl(field_id, (const uint64_t*)d_magnitudes, negative, n, omega, offset, num_rounds, challenge, user, roots, root_len, codewords_out, trees_out, true);
}
// The elements a tree was built over, at `count` positions: magnitudes (count x limbs) and, if wanted, their Sign::Minus flags --
// what FRI::reveal sends next to the authentication paths (fri.rs:224-233), without the codewords ever leaving the device.
int mzk_merkle_leaves(const mzk_merkle* t, const uint64_t* indices, size_t count, uint64_t* magnitudes, uint8_t* negative) {
  if (!t || ((!indices || !magnitudes) && count)) { set_error("merkle_leaves: null pointer"); return MZK_E_ARG; }
  if (t->kind != 0) { set_error("merkle_leaves: field-element trees only"); return MZK_E_ARG; }
  for (size_t q = 0; q < count; q++)
    if (indices[q] >= t->n) { set_error("merkle_leaves: index %llu out of range", (unsigned long long)indices[q]); return MZK_E_LENGTH; }
  if (count == 0) return MZK_OK;
  MZK_ENTER();
  WsFrame ws("mzk_merkle_leaves");
  MerkleScope ms(t);
  MZK_TRY(ms.rc);
  hipStream_t s = ms.s;
  WsGuard wsg(s);
  const size_t esz = field_bytes(t->field);
  const int lw = (int)field_words(t->field);
  u64* d_idx;
  MZK_TRY(ws.get(WS_MISC_C, count * 8 + count * esz + 64, (void**)&d_idx));
  u32* d_out = (u32*)(d_idx + count);
  MZK_HIP(hipMemcpyAsync(d_idx, indices, count * 8, hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(k_gather_leaves, dim3((unsigned)((count * lw + 255) / 256)), dim3(256), 0, s, (const u32*)t->d_leaves, lw, (const u64*)d_idx, count, d_out);
  MZK_HIP(hipGetLastError());
  MZK_HIP(hipMemcpyAsync(magnitudes, d_out, count * esz, hipMemcpyDeviceToHost, s));
  if (negative) for (size_t q = 0; q < count; q++) negative[q] = (!t->neg.empty() && t->neg[(size_t)indices[q]]) ? 1 : 0;
  MZK_HIP(hipStreamSynchronize(s));
  return MZK_OK;
}

}  // extern "C"

// ================================================================================================================================
// FRI::prove (zkstark/fri.rs:99-143) in one enqueue: commit (:144-209) with the proof stream on the device, sample_indices
// (:19-62) and reveal (:211-260).  Per round r the Merkle tree is hashed as in mzk_fri_commit; then k_fri_tx_round appends
// vec![root_r] to the device transcript, rehashes the whole serialization with SHAKE256 and writes alpha_r; the fold reads it
// from there.  After the last root k_fri_tx_last pushes the last codeword, squeezes the index seed and samples the top-level
// indices; k_fri_query gathers every layer's values and paths into the packed proof.  No host round trip inside.
// mzk_fri_prove_gl runs the same driver over the Goldilocks ids with the *_gl forms of the three kernels (mzk.h: 64-byte path entries).
#include "mzk_transcript.h"
namespace mzk {

// Round r of the proof stream: push vec![root_r] (u64 1 | u64 32 | root), the object count becomes r + 1; unless this is the
// last round, alpha_r = F::sample(SHAKE256(stream)[0 .. 32)) (fri.rs:168-176) into `alpha` (4 limbs, canonical: < 2^64).
__global__ __launch_bounds__(64) void k_fri_tx_round(u64* __restrict__ tx, int r, const u64* __restrict__ root, u64* __restrict__ proof_root,
                                                     u64* __restrict__ alpha, int squeeze) {
  __shared__ u32 dig[8];
  const int tid = threadIdx.x;
  if (tid < 6) {
    const u64 v = tid == 0 ? 1 : (tid == 1 ? 32 : root[tid - 2]);
    tx[1 + 6 * (size_t)r + tid] = v;
    if (tid >= 2) proof_root[tid - 2] = v;
  }
  if (tid == 0) tx[0] = (u64)r + 1;
  __syncthreads();
  if (!squeeze) return;
  if (tid < 2) fri_shake256_pair(reinterpret_cast<const u8*>(tx), 8 + 48 * ((size_t)r + 1), tid, dig);
  __syncthreads();
  if (tid < 4) alpha[tid] = tid == 0 ? mzk_tx::sample_digest_word3(((u64)dig[7] << 32) | dig[6]) : 0;
}

// After the last root: push the last codeword (one object of m leaves, each u64 length + bincode(FiniteFieldElement)), squeeze the
// seed (fri.rs:114-123), sample the top-level indices (fri.rs:40-62) and write status / indices / last codeword into the proof.
// size = n / 2, reduced = m (powers of two: the reductions are masks).  One workgroup; `seen` holds m bits (global scratch).
constexpr int TX_LAST_THREADS = 256;
template <int NW>
__global__ __launch_bounds__(TX_LAST_THREADS) void k_fri_tx_last(u8* __restrict__ tx, int rounds, const u32* __restrict__ cw, size_t m, size_t size,
                                                                  size_t number, u32* __restrict__ seen, u64* __restrict__ p_status,
                                                                  u64* __restrict__ p_top, u32* __restrict__ p_last) {
  __shared__ u64 scan[TX_LAST_THREADS];
  __shared__ u64 cand[TX_LAST_THREADS];
  __shared__ u32 seed32[8];
  __shared__ u64 s_count, s_done;
  const int tid = threadIdx.x;
  u64* tw = reinterpret_cast<u64*>(tx);
  const size_t obj = 8 + 48 * (size_t)rounds;      // the object's u64 string count, then the strings
  if (tid == 0) { tw[0] = (u64)rounds + 1; tw[obj / 8] = (u64)m; }
  size_t at = obj + 8;
  for (size_t base = 0; base < m; base += TX_LAST_THREADS) {
    const size_t j = base + tid;
    u32 w[NW];
    int k = 0;
    if (j < m) {
#pragma unroll
      for (int q = 0; q < NW; q++) { w[q] = cw[j * NW + q]; p_last[j * NW + q] = w[q]; if (w[q]) k = q + 1; }
    }
    const u64 rec = j < m ? 8 + 9 + 4 * (u64)k : 0;
    scan[tid] = rec;
    __syncthreads();
    for (int d = 1; d < TX_LAST_THREADS; d <<= 1) {          // inclusive scan of the record lengths
      const u64 add = tid >= d ? scan[tid - d] : 0;
      __syncthreads();
      scan[tid] += add;
      __syncthreads();
    }
    if (j < m) {
      u8* p = tx + at + scan[tid] - rec;
      const u64 len = 9 + 4 * (u64)k;
      for (int b = 0; b < 8; b++) p[b] = (u8)(len >> (8 * b));
      p[8] = k ? 1 : 0;                                       // Sign::Plus / NoSign (the fold sanitized the codeword)
      for (int b = 0; b < 8; b++) p[9 + b] = b == 0 ? (u8)k : 0;
      for (int q = 0; q < k; q++)
        for (int b = 0; b < 4; b++) p[17 + 4 * q + b] = (u8)(w[q] >> (8 * b));
    }
    at += scan[TX_LAST_THREADS - 1];
    __syncthreads();
  }
  if (tid < 2) fri_shake256_pair(tx, at, tid, seed32);
  for (size_t i = tid; i < (m + 31) / 32; i += TX_LAST_THREADS) seen[i] = 0;
  if (tid == 0) { s_count = 0; s_done = 0; }
  __syncthreads();
  u64 seed[4];
#pragma unroll
  for (int i = 0; i < 4; i++) seed[i] = ((u64)seed32[2 * i + 1] << 32) | seed32[2 * i];
  // counters in batches of 256, hashed side by side and accepted in counter order (the reference's loop, bounded)
  for (u64 c0 = 0; c0 < mzk_tx::SAMPLE_COUNTER_LIMIT && !s_done; c0 += TX_LAST_THREADS) {
    u64 h[4];
    mzk_tx::blake2b256_seed_counter(seed, c0 + tid, h);
    cand[tid] = mzk_tx::sample_digest_word3(h[3]) & (u64)(size - 1);
    __syncthreads();
    if (tid == 0) {
      u64 cnt = s_count;
      for (int t = 0; t < TX_LAST_THREADS && cnt < number; t++) {
        const u64 idx = cand[t], red = idx & (u64)(m - 1);
        const u32 bit = 1u << (red & 31);
        if (!(seen[red >> 5] & bit)) {
          seen[red >> 5] |= bit;
          p_top[cnt++] = idx;
        }
      }
      s_count = cnt;
      s_done = cnt >= number;
    }
    __syncthreads();
  }
  if (tid == 0) {
    for (u64 q = s_count; q < number; q++) p_top[q] = 0;
    *p_status = s_count >= number ? 0 : 1;
  }
}

// The query phase: block q = (layer i, kind a / b / c, test s).  a = top % (len_i / 2), b = a + len_i / 2 in round i's tree, c = a in
// round i + 1's.  Writes the value (limbs and Sign::Minus flag) and the path exactly as mzk_merkle_open_batch returns it: entry 0 the
// sibling leaf's bincode bytes, entries 1 .. depth-1 the digests; PATH_STRIDE bytes per entry, zero-padded, lengths beside.
struct FriQueryArgs {
  const u8* cw;          // all rounds' codewords back to back
  const u8* nodes;       // all rounds' digests back to back
  const u32* mag0;       // round 0's leaves as committed (the magnitudes, when signed; else the codeword itself)
  const u8* neg0;        // round 0's Sign::Minus flags or null
  const u64* top;
  u8* values; u8* signs; u8* paths; u64* lens;
  u64 n, tests;
  u64 cw_off[64], node_off[64];     // byte offsets of round r's codeword / digests
};
template <int NW>
__global__ __launch_bounds__(64) void k_fri_query(FriQueryArgs A) {
  const u64 T = A.tests, q = blockIdx.x;
  const int layer = (int)(q / (3 * T)), kind = (int)((q / T) % 3);
  const u64 s = q % T;
  const u64 half = (A.n >> layer) / 2;
  const u64 a = A.top[s] & (half - 1);
  const u64 idx = kind == 1 ? a + half : a;
  const int rnd = layer + (kind == 2);
  const u64 len = A.n >> rnd;
  const int depth = mzk_tx::log2_pow2(len);
  const u32* leaves = rnd == 0 ? A.mag0 : reinterpret_cast<const u32*>(A.cw + A.cw_off[rnd]);
  const u8* neg = rnd == 0 ? A.neg0 : nullptr;
  const u64* nodes = reinterpret_cast<const u64*>(A.nodes + A.node_off[rnd]);
  const int tid = threadIdx.x;
  if (tid < NW) reinterpret_cast<u32*>(A.values)[q * NW + tid] = leaves[idx * NW + tid];
  if (tid == 0) A.signs[q] = neg ? neg[idx] : 0;
  const u64 e0 = mzk_tx::fri_entry_base(A.n, T, layer, kind) + s * (u64)depth;
  const int l = tid;
  if (l >= 1 && l < depth) {
    const u64 start = len - (len >> (l - 1));
    const u64* src = nodes + 4 * (start + ((idx >> l) ^ 1));
    u64* dst = reinterpret_cast<u64*>(A.paths + (e0 + l) * mzk_tx::PATH_STRIDE);
#pragma unroll
    for (int k = 0; k < 4; k++) dst[k] = src[k];
    dst[4] = 0; dst[5] = 0;
    A.lens[e0 + l] = 32;
  }
  if (tid == 0) {
    const u64 sib = idx ^ 1;
    u32 w[NW];
    int k = 0;
#pragma unroll
    for (int j = 0; j < NW; j++) { w[j] = leaves[sib * NW + j]; if (w[j]) k = j + 1; }
    u8 buf[mzk_tx::PATH_STRIDE];
#pragma unroll
    for (int b = 0; b < mzk_tx::PATH_STRIDE; b++) buf[b] = 0;
    buf[0] = k ? ((neg && neg[sib]) ? 0xff : 1) : 0;
    buf[1] = (u8)k;
#pragma unroll
    for (int j = 0; j < NW; j++)
      if (j < k)
        for (int b = 0; b < 4; b++) buf[9 + 4 * j + b] = (u8)(w[j] >> (8 * b));
    u64* dst = reinterpret_cast<u64*>(A.paths + e0 * mzk_tx::PATH_STRIDE);
#pragma unroll
    for (int b = 0; b < mzk_tx::PATH_STRIDE / 8; b++) {
      u64 v = 0;
      for (int t = 0; t < 8; t++) v |= (u64)buf[8 * b + t] << (8 * t);
      dst[b] = v;
    }
    A.lens[e0] = 9 + 4 * (u64)k;
  }
}

// ---- the same three kernels over the Goldilocks ids (mzk_fri_prove_gl; NC = 1: M64, 3: M64X3) ------------------------------------------
// Round r: as k_fri_tx_round, with alpha_r = F::sample taken mod p (mzk_tx::sample_gl) -- the base value, which id 4 embeds as
// (v, 0, 0): `alpha` takes the same four words, the fold reads the first NC.
__global__ __launch_bounds__(64) void k_fri_tx_round_gl(u64* __restrict__ tx, int r, const u64* __restrict__ root, u64* __restrict__ proof_root,
                                                        u64* __restrict__ alpha, int squeeze) {
  __shared__ u32 dig[8];
  const int tid = threadIdx.x;
  if (tid < 6) {
    const u64 v = tid == 0 ? 1 : (tid == 1 ? 32 : root[tid - 2]);
    tx[1 + 6 * (size_t)r + tid] = v;
    if (tid >= 2) proof_root[tid - 2] = v;
  }
  if (tid == 0) tx[0] = (u64)r + 1;
  __syncthreads();
  if (!squeeze) return;
  if (tid < 2) fri_shake256_pair(reinterpret_cast<const u8*>(tx), 8 + 48 * ((size_t)r + 1), tid, dig);
  __syncthreads();
  if (tid < 4) alpha[tid] = tid == 0 ? mzk_tx::sample_gl(((u64)dig[7] << 32) | dig[6]) : 0;
}

// After the last root: as k_fri_tx_last, the strings being gl::leaf_bytes<NC> of the elements (8 .. 59 bytes, mzk_tx::fri_gl_record_put);
// a string's position is the prefix sum of the record lengths before it, a workgroup's worth of strings per step.  The stream is
// then rehashed by one lane pair (about 65 SHAKE blocks at m = 128 over M64X3).
template <int NC>
__global__ __launch_bounds__(TX_LAST_THREADS) void k_fri_tx_last_gl(u8* __restrict__ tx, int rounds, const u64* __restrict__ cw, size_t m, size_t size,
                                                                     size_t number, u32* __restrict__ seen, u64* __restrict__ p_status,
                                                                     u64* __restrict__ p_top, u64* __restrict__ p_last) {
  __shared__ u64 scan[TX_LAST_THREADS];
  __shared__ u64 cand[TX_LAST_THREADS];
  __shared__ u32 seed32[8];
  __shared__ u64 s_count, s_done;
  const int tid = threadIdx.x;
  u64* tw = reinterpret_cast<u64*>(tx);
  const size_t obj = 8 + 48 * (size_t)rounds;
  if (tid == 0) { tw[0] = (u64)rounds + 1; tw[obj / 8] = (u64)m; }
  size_t at = obj + 8;
  for (size_t base = 0; base < m; base += TX_LAST_THREADS) {
    const size_t j = base + tid;
    u64 c[NC];
#pragma unroll
    for (int q = 0; q < NC; q++) c[q] = 0;
    if (j < m) {
#pragma unroll
      for (int q = 0; q < NC; q++) { c[q] = cw[j * NC + q]; p_last[j * NC + q] = c[q]; }
    }
    const u64 rec = j < m ? mzk_tx::fri_gl_record_len<NC>(c) : 0;
    scan[tid] = rec;
    __syncthreads();
    for (int d = 1; d < TX_LAST_THREADS; d <<= 1) {          // inclusive scan of the record lengths
      const u64 add = tid >= d ? scan[tid - d] : 0;
      __syncthreads();
      scan[tid] += add;
      __syncthreads();
    }
    if (j < m) mzk_tx::fri_gl_record_put<NC>(c, tx + at + scan[tid] - rec);
    at += scan[TX_LAST_THREADS - 1];
    __syncthreads();
  }
  if (tid < 2) fri_shake256_pair(tx, at, tid, seed32);
  for (size_t i = tid; i < (m + 31) / 32; i += TX_LAST_THREADS) seen[i] = 0;
  if (tid == 0) { s_count = 0; s_done = 0; }
  __syncthreads();
  u64 seed[4];
#pragma unroll
  for (int i = 0; i < 4; i++) seed[i] = ((u64)seed32[2 * i + 1] << 32) | seed32[2 * i];
  // sample_indices exactly as k_fri_tx_last: batches of 256 counters, accepted in counter order, bounded
  for (u64 c0 = 0; c0 < mzk_tx::SAMPLE_COUNTER_LIMIT && !s_done; c0 += TX_LAST_THREADS) {
    u64 h[4];
    mzk_tx::blake2b256_seed_counter(seed, c0 + tid, h);
    cand[tid] = mzk_tx::sample_digest_word3(h[3]) & (u64)(size - 1);
    __syncthreads();
    if (tid == 0) {
      u64 cnt = s_count;
      for (int t = 0; t < TX_LAST_THREADS && cnt < number; t++) {
        const u64 idx = cand[t], red = idx & (u64)(m - 1);
        const u32 bit = 1u << (red & 31);
        if (!(seen[red >> 5] & bit)) {
          seen[red >> 5] |= bit;
          p_top[cnt++] = idx;
        }
      }
      s_count = cnt;
      s_done = cnt >= number;
    }
    __syncthreads();
  }
  if (tid == 0) {
    for (u64 q = s_count; q < number; q++) p_top[q] = 0;
    *p_status = s_count >= number ? 0 : 1;
  }
}

// The query phase: the blocks of k_fri_query.  A value is NC words and its sign byte 0; a path entry is a PATH_STRIDE_GL-byte slot, zero
// padded: entry 0 the sibling's leaf bytes, serialised in LDS as k_merkle_leaf_pairs_gl does, entries 1 .. depth-1 the digests.
template <int NC>
__global__ __launch_bounds__(64) void k_fri_query_gl(FriQueryArgs A) {
  constexpr int SLOT_WORDS = mzk_tx::PATH_STRIDE_GL / 8;
  __shared__ u64 slot[SLOT_WORDS];
  __shared__ int leaf_len;
  const u64 T = A.tests, q = blockIdx.x;
  const int layer = (int)(q / (3 * T)), kind = (int)((q / T) % 3);
  const u64 s = q % T;
  const u64 half = (A.n >> layer) / 2;
  const u64 a = A.top[s] & (half - 1);
  const u64 idx = kind == 1 ? a + half : a;
  const int rnd = layer + (kind == 2);
  const u64 len = A.n >> rnd;
  const int depth = mzk_tx::log2_pow2(len);
  const u64* leaves = reinterpret_cast<const u64*>(A.cw + A.cw_off[rnd]);
  const u64* nodes = reinterpret_cast<const u64*>(A.nodes + A.node_off[rnd]);
  const int tid = threadIdx.x;
  if (tid < NC) reinterpret_cast<u64*>(A.values)[q * NC + tid] = leaves[idx * NC + tid];
  if (tid == 0) A.signs[q] = 0;
  const u64 e0 = mzk_tx::fri_entry_base(A.n, T, layer, kind) + s * (u64)depth;
  const int l = tid;
  if (l >= 1 && l < depth) {
    const u64 start = len - (len >> (l - 1));
    const u64* src = nodes + 4 * (start + ((idx >> l) ^ 1));
    u64* dst = reinterpret_cast<u64*>(A.paths + (e0 + l) * mzk_tx::PATH_STRIDE_GL);
#pragma unroll
    for (int k = 0; k < 4; k++) dst[k] = src[k];
#pragma unroll
    for (int k = 4; k < SLOT_WORDS; k++) dst[k] = 0;
    A.lens[e0 + l] = 32;
  }
  if (tid < SLOT_WORDS) slot[tid] = 0;
  __syncthreads();
  if (tid == 0) {
    const u64 sib = idx ^ 1;
    u64 c[NC];
#pragma unroll
    for (int k = 0; k < NC; k++) c[k] = leaves[sib * NC + k];
    u8* bytes = reinterpret_cast<u8*>(slot);
    leaf_len = gl::leaf_bytes<NC>(c, 0, [&](int pos, u32 byte) { bytes[pos] = (u8)byte; });
  }
  __syncthreads();
  if (tid < SLOT_WORDS) reinterpret_cast<u64*>(A.paths + e0 * mzk_tx::PATH_STRIDE_GL)[tid] = slot[tid];
  if (tid == 0) A.lens[e0] = (u64)leaf_len;
}

// Validation shared by the entry points; fills the layout.  Nothing is enqueued.  gl: the mzk_fri_*_gl entry points (field ids 3 and 4
// only, 64-byte path entries); otherwise ids 0 and 1 only.
static int fri_prove_check(int field_id, size_t n, size_t expansion_factor, size_t tests, mzk_tx::FriLayout* L, bool gl = false) {
  const char* who = gl ? "fri_prove_gl" : "fri_prove";
  if (gl) {
    if (!field_is_gl(field_id)) { set_error("fri_prove_gl: bad field id %d", field_id); return MZK_E_ARG; }
  } else MZK_TRY(field_check(field_id, "fri_prove"));
  if (n == 0) { set_error("%s: empty codeword", who); return MZK_E_LENGTH; }
  if (!is_pow2(n)) { set_error("%s: codeword length must be a power of two", who); return MZK_E_NOT_POW2; }
  if (gl) mzk_tx::fri_layout_gl(n, expansion_factor, tests, field_limbs64(field_id), L);
  else mzk_tx::fri_layout(n, expansion_factor, tests, field_limbs64(field_id), L);
  if (L->rounds < 2) {
    set_error("%s: num_rounds = %d for domain length %zu, expansion factor %zu, %zu colinearity tests; FRI::prove reads codewords[1] (fri.rs:117-121)",
              who, L->rounds, n, expansion_factor, tests);
    return MZK_E_LENGTH;
  }
  if (tests > L->last_len) {
    set_error("cannot sample more indices than available in last codeword; requested: %zu, available: %llu", tests, (unsigned long long)L->last_len);
    return MZK_E_ARG;
  }
  if (L->rounds > 63) { set_error("%s: too many rounds", who); return MZK_E_LENGTH; }
  // expansion factor 0 with no tests halves down to ONE element, which has no tree (and an id-4 leaf no room in a root record)
  if (gl && L->last_len < 2) { set_error("fri_prove_gl: a one-element last round"); return MZK_E_LENGTH; }
  return MZK_OK;
}

static int fri_prove_impl(int field_id, const void* src, const void* negative, bool on_device, size_t n, const uint64_t* omega, const uint64_t* offset,
                          size_t expansion_factor, size_t tests, void* proof_out, size_t proof_cap, hipStream_t s_in, bool gl = false) {
  mzk_tx::FriLayout L;
  const char* who = gl ? "fri_prove_gl" : "fri_prove";
  MZK_TRY(fri_prove_check(field_id, n, expansion_factor, tests, &L, gl));
  if (!src || !omega || !offset || !proof_out) { set_error("%s: null pointer", who); return MZK_E_ARG; }
  if (proof_cap < L.total) { set_error("%s: proof buffer of %zu bytes, the layout needs %llu", who, proof_cap, (unsigned long long)L.total); return MZK_E_LENGTH; }
  if (gl) {      // canonical words; omega and offset of id 4 in the base field, as everywhere (mzk.h)
    MZK_TRY(gl_param_check(field_id, omega, who, "parameter", true));
    MZK_TRY(gl_param_check(field_id, offset, who, "parameter", true));
  } else if (!h_is_canonical(host_field(field_id), omega) || !h_is_canonical(host_field(field_id), offset)) {
    set_error("fri_prove: parameter not canonical");
    return MZK_E_RANGE;
  }
  MZK_ENTER();
  WsFrame ws("fri_prove_impl");
  hipStream_t s = on_device ? s_in : ctx().stream;
  WsGuard wsg(s);
  const int R = L.rounds, nl = field_limbs64(field_id);
  const size_t esz = field_bytes(field_id);
  auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
  // one workspace block: codewords of all rounds | digests of all rounds | round-0 magnitudes and signs | transcript | alphas | seen
  // bits | the proof (host form).  Every tree lives here until the query kernel is done.
  size_t cw_total = 0, node_total = 0;
  uint64_t cw_off[64], node_off[64];
  for (int r = 0; r < R; r++) { cw_off[r] = cw_total; node_off[r] = node_total; cw_total += (n >> r) * esz; node_total += ((n >> r) - 1) * 32; }
  const size_t o_nodes = al(cw_total), o_mag = o_nodes + al(node_total), o_neg = o_mag + (negative ? al(n * esz) : 0);
  const size_t o_tx = o_neg + (negative && !on_device ? al(n) : 0);
  const size_t o_alpha = o_tx + al((gl ? mzk_tx::fri_transcript_cap_gl(L, nl) : mzk_tx::fri_transcript_cap(L, nl)) + 16), o_seen = o_alpha + al(32 * (size_t)R);
  const size_t o_proof = o_seen + al((L.last_len + 31) / 32 * 4), total = o_proof + (on_device ? 0 : al(L.total));
  uint8_t* blk;
  MZK_TRY(ws.get(WS_MISC_F, total, (void**)&blk));
  uint8_t* cw = blk;
  uint8_t* nodes = blk + o_nodes;
  uint8_t* proof = on_device ? (uint8_t*)proof_out : blk + o_proof;
  u64* tx = (u64*)(blk + o_tx);
  u64* alphas = (u64*)(blk + o_alpha);
  const hipMemcpyKind kind = on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
  MZK_HIP(hipMemcpyAsync(cw, src, n * esz, kind, s));
  const u8* d_neg = nullptr;
  const u32* mag0 = (const u32*)cw;
  if (negative) {      // round 0 commits to the magnitudes with their signs (fri.rs:160-166); the fold reads the canonical values
    MZK_HIP(hipMemcpyAsync(blk + o_mag, src, n * esz, kind, s));
    mag0 = (const u32*)(blk + o_mag);
    if (on_device) d_neg = (const u8*)negative;
    else {
      MZK_HIP(hipMemcpyAsync(blk + o_neg, negative, n, hipMemcpyHostToDevice, s));
      d_neg = blk + o_neg;
    }
  }
  uint64_t om[4] = {0, 0, 0, 0}, of[4] = {0, 0, 0, 0};
  memcpy(om, omega, 8 * nl);
  memcpy(of, offset, 8 * nl);
  FriFoldConsts fc;
  MZK_TRY(fri_fold_consts(field_id, of, om, &fc));
  for (int r = 0; r < R; r++) {
    const size_t len = n >> r;
    const void* leaves = r == 0 ? (const void*)mag0 : (const void*)(cw + cw_off[r]);
    u64* nd = (u64*)(nodes + node_off[r]);
    MZK_TRY(merkle_hash_levels(0, field_id, leaves, nullptr, len, nd, s, r == 0 ? d_neg : nullptr));
    const bool last = r == R - 1;
    hipLaunchKernelGGL(gl ? k_fri_tx_round_gl : k_fri_tx_round, dim3(1), dim3(64), 0, s, tx, r, (const u64*)(nd + 4 * (len - 2)),
                       (u64*)(proof + L.off[mzk_tx::SEC_ROOTS] + 32 * (size_t)r), alphas + 4 * r, last ? 0 : 1);
    MZK_HIP(hipGetLastError());
    if (r == 0 && negative) {
      MZK_TRY(canonicalize_signed(field_id, cw, d_neg, n, s));
    }
    if (last) break;
    MZK_TRY(fri_fold_dev_alpha(field_id, cw + cw_off[r], len, alphas + 4 * r, fc, cw + cw_off[r + 1], s));
    fri_fold_consts_square(field_id, &fc);
  }
  const u32* last_cw = (const u32*)(cw + cw_off[R - 1]);
  auto sec = [&](int k) { return proof + L.off[k]; };
  if (gl) {
    MZK_TRY(with_gl(field_id, [&](auto tag) {
      hipLaunchKernelGGL((k_fri_tx_last_gl<decltype(tag)::NC>), dim3(1), dim3(TX_LAST_THREADS), 0, s, (u8*)tx, R, (const u64*)last_cw, (size_t)L.last_len, n / 2, tests,
                         (u32*)(blk + o_seen), (u64*)sec(mzk_tx::SEC_STATUS), (u64*)sec(mzk_tx::SEC_TOP_INDICES), (u64*)sec(mzk_tx::SEC_LAST_CODEWORD));
      return MZK_OK;
    }));
  } else {
    MZK_TRY(MZK_FIELD_LAUNCH(field_id, k_fri_tx_last<P::NW>, dim3(1), dim3(TX_LAST_THREADS), 0, s, (u8*)tx, R, last_cw, (size_t)L.last_len, n / 2, tests, (u32*)(blk + o_seen), (u64*)sec(mzk_tx::SEC_STATUS), (u64*)sec(mzk_tx::SEC_TOP_INDICES), (u32*)sec(mzk_tx::SEC_LAST_CODEWORD)));
  }
  MZK_HIP(hipGetLastError());
  const size_t queries = 3 * tests * (size_t)(R - 1);
  if (queries) {
    FriQueryArgs A;
    A.cw = cw; A.nodes = nodes; A.mag0 = mag0; A.neg0 = d_neg; A.top = (const u64*)sec(mzk_tx::SEC_TOP_INDICES);
    A.values = sec(mzk_tx::SEC_VALUES); A.signs = sec(mzk_tx::SEC_SIGNS); A.paths = sec(mzk_tx::SEC_PATHS); A.lens = (u64*)sec(mzk_tx::SEC_PATH_LENS);
    A.n = n; A.tests = tests;
    for (int r = 0; r < 64; r++) { A.cw_off[r] = r < R ? cw_off[r] : 0; A.node_off[r] = r < R ? node_off[r] : 0; }
    if (gl) {
      MZK_TRY(with_gl(field_id, [&](auto tag) {
        hipLaunchKernelGGL((k_fri_query_gl<decltype(tag)::NC>), dim3((unsigned)queries), dim3(64), 0, s, A);
        return MZK_OK;
      }));
    } else {
      MZK_TRY(MZK_FIELD_LAUNCH(field_id, k_fri_query<P::NW>, dim3((unsigned)queries), dim3(64), 0, s, A));
    }
    MZK_HIP(hipGetLastError());
  }
  if (on_device) return MZK_OK;
  MZK_TRY(d2h_sync(proof_out, proof, L.total, s));
  uint64_t status;
  memcpy(&status, proof_out, 8);
  if (status != 0) {
    set_error("%s: sample_indices found %zu distinct reduced indices in %llu counters", who, tests, (unsigned long long)mzk_tx::SAMPLE_COUNTER_LIMIT);
    return MZK_E_RANGE;
  }
  return MZK_OK;
}

// mzk_fri_proof_layout / _gl: host only
static int fri_proof_layout_impl(int field_id, size_t n, size_t expansion_factor, size_t num_colinearity_tests, int* num_rounds, uint64_t* offsets,
                                 uint64_t* sizes, uint64_t* total_bytes, bool gl) {
  mzk_tx::FriLayout L;
  MZK_TRY(fri_prove_check(field_id, n, expansion_factor, num_colinearity_tests, &L, gl));
  if (num_rounds) *num_rounds = L.rounds;
  for (int k = 0; k < mzk_tx::SEC_COUNT; k++) {
    if (offsets) offsets[k] = L.off[k];
    if (sizes) sizes[k] = L.size[k];
  }
  if (total_bytes) *total_bytes = L.total;
  return MZK_OK;
}

}  // namespace mzk

extern "C" {

int mzk_fri_proof_layout(int field_id, size_t n, size_t expansion_factor, size_t num_colinearity_tests, int* num_rounds, uint64_t* offsets,
                         uint64_t* sizes, uint64_t* total_bytes) {
  return fri_proof_layout_impl(field_id, n, expansion_factor, num_colinearity_tests, num_rounds, offsets, sizes, total_bytes, false);
}
int mzk_fri_proof_layout_gl(int gl_field_id, size_t n, size_t expansion_factor, size_t num_colinearity_tests, int* num_rounds, uint64_t* offsets,
                            uint64_t* sizes, uint64_t* total_bytes) {
  return fri_proof_layout_impl(gl_field_id, n, expansion_factor, num_colinearity_tests, num_rounds, offsets, sizes, total_bytes, true);
}
int mzk_fri_prove(int field_id, const uint64_t* magnitudes, const uint8_t* negative, size_t n, const uint64_t* omega, const uint64_t* offset,
                  size_t expansion_factor, size_t num_colinearity_tests, uint8_t* proof_out, size_t proof_cap) {
  return fri_prove_impl(field_id, magnitudes, negative, false, n, omega, offset, expansion_factor, num_colinearity_tests, proof_out, proof_cap, nullptr);
}
int mzk_fri_prove_dev(int field_id, const void* d_magnitudes, const void* d_negative, size_t n, const uint64_t* omega, const uint64_t* offset,
                      size_t expansion_factor, size_t num_colinearity_tests, void* d_proof, size_t proof_cap, void* stream) {
  return fri_prove_impl(field_id, d_magnitudes, d_negative, true, n, omega, offset, expansion_factor, num_colinearity_tests, d_proof, proof_cap,
                        (hipStream_t)stream);
}
// FRI::prove over the Goldilocks ids: canonical elements only (no signs), 64-byte path entries
int mzk_fri_prove_gl(int gl_field_id, const uint64_t* codeword, size_t n, const uint64_t* omega, const uint64_t* offset, size_t expansion_factor,
                     size_t num_colinearity_tests, uint8_t* proof_out, size_t proof_cap) {
  return fri_prove_impl(gl_field_id, codeword, nullptr, false, n, omega, offset, expansion_factor, num_colinearity_tests, proof_out, proof_cap, nullptr, true);
}
int mzk_fri_prove_gl_dev(int gl_field_id, const void* d_codeword, size_t n, const uint64_t* omega, const uint64_t* offset, size_t expansion_factor,
                         size_t num_colinearity_tests, void* d_proof, size_t proof_cap, void* stream) {
  return fri_prove_impl(gl_field_id, d_codeword, nullptr, true, n, omega, offset, expansion_factor, num_colinearity_tests, d_proof, proof_cap, (hipStream_t)stream,
                        true);
}

}  // extern "C"
