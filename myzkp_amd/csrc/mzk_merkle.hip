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
#include "mzk_elem.h"
#include "mzk_merkle.h"           // the handle type and what mzk_fri.hip calls of this file
#include "mzk_keccak.h"           // keccak_f: the permutation by one lane
#include "mzk_keccak_pair.h"
#include "mzk_gl.h"
#include "mzk_merkle_plan.h"      // the level schedule and its thresholds (LEAF_PAIR_MAX, LEVEL_PAIR_MAX, TAIL_NODES)
#include "mzk_merkle_open_plan.h" // openings: the scratch and output layout, host_leaf, the unpack

namespace mzk {

typedef uint64_t u64;
typedef uint8_t u8;

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
    gload_words<NW>(elems, 2 * i + e, w);
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
    gload_words<NW>(elems, 2 * i, w0);
    int k0 = 0;
#pragma unroll
    for (int j = 0; j < NW; j++) if (w0[j]) k0 = j + 1;
    if (parity) {
      gload_words<NW>(elems, 2 * i + 1, w);
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
int canonicalize_signed(int fid, void* d_elems, const void* d_neg, size_t n, hipStream_t s) {
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

namespace mzk {

// end of a successful build on stream s of the current context
// complete_on_return: the caller synchronizes the stream before it hands the tree out (mzk_fri_commit does once, after its last round --
// since round 6 a round's root reaches the transcript through the mailbox without a synchronize; an error return frees the trees, and
// hipFree waits for the device), so there is nothing to order later calls behind: no event (one marker packet per round less)
int merkle_stamp(mzk_merkle* t, hipStream_t s, bool complete_on_return) {
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
int merkle_hash_levels(int kind, int fid, const void* d_leaves, const u64* d_off, size_t n, u64* d_nodes, hipStream_t s,
                       const u8* d_neg, size_t trees, u32* mailbox, u32 seq, bool* mailed) {
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
static u32 g_mailbox_seq[MZK_MAX_CTX];        // per context: the number of the last root a tail kernel was asked to post
int merkle_mailbox(RootMailbox* mb) {
  Context& c = ctx();
  if (!c.bounce) MZK_HIP(hipHostMalloc(&c.bounce, SMALL_D2H_MAX, hipHostMallocPortable));
  static const int enabled = tune_int("MZK_ROOT_MAILBOX", 1);     // tuning build: 0 = copy + synchronize (A/B)
  mb->p = enabled ? (u32*)c.bounce + 512 : nullptr;                 // the second half of the landing zone: d2h_sync uses the first bytes
  mb->seq = ++g_mailbox_seq[c.index];
  if (mb->seq == 0) mb->seq = ++g_mailbox_seq[c.index];
  if (mb->p) ((volatile u32*)mb->p)[8] = 0;                         // (a larger d2h_sync may have run over this half since the last root)
  return MZK_OK;
}
int merkle_root_to_host(uint8_t* root, const u64* d_root, const RootMailbox& mb, bool mailed, hipStream_t s) {
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

// (the leaf bytes of one element on the host: host_leaf, mzk_merkle_open_plan.h)
MerkleOwner merkle_new(int kind, int fid, size_t n, hipStream_t stream) {
  MerkleOwner t(new mzk_merkle());
  t->kind = kind; t->field = fid; t->n = n; t->stream = stream;
  t->ragged = !is_pow2(n);
  if (t->ragged) {      // the item tree: m = 2^floor(log2 n) items (k_merkle_ragged_items)
    while (((size_t)2 << t->depth) <= n) t->depth++;
    t->m = (size_t)1 << t->depth;
  } else {
    t->depth = (int)ilog2(n);
  }
  return t;
}
int merkle_single_leaf_root(int fid, const void* d_leaf, bool negative, uint8_t* out, size_t cap, size_t* len, hipStream_t stream) {
  uint64_t limbs[4];
  uint8_t buf[HOST_LEAF_MAX];
  MZK_TRY(d2h_sync(limbs, d_leaf, field_bytes(fid), stream));
  *len = host_leaf(fid, limbs, buf, negative);
  if (cap < *len) return MZK_E_LENGTH;
  memcpy(out, buf, *len);
  return MZK_OK;
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
  MerkleOwner t = merkle_new(1, -1, n, s);
  const int D = t->depth;
  const size_t m = t->m;
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
  u64 *d_off, *d_ioff;
  u32* d_ns;
  MZK_TRY(t->own_leaves.alloc(leaf_bytes ? leaf_bytes : 16, "merkle: leaves"));
  MZK_TRY(t->own_items.alloc(io ? io : 16, "merkle: items"));
  MZK_TRY(t->own_nodes.alloc((m - 1) * 32, "merkle: digests"));
  t->d_leaves = t->own_leaves.get(); t->d_items = t->own_items.get(); t->d_nodes = t->own_nodes.as<u64>();
  MZK_TRY(ws.get(WS_MISC_D, (n + 1) * 8, (void**)&d_off));
  MZK_TRY(ws.get(WS_MISC_E, (m + 1) * 8, (void**)&d_ioff));
  MZK_TRY(ws.get(WS_MISC_F, (m + 1) * 4, (void**)&d_ns));
  if (leaf_bytes) MZK_HIP(hipMemcpyAsync(t->d_leaves, leaves, leaf_bytes, hipMemcpyHostToDevice, s));
  MZK_HIP(hipMemcpyAsync(d_off, offsets, (n + 1) * 8, hipMemcpyHostToDevice, s));
  MZK_HIP(hipMemcpyAsync(d_ioff, t->item_off.data(), (m + 1) * 8, hipMemcpyHostToDevice, s));
  MZK_HIP(hipMemcpyAsync(d_ns, t->node_start.data(), (m + 1) * 4, hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(k_merkle_ragged_items, dim3((unsigned)((m + 127) / 128)), dim3(128), 0, s, (const u8*)t->d_leaves, (const u64*)d_off, (const u32*)d_ns, m,
                     (const u64*)d_ioff, (u8*)t->d_items);
  MZK_TRY(merkle_hash_levels(1, -1, t->d_items, d_ioff, m, t->d_nodes, s));
  MZK_HIP(hipStreamSynchronize(s));
  MZK_TRY(merkle_stamp(t.get(), s));
  *out = t.release();
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
  MerkleOwner t = merkle_new(kind, fid, n, s);
  MZK_TRY(t->own_leaves.alloc(leaf_bytes ? leaf_bytes : 16, "merkle: leaves"));
  t->d_leaves = t->own_leaves.get();
  if (leaf_bytes) MZK_HIP(hipMemcpyAsync(t->d_leaves, src, leaf_bytes, src_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s));
  if (n > 1) MZK_TRY(t->own_nodes.alloc((n - 1) * 32, "merkle: digests"));
  t->d_nodes = t->own_nodes.as<u64>();
  u64* d_off = nullptr;
  if (kind == 1) {
    t->offsets.assign(offsets, offsets + n + 1);
    MZK_TRY(ws.get(WS_MISC_D, (n + 1) * 8, (void**)&d_off));
    MZK_HIP(hipMemcpyAsync(d_off, offsets, (n + 1) * 8, hipMemcpyHostToDevice, s));
  }
  u8* d_neg = nullptr;
  if (kind == 0 && neg_host) {
    t->neg.assign(neg_host, neg_host + n);
    MZK_TRY(ws.get(WS_MISC_E, n, (void**)&d_neg));
    MZK_HIP(hipMemcpyAsync(d_neg, neg_host, n, hipMemcpyHostToDevice, s));
  }
  MZK_TRY(merkle_hash_levels(kind, fid, t->d_leaves, d_off, n, t->d_nodes, s, d_neg));
  if (kind == 1) MZK_HIP(hipStreamSynchronize(s));
  MZK_TRY(merkle_stamp(t.get(), s));
  *out = t.release();
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
    size_t len = 0;
    if (t->kind == 0) {
      const int rc = merkle_single_leaf_root(t->field, t->d_leaves, !t->neg.empty() && t->neg[0], root, cap, &len, ms.s);
      if (rc == MZK_E_LENGTH) set_error("merkle_root: buffer too small (%zu < %zu)", cap, len);
      MZK_TRY(rc);
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
  // Byte leaves.  Either form of tree names the entries that lead the path (device source, length), the size of the tree the digests
  // are gathered from and the position in it; the digests follow the leading entries.
  struct { const uint8_t* src; size_t len; } lead[2];
  int n_lead = 0;
  size_t size, pos;
  if (t->ragged) {
    // subtree p (depth D) that holds the leaf.  Merkle::open only terminates when its descent ends in a TWO-leaf
    // slice (merkle.rs:32-34); a one-leaf slice recurses forever (mid = 0), so those indices are an error here.
    const size_t p = (size_t)(std::upper_bound(t->node_start.begin(), t->node_start.end(), (uint32_t)index) - t->node_start.begin()) - 1;
    const uint32_t first = t->node_start[p], cnt = t->node_start[p + 1] - first;
    const size_t sibp = p ^ 1;
    const uint32_t sib_cnt = t->node_start[sibp + 1] - t->node_start[sibp];
    if (cnt == 1 && sib_cnt != 1) {
      set_error("merkle_open: leaf %zu is the one-leaf half of a three-leaf slice; Merkle::open recurses forever there (merkle.rs:36-45)", index);
      return MZK_E_LENGTH;
    }
    // cnt == 2: the recursion ends inside subtree p (entry 0 = the other leaf), then climbs the item tree;
    // cnt == 1 with a one-leaf sibling: it ends one level higher, on the two-leaf slice {p, p ^ 1} -- the item path itself.
    if (cnt == 2) {
      const size_t other = first + (1 - (index - first));
      lead[n_lead++] = {(const uint8_t*)t->d_leaves + t->offsets[other], (size_t)(t->offsets[other + 1] - t->offsets[other])};
    }
    lead[n_lead++] = {(const uint8_t*)t->d_items + t->item_off[sibp], (size_t)(t->item_off[sibp + 1] - t->item_off[sibp])};   // sibling item: a leaf or a digest
    size = t->m;
    pos = p;
  } else {
    const size_t sib = index ^ 1;      // entry 0 is the sibling LEAF, verbatim
    lead[n_lead++] = {(const uint8_t*)t->d_leaves + t->offsets[sib], (size_t)(t->offsets[sib + 1] - t->offsets[sib])};
    size = t->n;
    pos = index;
  }
  const int k = n_lead - 1;      // the digest of level l is entry l + k
  for (int e = 0; e < n_lead; e++)
    if (stride < lead[e].len) { set_error("merkle_open: stride %zu < %s length %zu", stride, t->ragged ? "entry" : "leaf", lead[e].len); return MZK_E_LENGTH; }
  for (int e = 0; e < n_lead; e++) {
    if (lead[e].len) MZK_HIP(hipMemcpyAsync(path + (size_t)e * stride, lead[e].src, lead[e].len, hipMemcpyDeviceToHost, s));
    path_len[e] = lead[e].len;
  }
  if (t->depth > 1) {
    u64* d_out;
    MZK_TRY(ws.get(WS_MISC_C, (size_t)t->depth * 32, (void**)&d_out));
    hipLaunchKernelGGL(k_merkle_gather, dim3(1), dim3(64), 0, s, (const u64*)t->d_nodes, size, pos, t->depth, d_out);
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

}  // extern "C"

namespace mzk {
// what the batched openings serve: field-element trees of two or more leaves, a power of two of them (`t`: the tree's place in the call)
static int merkle_open_tree_check(const mzk_merkle* tr, size_t t, const char* who) {
  if (tr->n < 2) { set_error("merkle_open: needs at least two leaves (merkle.rs:32)"); return MZK_E_LENGTH; }
  if (tr->ragged || tr->kind != 0) {
    set_error("%s: field-element trees with a power-of-two leaf count only (tree %zu: %s); open its paths one by one", who, t,
              tr->kind != 0 ? "byte leaves" : "ragged");
    return MZK_E_ARG;
  }
  return MZK_OK;
}
// Openings of SEVERAL field-element trees in one gather and one synchronisation: what mzk_merkle_open_multi documents.  Tree t takes the
// next counts[t] entries of `indices`; the layout of the scratch and of paths / path_lens, and the unpack, are mzk_merkle_open_plan.h's.
int merkle_open_trees(const mzk_merkle* const* trees, size_t n_trees, const uint64_t* indices, const size_t* counts, uint8_t* paths, size_t stride,
                      uint64_t* path_lens, size_t* depths, const char* who) {
  if (!trees || !counts || !depths) { set_error("%s: null pointer", who); return MZK_E_ARG; }
  std::vector<MerkleOpenTree> plan(n_trees);
  MerkleOpenAt total;
  const mzk_merkle* first = nullptr;
  for (size_t t = 0; t < n_trees; t++) {
    const mzk_merkle* tr = trees[t];
    depths[t] = tr ? (size_t)tr->depth : 0;
    if (counts[t] == 0) continue;
    if (!tr || !indices || !paths || !path_lens) { set_error("%s: null pointer", who); return MZK_E_ARG; }
    MZK_TRY(merkle_open_tree_check(tr, t, who));
    for (size_t q = 0; q < counts[t]; q++)
      if (indices[total.index + q] >= tr->n) { set_error("merkle_open: index %llu out of range (tree %zu)", (unsigned long long)indices[total.index + q], t); return MZK_E_LENGTH; }
    if (!first) first = tr;
    if (tr->ctx_index != first->ctx_index || tr->device != first->device) {
      set_error("%s: tree %zu lives on context %d, the first opened tree on context %d; one call opens trees of one context", who, t, tr->ctx_index,
                first->ctx_index);
      return MZK_E_ARG;
    }
    plan[t].field = tr->field; plan[t].depth = tr->depth; plan[t].count = counts[t];
    plan[t].neg = tr->neg.empty() ? nullptr : tr->neg.data();
    total.advance(plan[t]);
  }
  if (total.index == 0) return MZK_OK;
  if (stride < 32) { set_error("merkle_open: stride < 32"); return MZK_E_LENGTH; }
  MZK_ENTER();
  WsFrame ws(who);
  MerkleScope ms(first);
  MZK_TRY(ms.rc);
  hipStream_t s = ms.s;
  for (size_t t = 0; t < n_trees; t++)      // every opened tree's build, not only the first one's (whose event MerkleScope has waited on)
    if (counts[t] && trees[t] != first && trees[t]->built) MZK_HIP(hipStreamWaitEvent(s, trees[t]->built, 0));
  WsGuard wsg(s);
  u64* d_idx;
  MZK_TRY(ws.get(WS_MISC_C, merkle_open_scratch_bytes(total), (void**)&d_idx));
  u64* d_on = d_idx + total.index;
  u32* d_ol = (u32*)(d_on + total.node);
  MZK_HIP(hipMemcpyAsync(d_idx, indices, total.index * 8, hipMemcpyHostToDevice, s));
  MerkleOpenAt at;
  for (size_t t = 0; t < n_trees; t++) {
    if (counts[t] == 0) continue;
    const mzk_merkle* tr = trees[t];
    hipLaunchKernelGGL(k_merkle_gather_batch, dim3((unsigned)counts[t]), dim3(64), 0, s, (const u64*)tr->d_nodes, (const u32*)tr->d_leaves, field_words(tr->field),
                       tr->n, (const u64*)(d_idx + at.index), tr->depth, d_on + at.node, d_ol + at.leaf);
    at.advance(plan[t]);
  }
  MZK_HIP(hipGetLastError());
  std::vector<uint64_t> hn(total.node + 1);
  std::vector<uint32_t> hl(total.leaf + 1);
  if (total.node) MZK_HIP(hipMemcpyAsync(hn.data(), d_on, total.node * 8, hipMemcpyDeviceToHost, s));
  MZK_TRY(d2h_sync(hl.data(), d_ol, total.leaf * 4, s));
  size_t bad_entry = 0, bad_len = 0;
  const int rc = merkle_open_unpack(plan.data(), n_trees, indices, hn.data(), hl.data(), paths, stride, path_lens, &bad_entry, &bad_len);
  if (rc != MZK_OK) set_error("merkle_open: stride %zu < leaf length %zu (path entry %zu)", stride, bad_len, bad_entry);
  return rc;
}
}  // namespace mzk

extern "C" {

// `count` openings of one tree: paths[(q * depth + l) * stride ..] / path_lens[q * depth + l] as mzk_merkle_open writes them
// for index indices[q]; *depth entries per path.  Field-element trees with a power-of-two leaf count (every codeword of
// the provers): ONE gather launch and ONE copy for all paths.  Byte-leaf and ragged trees: MZK_E_ARG (open one by one).
int mzk_merkle_open_batch(const mzk_merkle* t, const uint64_t* indices, size_t count, uint8_t* paths, size_t stride, uint64_t* path_lens,
                          size_t* depth) {
  if (!t || !depth) { set_error("merkle_open_batch: null pointer"); return MZK_E_ARG; }
  if (count == 0) {      // nothing to open: the tree is still refused if it could not be opened, and *depth is written; no context is entered
    MZK_TRY(merkle_open_tree_check(t, 0, "merkle_open_batch"));
    *depth = (size_t)t->depth;
    return MZK_OK;
  }
  return merkle_open_trees(&t, 1, indices, &count, paths, stride, path_lens, depth, "merkle_open_batch");
}

// Openings of SEVERAL trees in one call: the query phase of FRI::prove (fri.rs:127-137, reveal :211-260) opens the a / b indices
// in round i's tree and the c indices in round i+1's, for every round -- with the trees of mzk_fri_commit_keep_trees that is one
// call, one copy back and one synchronisation instead of two of each per round (48 us per call measured).  Tree t takes the
// next counts[t] entries of `indices`; its paths follow tree t-1's in paths / path_lens, laid out as mzk_merkle_open_batch
// lays them out with depths[t] entries per path.  counts[t] == 0 skips tree t (which may then be NULL).
int mzk_merkle_open_multi(const mzk_merkle* const* trees, size_t n_trees, const uint64_t* indices, const size_t* counts, uint8_t* paths,
                          size_t stride, uint64_t* path_lens, size_t* depths) {
  return merkle_open_trees(trees, n_trees, indices, counts, paths, stride, path_lens, depths, "merkle_open_multi");
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
    const int rc = merkle_single_leaf_root(field_id, d_elems, false, root, cap, root_len, s);
    if (rc == MZK_E_LENGTH) set_error("merkle: root buffer too small");
    return rc;
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
