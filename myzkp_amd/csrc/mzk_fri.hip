// mzk_fri.hip -- FRI::commit and FRI::prove (zkstark/fri.rs:99-260) over the SHA3 Merkle trees of mzk_merkle.hip: the host driver of the
// commit rounds, and the prover in one enqueue with the Fiat-Shamir proof stream, the index sampling and the query phase on the device.
#include "mzk_common.h"
#include "mzk_merkle.h"
#include "mzk_keccak_pair.h"
#include "mzk_gl.h"
#include "mzk_transcript.h"

using namespace mzk;

extern "C" {

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
      size_t leaf_len = 0;
      const int rc = merkle_single_leaf_root(field_id, cur, r == 0 && negative && negative[0], root, 48, &leaf_len, s);
      if (rc == MZK_E_LENGTH) set_error("fri_commit: the one-element round %d does not fit the 48-byte root slot (%zu bytes)", r, leaf_len);
      MZK_TRY(rc);
      root_len[r] = leaf_len;
    } else {
      RootMailbox mb;
      bool mailed = false;
      MZK_TRY(merkle_mailbox(&mb));
      MZK_TRY(merkle_hash_levels(0, field_id, cur, nullptr, len, d_nodes, s, r == 0 ? d_neg : nullptr, 1, mb.p, mb.seq, &mailed));
      if (trees_out) {      // keep this round's tree: its leaves and digests stay where they were computed, in the shared block
        mzk_merkle* t = (trees_out[r] = merkle_new(0, field_id, len, s).release());      // fri_commit_impl frees trees_out on failure
        t->d_nodes = d_nodes; t->d_leaves = cur;
        t->shared = shared;
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
}  // extern "C"

// ================================================================================================================================
// FRI::prove (zkstark/fri.rs:99-143) in one enqueue: commit (:144-209) with the proof stream on the device, sample_indices
// (:19-62) and reveal (:211-260).  Per round r the Merkle tree is hashed as in mzk_fri_commit; then k_fri_tx_round appends
// vec![root_r] to the device transcript, rehashes the whole serialization with SHAKE256 and writes alpha_r; the fold reads it
// from there.  After the last root k_fri_tx_last pushes the last codeword, squeezes the index seed and samples the top-level
// indices; k_fri_query gathers every layer's values and paths into the packed proof.  No host round trip inside.
// The three kernels are written once over a leaf form of mzk_transcript.h: FriLeafLimbs<NW> for M128 and Fr (mzk_fri_prove, 48-byte path
// entries), FriLeafGl<NC> for the Goldilocks ids (mzk_fri_prove_gl, 64-byte path entries, no signs).
namespace mzk {

// Round r of the proof stream: push vec![root_r] (u64 1 | u64 32 | root), the object count becomes r + 1; unless this is the
// last round, alpha_r = F::sample(SHAKE256(stream)[0 .. 32)) (fri.rs:168-176) into `alpha` (4 limbs, canonical: < 2^64).
// REDUCE_GL: the sample taken mod the Goldilocks prime (mzk_tx::sample_gl) -- the base value, which id 4 embeds as (v, 0, 0): `alpha`
// takes the same four words, the fold reads the first NC.
template <bool REDUCE_GL>
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
  const u64 w3 = ((u64)dig[7] << 32) | dig[6];
  if (tid < 4) alpha[tid] = tid == 0 ? (REDUCE_GL ? mzk_tx::sample_gl(w3) : mzk_tx::sample_digest_word3(w3)) : 0;
}

// After the last root: push the last codeword (one object of m records, each u64 length + the element's leaf: LEAF::record_put), squeeze
// the seed (fri.rs:114-123), sample the top-level indices (fri.rs:40-62) and write status / indices / last codeword into the proof.
// A record's position is the prefix sum of the record lengths before it, a workgroup's worth of records per step; the stream is then
// rehashed by one lane pair (about 65 SHAKE blocks at m = 128 over M64X3).
// size = n / 2, reduced = m (powers of two: the reductions are masks).  One workgroup; `seen` holds m bits (global scratch).
constexpr int TX_LAST_THREADS = 256;
template <class LEAF>
__global__ __launch_bounds__(TX_LAST_THREADS) void k_fri_tx_last(u8* __restrict__ tx, int rounds, const typename LEAF::word* __restrict__ cw, size_t m,
                                                                  size_t size, size_t number, u32* __restrict__ seen, u64* __restrict__ p_status,
                                                                  u64* __restrict__ p_top, typename LEAF::word* __restrict__ p_last) {
  constexpr int W = LEAF::WORDS;
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
    typename LEAF::word w[W];
#pragma unroll
    for (int q = 0; q < W; q++) w[q] = 0;
    if (j < m) {
#pragma unroll
      for (int q = 0; q < W; q++) { w[q] = cw[j * W + q]; p_last[j * W + q] = w[q]; }
    }
    const u64 rec = j < m ? LEAF::record_len(w) : 0;
    scan[tid] = rec;
    __syncthreads();
    for (int d = 1; d < TX_LAST_THREADS; d <<= 1) {          // inclusive scan of the record lengths
      const u64 add = tid >= d ? scan[tid - d] : 0;
      __syncthreads();
      scan[tid] += add;
      __syncthreads();
    }
    if (j < m) LEAF::record_put(w, false, tx + at + scan[tid] - rec);      // Sign::Plus / NoSign: the fold sanitized the codeword
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
// round i + 1's.  Writes the value (words and Sign::Minus flag) and the path exactly as mzk_merkle_open_batch returns it: entry 0 the
// sibling's leaf bytes, serialised in LDS, entries 1 .. depth-1 the digests; LEAF::STRIDE bytes per entry, zero-padded, lengths beside.
struct FriQueryArgs {
  const u8* cw;          // all rounds' codewords back to back
  const u8* nodes;       // all rounds' digests back to back
  const u8* leaves0;     // round 0's leaves as committed (the magnitudes, when signed; else the codeword itself)
  const u8* neg0;        // round 0's Sign::Minus flags or null (always null for the Goldilocks ids)
  const u64* top;
  u8* values; u8* signs; u8* paths; u64* lens;
  u64 n, tests;
  u64 cw_off[64], node_off[64];     // byte offsets of round r's codeword / digests
};
template <class LEAF>
__global__ __launch_bounds__(64) void k_fri_query(FriQueryArgs A) {
  typedef typename LEAF::word word;
  constexpr int W = LEAF::WORDS, SLOT_WORDS = LEAF::STRIDE / 8;
  __shared__ u64 slot[SLOT_WORDS];
  __shared__ u64 leaf_len;
  const u64 T = A.tests, q = blockIdx.x;
  const int layer = (int)(q / (3 * T)), kind = (int)((q / T) % 3);
  const u64 s = q % T;
  const u64 half = (A.n >> layer) / 2;
  const u64 a = A.top[s] & (half - 1);
  const u64 idx = kind == 1 ? a + half : a;
  const int rnd = layer + (kind == 2);
  const u64 len = A.n >> rnd;
  const int depth = mzk_tx::log2_pow2(len);
  const word* leaves = reinterpret_cast<const word*>(rnd == 0 ? A.leaves0 : A.cw + A.cw_off[rnd]);
  const u8* neg = rnd == 0 ? A.neg0 : nullptr;
  const u64* nodes = reinterpret_cast<const u64*>(A.nodes + A.node_off[rnd]);
  const int tid = threadIdx.x;
  if (tid < W) reinterpret_cast<word*>(A.values)[q * W + tid] = leaves[idx * W + tid];
  if (tid == 0) A.signs[q] = neg ? neg[idx] : 0;
  const u64 e0 = mzk_tx::fri_entry_base(A.n, T, layer, kind) + s * (u64)depth;
  const int l = tid;
  if (l >= 1 && l < depth) {
    const u64 start = len - (len >> (l - 1));
    const u64* src = nodes + 4 * (start + ((idx >> l) ^ 1));
    u64* dst = reinterpret_cast<u64*>(A.paths + (e0 + l) * LEAF::STRIDE);
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
    word w[W];
#pragma unroll
    for (int k = 0; k < W; k++) w[k] = leaves[sib * W + k];
    leaf_len = LEAF::leaf_put(w, neg && neg[sib], reinterpret_cast<u8*>(slot));
  }
  __syncthreads();
  if (tid < SLOT_WORDS) reinterpret_cast<u64*>(A.paths + e0 * LEAF::STRIDE)[tid] = slot[tid];
  if (tid == 0) A.lens[e0] = leaf_len;
}

// The leaf form of a field id: f(FriLeafLimbs<NW>()) for M128 and Fr, f(FriLeafGl<NC>()) for the Goldilocks ids; f returns int.
template <class F> static int with_fri_leaf(int fid, F&& f) {
  if (field_is_gl(fid)) return with_gl(fid, [&](auto tag) { return f(mzk_tx::FriLeafGl<decltype(tag)::NC>()); });
  return with_field(fid, [&](auto tag) { return f(mzk_tx::FriLeafLimbs<decltype(tag)::P::NW>()); });
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
  mzk_tx::fri_layout_stride(n, expansion_factor, tests, field_limbs64(field_id), gl ? mzk_tx::PATH_STRIDE_GL : mzk_tx::PATH_STRIDE, L);
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

// The enqueue of one proof over the leaf form of the (validated) field id
template <class LEAF>
static int fri_prove_enqueue(int field_id, const mzk_tx::FriLayout& L, const void* src, const void* negative, bool on_device, size_t n, const uint64_t* omega,
                             const uint64_t* offset, size_t tests, void* proof_out, hipStream_t s_in, const char* who) {
  typedef typename LEAF::word word;
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
  const size_t o_alpha = o_tx + al(mzk_tx::fri_transcript_cap<LEAF>(L) + 16), o_seen = o_alpha + al(32 * (size_t)R);
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
  const u8* leaves0 = cw;
  if (negative) {      // round 0 commits to the magnitudes with their signs (fri.rs:160-166); the fold reads the canonical values
    MZK_HIP(hipMemcpyAsync(blk + o_mag, src, n * esz, kind, s));
    leaves0 = blk + o_mag;
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
    const void* leaves = r == 0 ? (const void*)leaves0 : (const void*)(cw + cw_off[r]);
    u64* nd = (u64*)(nodes + node_off[r]);
    MZK_TRY(merkle_hash_levels(0, field_id, leaves, nullptr, len, nd, s, r == 0 ? d_neg : nullptr));
    const bool last = r == R - 1;
    hipLaunchKernelGGL(k_fri_tx_round<LEAF::GL>, dim3(1), dim3(64), 0, s, tx, r, (const u64*)(nd + 4 * (len - 2)),
                       (u64*)(proof + L.off[mzk_tx::SEC_ROOTS] + 32 * (size_t)r), alphas + 4 * r, last ? 0 : 1);
    MZK_HIP(hipGetLastError());
    if (r == 0 && negative) {
      MZK_TRY(canonicalize_signed(field_id, cw, d_neg, n, s));
    }
    if (last) break;
    MZK_TRY(fri_fold_dev_alpha(field_id, cw + cw_off[r], len, alphas + 4 * r, fc, cw + cw_off[r + 1], s));
    fri_fold_consts_square(field_id, &fc);
  }
  auto sec = [&](int k) { return proof + L.off[k]; };
  hipLaunchKernelGGL(k_fri_tx_last<LEAF>, dim3(1), dim3(TX_LAST_THREADS), 0, s, (u8*)tx, R, (const word*)(cw + cw_off[R - 1]), (size_t)L.last_len, n / 2, tests,
                     (u32*)(blk + o_seen), (u64*)sec(mzk_tx::SEC_STATUS), (u64*)sec(mzk_tx::SEC_TOP_INDICES), (word*)sec(mzk_tx::SEC_LAST_CODEWORD));
  MZK_HIP(hipGetLastError());
  const size_t queries = 3 * tests * (size_t)(R - 1);
  if (queries) {
    FriQueryArgs A;
    A.cw = cw; A.nodes = nodes; A.leaves0 = leaves0; A.neg0 = d_neg; A.top = (const u64*)sec(mzk_tx::SEC_TOP_INDICES);
    A.values = sec(mzk_tx::SEC_VALUES); A.signs = sec(mzk_tx::SEC_SIGNS); A.paths = sec(mzk_tx::SEC_PATHS); A.lens = (u64*)sec(mzk_tx::SEC_PATH_LENS);
    A.n = n; A.tests = tests;
    for (int r = 0; r < 64; r++) { A.cw_off[r] = r < R ? cw_off[r] : 0; A.node_off[r] = r < R ? node_off[r] : 0; }
    hipLaunchKernelGGL(k_fri_query<LEAF>, dim3((unsigned)queries), dim3(64), 0, s, A);
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
  return with_fri_leaf(field_id, [&](auto leaf) {
    return fri_prove_enqueue<decltype(leaf)>(field_id, L, src, negative, on_device, n, omega, offset, tests, proof_out, s_in, who);
  });
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
