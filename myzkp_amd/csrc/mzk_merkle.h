// mzk_merkle.h -- what FRI::commit and FRI::prove (mzk_fri.hip) use of the SHA3 Merkle trees of mzk_merkle.hip: the handle type, the
// level hashing, the root mailbox and the host form of one leaf.  Host code only; the definitions are in mzk_merkle.hip.
#pragma once
#include <memory>
#include "mzk_common.h"
#include "mzk_merkle_open_plan.h"      // host_leaf, HOST_LEAF_MAX

struct mzk_merkle {       // made by merkle_new alone
  int kind = 0;          // 0 = field elements, 1 = byte leaves
  int field = -1;
  size_t n = 0;
  int depth = 0;         // log2 n (ragged: floor(log2 n), the depth of the item tree)
  mzk::u64* d_nodes = nullptr;     // n - 1 digests: level 1 (n/2), level 2 (n/4), ..., root
  void* d_leaves = nullptr;        // copy of the elements / the leaf bytes (needed by open and by n == 1)
  mzk::DevMem own_nodes, own_leaves, own_items;     // what d_nodes, d_leaves and d_items point to, where the handle owns it alone
  std::vector<uint64_t> offsets;   // byte leaves only
  std::vector<uint8_t> neg;        // field leaves given as (magnitude, sign): 1 = Sign::Minus; empty = all non-negative
  hipStream_t stream = nullptr;    // the stream the tree was BUILT on (a caller stream for the *_dev builders); never used again
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
  std::shared_ptr<mzk::DevMem> shared;
  bool ragged = false;
  size_t m = 0;
  void* d_items = nullptr;
  std::vector<uint64_t> item_off;
  std::vector<uint32_t> node_start;
};

namespace mzk {

// A handle over n leaves with kind, field, n, stream, depth -- and for a leaf count that is no power of two `ragged` and m -- filled in,
// owning nothing on the device yet.  The owner frees it (mzk_merkle_free) unless released.
struct MerkleFree { void operator()(mzk_merkle* t) const { mzk_merkle_free(t); } };
typedef std::unique_ptr<mzk_merkle, MerkleFree> MerkleOwner;
MerkleOwner merkle_new(int kind, int fid, size_t n, hipStream_t stream);
// "The root of a one-leaf tree is the leaf itself" (merkle.rs:17-19) for a field element on the device: its leaf bytes to out, their
// length to *len; the stream is idle on return.  MZK_E_LENGTH without a message when cap is below *len: the caller words it.
int merkle_single_leaf_root(int fid, const void* d_leaf, bool negative, uint8_t* out, size_t cap, size_t* len, hipStream_t stream);
// mzk_merkle_open_multi under the name `who` of the entry point that was called (its messages start with it)
int merkle_open_trees(const mzk_merkle* const* trees, size_t n_trees, const uint64_t* indices, const size_t* counts, uint8_t* paths, size_t stride,
                      uint64_t* path_lens, size_t* depths, const char* who);
int canonicalize_signed(int fid, void* d_elems, const void* d_neg, size_t n, hipStream_t s);
int merkle_stamp(mzk_merkle* t, hipStream_t s, bool complete_on_return = false);
int merkle_hash_levels(int kind, int fid, const void* d_leaves, const u64* d_off, size_t n, u64* d_nodes, hipStream_t s,
                       const uint8_t* d_neg = nullptr, size_t trees = 1, u32* mailbox = nullptr, u32 seq = 0, bool* mailed = nullptr);
struct RootMailbox { u32* p; u32 seq; };
int merkle_mailbox(RootMailbox* mb);
int merkle_root_to_host(uint8_t* root, const u64* d_root, const RootMailbox& mb, bool mailed, hipStream_t s);

}  // namespace mzk
