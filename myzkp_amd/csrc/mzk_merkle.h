// mzk_merkle.h -- what FRI::commit and FRI::prove (mzk_fri.hip) use of the SHA3 Merkle trees of mzk_merkle.hip: the handle type, the
// level hashing, the root mailbox and the host form of one leaf.  Host code only; the definitions are in mzk_merkle.hip.
#pragma once
#include "mzk_common.h"

struct mzk_merkle {
  int kind;              // 0 = field elements, 1 = byte leaves
  int field;
  size_t n;
  int depth;             // log2 n
  mzk::u64* d_nodes;     // n - 1 digests: level 1 (n/2), level 2 (n/4), ..., root
  void* d_leaves;        // copy of the elements / the leaf bytes (needed by open and by n == 1)
  mzk::DevMem own_nodes, own_leaves, own_items;     // what d_nodes, d_leaves and d_items point to, where the handle owns it alone
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
  std::shared_ptr<mzk::DevMem> shared;
  bool ragged = false;
  size_t m = 0;
  void* d_items = nullptr;
  std::vector<uint64_t> item_off;
  std::vector<uint32_t> node_start;
};

namespace mzk {

int canonicalize_signed(int fid, void* d_elems, const void* d_neg, size_t n, hipStream_t s);
int merkle_stamp(mzk_merkle* t, hipStream_t s, bool complete_on_return = false);
int merkle_hash_levels(int kind, int fid, const void* d_leaves, const u64* d_off, size_t n, u64* d_nodes, hipStream_t s,
                       const uint8_t* d_neg = nullptr, size_t trees = 1, u32* mailbox = nullptr, u32 seq = 0, bool* mailed = nullptr);
struct RootMailbox { u32* p; u32 seq; };
int merkle_mailbox(RootMailbox* mb);
int merkle_root_to_host(uint8_t* root, const u64* d_root, const RootMailbox& mb, bool mailed, hipStream_t s);
size_t host_leaf(int fid, const uint64_t* limbs, uint8_t* out, bool negative = false);

}  // namespace mzk
