// mzk_merkle_open_plan.h -- the host side of opening field-element Merkle trees (merkle_open_trees, mzk_merkle.hip): where each opened
// tree's share of the gather scratch and of the caller's output lies, the leaf bytes of one element, and the unpack of what the gather
// kernel left into paths / path_lens.  Host-only C++17 with no HIP include, so that the index arithmetic can be compiled and checked on
// its own (tests/test_hostcheck_merkle_open.py).  Nothing here touches the device, the workspace or the error text.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>
#include "../../include/mzk.h"
#include "mzk_hostfield.h"        // field_is_gl, field_limbs64, field_words
#include "mzk_transcript.h"       // mzk_tx::fri_leaf_put, and through it gl::leaf_bytes

namespace mzk {

// The leaf bytes of one element of field `fid` on the host (at most HOST_LEAF_MAX: a 59-byte M64X3 leaf is the longest): used for
// the root of a one-leaf tree and for the sibling leaf of an authentication path (both are a copy of input bytes, not computation).
// Fr / M128: bincode(FiniteFieldElement) of the magnitude and its sign.
constexpr size_t HOST_LEAF_MAX = 64;
inline size_t host_leaf(int fid, const uint64_t* limbs, uint8_t* out, bool negative = false) {
  if (field_is_gl(fid)) {
    auto put = [&](int pos, uint32_t byte) { out[pos] = (uint8_t)byte; };
    return (size_t)(fid == MZK_FIELD_M64X3 ? gl::leaf_bytes<3>(limbs, 0, put) : gl::leaf_bytes<1>(limbs, 0, put));
  }
  uint32_t w[8];
  const int nl = field_limbs64(fid);
  memcpy(w, limbs, 8 * (size_t)nl);
  return (size_t)(nl == 2 ? mzk_tx::fri_leaf_put<4>(w, negative, out) : mzk_tx::fri_leaf_put<8>(w, negative, out));
}

// One tree of a call as the layout and the unpack see it: it takes the next `count` indices.  count == 0: the tree is skipped and the
// other members are not read.  neg: its Sign::Minus flags by leaf, or null (every leaf non-negative).
struct MerkleOpenTree {
  int field = -1;
  int depth = 0;
  size_t count = 0;
  const uint8_t* neg = nullptr;
};

// Where a tree's share begins, in elements of each array: `index` in the index list, `node` in the gathered digests (u64 words: count x
// (depth - 1) digests of 4), `leaf` in the gathered sibling limbs (u32 words: count x field_words) and `entry` in paths / path_lens
// (count x depth entries).  After the last tree: the totals.
struct MerkleOpenAt {
  size_t index = 0, node = 0, leaf = 0, entry = 0;
  void advance(const MerkleOpenTree& t) {      // past tree t's share
    if (t.count == 0) return;
    index += t.count;
    node += t.count * (size_t)(t.depth - 1) * 4;
    leaf += t.count * (size_t)field_words(t.field);
    entry += t.count * (size_t)t.depth;
  }
};
inline MerkleOpenAt merkle_open_totals(const MerkleOpenTree* trees, size_t n_trees) {
  MerkleOpenAt at;
  for (size_t t = 0; t < n_trees; t++) at.advance(trees[t]);
  return at;
}
// The scratch of one call is [indices | digests | sibling limbs]: the u64 word at which the digests begin is total.index, the sibling
// limbs begin total.node words behind that.
inline size_t merkle_open_scratch_bytes(const MerkleOpenAt& total) { return total.index * 8 + total.node * 8 + total.leaf * 4 + 64; }

// Gathered digests `nodes` and sibling limbs `leaves` (both laid out as above) -> the caller's paths and path_lens: per opened index
// `depth` entries `stride` bytes apart -- entry 0 the sibling leaf's bytes, entry l the sibling digest of level l -- and their lengths.
// An entry receives its bytes and no more: what lies behind them in the stride stays the caller's.
// MZK_E_LENGTH: a sibling leaf of *bad_len bytes does not fit the stride; *bad_entry is its entry, and nothing was written from that
// entry on.
inline int merkle_open_unpack(const MerkleOpenTree* trees, size_t n_trees, const uint64_t* indices, const uint64_t* nodes, const uint32_t* leaves,
                              uint8_t* paths, size_t stride, uint64_t* path_lens, size_t* bad_entry, size_t* bad_len) {
  MerkleOpenAt at;
  for (size_t t = 0; t < n_trees; t++) {
    const MerkleOpenTree& tr = trees[t];
    if (tr.count == 0) continue;
    const size_t lw = (size_t)field_words(tr.field), depth = (size_t)tr.depth;
    for (size_t q = 0; q < tr.count; q++) {
      uint64_t limbs[4] = {0, 0, 0, 0};
      memcpy(limbs, leaves + at.leaf + q * lw, lw * 4);
      uint8_t buf[HOST_LEAF_MAX];
      const size_t sib = (size_t)indices[at.index + q] ^ 1;
      const size_t len = host_leaf(tr.field, limbs, buf, tr.neg && tr.neg[sib]);
      const size_t entry = at.entry + q * depth;
      if (stride < len) { *bad_entry = entry; *bad_len = len; return MZK_E_LENGTH; }
      memcpy(paths + entry * stride, buf, len);
      path_lens[entry] = len;
      for (size_t l = 1; l < depth; l++) {
        memcpy(paths + (entry + l) * stride, nodes + at.node + (q * (depth - 1) + (l - 1)) * 4, 32);
        path_lens[entry + l] = 32;
      }
    }
    at.advance(tr);
  }
  return MZK_OK;
}

}  // namespace mzk
