// mzk_merkle_plan.h -- which kernels hash the levels of a Merkle tree (merkle_hash_levels, mzk_merkle.hip), decided on the host before
// anything is launched: a short list of steps, a pure function of the leaf count, the tree count and the leaf kind.  Host-only C++17
// with no HIP include, so that the schedule can be compiled and checked on its own (tests/test_hostcheck_merkle_plan.py).
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace mzk {

constexpr int LEAF_THREADS = 128;                       // threads per workgroup of every leaf kernel
constexpr size_t LEAF_PAIR_MAX = (size_t)1 << 15;      // pairs: up to here field leaves are hashed by lane pairs (k_merkle_leaf_pairs_lp)
constexpr size_t LEVEL_PAIR_MAX = 16384;               // hashes: up to here an inner level is hashed by lane pairs (level_pair, level_pair_multi)
constexpr int TAIL_NODES = 512;                         // the most nodes k_merkle_tail takes: the last levels in one workgroup

// What the leaves are.  MERKLE_LEAVES_FIELD: Fr / M128 elements, by lane pairs up to LEAF_PAIR_MAX pairs; MERKLE_LEAVES_FIELD_PLAIN: the
// same with the lane-pair kernel switched off (tuning build, MZK_LEAF_LANE_PAIRS=0): one lane per pair at every size.
enum MerkleLeafKind { MERKLE_LEAVES_FIELD = 0, MERKLE_LEAVES_FIELD_PLAIN = 1, MERKLE_LEAVES_GL = 2, MERKLE_LEAVES_BYTES = 3 };

enum MerkleKernel {
  MK_LEAF_LP = 0,      // k_merkle_leaf_pairs_lp<NW>: two lanes per leaf pair
  MK_LEAF_PLAIN = 1,   // k_merkle_leaf_pairs<NW>: one lane per leaf pair
  MK_LEAF_GL = 2,      // k_merkle_leaf_pairs_gl<NC>
  MK_LEAF_BYTES = 3,   // k_merkle_leaf_pairs_bytes
  MK_LEVEL = 4,        // k_merkle_level: one lane per hash
  MK_LEVEL_PAIR = 5,   // k_merkle_level_pair: two lanes per hash
  MK_MULTI2 = 6,       // k_merkle_level_pair_multi<2>: two levels in one launch
  MK_MULTI3 = 7,       // k_merkle_level_pair_multi<3>: three
  MK_TAIL = 8          // k_merkle_tail: every remaining level in one workgroup
};

// One launch.  It reads `nodes_in` nodes (the leaves for a leaf step, else the digests of the level below, which end where its own
// output begins), hashes `parents` of them into its first output level and halves on through `levels` levels in all; that first level
// starts `out_offset` digests into the tree's digest array (level 1, level 2, ... back to back: n - trees digests).
struct MerkleStep {
  int kernel;
  size_t nodes_in, parents;
  int levels;
  size_t grid;         // workgroups (the launch takes 32 bits: checked by the host test for every size the ABI admits)
  unsigned block;      // threads per workgroup
  size_t out_offset;
};

constexpr int MERKLE_MAX_STEPS = 72;      // a leaf step, at most one step per level of a 2^64-leaf tree, a tail
struct MerklePlan {
  int nsteps = 0;
  MerkleStep steps[MERKLE_MAX_STEPS];
};

// n leaves in all, `trees` trees of one power-of-two size back to back (n = trees * leaves per tree).  Level l of the whole array is
// level l of every tree side by side, so the plan hashes down to `trees` nodes: the roots.  n < 2: nothing to hash.
static inline MerklePlan merkle_plan(size_t n, size_t trees, int leaf_kind) {
  MerklePlan P;
  if (n < 2) return P;
  auto push = [&](int kernel, size_t nodes_in, size_t parents, int levels, size_t grid, unsigned block, size_t out_offset) {
    P.steps[P.nsteps++] = MerkleStep{kernel, nodes_in, parents, levels, grid, block, out_offset};
  };
  const size_t pairs = n / 2;
  const size_t blocks = (pairs + 127) / 128;
  if (leaf_kind == MERKLE_LEAVES_BYTES) push(MK_LEAF_BYTES, n, pairs, 1, blocks, 128, 0);
  else if (leaf_kind == MERKLE_LEAVES_GL) push(MK_LEAF_GL, n, pairs, 1, blocks, LEAF_THREADS, 0);
  else if (leaf_kind == MERKLE_LEAVES_FIELD && pairs <= LEAF_PAIR_MAX)
    push(MK_LEAF_LP, n, pairs, 1, (pairs + LEAF_THREADS / 2 - 1) / (LEAF_THREADS / 2), LEAF_THREADS, 0);
  else push(MK_LEAF_PLAIN, n, pairs, 1, blocks, LEAF_THREADS, 0);
  size_t at = 0, count = pairs;      // the level below: `count` digests from digest `at` on
  while (count > (size_t)TAIL_NODES && count > trees) {
    const size_t above = at + count;
    if (count / 2 <= LEVEL_PAIR_MAX && (count >> 3) >= (size_t)TAIL_NODES && (count >> 3) >= trees) {          // three levels in one launch
      push(MK_MULTI3, count, count / 2, 3, (count / 2 + 255) / 256, 512, above);
      at = above + count / 2 + count / 4;
      count >>= 3;
      continue;
    }
    if (count / 2 <= LEVEL_PAIR_MAX && (count >> 2) >= (size_t)TAIL_NODES && (count >> 2) >= trees) {          // two
      push(MK_MULTI2, count, count / 2, 2, (count / 2 + 127) / 128, 256, above);
      at = above + count / 2;
      count >>= 2;
      continue;
    }
    if (count / 2 <= LEVEL_PAIR_MAX) push(MK_LEVEL_PAIR, count, count / 2, 1, (count + 127) / 128, 128, above);
    else push(MK_LEVEL, count, count / 2, 1, (count / 2 + 127) / 128, 128, above);
    at = above;
    count /= 2;
  }
  if (count > trees) {
    int levels = 0;
    for (size_t c = count; c > trees; c /= 2) levels++;
    push(MK_TAIL, count, count / 2, levels, 1, (unsigned)TAIL_NODES, at + count);
  }
  return P;
}

}  // namespace mzk
