// mzk_das_plan.h -- how the row, column and data-root Merkle trees of a batch of data-availability squares are hashed (mzk_das.hip),
// decided on the host before anything is launched: the item form of every tree, the trees a workgroup takes, grids, LDS bytes and
// the node storage a handle keeps, a pure function of (rows, cols, squares); and which views of a byte matrix are admitted.  Host-only
// C++17 with no HIP include, so that all of it can be compiled and checked on its own (tests/test_hostcheck_das_plan.py).
//
// The tree is Merkle::commit (algebra/merkle.rs:15-25) over one-byte leaves: a slice splits at mid = len / 2, so at depth
// D = floor(log2 n) there are M = 2^D subtrees ("items") of one or two leaves and a full binary tree above them (the identity
// k_merkle_ragged_items documents).  Item p is found by walking the bits of p from the root: 0 = the floor half, 1 = the ceil half.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include "../../include/mzk.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MZK_DAS_HD __host__ __device__
#else
#define MZK_DAS_HD
#endif

namespace mzk {

constexpr size_t DAS_MIN_N = 2;                          // from two leaves on every root is a 32-byte digest
constexpr size_t DAS_MAX_N = 255;                        // the codes' own bound (mzk_rs_plan.h RS_MAX_N)
constexpr size_t DAS_MAX_TREES = (size_t)1 << 31;        // squares * (rows + cols)
constexpr unsigned DAS_TREE_BLOCK = 256;                 // threads per workgroup of k_das_trees
constexpr unsigned DAS_WG_ITEMS = 512;                   // items per workgroup: G = DAS_WG_ITEMS / M trees, two items per lane at the bottom
constexpr unsigned DAS_NODE = 32;                        // bytes of a stored node (a one-leaf item: the byte, then zeros)
constexpr size_t DAS_TREE_LDS = 2 * DAS_WG_ITEMS * DAS_NODE;      // every level of the G trees, items to roots
constexpr unsigned DAS_ROOT_BLOCK = 512;                 // k_das_data_roots: one lane pair per item, at most 256 items
constexpr size_t DAS_ROOT_LDS = 2 * 256 * DAS_NODE;     // two levels, ping-pong
constexpr size_t DAS_MAX_GRID = (size_t)1 << 20;         // workgroups of one launch; more work is walked in `iters` rounds
constexpr size_t DAS_MAX_LDS = 64 * 1024;                // static LDS: no opt-in for large dynamic LDS is needed

struct DasTree { int n, depth, items; };                 // leaves, D, M = 2^D
struct DasLaunch {
  size_t grid;
  unsigned block;
  unsigned iters;
  size_t lds;
};

struct DasPlan {
  int err = MZK_OK;
  char msg[160] = {0};
  size_t rows = 0, cols = 0, squares = 0;
  DasTree row_tree = {}, col_tree = {}, root_tree = {};          // a row tree has `cols` leaves, a column tree `rows`, the data-root tree rows + cols
  size_t row_trees = 0, col_trees = 0;                            // squares * rows, squares * cols: flat, square-major
  unsigned row_g = 0, col_g = 0;                                  // trees per workgroup
  size_t row_wgs = 0, col_wgs = 0;                                // workgroups' worth of work: row trees first, then column trees
  DasLaunch trees = {}, roots = {};
  size_t row_node_bytes = 0, col_node_bytes = 0;                  // items and every level below the roots, level-major over the flat trees
  size_t root_bytes = 0, symbol_bytes = 0, handle_bytes = 0;      // row, column and data roots; the copy of the symbols; all a handle keeps
};

static inline DasTree das_tree(size_t n) {
  DasTree t;
  t.n = (int)n;
  t.depth = 0;
  while (((size_t)2 << t.depth) <= n) t.depth++;
  t.items = 1 << t.depth;
  return t;
}

// Item p of a tree of n leaves, M = 2^depth items: its first leaf and its size (1 or 2).
MZK_DAS_HD static inline void das_item(int n, int depth, int p, int* start, int* size) {
  int s = 0, k = n;
  for (int b = depth - 1; b >= 0; b--) {
    const int l = k / 2;
    if ((p >> b) & 1) { s += l; k -= l; } else k = l;
  }
  *start = s;
  *size = k;
}
// The item that holds leaf `index`: p, its first leaf, its size and the size of its sibling item p ^ 1 (depth >= 1).
MZK_DAS_HD static inline void das_locate(int n, int depth, int index, int* p, int* start, int* size, int* sib_size) {
  int s = 0, k = n, q = 0, parent = n;
  for (int b = depth - 1; b >= 0; b--) {
    const int l = k / 2;
    parent = k;
    if (index >= s + l) { s += l; k -= l; q = 2 * q + 1; } else { k = l; q = 2 * q; }
  }
  *p = q; *start = s; *size = k; *sib_size = parent - k;
}
// Entries of Merkle::open(index) (merkle.rs:28-46): depth + 1 from a two-leaf item, depth from a one-leaf item beside a one-leaf item,
// 0 where the reference recurses forever (a one-leaf item beside a two-leaf one: the 1 | 2 split of a three-leaf slice).
MZK_DAS_HD static inline int das_path_depth(int depth, int size, int sib_size) { return size == 2 ? depth + 1 : (sib_size == 1 ? depth : 0); }

// Slot h of a workgroup's item phase (h < DAS_WG_ITEMS) -> tree g of its G = 2^g_log trees and item p of that tree.  Row trees: the lanes
// run along a tree's items.  Column trees: the lanes run along the G adjacent columns, so that one step down the rows reads G contiguous bytes.
MZK_DAS_HD static inline void das_item_slot(bool col, int h, int depth, int g_log, int* g, int* p) {
  if (col) { *g = h & ((1 << g_log) - 1); *p = h >> g_log; }
  else { *g = h >> depth; *p = h & ((1 << depth) - 1); }
}

// nodes of level l (0 = the items) of T trees of M items start this many nodes into the side's storage; level `depth` is the roots
MZK_DAS_HD static inline size_t das_level_offset(size_t trees, int items, int level) { return trees * (2 * (size_t)items - ((2 * (size_t)items) >> level)); }

static inline DasLaunch das_launch(size_t wgs, unsigned block, size_t lds) {
  DasLaunch L;
  L.block = block;
  L.lds = lds;
  L.grid = wgs < DAS_MAX_GRID ? wgs : DAS_MAX_GRID;
  L.iters = (unsigned)((wgs + L.grid - 1) / L.grid);
  return L;
}

// The view: symbol (r, c) of square q at base + q * square_stride + r * row_stride + c.
static inline DasPlan das_plan(size_t rows, size_t cols, size_t row_stride, size_t square_stride, size_t squares) {
  DasPlan P;
  auto refuse = [&](const char* fmt, size_t a, size_t b, size_t c) { P.err = MZK_E_ARG; snprintf(P.msg, sizeof P.msg, fmt, a, b, c); return P; };
  if (rows < DAS_MIN_N || rows > DAS_MAX_N) return refuse("das: rows = %zu is outside 2 .. 255 (the codes' own bound; a one-leaf tree commits to the leaf itself)", rows, 0, 0);
  if (cols < DAS_MIN_N || cols > DAS_MAX_N) return refuse("das: cols = %zu is outside 2 .. 255 (the codes' own bound; a one-leaf tree commits to the leaf itself)", cols, 0, 0);
  if (squares < 1 || squares > DAS_MAX_TREES / (rows + cols))
    return refuse("das: squares = %zu is outside 1 .. 2^31 / (rows + cols) = %zu", squares, DAS_MAX_TREES / (rows + cols), 0);
  if (row_stride < cols) return refuse("das: row_stride = %zu is below cols = %zu", row_stride, cols, 0);
  if (row_stride > ((size_t)1 << 40) || square_stride > ((size_t)1 << 40)) return refuse("das: row_stride = %zu / square_stride = %zu is beyond 2^40", row_stride, square_stride, 0);
  if (squares > 1 && square_stride < (rows - 1) * row_stride + cols)
    return refuse("das: square_stride = %zu is below (rows - 1) * row_stride + cols = %zu: the squares overlap", square_stride, (rows - 1) * row_stride + cols, 0);
  P.rows = rows; P.cols = cols; P.squares = squares;
  P.row_tree = das_tree(cols);
  P.col_tree = das_tree(rows);
  P.root_tree = das_tree(rows + cols);
  P.row_trees = squares * rows;
  P.col_trees = squares * cols;
  P.row_g = DAS_WG_ITEMS / (unsigned)P.row_tree.items;
  P.col_g = DAS_WG_ITEMS / (unsigned)P.col_tree.items;
  P.row_wgs = (P.row_trees + P.row_g - 1) / P.row_g;
  P.col_wgs = (P.col_trees + P.col_g - 1) / P.col_g;
  P.trees = das_launch(P.row_wgs + P.col_wgs, DAS_TREE_BLOCK, DAS_TREE_LDS);
  P.roots = das_launch(squares, DAS_ROOT_BLOCK, DAS_ROOT_LDS);
  P.row_node_bytes = das_level_offset(P.row_trees, P.row_tree.items, P.row_tree.depth) * DAS_NODE;
  P.col_node_bytes = das_level_offset(P.col_trees, P.col_tree.items, P.col_tree.depth) * DAS_NODE;
  P.root_bytes = (P.row_trees + P.col_trees + squares) * DAS_NODE;
  P.symbol_bytes = squares * rows * cols;
  P.handle_bytes = P.row_node_bytes + P.col_node_bytes + P.root_bytes + P.symbol_bytes;
  return P;
}

// the ABI's view of a plan (include/mzk.h: MZK_DAS_PLAN_WORDS values)
static inline void das_plan_export(const DasPlan& P, uint64_t* o) {
  o[MZK_DAS_PLAN_ROWS] = P.rows; o[MZK_DAS_PLAN_COLS] = P.cols; o[MZK_DAS_PLAN_SQUARES] = P.squares;
  o[MZK_DAS_PLAN_ROW_ITEMS] = (uint64_t)P.row_tree.items; o[MZK_DAS_PLAN_ROW_DEPTH] = (uint64_t)P.row_tree.depth;
  o[MZK_DAS_PLAN_COL_ITEMS] = (uint64_t)P.col_tree.items; o[MZK_DAS_PLAN_COL_DEPTH] = (uint64_t)P.col_tree.depth;
  o[MZK_DAS_PLAN_ROOT_ITEMS] = (uint64_t)P.root_tree.items; o[MZK_DAS_PLAN_ROOT_DEPTH] = (uint64_t)P.root_tree.depth;
  o[MZK_DAS_PLAN_ROW_TREES_PER_WG] = P.row_g; o[MZK_DAS_PLAN_COL_TREES_PER_WG] = P.col_g;
  o[MZK_DAS_PLAN_ROW_WGS] = P.row_wgs; o[MZK_DAS_PLAN_COL_WGS] = P.col_wgs;
  o[MZK_DAS_PLAN_TREE_GRID] = P.trees.grid; o[MZK_DAS_PLAN_TREE_ITERS] = P.trees.iters; o[MZK_DAS_PLAN_TREE_BLOCK] = P.trees.block; o[MZK_DAS_PLAN_TREE_LDS] = P.trees.lds;
  o[MZK_DAS_PLAN_ROOT_GRID] = P.roots.grid; o[MZK_DAS_PLAN_ROOT_ITERS] = P.roots.iters; o[MZK_DAS_PLAN_ROOT_BLOCK] = P.roots.block; o[MZK_DAS_PLAN_ROOT_LDS] = P.roots.lds;
  o[MZK_DAS_PLAN_NODE_BYTES] = P.handle_bytes;
  o[MZK_DAS_PLAN_PATH_MAX] = MZK_DAS_PATH_MAX;
}

}  // namespace mzk
