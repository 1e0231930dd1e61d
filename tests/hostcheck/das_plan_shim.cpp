// The plan of Celestia's commitment (myzkp_amd/csrc/mzk_das_plan.h) run on the host for tests/test_hostcheck_das_plan.py.  Stand-alone,
// no arguments.  Prints
//   T n depth items <item sizes as digits>           for every leaf count 2 .. 510 (das_tree, das_item)
//   L n <per leaf: path depth as a digit>            for every leaf count 2 .. 255 (das_locate, das_path_depth), after checking in place
//                                                    that das_locate agrees with das_item
//   S col n trees bad                                the item phase of every workgroup walked slot by slot (das_item_slot): bad = (tree, item)
//                                                    pairs not taken exactly once, or taken by a slot outside the workgroup's trees
//   K rows cols  row_items row_depth col_items col_depth root_items root_depth row_g col_g      for every admitted (rows, cols)
//   B squares  row_wgs col_wgs  grid block iters lds (trees)  grid block iters lds (roots)  row_node_bytes col_node_bytes root_bytes
//              symbol_bytes handle_bytes  exported_node_bytes                                     for every squares of that (rows, cols)
//   R rows cols row_stride square_stride squares err <message>                                   for every refused shape
// then "ok <shapes>".  Built once plain and once with -fsanitize=address,undefined.
#include <inttypes.h>
#include <stdio.h>
#include <string.h>
#include <vector>
#include "../../myzkp_amd/csrc/mzk_das_plan.h"

using namespace mzk;

static long walk_slots(bool col, int n, size_t trees) {
  const DasTree t = das_tree((size_t)n);
  const int G = (int)DAS_WG_ITEMS / t.items;
  int g_log = 0;
  while ((1 << g_log) < G) g_log++;
  const size_t wgs = (trees + (size_t)G - 1) / (size_t)G;
  std::vector<int> taken(trees * (size_t)t.items, 0);
  long bad = 0;
  for (size_t wg = 0; wg < wgs; wg++)
    for (int h = 0; h < (int)DAS_WG_ITEMS; h++) {
      int g, p;
      das_item_slot(col, h, t.depth, g_log, &g, &p);
      if (g < 0 || g >= G || p < 0 || p >= t.items) { bad++; continue; }
      const size_t tree = wg * (size_t)G + (size_t)g;
      if (tree >= trees) continue;                          // the kernel skips the slot
      taken[tree * (size_t)t.items + (size_t)p]++;
    }
  for (int v : taken) bad += v != 1;
  return bad;
}

int main() {
  for (int n = 2; n <= 510; n++) {
    const DasTree t = das_tree((size_t)n);
    printf("T %d %d %d ", n, t.depth, t.items);
    int at = 0;
    for (int p = 0; p < t.items; p++) {
      int start, size;
      das_item(n, t.depth, p, &start, &size);
      if (start != at) { fprintf(stderr, "n = %d: item %d starts at %d, not %d\n", n, p, start, at); return 1; }
      at += size;
      printf("%d", size);
    }
    if (at != n) { fprintf(stderr, "n = %d: items cover %d leaves\n", n, at); return 1; }
    printf("\n");
  }
  for (int n = 2; n <= 255; n++) {
    const DasTree t = das_tree((size_t)n);
    printf("L %d ", n);
    for (int i = 0; i < n; i++) {
      int p, start, size, sib, s2, z2, s3, z3;
      das_locate(n, t.depth, i, &p, &start, &size, &sib);
      das_item(n, t.depth, p, &s2, &z2);
      das_item(n, t.depth, p ^ 1, &s3, &z3);
      if (s2 != start || z2 != size || z3 != sib || i < start || i >= start + size) { fprintf(stderr, "n = %d leaf %d: das_locate disagrees with das_item\n", n, i); return 1; }
      printf("%d", das_path_depth(t.depth, size, sib));
    }
    printf("\n");
  }
  for (int col = 0; col < 2; col++)
    for (int n = 2; n <= 255; n++) {
      const size_t counts[] = {1, (size_t)n, 2 * (size_t)n + 1, 3 * (size_t)n, n <= 17 ? 65 * (size_t)n : 5};
      for (size_t trees : counts) printf("S %d %d %zu %ld\n", col, n, trees, walk_slots(col != 0, n, trees));
    }

  const size_t squares[] = {1, 2, 3, 64, 65, (size_t)1 << 20};
  size_t shapes = 0;
  for (size_t rows = 2; rows <= 255; rows++)
    for (size_t cols = 2; cols <= 255; cols++) {
      const DasPlan P0 = das_plan(rows, cols, cols, rows * cols, 1);
      if (P0.err != MZK_OK) { fprintf(stderr, "(%zu, %zu) refused: %s\n", rows, cols, P0.msg); return 1; }
      printf("K %zu %zu  %d %d %d %d %d %d %u %u\n", rows, cols, P0.row_tree.items, P0.row_tree.depth, P0.col_tree.items, P0.col_tree.depth, P0.root_tree.items,
             P0.root_tree.depth, P0.row_g, P0.col_g);
      for (size_t q : squares) {
        const DasPlan P = das_plan(rows, cols, cols + 3, rows * (cols + 3) + 7, q);         // a strided view: the plan does not depend on the strides
        if (P.err != MZK_OK || P.row_g != P0.row_g || P.col_g != P0.col_g || P.row_tree.items != P0.row_tree.items || P.col_tree.items != P0.col_tree.items) {
          fprintf(stderr, "(%zu, %zu, %zu): plan depends on the batch or the strides: %s\n", rows, cols, q, P.msg);
          return 1;
        }
        uint64_t E[MZK_DAS_PLAN_WORDS];
        das_plan_export(P, E);
        printf("B %zu  %zu %zu  %zu %u %u %zu  %zu %u %u %zu  %zu %zu %zu %zu %zu  %" PRIu64 "\n", q, P.row_wgs, P.col_wgs, P.trees.grid, P.trees.block, P.trees.iters, P.trees.lds,
               P.roots.grid, P.roots.block, P.roots.iters, P.roots.lds, P.row_node_bytes, P.col_node_bytes, P.root_bytes, P.symbol_bytes, P.handle_bytes, E[MZK_DAS_PLAN_NODE_BYTES]);
      }
      shapes++;
    }
  const size_t big = (size_t)1 << 31;
  const size_t refused[][5] = {
      {0, 8, 8, 0, 1}, {1, 8, 8, 8, 1}, {256, 8, 8, 2048, 1}, {8, 0, 0, 0, 1}, {8, 1, 1, 8, 1}, {8, 256, 256, 2048, 1},
      {8, 8, 7, 64, 1}, {8, 8, 8, 63, 2}, {8, 8, 11, 84, 2}, {8, 8, 8, 64, 0}, {8, 8, 8, 64, big / 16 + 1}, {255, 255, 255, 65025, big / 510 + 1}, {2, 2, 2, 4, big}};
  for (const auto& r : refused) {
    const DasPlan P = das_plan(r[0], r[1], r[2], r[3], r[4]);
    printf("R %zu %zu %zu %zu %zu %d %s\n", r[0], r[1], r[2], r[3], r[4], P.err, P.msg);
  }
  // the largest admitted batches are admitted
  if (das_plan(8, 8, 8, 64, big / 16).err != MZK_OK || das_plan(255, 255, 255, 65025, big / 510).err != MZK_OK || das_plan(2, 2, 2, 4, big / 4).err != MZK_OK ||
      das_plan(8, 8, 8, 63, 1).err != MZK_OK || das_plan(8, 8, 11, 85, 2).err != MZK_OK) {
    fprintf(stderr, "an admitted boundary shape was refused\n");
    return 1;
  }
  printf("ok %zu\n", shapes);
  return 0;
}
