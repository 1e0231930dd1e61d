// The Merkle level schedule (merkle_plan, myzkp_amd/csrc/mzk_merkle_plan.h) run on the host for tests/test_hostcheck_merkle_plan.py.
// Stand-alone: reads "n trees leaf_kind" lines from the file given as argv[1] and prints, per line,
//   P n trees leaf_kind nsteps  { kernel nodes_in parents levels grid block out_offset } x nsteps
// then the thresholds and "ok <lines>".  Built with -fsanitize=address,undefined.
#include <inttypes.h>
#include <stdio.h>
#include "../../myzkp_amd/csrc/mzk_merkle_plan.h"

using namespace mzk;

int main(int argc, char** argv) {
  if (argc < 2) { fprintf(stderr, "usage: merkle_plan_shim shapes.txt\n"); return 2; }
  FILE* f = fopen(argv[1], "r");
  if (!f) { perror(argv[1]); return 2; }
  uint64_t n, trees;
  int kind;
  size_t lines = 0;
  while (fscanf(f, "%" SCNu64 " %" SCNu64 " %d", &n, &trees, &kind) == 3) {
    const MerklePlan P = merkle_plan((size_t)n, (size_t)trees, kind);
    if (P.nsteps < 0 || P.nsteps > MERKLE_MAX_STEPS) { fprintf(stderr, "step count %d out of range\n", P.nsteps); return 1; }
    printf("P %" PRIu64 " %" PRIu64 " %d %d", n, trees, kind, P.nsteps);
    for (int i = 0; i < P.nsteps; i++) {
      const MerkleStep& s = P.steps[i];
      printf(" %d %zu %zu %d %zu %u %zu", s.kernel, s.nodes_in, s.parents, s.levels, s.grid, s.block, s.out_offset);
    }
    printf("\n");
    lines++;
  }
  fclose(f);
  printf("T %zu %zu %d %d\n", LEAF_PAIR_MAX, LEVEL_PAIR_MAX, TAIL_NODES, LEAF_THREADS);
  printf("ok %zu\n", lines);
  return 0;
}
