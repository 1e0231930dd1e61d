// The digit walk of the window-table layouts (raw_window / walk_digits_whole / digit_bias_word / walk_digits_merged<C>,
// myzkp_amd/csrc/mzk_msm_plan.h) run on the host for tests/test_hostcheck_digit_walk.py: the code the sort's kernels run, over scalars
// the test writes into a file.  A stand-alone program (built with -fsanitize=address,undefined; every scalar sits in a heap block of
// exactly its eight words, so a window read past the scalar is an AddressSanitizer report):
//     digit_walk_shim <scalars: one hex number below 2^256 per line> <table stride>
// prints, for scalar number i (used as the point index too),
//     W i c sets  slot key payload ...      walk_digits_whole, every layout: 8..22 bits with one bucket set, 14..17 with two and four
//     M i C  slot key payload ...           walk_digits_merged<C>, C = 8..22
// and "ok <scalars>" at the end.  The checking is the Python side's, in integers.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <utility>
#include <vector>
#include "../../myzkp_amd/csrc/mzk_msm_plan.h"

using namespace mzk;

static bool parse_hex(const char* line, uint32_t* w) {
  size_t len = strlen(line);
  while (len && (line[len - 1] == '\n' || line[len - 1] == '\r' || line[len - 1] == ' ')) len--;
  if (len == 0 || len > 64) return false;
  memset(w, 0, 8 * sizeof(uint32_t));
  for (size_t j = 0; j < len; j++) {
    const char ch = line[len - 1 - j];
    const int v = ch >= '0' && ch <= '9' ? ch - '0' : ch >= 'a' && ch <= 'f' ? ch - 'a' + 10 : -1;
    if (v < 0) return false;
    w[j / 8] |= (uint32_t)v << (4 * (j % 8));
  }
  return true;
}

struct Printer {
  void operator()(int slot, uint32_t key, uint32_t payload) const { printf(" %d %u %u", slot, key, payload); }
};

template <int C>
static void merged_one(const uint32_t* w, size_t stride, size_t i) {
  printf("M %zu %d", i, C);
  walk_digits_merged<C>(w, stride, i, Printer());
  printf("\n");
}
template <int... Cs>
static void merged_all(const uint32_t* w, size_t stride, size_t i, std::integer_sequence<int, Cs...>) {
  (merged_one<8 + Cs>(w, stride, i), ...);
}

static void whole_one(const uint32_t* w, size_t stride, size_t i, int c, int sets) {
  DigitLayout L{};
  L.c = c, L.nwin = msm_table_windows(c), L.merged = 1, L.sets = sets, L.table_stride = stride, L.glv = 0, L.phi_offset = 0;
  printf("W %zu %d %d", i, c, sets);
  walk_digits_whole(w, L, i, Printer());
  printf("\n");
}

int main(int argc, char** argv) {
  if (argc != 3) { fprintf(stderr, "usage: digit_walk_shim <scalars> <table stride>\n"); return 2; }
  FILE* f = fopen(argv[1], "r");
  if (!f) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
  const size_t stride = (size_t)strtoull(argv[2], nullptr, 10);
  char line[128];
  size_t i = 0;
  for (; fgets(line, sizeof line, f); i++) {
    uint32_t* w = (uint32_t*)malloc(8 * sizeof(uint32_t));
    if (!parse_hex(line, w)) { fprintf(stderr, "line %zu is no hex number below 2^256\n", i + 1); free(w); fclose(f); return 2; }
    for (int c = 8; c <= 22; c++) whole_one(w, stride, i, c, 1);
    for (int c = 14; c <= 17; c++) { whole_one(w, stride, i, c, 2); whole_one(w, stride, i, c, 4); }
    merged_all(w, stride, i, std::make_integer_sequence<int, 15>());
    free(w);
  }
  fclose(f);
  printf("ok %zu\n", i);
  return 0;
}
