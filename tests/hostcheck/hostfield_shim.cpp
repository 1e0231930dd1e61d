// The host field arithmetic (myzkp_amd/csrc/mzk_hostfield.h) as a stand-alone program, tests/test_hostcheck_hostfield.py: it reads one
// operation per line from the file it is given, values in hex, and prints one result line each; the test compares with Python integers.
// Stand-alone: g++ -fsanitize=address,undefined.
//   hostfield_shim FIELD_ID FILE
//     add A B | sub A B | neg A | mul A B | slow A B | pow A E | inv A | ninv K | mont A      -> the result in hex (mont: the eight words)
//     root W ORDER                                                                          -> "<code> <assertion text>"
//     shoup V                                                                               -> the 32 words of an entry preset to deadbeef
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <stdint.h>
#include "../../myzkp_amd/csrc/mzk_hostfield.h"

using namespace mzk;

static void parse(const char* hex, uint64_t v[4]) {
  v[0] = v[1] = v[2] = v[3] = 0;
  const size_t n = strlen(hex);
  if (n > 64) { fprintf(stderr, "value too long: %s\n", hex); exit(2); }
  for (size_t i = 0; i < n; i++) {
    const char c = hex[n - 1 - i];
    const uint64_t d = (uint64_t)(c <= '9' ? c - '0' : c - 'a' + 10);
    v[i / 16] |= d << (4 * (i % 16));
  }
}
static void print(const HostField* f, const uint64_t* v) {
  for (int i = f->nl - 1; i >= 0; i--) printf("%016llx", (unsigned long long)v[i]);
  printf("\n");
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  const HostField* f = host_field(atoi(argv[1]));
  FILE* in = fopen(argv[2], "r");
  if (!f || !in) return 2;
  char op[16], s1[80], s2[80];
  char line[256];
  while (fgets(line, sizeof line, in)) {
    s1[0] = s2[0] = 0;
    if (sscanf(line, "%15s %79s %79s", op, s1, s2) < 2) continue;
    uint64_t a[4], b[4], r[4] = {0, 0, 0, 0};
    parse(s1, a);
    parse(s2, b);
    if (!strcmp(op, "add")) { h_addmod(f, r, a, b); print(f, r); }
    else if (!strcmp(op, "sub")) { h_submod(f, r, a, b); print(f, r); }
    else if (!strcmp(op, "neg")) { h_negmod(f, r, a); print(f, r); }
    else if (!strcmp(op, "mul")) { h_mulmod(f, r, a, b); print(f, r); }
    else if (!strcmp(op, "slow")) { h_mulmod_slow(f, r, a, b); print(f, r); }
    else if (!strcmp(op, "pow")) { h_powmod_u64(f, r, a, b[0]); print(f, r); }
    else if (!strcmp(op, "inv")) { h_invmod(f, r, a); print(f, r); }
    else if (!strcmp(op, "ninv")) { h_ninv_pow2(f, (unsigned)a[0], r); print(f, r); }
    else if (!strcmp(op, "mont")) {
      uint32_t w[8];
      h_mont_words(f, a, w);
      for (int i = 7; i >= 0; i--) printf("%08x", w[i]);
      printf("\n");
    } else if (!strcmp(op, "root")) {
      const char* msg = nullptr;
      const int rc = h_root_check(f, a, b[0], &msg);
      printf("%d %s\n", rc, msg);
    } else if (!strcmp(op, "shoup")) {
      uint32_t e[SHOUP_ENTRY_WORDS];
      for (int i = 0; i < SHOUP_ENTRY_WORDS; i++) e[i] = 0xdeadbeefu;
      h_shoup_entry(f, a, e);
      for (int i = 0; i < SHOUP_ENTRY_WORDS; i++) printf("%x%c", e[i], i + 1 < SHOUP_ENTRY_WORDS ? ' ' : '\n');
    } else { fprintf(stderr, "unknown operation %s\n", op); return 2; }
  }
  fclose(in);
  // the consistency checks that need no operand: canonical, zero, one
  const uint64_t zero[4] = {0, 0, 0, 0}, one[4] = {1, 0, 0, 0};
  if (!h_is_zero(f, zero) || h_is_zero(f, one) || !h_is_one(f, one) || h_is_one(f, zero) || !h_is_canonical(f, one) || h_is_canonical(f, f->p) ||
      h_cmp(f->p, one, f->nl) != 1 || host_field(atoi(argv[1])) != f) { printf("predicates wrong\n"); return 1; }
  printf("ok\n");
  return 0;
}
