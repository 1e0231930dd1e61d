// The host parameters of the subgroup-prefix interpolation and zerofier (myzkp_amd/csrc/mzk_prefix_plan.h) as a stand-alone program,
// tests/test_hostcheck_prefix_plan.py: it reads operations from the file it is given, values in hex, and prints one result line each;
// the test compares with Python integers.  Stand-alone: g++ -fsanitize=address,undefined; a domain is held in a buffer of exactly its n
// points, so a look past the prefix is a heap-buffer-overflow.
//   prefix_plan_shim FIELD_ID FILE
//     candidate N_POINTS X_0 ... X_(n-1)      -> "1 <N>" or "0"
//     inverse G N_POINTS M                    -> the m x m entries of Ainv, row-major, or "none"
//     zerofier G N_POINTS N                   -> rho_0 w_0 rho_1 w_1 ..., or "none"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <stdint.h>
#include <vector>
#include "../../myzkp_amd/csrc/mzk_prefix_plan.h"

using namespace mzk;

static bool next_value(FILE* in, uint64_t v[4]) {
  char hex[80];
  if (fscanf(in, "%79s", hex) != 1) return false;
  v[0] = v[1] = v[2] = v[3] = 0;
  const size_t n = strlen(hex);
  if (n > 64) { fprintf(stderr, "value too long: %s\n", hex); exit(2); }
  for (size_t i = 0; i < n; i++) {
    const char c = hex[n - 1 - i];
    const uint64_t d = (uint64_t)(c <= '9' ? c - '0' : c - 'a' + 10);
    v[i / 16] |= d << (4 * (i % 16));
  }
  return true;
}
static void print_all(const HostField* f, const std::vector<uint64_t>& v) {
  const size_t nl = (size_t)f->nl;
  for (size_t e = 0; e < v.size() / nl; e++) {
    if (e) printf(" ");
    for (size_t i = nl; i-- > 0;) printf("%016llx", (unsigned long long)v[e * nl + i]);
  }
  printf("\n");
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  const HostField* f = host_field(atoi(argv[1]));
  FILE* in = fopen(argv[2], "r");
  if (!f || !in) return 2;
  const size_t nl = (size_t)f->nl;
  char op[16];
  uint64_t a[4], b[4], c[4];
  while (fscanf(in, "%15s", op) == 1) {
    if (!strcmp(op, "candidate")) {
      if (!next_value(in, a)) return 2;
      const size_t n = (size_t)a[0];
      std::vector<uint64_t> domain(n * nl);
      for (size_t i = 0; i < n; i++) {
        if (!next_value(in, b)) return 2;
        memcpy(domain.data() + i * nl, b, 8 * nl);
      }
      size_t N = 0;
      if (prefix_candidate(f, domain.data(), n, &N)) printf("1 %zu\n", N);
      else printf("0\n");
    } else if (!strcmp(op, "inverse") || !strcmp(op, "zerofier")) {
      if (!next_value(in, a) || !next_value(in, b) || !next_value(in, c)) return 2;
      std::vector<uint64_t> g(a, a + nl), out;      // the generator in a buffer of one element
      const bool ok = op[0] == 'i' ? prefix_system_inverse(f, g.data(), (size_t)b[0], (size_t)c[0], &out) : prefix_zerofier_params(f, g.data(), (size_t)b[0], (size_t)c[0], &out);
      if (ok) print_all(f, out);
      else printf("none\n");
    } else { fprintf(stderr, "unknown operation %s\n", op); return 2; }
  }
  fclose(in);
  printf("ok\n");
  return 0;
}
