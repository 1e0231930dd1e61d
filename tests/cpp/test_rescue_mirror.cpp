// The reference's test_rescue_prime (zkstark/rescueprime.rs:602-654, up to the boundary constraints: transition_constraints stays with
// the caller) through the C++ mirror (myzkp_amd/host/myzkp.hpp: struct RescuePrime), line for line, then the ten-link chain of
// test_fast_stark.  The parameters come from the file tests/test_gpu_rescue_cpp.py dumps out of tests/golden/rescue_prime_m128.json:
//   m n alpha alphainv, then m * m + 2 n m elements, then the two known answers (input hash input hash) and the chain's input, all hex.
// Prints what it computed as hex for that test to compare with the model.
#include <cstdio>
#include <cstring>
#include <string>
#include "../../myzkp_amd/host/myzkp.hpp"
using namespace myzkp;
typedef FiniteFieldElement<M128> F;

static int failures = 0;
#define CHECK(c) do { if (!(c)) { printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); failures++; } } while (0)

static bool hex_limbs(const char* s, uint64_t* l, int n) {
  for (int i = 0; i < n; i++) l[i] = 0;
  const int len = (int)strlen(s);
  for (int k = 0; k < len; k++) {
    const char ch = s[len - 1 - k];
    const int d = ch >= '0' && ch <= '9' ? ch - '0' : ch >= 'a' && ch <= 'f' ? ch - 'a' + 10 : -1;
    if (d < 0 || (k / 16 >= n && d)) return false;
    if (k / 16 < n) l[k / 16] |= (uint64_t)d << (4 * (k % 16));
  }
  return true;
}
static bool read_f(FILE* f, F* out) {
  char tok[80];
  uint64_t l[2];
  if (fscanf(f, "%79s", tok) != 1 || !hex_limbs(tok, l, 2)) return false;
  *out = F::from_limbs(l);
  return true;
}
static void put(const char* what, const F& v) { printf("%s %016llx%016llx\n", what, (unsigned long long)v.value[1], (unsigned long long)v.value[0]); }

int main(int argc, char** argv) {
  if (argc != 2) { printf("usage: test_rescue_mirror <parameters>\n"); return 2; }
  FILE* f = fopen(argv[1], "r");
  if (!f) { printf("cannot open %s\n", argv[1]); return 2; }
  size_t m, n;
  char a_hex[80], ai_hex[80];
  if (fscanf(f, "%zu %zu %79s %79s", &m, &n, a_hex, ai_hex) != 4) return 2;
  uint64_t alpha[1];
  std::array<uint64_t, 4> alphainv;
  if (!hex_limbs(a_hex, alpha, 1) || !hex_limbs(ai_hex, alphainv.data(), 4)) return 2;
  std::vector<std::vector<F>> mds(m, std::vector<F>(m));
  std::vector<F> rc(2 * n * m);
  for (auto& row : mds) for (auto& v : row) if (!read_f(f, &v)) return 2;
  for (auto& v : rc) if (!read_f(f, &v)) return 2;
  F in1, out1, a, b, start;
  if (!read_f(f, &in1) || !read_f(f, &out1) || !read_f(f, &a) || !read_f(f, &b) || !read_f(f, &start)) return 2;
  fclose(f);
  try {
    expect(mzk_init(0));
    const RescuePrime<F> rp(m, n, alpha[0], alphainv, mds, rc);

    CHECK(rp.hash(in1) == out1);
    CHECK(rp.hash(a) == b);
    put("hash.0", rp.hash(in1));
    put("hash.1", rp.hash(a));

    const auto trace = rp.trace(a);
    CHECK(trace.size() == n + 1 && trace[0].size() == m);
    CHECK(trace[0][0] == a);
    CHECK(trace.back()[0] == b);
    for (size_t i = 0; i < m; i++) {
      put(("trace.first." + std::to_string(i)).c_str(), trace[0][i]);
      put(("trace.last." + std::to_string(i)).c_str(), trace.back()[i]);
    }

    const auto boundary_constraints = rp.boundary_constraints(b);
    CHECK(boundary_constraints.size() == 2);
    for (const auto& [cycle, element, value] : boundary_constraints) CHECK(trace[cycle][element] == value);

    // test_fast_stark: ten links from 123456789
    const auto links = rp.chain(start, 10);
    CHECK(links.size() == 10);
    F x = start;
    for (size_t l = 0; l < links.size(); l++) {
      x = rp.hash(x);
      CHECK(x == links[l]);
      put(("chain." + std::to_string(l)).c_str(), links[l]);
    }
  } catch (const Panic& e) {
    printf("FAIL panic: %s\n", e.what());
    failures++;
  }
  if (failures == 0) printf("rescue mirror tests passed\n");
  return failures != 0;
}
