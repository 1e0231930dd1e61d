// fri_prove<F> of the C++ mirror (myzkp_amd/host/myzkp.hpp) for the Goldilocks tags FiniteFieldElement<M64> and
// ExtendedFieldElement<M64, Ip3>: FRI::prove (zkstark/fri.rs:99-143) through mzk_fri_prove_gl and its 64-byte path entries.
// Prints roots, top-level indices, the last codeword, every revealed value and every path entry as hex for
// tests/test_gpu_fri_prove_gl_cpp.py, which compares them with tests/goldilocks_model.py.  The codeword: word i of a vector seeded s is
// ((i + 1) * s) mod 2^64, reduced once below p.
#include <cstdio>
#include "../../myzkp_amd/host/myzkp.hpp"
using namespace myzkp;

static int failures = 0;
#define CHECK(c) do { if (!(c)) { printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); failures++; } } while (0)

static const uint64_t GL_P = 0xFFFFFFFF00000001ULL;
template <class F> static std::vector<F> synth(size_t n, uint64_t seed) {
  std::vector<F> v(n);
  const size_t nl = F().value.size();
  for (size_t i = 0; i < n; i++)
    for (size_t k = 0; k < nl; k++) {
      const uint64_t w = (i * nl + k + 1) * seed;
      v[i].value[k] = w >= GL_P ? w - GL_P : w;
    }
  return v;
}
static void put_bytes(const std::vector<uint8_t>& b) {
  if (b.empty()) printf(" -");
  else { printf(" "); for (uint8_t x : b) printf("%02x", x); }
}
template <class F> static void put_elem(const F& e) {
  for (uint64_t w : e.value) printf(" %llx", (unsigned long long)w);
}

template <class F> static void run(const char* tag, unsigned log2_n, size_t expansion, size_t tests) {
  const size_t n = (size_t)1 << log2_n;
  const auto w3 = get_nth_root_of_m64(log2_n);
  const F omega = F::from_value(w3.value[0]), offset = F::from_value(7);
  const auto cw = synth<F>(n, 0x9E3779B97F4A7C15ULL);
  const FriProof<F> p = fri_prove(cw, omega, offset, expansion, tests);
  CHECK(p.top_level_indices.size() == tests && p.revealed_layers.size() + 1 == p.merkle_roots.size());
  for (size_t r = 0; r < p.merkle_roots.size(); r++) { printf("%s.%u.root %zu", tag, log2_n, r); put_bytes(p.merkle_roots[r]); printf("\n"); }
  for (size_t s = 0; s < tests; s++) printf("%s.%u.top %zu %zx\n", tag, log2_n, s, p.top_level_indices[s]);
  for (size_t j = 0; j < p.last_codeword.size(); j++) { printf("%s.%u.last %zu", tag, log2_n, j); put_elem(p.last_codeword[j]); printf("\n"); }
  for (size_t i = 0; i < p.revealed_layers.size(); i++) {
    const auto& L = p.revealed_layers[i];
    const std::pair<std::vector<F>, std::vector<MerklePath>>* parts[3] = {&L.a, &L.b, &L.c};
    for (int k = 0; k < 3; k++) {
      CHECK(parts[k]->first.size() == tests && parts[k]->second.size() == tests);
      for (size_t s = 0; s < tests; s++) {
        printf("%s.%u.value.%zu.%c %zu", tag, log2_n, i, "abc"[k], s);
        put_elem(parts[k]->first[s]);
        printf("\n");
        printf("%s.%u.path.%zu.%c %zu", tag, log2_n, i, "abc"[k], s);
        for (const auto& e : parts[k]->second[s]) put_bytes(e);
        printf("\n");
      }
    }
  }
}

int main() {
  expect(mzk_init(0));
  run<ExtendedFieldElement<M64, Ip3>>("m64x3", 6, 4, 4);
  run<ExtendedFieldElement<M64, Ip3>>("m64x3", 10, 16, 17);
  run<FiniteFieldElement<M64>>("m64", 6, 4, 4);
  run<FiniteFieldElement<M64>>("m64", 10, 16, 17);
  // what the entry points refuse surfaces as Panic with the library's status
  try {
    (void)fri_prove(synth<FiniteFieldElement<M64>>(1024, 3), FiniteFieldElement<M64>::from_value(get_nth_root_of_m64(10).value[0]),
                    FiniteFieldElement<M64>::from_value(7), 512, 17);
    CHECK(false);
  } catch (const Panic& p) { CHECK(p.code == MZK_E_LENGTH); }
  mzk_shutdown();
  if (failures) { printf("%d failures\n", failures); return 1; }
  printf("fri_prove_gl mirror tests passed\n");
  return 0;
}
