// The Goldilocks tags of the C++ mirror (myzkp_amd/host/myzkp.hpp: FiniteFieldElement<M64> and ExtendedFieldElement<M64, Ip3>)
// through the generic functions the reference's FRI uses: ntt / intt (algebra/ntt.rs:7-64), fast_coset_evaluate (ntt.rs:254-269) and
// one split-and-fold (zkstark/fri.rs:182-193), with the root from get_nth_root_of_m64 (fri.rs:449-473).
// Self-checks the round trip and prints every output as hex words for tests/test_gpu_goldilocks_cpp.py, which compares them with
// tests/goldilocks_model.py.  Inputs: word i of a vector seeded s is ((i + 1) * s) mod 2^64, reduced once below p.
#include <cstdio>
#include "../../myzkp_amd/host/myzkp.hpp"
using namespace myzkp;

static int failures = 0;
#define CHECK(c) do { if (!(c)) { printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); failures++; } } while (0)

static const uint64_t GL_P = 0xFFFFFFFF00000001ULL;
static uint64_t word(uint64_t i, uint64_t seed) {
  const uint64_t v = (i + 1) * seed;
  return v >= GL_P ? v - GL_P : v;
}
template <class F> static std::vector<F> synth(size_t n, uint64_t seed) {
  std::vector<F> v(n);
  const size_t nl = F().value.size();
  for (size_t i = 0; i < n; i++)
    for (size_t k = 0; k < nl; k++) v[i].value[k] = word(i * nl + k, seed);
  return v;
}
template <class F> static void put(const char* tag, const char* what, const std::vector<F>& v) {
  for (size_t i = 0; i < v.size(); i++) {
    printf("%s.%s %zu", tag, what, i);
    for (uint64_t w : v[i].value) printf(" %llx", (unsigned long long)w);
    printf("\n");
  }
}

template <class F> static void run(const char* tag, const F& omega) {
  CHECK(Polynomial<F>::field_id() == F::FIELD_ID);
  const size_t n = 64;
  const auto v = synth<F>(n, 0x9E3779B97F4A7C15ULL);
  const auto t = ntt(omega, v);
  CHECK(intt(omega, t) == v);
  put(tag, "ntt", t);
  Polynomial<F> poly{synth<F>(24, 0xD1B54A32D192ED03ULL)};
  const F offset = F::from_value(7);
  const auto cw = fast_coset_evaluate(poly, offset, omega, n);
  CHECK(cw.size() == n);
  put(tag, "lde", cw);
  const F alpha = synth<F>(1, 0xA0761D6478BD642FULL)[0];        // every coefficient non-zero for the extension
  const auto folded = fri_split_and_fold(cw, alpha, offset, omega);
  CHECK(folded.size() == n / 2);
  put(tag, "fold", folded);
  // the reference's panics surface as Panic with the library's status
  try { (void)fast_coset_evaluate(Polynomial<F>{synth<F>(n + 1, 3)}, offset, omega, n); CHECK(false); } catch (const Panic& p) { CHECK(p.code == MZK_E_LENGTH); }
}

int main() {
  expect(mzk_init(0));
  const auto w3 = get_nth_root_of_m64(6);
  CHECK(w3.value[1] == 0 && w3.value[2] == 0);
  run<ExtendedFieldElement<M64, Ip3>>("m64x3", w3);
  run<FiniteFieldElement<M64>>("m64", FiniteFieldElement<M64>::from_value(w3.value[0]));
  // the older tags still resolve to their ids
  CHECK(Polynomial<FqOrder>::field_id() == MZK_FIELD_FR && Polynomial<FiniteFieldElement<M128>>::field_id() == MZK_FIELD_M128);
  mzk_shutdown();
  if (failures) { printf("%d failures\n", failures); return 1; }
  printf("goldilocks mirror tests passed\n");
  return 0;
}
