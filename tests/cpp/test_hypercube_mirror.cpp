// SumCheckProverGPU::prove(max_degree, factors, header) of the C++ mirror (myzkp_amd/host/myzkp.hpp) on MPolynomial factors: el = 9,
// k = 3, d = 3 with the reference-shaped header.  Factor f has the terms t = 0 .. 10 + 7 f: coefficient limb 0 = (t + 1) * SEED[f], the
// support of term t is the low el bits of (t + 1) * (2 f + 3) * 37 (variable i <-> bit el-1-i), exponent 1 -- except factor 1, whose
// exponents are 1 + (t + i) % 3 (not multilinear), and whose last two terms are x0^2 and x0^5.  Factor 2's keys are cut after their last
// non-zero exponent (short keys).  Prints, for the prover on the factors and for the table overload on tables from
// evals_over_boolean_hypercube(factor, el), the claimed sum and the proof stream; tests/test_gpu_hypercube_cpp.py compares both with
// the model.
#include <cstdio>
#include "../../myzkp_amd/host/myzkp.hpp"
using namespace myzkp;

static int failures = 0;
#define CHECK(c) do { if (!(c)) { printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); failures++; } } while (0)

static const uint64_t SEED[3] = {0x9E3779B97F4A7C15ULL, 0xD1B54A32D192ED03ULL, 0xA0761D6478BD642FULL};

static void put(const char* tag, const FqOrder& sum, const std::vector<uint8_t>& proof) {
  printf("%s.sum", tag);
  for (uint64_t w : sum.value) printf(" %llx", (unsigned long long)w);
  printf("\n%s.proof ", tag);
  for (uint8_t b : proof) printf("%02x", b);
  printf("\n");
}

int main() {
  expect(mzk_init(0));
  const size_t el = 9, k = 3, d = 3;
  std::vector<MPolynomial<FqOrder>> factors(k);
  std::vector<std::vector<uint8_t>> factor_bytes;
  for (size_t f = 0; f < k; f++) {
    for (size_t t = 0; t <= 10 + 7 * f; t++) {
      const size_t mask = ((t + 1) * (2 * f + 3) * 37) & (((size_t)1 << el) - 1);
      std::vector<size_t> key(el, 0);
      for (size_t i = 0; i < el; i++)
        if ((mask >> (el - 1 - i)) & 1) key[i] = f == 1 ? 1 + (t + i) % 3 : 1;
      if (f == 2) while (!key.empty() && key.back() == 0) key.pop_back();
      FqOrder c;
      c.value[0] = (t + 1) * SEED[f];
      factors[f].dictionary[key] = c;
    }
    factor_bytes.push_back(std::vector<uint8_t>(f + 2, (uint8_t)(0xA0 + f)));
  }
  {
    std::vector<size_t> a(el, 0), b(el, 0);
    a[0] = 2; b[0] = 5;
    FqOrder c2, c5;
    c2.value[0] = 1002; c5.value[0] = 1005;
    factors[1].dictionary[a] = c2;
    factors[1].dictionary[b] = c5;
  }
  const auto header = SumCheckProverGPU::reference_header(d, el, factor_bytes);
  SumCheckProverGPU prover;
  const auto pr = prover.prove(d, factors, header);
  put("terms", pr.first, pr.second);
  std::vector<std::vector<FqOrder>> tables;
  for (size_t f = 0; f < k; f++) tables.push_back(SumCheckProverGPU::evals_over_boolean_hypercube(factors[f], el));
  CHECK(tables[0].size() == (size_t)1 << el);
  const auto pr2 = prover.prove(d, tables, header);
  put("tables", pr2.first, pr2.second);
  CHECK(pr.first == pr2.first);
  CHECK(pr.second == pr2.second);
  // the library's refusals surface as Panic
  try { (void)prover.prove(0, factors, header); CHECK(false); } catch (const Panic& p) { CHECK(p.code == MZK_E_ARG); }
  try { (void)prover.prove(d, std::vector<MPolynomial<FqOrder>>(1), {}); CHECK(false); } catch (const Panic& p) { CHECK(p.code == MZK_E_LENGTH); }
  if (failures) { printf("%d failures\n", failures); return 1; }
  printf("hypercube mirror tests passed\n");
  return 0;
}
