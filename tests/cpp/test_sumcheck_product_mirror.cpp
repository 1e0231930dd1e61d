// SumCheckProverGPU of the C++ mirror (myzkp_amd/host/myzkp.hpp) on el = 8, k = 3, d = 3 with the reference-shaped header.  Prints
// the claimed sum as hex words and the proof stream as hex bytes; tests/test_gpu_sumcheck_product_cpp.py compares the sum and the
// stream's SHA-256 with tests/sumcheck_product_model.py.  Tables: value x of factor f has limb 0 = (x + 1) * SEED[f] and limb 1 =
// (x + 7) * SEED[f] (mod 2^64; a 128-bit value, far below p); factor f's header bytes are f + 2 bytes of value 0xA0 + f.
// The same values taken as dense multilinear coefficients go through evals_over_boolean_hypercube and are proved as well.
#include <cstdio>
#include "../../myzkp_amd/host/myzkp.hpp"
using namespace myzkp;

static int failures = 0;
#define CHECK(c) do { if (!(c)) { printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); failures++; } } while (0)

static const uint64_t SEED[3] = {0x9E3779B97F4A7C15ULL, 0xD1B54A32D192ED03ULL, 0xA0761D6478BD642FULL};

static std::vector<FqOrder> synth(size_t n, uint64_t seed) {
  std::vector<FqOrder> v(n);
  for (size_t x = 0; x < n; x++) {
    v[x].value[0] = (x + 1) * seed;
    v[x].value[1] = (x + 7) * seed;
  }
  return v;
}
static void put(const char* tag, const FqOrder& sum, const std::vector<uint8_t>& proof) {
  printf("%s.sum", tag);
  for (uint64_t w : sum.value) printf(" %llx", (unsigned long long)w);
  printf("\n%s.proof ", tag);
  for (uint8_t b : proof) printf("%02x", b);
  printf("\n");
}

int main() {
  expect(mzk_init(0));
  const size_t el = 8, k = 3, d = 3, n = (size_t)1 << el;
  std::vector<std::vector<FqOrder>> tables, coefs;
  std::vector<std::vector<uint8_t>> factor_bytes;
  for (size_t f = 0; f < k; f++) {
    tables.push_back(synth(n, SEED[f]));
    factor_bytes.push_back(std::vector<uint8_t>(f + 2, (uint8_t)(0xA0 + f)));
  }
  const auto header = SumCheckProverGPU::reference_header(d, el, factor_bytes);
  CHECK(header.size() == 3 + k);
  CHECK(SumCheckProverGPU::frame_header(header).size() == 3 * 24 + (16 + 2) + (16 + 3) + (16 + 4));
  SumCheckProverGPU prover;
  const auto pr = prover.prove(d, tables, header);
  put("tables", pr.first, pr.second);
  // the reference's full flow: coefficients -> tables -> proof
  std::vector<std::vector<FqOrder>> from_coef;
  for (size_t f = 0; f < k; f++) from_coef.push_back(SumCheckProverGPU::evals_over_boolean_hypercube(tables[f]));
  CHECK(from_coef[0][0] == tables[0][0]);            // the empty subset: evals[0] = coef[0]
  const auto pr2 = prover.prove(d, from_coef, header);
  put("coefs", pr2.first, pr2.second);
  // the library's refusals surface as Panic
  try { (void)prover.prove(0, tables, header); CHECK(false); } catch (const Panic& p) { CHECK(p.code == MZK_E_ARG); }
  try { (void)prover.prove(d, {{FqOrder()}}, {}); CHECK(false); } catch (const Panic& p) { CHECK(p.code == MZK_E_LENGTH); }
  if (failures) { printf("%d failures\n", failures); return 1; }
  printf("sumcheck product mirror tests passed\n");
  return 0;
}
