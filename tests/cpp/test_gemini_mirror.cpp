// The Gemini / sum-check part of the C++ mirror (myzkp_amd/host/myzkp.hpp: batch::split_and_fold, commit_gemini, open_gemini,
// prove_sumcheck) run the way the reference's tests run them:
//   test_gemini             <- algebra/gemini.rs:288-328 (coef 1..8, rhos 2, 3, 4, beta = 1234)
//   test_sumcheck_pipeline  <- algebra/sumcheck.rs:230-248 (the transcript is stood in for: the challenges come from argv)
// Usage: test_gemini_mirror <alpha> <max_d> <r_0> .. <r_{el-1}> <beta> (decimal).  Self-checks what the C++ side can (mu, the
// sum-check round relations, the error paths) and prints every value and point as hex limbs for tests/test_gpu_gemini_cpp.py to
// compare with tests/golden/gemini_vectors.json.
#include <cstdio>
#include <cstdlib>
#include "../../myzkp_amd/host/myzkp.hpp"
using namespace myzkp;

static int failures = 0;
#define CHECK(c) do { if (!(c)) { printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); failures++; } } while (0)

static FqOrder dec(const char* s) {      // decimal -> canonical limbs (the values given are below the modulus)
  uint64_t l[4] = {0, 0, 0, 0};
  for (; *s; s++) {
    unsigned __int128 carry = (unsigned)(*s - '0');
    for (int i = 0; i < 4; i++) {
      const unsigned __int128 t = (unsigned __int128)l[i] * 10 + carry;
      l[i] = (uint64_t)t;
      carry = t >> 64;
    }
  }
  return FqOrder::from_limbs(l);
}
static void put(const char* key, size_t i, const FqOrder& v) {
  printf("%s %zu", key, i);
  for (uint64_t w : v.value) printf(" %llx", (unsigned long long)w);
  printf("\n");
}
static void put(const char* key, size_t i, const G1Point& p) {
  uint64_t w[8];
  p.to_wire(w);
  printf("%s %zu", key, i);
  for (uint64_t x : w) printf(" %llx", (unsigned long long)x);
  printf("\n");
}
static void put_proof(const char* tag, const std::vector<CommitmentKZG>& c, const batch::ProofGemini& pr) {
  std::string t(tag);
  for (size_t i = 0; i < c.size(); i++) put((t + ".commit").c_str(), i, c[i]);
  for (size_t i = 0; i < pr.es.size(); i++) {
    for (int k = 0; k < 3; k++) put((t + ".y").c_str(), 3 * i + k, pr.es[i].ys[k]);
    put((t + ".w").c_str(), i, pr.es[i].w);
  }
  for (size_t i = 0; i < pr.degree_proofs.size(); i++) put((t + ".deg").c_str(), i, pr.degree_proofs[i]);
}

int main(int argc, char** argv) {
  if (argc < 5) { printf("usage: %s alpha max_d r_0 .. r_{el-1} beta\n", argv[0]); return 2; }
  expect(mzk_init(0));
  const FqOrder alpha = dec(argv[1]);
  const size_t max_d = (size_t)atoll(argv[2]);
  auto pk = setup_kzg_with_alpha(BN128::generator_g1(), alpha, max_d);
  batch::SrsHandle srs(pk);
  // test_gemini
  std::vector<FqOrder> coef;
  for (uint64_t i = 0; i < 8; i++) coef.push_back(FqOrder::from_value(i + 1));
  const std::vector<FqOrder> rhos = {FqOrder::from_value(2), FqOrder::from_value(3), FqOrder::from_value(4)};
  auto fs = batch::split_and_fold(coef, rhos);
  CHECK(fs.size() == 4 && fs[3].coef.size() == 1 && fs[3].coef[0] == FqOrder::from_value(382));   // mu = <coef, tensor(1, rho_i)>
  put_proof("gemini", batch::commit_gemini(fs, srs), batch::open_gemini(fs, FqOrder::from_value(1234), srs));
  // test_sumcheck_pipeline: g = 1 + 2 x0 + 3 x1 + 4 x1 x2 + 5 x0 x1 x2 in get_coefs_in_order's order
  std::vector<FqOrder> g(8, FqOrder::from_value(0));
  g[0] = FqOrder::from_value(1); g[1] = FqOrder::from_value(2); g[2] = FqOrder::from_value(3); g[6] = FqOrder::from_value(4); g[7] = FqOrder::from_value(5);
  std::vector<FqOrder> chal;
  for (int i = 3; i < argc; i++) chal.push_back(dec(argv[i]));
  CHECK(chal.size() == 4);
  int calls = 0;
  auto pr = batch::prove_sumcheck(g, FqOrder::from_value(41), [&](int round, const FqOrder* gj) {
    CHECK((gj == nullptr) == (round == 3));
    calls++;
    return chal[(size_t)round];
  }, srs);
  CHECK(calls == 4 && pr.el == 3 && pr.gs.size() == 3 && pr.c_g.size() == 4 && pr.pi.es.size() == 3 && pr.pi.degree_proofs.size() == 4);
  for (size_t j = 0; j < pr.gs.size(); j++) { put("sumcheck.a", j, pr.gs[j].first); put("sumcheck.b", j, pr.gs[j].second); }
  for (size_t j = 0; j < pr.rs.size(); j++) { CHECK(pr.rs[j] == chal[j]); put("sumcheck.r", j, pr.rs[j]); }
  CHECK(pr.beta == chal[3]);
  put("sumcheck.beta", 0, pr.beta);
  put_proof("sumcheck", pr.c_g, pr.pi);
  // a throwing challenge comes back as the same exception; a failing precondition as a Panic with the ABI code
  bool thrown = false;
  try {
    batch::prove_sumcheck(g, FqOrder::from_value(41), [](int round, const FqOrder*) -> FqOrder {
      if (round == 1) throw std::logic_error("transcript");
      return FqOrder::from_value(5);
    }, srs);
  } catch (const std::logic_error& e) { thrown = std::string(e.what()) == "transcript"; }
  CHECK(thrown);
  int code = 0;
  try { batch::split_and_fold(std::vector<FqOrder>(6, FqOrder::from_value(1)), rhos); } catch (const Panic& p) { code = p.code; }
  CHECK(code == MZK_E_NOT_POW2);
  code = 0;
  try { batch::prove_sumcheck(std::vector<FqOrder>(1, FqOrder::from_value(1)), FqOrder::from_value(1), [](int, const FqOrder*) { return FqOrder::from_value(1); }, srs); }
  catch (const Panic& p) { code = p.code; }
  CHECK(code == MZK_E_LENGTH);
  if (failures) { printf("%d failures\n", failures); return 1; }
  printf("gemini mirror tests passed\n");
  return 0;
}
