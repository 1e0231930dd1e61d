// The MPolynomial part of the C++ mirror (myzkp_amd/host/myzkp.hpp: MPolynomial::evaluate_symbolic, evaluate_symbolic_many,
// weighted_combination) run the way the reference's tests run them:
//   test_evaluate_symbolic / test_evaluate_symbolic_constant  <- algebra/mpolynomials.rs:614-688 (self-checked here, over both fields)
// and on the cases of a text file (argv[1]; whitespace-separated decimal numbers, written by tests/test_gpu_mpoly_cpp.py from
// tests/golden/mpoly_vectors.json):
//   field  n_vars  { len coef.. }  n_constraints { n_terms { coef exp.. } }  n_polys { weight shift len coef.. }     per case, until EOF
// Every result is printed as hex limbs:  compose <case> <constraint> <index> limbs..  /  lincomb <case> 0 <index> limbs..
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include "../../myzkp_amd/host/myzkp.hpp"
using namespace myzkp;

static int failures = 0;
#define CHECK(c) do { if (!(c)) { printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); failures++; } } while (0)

template <class F> static F dec(const std::string& s) {      // decimal -> canonical limbs (the values given are below the modulus)
  F r;
  for (char ch : s) {
    unsigned __int128 carry = (unsigned)(ch - '0');
    for (size_t i = 0; i < r.value.size(); i++) {
      const unsigned __int128 t = (unsigned __int128)r.value[i] * 10 + carry;
      r.value[i] = (uint64_t)t;
      carry = t >> 64;
    }
  }
  return r;
}
template <class F> static void put(const char* key, size_t c, size_t a, const Polynomial<F>& p) {
  printf("%s.len %zu %zu %zu\n", key, c, a, p.coef.size());
  for (size_t i = 0; i < p.coef.size(); i++) {
    printf("%s %zu %zu %zu", key, c, a, i);
    for (uint64_t w : p.coef[i].value) printf(" %llx", (unsigned long long)w);
    printf("\n");
  }
}

template <class F> static void known_answers() {
  // 2x + 3y at (t + 1, t^2) = 3 t^2 + 2 t + 2; the constant 5 at the same point
  MPolynomial<F> m, c;
  m.dictionary[{1, 0}] = F::from_value(2);
  m.dictionary[{0, 1}] = F::from_value(3);
  c.dictionary[{0, 0}] = F::from_value(5);
  const std::vector<Polynomial<F>> point = {Polynomial<F>{{F::from_value(1), F::from_value(1)}}, Polynomial<F>{{F::zero(), F::zero(), F::from_value(1)}}};
  const Polynomial<F> r = m.evaluate_symbolic(point);
  CHECK(r.coef.size() == 3 && r.coef[0] == F::from_value(2) && r.coef[1] == F::from_value(2) && r.coef[2] == F::from_value(3));
  const Polynomial<F> k = c.evaluate_symbolic(point);
  CHECK(k.coef.size() == 1 && k.coef[0] == F::from_value(5));
  // both in one call, and a key shorter than the point (padded like Add / Mul pad it)
  MPolynomial<F> s;
  s.dictionary[{2}] = F::from_value(1);
  const auto many = MPolynomial<F>::evaluate_symbolic_many({m, c, s, MPolynomial<F>()}, point);
  CHECK(many.size() == 4 && many[0].coef == r.coef && many[1].coef == k.coef && many[3].coef.empty());
  CHECK(many[2].coef.size() == 3 && many[2].coef[0] == F::from_value(1) && many[2].coef[1] == F::from_value(2) && many[2].coef[2] == F::from_value(1));
  // the weighted sum: 2 * (1 + t) + 3 * X^2 * (1 + t) = 2 + 2 t + 3 t^2 + 3 t^3; a cancelling pair is the zero polynomial
  const Polynomial<F> w = weighted_combination<F>({point[0], point[0]}, {F::from_value(2), F::from_value(3)}, {0, 2});
  CHECK(w.coef.size() == 4 && w.coef[0] == F::from_value(2) && w.coef[1] == F::from_value(2) && w.coef[2] == F::from_value(3) && w.coef[3] == F::from_value(3));
  bool threw = false;
  try { weighted_combination<F>({point[0]}, {F::from_value(2)}, {0, 1}); } catch (const Panic& e) { threw = e.code == MZK_E_LENGTH; }
  CHECK(threw);
  threw = false;
  MPolynomial<F> wide;
  wide.dictionary[{1, 0, 1}] = F::from_value(1);
  try { wide.evaluate_symbolic(point); } catch (const Panic& e) { threw = e.code == MZK_E_LENGTH; }
  CHECK(threw);
}

template <class F> static void run_case(std::ifstream& in, size_t index) {
  std::string tok;
  size_t nv, nc, np;
  in >> nv;
  std::vector<Polynomial<F>> point(nv);
  for (auto& q : point) {
    size_t len;
    in >> len;
    for (size_t i = 0; i < len; i++) { in >> tok; q.coef.push_back(dec<F>(tok)); }
  }
  in >> nc;
  std::vector<MPolynomial<F>> ms(nc);
  std::vector<uint64_t> coefs;
  std::vector<uint32_t> exps;
  std::vector<size_t> toff(1, 0);
  bool duplicates = false;
  for (auto& m : ms) {
    size_t nt;
    in >> nt;
    for (size_t t = 0; t < nt; t++) {
      in >> tok;
      const F c = dec<F>(tok);
      std::vector<size_t> k(nv);
      for (auto& e : k) in >> e;
      duplicates |= m.dictionary.count(k) != 0;
      m.dictionary[k] = c;
    }
  }
  if (!duplicates && nc) {       // a dictionary cannot hold duplicate rows: such cases go through the flat table in the Python tests only
    const auto res = MPolynomial<F>::evaluate_symbolic_many(ms, point);
    for (size_t a = 0; a < nc; a++) put("compose", index, a, res[a]);
    for (size_t a = 0; a < nc; a++) CHECK(ms[a].evaluate_symbolic(point).coef == res[a].coef);
  }
  in >> np;
  std::vector<Polynomial<F>> terms(np);
  std::vector<F> weights(np);
  std::vector<size_t> shifts(np);
  for (size_t i = 0; i < np; i++) {
    size_t len;
    in >> tok >> shifts[i] >> len;
    weights[i] = dec<F>(tok);
    for (size_t j = 0; j < len; j++) { in >> tok; terms[i].coef.push_back(dec<F>(tok)); }
  }
  if (np) put("lincomb", index, 0, weighted_combination<F>(terms, weights, shifts));
}

int main(int argc, char** argv) {
  try {
    expect(mzk_init(0));
    known_answers<FiniteFieldElement<M128>>();
    known_answers<FqOrder>();
    if (argc > 1) {
      std::ifstream in(argv[1]);
      int field;
      for (size_t index = 0; in >> field; index++) {
        if (field == MZK_FIELD_M128) run_case<FiniteFieldElement<M128>>(in, index);
        else run_case<FqOrder>(in, index);
      }
    }
  } catch (const std::exception& e) {
    printf("FAIL exception: %s\n", e.what());
    failures++;
  }
  if (failures == 0) printf("mpoly mirror tests passed\n");
  return failures ? 1 : 0;
}
