// The FastStark part of the C++ mirror (myzkp_amd/host/myzkp.hpp: boundary_quotients, fast_stark_dims):
//   known answers, self-checked here over both fields -- (X - 1)(X - 2)(X + 3) divided by its roots, an inexact division, more roots
//   than coefficients, the reference's own parameters (Rescue-Prime: 28 cycles, 2 registers, expansion 4, 2 colinearity checks);
//   and the cases of a text file (argv[1]; whitespace-separated decimal numbers, written by tests/test_gpu_stark_cpp.py):
//     field  n_rows { len coef..  n_roots root.. }     per case, until EOF
// Every quotient is printed as hex limbs:  quotient <case> <row> <index> limbs..
// A case whose first number is 100 + field is a whole proof through FastStark<F> (run_prove below).
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

template <class F> static void known_answers() {
  const auto v = [](uint64_t x) { return F::from_value(x); };
  // (X - 1)(X - 2)(X - 3) = X^3 - 6 X^2 + 11 X - 6, shifted by +6 X^2 + 6 to keep the coefficients small and positive:
  // f = X^3 + 11 X = X (X^2 + 11); f / (X - 0) = X^2 + 11 exactly; floor(f / ((X - 0)(X - 1))) = X + 1 (remainder 12 X dropped)
  const Polynomial<F> f{{v(0), v(11), v(0), v(1)}};
  auto q = boundary_quotients<F>({f, f, f, f}, {{v(0)}, {v(0), v(1)}, {}, {v(1), v(2), v(3), v(4)}});
  CHECK(q.size() == 4);
  CHECK(q[0].coef.size() == 3 && q[0].coef[0] == v(11) && q[0].coef[1] == v(0) && q[0].coef[2] == v(1));
  CHECK(q[1].coef.size() == 2 && q[1].coef[0] == v(1) && q[1].coef[1] == v(1));
  CHECK(q[2].coef == f.coef);                     // no boundary on this register: the polynomial itself
  CHECK(q[3].coef.empty());                       // degree 3 against a zerofier of degree 4: the zero polynomial
  bool threw = false;
  try { boundary_quotients<F>({f}, {}); } catch (const Panic& e) { threw = e.code == MZK_E_LENGTH; }
  CHECK(threw);
  // the sizes of the reference's test_fast_stark; the AIR's shape is what matters: both constraints reach (78, 3, ..) -> bound 78 + 35 * 3
  MPolynomial<F> a, b;
  a.dictionary[{78, 0, 0, 0, 0}] = v(1);
  a.dictionary[{0, 3, 0, 0, 0}] = v(1);
  b.dictionary[{0, 0, 0, 0, 3}] = v(1);
  const mzk_stark_dims d = fast_stark_dims<F>(4, 2, 2, 28, 2, {a, b}, {{0, 1}, {27, 0}});
  CHECK(d.num_randomizers == 8 && d.randomized_trace_length == 36 && d.omicron_domain_length == 128 && d.fri_domain_length == 512);
  CHECK(d.transition_degree_bounds[0] == 105 && d.transition_quotient_degree_bounds[0] == 78 && d.transition_quotient_degree_bounds[1] == 78);
  CHECK(d.max_degree == 127 && d.randomizer_length == 128 && d.boundary_quotient_degree_bounds[0] == 34 && d.boundary_shifts[1] == 93);
  CHECK(d.fri_num_rounds == 6 && d.num_indices == 8 && d.n_weights == 9);
  threw = false;
  try { fast_stark_dims<F>(3, 2, 2, 28, 2, {a, b}, {}); } catch (const Panic& e) { threw = e.code == MZK_E_NOT_POW2; }
  CHECK(threw);
}

// "prove" case of the file:  expansion checks registers cycles degree generator  n_constraints { n_terms { coef exp.. } }
//   n_rows { register values }  n_boundary { cycle register value }  n_randomizer { coef }
// prints the roots, the duplicated indices, the opened points and a byte sum of every path: the driver compares them with the model's proof
template <class F> static void run_prove(std::ifstream& in, size_t index) {
  std::string tok;
  size_t e, t, m, cycles, degree, nc, rows, nb, nr;
  in >> e >> t >> m >> cycles >> degree >> tok;
  const F generator = dec<F>(tok);
  in >> nc;
  std::vector<MPolynomial<F>> air(nc);
  for (auto& a : air) {
    size_t nt;
    in >> nt;
    for (size_t i = 0; i < nt; i++) {
      in >> tok;
      std::vector<size_t> k(1 + 2 * m);
      for (auto& x : k) in >> x;
      a.dictionary[k] = dec<F>(tok);
    }
  }
  in >> rows;
  std::vector<std::vector<F>> trace(rows, std::vector<F>(m));
  for (auto& row : trace) for (auto& v : row) { in >> tok; v = dec<F>(tok); }
  in >> nb;
  typename FastStark<F>::Boundary boundary;
  for (size_t i = 0; i < nb; i++) { size_t c, r; in >> c >> r >> tok; boundary.emplace_back(c, r, dec<F>(tok)); }
  in >> nr;
  Polynomial<F> randomizer;
  for (size_t i = 0; i < nr; i++) { in >> tok; randomizer.coef.push_back(dec<F>(tok)); }
  FastStark<F> stark(e, t, m, cycles, degree, generator, air);
  const auto hex = [](const uint8_t* b, size_t n) { std::string s; char buf[3]; for (size_t i = 0; i < n; i++) { snprintf(buf, 3, "%02x", b[i]); s += buf; } return s; };
  printf("tzroot %zu %s\n", index, hex(stark.preprocess().data(), 32).c_str());
  const FastStarkProof<F> p = stark.prove(trace, boundary, randomizer);
  const FastStarkProof<F> again = stark.prove(trace, boundary, randomizer);
  CHECK(again.fri_proof == p.fri_proof && again.bqc_paths == p.bqc_paths && again.bqc_roots == p.bqc_roots);
  for (const auto& r : p.bqc_roots) printf("bqcroot %zu %s\n", index, hex(r.data(), 32).c_str());
  printf("rdcroot %zu %s\n", index, hex(p.rdc_root.data(), 32).c_str());
  printf("indices %zu", index);
  for (size_t i : p.duplicated_indices) printf(" %zu", i);
  printf("\n");
  const auto pts = [&](const char* key, const std::vector<F>& v) {
    for (size_t i = 0; i < v.size(); i++) { printf("%s %zu %zu", key, index, i); for (uint64_t w : v[i].value) printf(" %llx", (unsigned long long)w); printf("\n"); }
  };
  pts("bqcpoint", p.bqc_points); pts("rdcpoint", p.rdc_points); pts("tzcpoint", p.tzc_points);
  const auto pth = [&](const char* key, const std::vector<StarkPath>& v) {
    for (size_t q = 0; q < v.size(); q++) { printf("%s %zu %zu", key, index, q); for (const auto& en : v[q]) printf(" %s", hex(en.data(), en.size()).c_str()); printf("\n"); }
  };
  pth("bqcpath", p.bqc_paths); pth("rdcpath", p.rdc_paths); pth("tzcpath", p.tzc_paths);
}

template <class F> static void run_case(std::ifstream& in, size_t index) {
  std::string tok;
  size_t rows;
  in >> rows;
  std::vector<Polynomial<F>> polys(rows);
  std::vector<std::vector<F>> roots(rows);
  for (size_t s = 0; s < rows; s++) {
    size_t len, nr;
    in >> len;
    for (size_t i = 0; i < len; i++) { in >> tok; polys[s].coef.push_back(dec<F>(tok)); }
    in >> nr;
    for (size_t i = 0; i < nr; i++) { in >> tok; roots[s].push_back(dec<F>(tok)); }
  }
  const auto q = boundary_quotients<F>(polys, roots);
  for (size_t s = 0; s < rows; s++) {
    printf("quotient.len %zu %zu %zu\n", index, s, q[s].coef.size());
    for (size_t i = 0; i < q[s].coef.size(); i++) {
      printf("quotient %zu %zu %zu", index, s, i);
      for (uint64_t w : q[s].coef[i].value) printf(" %llx", (unsigned long long)w);
      printf("\n");
    }
  }
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
        if (field == 100 + MZK_FIELD_M128) run_prove<FiniteFieldElement<M128>>(in, index);
        else if (field == MZK_FIELD_M128) run_case<FiniteFieldElement<M128>>(in, index);
        else run_case<FqOrder>(in, index);
      }
    }
  } catch (const std::exception& e) {
    printf("FAIL exception: %s\n", e.what());
    failures++;
  }
  if (failures == 0) printf("stark mirror tests passed\n");
  return failures ? 1 : 0;
}
