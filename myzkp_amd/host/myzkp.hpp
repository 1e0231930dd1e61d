// myzkp.hpp -- host-side mirror of MyZKP's Rust surface for the MSM / NTT path, over the C ABI.
//
// The reference is Rust and rustc is not available in this environment, so the host side above
// include/mzk.h is written in C++ with the SAME names, argument meaning and error behaviour as the
// Rust items it mirrors (paths relative to myzkp/src/modules/):
//
//   FiniteFieldElement<M>, ModulusValue      algebra/field.rs:87-133, :94-96
//   EllipticCurvePoint (BN254 G1 only)       algebra/curve/curve.rs:17-46, curve/bn128.rs:31
//   Polynomial<F>                            algebra/polynomial.rs:69-74
//     ::eval_with_powers_on_curve            polynomial.rs:156-165      -> mzk_msm_g1_bn254
//     ::fft_multiply                         polynomial.rs:242-276      -> mzk_fft_multiply
//     ::scale                                polynomial.rs:167-174      -> mzk_poly_scale
//   ntt / intt / fast_multiply / fast_coset_evaluate   algebra/ntt.rs:7-116, :254-269
//   PublicKeyKZG, ProofKZG, setup_kzg_with_alpha / commit_kzg / open_kzg   algebra/kzg.rs:8-72
//   get_nth_root_of_m128                     zkstark/fri.rs:423-447
//   fast_coset_divide                        algebra/ntt.rs:271-330
//   G2Point, eval_with_powers_on_curve_g2, setup_kzg_powers_2_with_alpha   curve/bn128.rs:33-49, algebra/kzg.rs:42-55,114
//   accumulate_curve_points (G1 and G2)     zksnark/utils.rs:83-92
//   Merkle::commit / open, commit_codeword   algebra/merkle.rs:15-46, zkstark/fri.rs:160-166
//   fri_split_and_fold, fri_commit           zkstark/fri.rs:144-209
//   FriProof, fri_prove                      zkstark/fri.rs:71-143      -> mzk_fri_prove (M64, <M64, Ip3>: mzk_fri_prove_gl)
//   boundary_quotients, fast_stark_dims      zkstark/fast_stark.rs:217-224, :573-616 -> mzk_poly_div_roots, mzk_stark_plan
//   FastStark (preprocess, prove), FastStarkProof   zkstark/fast_stark.rs:22-75, :177-396 -> mzk_stark_new, mzk_stark_prove
//   batch::split_and_fold / commit_gemini / open_gemini / prove_sumcheck   algebra/gemini.rs:51-144, algebra/sumcheck.rs:128-167
//   ReedSolomon, ReedSolomon2D, setup_rs1d / encode_rs1d / decode_rs1d, setup_rs2d / encode_rs2d / decode_rs2d
//                                            algebra/reedsolomon.rs:20-350, :396-455 -> mzk_rs_*, mzk_rs2d_*
//
// Values are held canonical (u64 limbs) -- the ABI wire format; arithmetic on single elements that the
// reference does on the host (a handful of scalar ops in tests) is not offered here: this header only
// marshals the bulk operations to the GPU.  Rust panics become C++ exceptions carrying the same text.
#pragma once
#include <algorithm>
#include <array>
#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <string>
#include <tuple>
#include <type_traits>
#include <utility>
#include <map>
#include <memory>
#include <optional>
#include <vector>
#include <exception>
#include "../../include/mzk.h"

namespace myzkp {

struct Panic : std::runtime_error {
  int code;
  Panic(int c, const std::string& m) : std::runtime_error(m), code(c) {}
};
inline void expect(int rc) {
  if (rc != MZK_OK) throw Panic(rc, mzk_last_error());
}
// scratch memory of the library (no reference counterpart: the reference's Vec buffers die with each call): what a context may keep
// between calls, and an explicit release; MZK_E_NOMEM surfaces through expect() like every other status
inline void set_workspace_budget(size_t bytes) { expect(mzk_set_workspace_budget(bytes)); }
inline size_t trim_workspace() { size_t r = 0; expect(mzk_trim_workspace(&r)); return r; }

// ---- ModulusValue phantom types (field.rs:94-96, :408-431; bn128.rs:19-30; fri.rs:408) -------------
struct ModEIP197 { static constexpr int FIELD_ID = MZK_FIELD_FR; static constexpr int LIMBS = 4; };
struct BN128Modulus { static constexpr int FIELD_ID = MZK_FIELD_FQ; static constexpr int LIMBS = 4; };
struct M128 { static constexpr int FIELD_ID = MZK_FIELD_M128; static constexpr int LIMBS = 2; };
struct M64 { static constexpr int FIELD_ID = MZK_FIELD_M64; static constexpr int LIMBS = 1; };     // Goldilocks, fri.rs:409
struct Ip3 { static constexpr int FIELD_ID = MZK_FIELD_M64X3; static constexpr int LIMBS = 3; };   // x^3 - x + 1 over M64, fri.rs:410-421

template <class M> struct FiniteFieldElement {
  static constexpr int FIELD_ID = M::FIELD_ID;
  std::array<uint64_t, M::LIMBS> value{};  // canonical little-endian limbs (sanitize()d, field.rs:260-270)
  FiniteFieldElement() = default;
  static FiniteFieldElement from_value(uint64_t v) {  // Ring::from_value for small values
    FiniteFieldElement e;
    e.value[0] = v;
    return e;
  }
  static FiniteFieldElement from_limbs(const uint64_t* l) {
    FiniteFieldElement e;
    std::memcpy(e.value.data(), l, 8 * M::LIMBS);
    return e;
  }
  static FiniteFieldElement zero() { return FiniteFieldElement(); }
  static FiniteFieldElement one() { return from_value(1); }
  bool is_zero() const {
    for (auto x : value) if (x) return false;
    return true;
  }
  bool operator==(const FiniteFieldElement& o) const { return value == o.value; }
  bool operator!=(const FiniteFieldElement& o) const { return !(*this == o); }
};
// ExtendedFieldElement<M, P> (efield.rs) for the one extension on the FRI path, <M64, Ip3>: value = the canonical coefficients c0, c1, c2
// of c0 + c1 x + c2 x^2 (each sanitize()d, trailing zeros kept: the wire format always has three)
template <class M, class P> struct ExtendedFieldElement {
  static constexpr int FIELD_ID = P::FIELD_ID;
  std::array<uint64_t, P::LIMBS> value{};
  ExtendedFieldElement() = default;
  static ExtendedFieldElement from_value(uint64_t v) {  // the base value v, embedded
    ExtendedFieldElement e;
    e.value[0] = v;
    return e;
  }
  static ExtendedFieldElement from_limbs(const uint64_t* l) {
    ExtendedFieldElement e;
    std::memcpy(e.value.data(), l, 8 * P::LIMBS);
    return e;
  }
  static ExtendedFieldElement zero() { return ExtendedFieldElement(); }
  static ExtendedFieldElement one() { return from_value(1); }
  bool is_zero() const {
    for (auto x : value) if (x) return false;
    return true;
  }
  bool operator==(const ExtendedFieldElement& o) const { return value == o.value; }
  bool operator!=(const ExtendedFieldElement& o) const { return !(*this == o); }
};
using FqOrder = FiniteFieldElement<ModEIP197>;  // bn128.rs:30
using Fq = FiniteFieldElement<BN128Modulus>;    // bn128.rs:29

// ---- EllipticCurvePoint<Fq, BN128Curve> = G1Point (curve.rs:17-46; bn128.rs:31) ------------------------
struct G1Point {
  bool infinity = true;  // x, y = None in the reference
  Fq x, y;
  static G1Point point_at_infinity() { return G1Point(); }
  static G1Point new_point(const Fq& x, const Fq& y) {
    G1Point p;
    p.infinity = false; p.x = x; p.y = y;
    return p;
  }
  bool is_point_at_infinity() const { return infinity; }
  bool operator==(const G1Point& o) const { return infinity == o.infinity && (infinity || (x == o.x && y == o.y)); }
  void to_wire(uint64_t* w) const {  // all-zero = infinity
    if (infinity) { std::memset(w, 0, 64); return; }
    std::memcpy(w, x.value.data(), 32);
    std::memcpy(w + 4, y.value.data(), 32);
  }
  static G1Point from_wire(const uint64_t* w) {
    bool z = true;
    for (int i = 0; i < 8; i++) z = z && w[i] == 0;
    if (z) return point_at_infinity();
    return new_point(Fq::from_limbs(w), Fq::from_limbs(w + 4));
  }
};
struct BN128 {  // bn128.rs:183-216
  static G1Point generator_g1() { return G1Point::new_point(Fq::from_value(1), Fq::from_value(2)); }
};

template <class F> static std::vector<uint64_t> to_wire(const std::vector<F>& v) {
  std::vector<uint64_t> w(v.size() * F().value.size());
  for (size_t i = 0; i < v.size(); i++) std::memcpy(&w[i * v[i].value.size()], v[i].value.data(), 8 * v[i].value.size());
  return w;
}
template <class F> static std::vector<F> from_wire(const std::vector<uint64_t>& w, size_t n) {
  std::vector<F> v(n);
  for (size_t i = 0; i < n; i++) std::memcpy(v[i].value.data(), &w[i * v[i].value.size()], 8 * v[i].value.size());
  return v;
}
static inline std::vector<uint64_t> points_to_wire(const std::vector<G1Point>& p) {
  std::vector<uint64_t> w(p.size() * 8);
  for (size_t i = 0; i < p.size(); i++) p[i].to_wire(&w[8 * i]);
  return w;
}

// ---- Polynomial<F> (polynomial.rs:69-74), coefficients in ascending degree ---------------------------
template <class F> struct Polynomial {
  std::vector<F> coef;

  // polynomial.rs:156-165.  `powers.len() < coef.len()` is the reference's slice-index panic.
  G1Point eval_with_powers_on_curve(const std::vector<G1Point>& powers) const {
    static_assert(std::is_same<F, FqOrder>::value, "MSM scalars live in FqOrder");
    if (powers.size() < coef.size())
      throw Panic(MZK_E_LENGTH, "index out of bounds: the len is " + std::to_string(powers.size()) + " but the index is " + std::to_string(powers.size()));
    auto s = to_wire(coef);
    std::vector<uint64_t> p(coef.size() * 8);
    for (size_t i = 0; i < coef.size(); i++) powers[i].to_wire(&p[8 * i]);
    uint64_t out[8];
    expect(mzk_msm_g1_bn254(s.data(), p.data(), coef.size(), out));
    return G1Point::from_wire(out);
  }

  // polynomial.rs:242-276
  Polynomial fft_multiply(const Polynomial& other, const F& omega) const {
    auto a = to_wire(coef), b = to_wire(other.coef);
    std::vector<uint64_t> out((coef.size() + other.coef.size() + 1) * F().value.size());
    size_t n = 0;
    expect(mzk_fft_multiply(field_id(), a.data(), coef.size(), b.data(), other.coef.size(), omega.value.data(), out.data(), &n));
    return Polynomial{from_wire<F>(out, n)};
  }
  // polynomial.rs:167-174: coef[i] * offset^i
  Polynomial scale(const F& offset) const {
    auto a = to_wire(coef);
    std::vector<uint64_t> out(a.size());
    expect(mzk_poly_scale(field_id(), a.data(), coef.size(), offset.value.data(), nullptr, out.data()));
    return Polynomial{from_wire<F>(out, coef.size())};
  }
  static int field_id() { return F::FIELD_ID; }      // from the element type's modulus tag
};

// ---- algebra/ntt.rs ---------------------------------------------------------------------------------------
template <class F> std::vector<F> ntt(const F& primitive_root, const std::vector<F>& values) {  // ntt.rs:7-48
  auto in = to_wire(values);
  std::vector<uint64_t> out(in.size());
  expect(mzk_ntt(Polynomial<F>::field_id(), primitive_root.value.data(), in.data(), out.data(), values.size(), 0));
  return from_wire<F>(out, values.size());
}
template <class F> std::vector<F> intt(const F& primitive_root, const std::vector<F>& values) {  // ntt.rs:50-64
  auto in = to_wire(values);
  std::vector<uint64_t> out(in.size());
  expect(mzk_ntt(Polynomial<F>::field_id(), primitive_root.value.data(), in.data(), out.data(), values.size(), 1));
  return from_wire<F>(out, values.size());
}
template <class F>
Polynomial<F> fast_multiply(const Polynomial<F>& lhs, const Polynomial<F>& rhs, const F& primitive_root, size_t root_order) {  // ntt.rs:66-116
  auto a = to_wire(lhs.coef), b = to_wire(rhs.coef);
  const size_t cap = std::max(root_order, lhs.coef.size() + rhs.coef.size()) + 1;
  std::vector<uint64_t> out(cap * F().value.size());
  size_t n = 0;
  expect(mzk_fast_multiply(Polynomial<F>::field_id(), a.data(), lhs.coef.size(), b.data(), rhs.coef.size(),
                           primitive_root.value.data(), root_order, out.data(), &n));
  return Polynomial<F>{from_wire<F>(out, n)};
}
template <class F>
std::vector<F> fast_coset_evaluate(const Polynomial<F>& polynomial, const F& offset, const F& generator, size_t order) {  // ntt.rs:254-269
  auto c = to_wire(polynomial.coef);
  std::vector<uint64_t> out(order * F().value.size());
  expect(mzk_coset_lde(Polynomial<F>::field_id(), c.data(), polynomial.coef.size(), offset.value.data(), generator.value.data(),
                       out.data(), order));
  return from_wire<F>(out, order);
}
// zkstark/fri.rs:423-447 (n given as log2)
inline FiniteFieldElement<M128> get_nth_root_of_m128(unsigned log2_n) {
  FiniteFieldElement<M128> r;
  expect(mzk_root_of_unity(MZK_FIELD_M128, log2_n, r.value.data()));
  return r;
}
// zkstark/fri.rs:449-473: a base value (every root of 2-power order is), embedded in the extension
inline ExtendedFieldElement<M64, Ip3> get_nth_root_of_m64(unsigned log2_n) {
  ExtendedFieldElement<M64, Ip3> r;
  expect(mzk_root_of_unity(MZK_FIELD_M64X3, log2_n, r.value.data()));
  return r;
}
inline FqOrder get_nth_root_of_fr(unsigned log2_n) {  // the reference ships none
  FqOrder r;
  expect(mzk_root_of_unity(MZK_FIELD_FR, log2_n, r.value.data()));
  return r;
}

// ---- algebra/kzg.rs ---------------------------------------------------------------------------------------
struct PublicKeyKZG { std::vector<G1Point> powers_1; };  // kzg.rs:8-11 (powers_2 lives in G2: out of scope)
using CommitmentKZG = G1Point;                            // kzg.rs:13
struct ProofKZG { FqOrder y; G1Point w; };                // kzg.rs:15-18

// setup_kzg (kzg.rs:27-40) with the trapdoor supplied (the reference draws it from thread_rng)
inline PublicKeyKZG setup_kzg_with_alpha(const G1Point& g1, const FqOrder& alpha, size_t max_d) {
  uint64_t g[8];
  g1.to_wire(g);
  std::vector<uint64_t> out((max_d + 1) * 8);
  expect(mzk_kzg_setup_g1(alpha.value.data(), g, max_d, out.data()));
  PublicKeyKZG pk;
  pk.powers_1.resize(max_d + 1);
  for (size_t i = 0; i <= max_d; i++) pk.powers_1[i] = G1Point::from_wire(&out[8 * i]);
  return pk;
}
inline CommitmentKZG commit_kzg(const Polynomial<FqOrder>& f, const PublicKeyKZG& pk) {  // kzg.rs:57-59
  return f.eval_with_powers_on_curve(pk.powers_1);
}
inline ProofKZG open_kzg(const Polynomial<FqOrder>& f, const FqOrder& u, const PublicKeyKZG& pk) {  // kzg.rs:61-72
  if (f.coef.size() > 1 && pk.powers_1.size() < f.coef.size() - 1)
    throw Panic(MZK_E_LENGTH, "index out of bounds: the len is " + std::to_string(pk.powers_1.size()) + " but the index is " + std::to_string(pk.powers_1.size()));
  auto c = to_wire(f.coef);
  auto p = points_to_wire(pk.powers_1);
  ProofKZG pr;
  uint64_t w[8];
  expect(mzk_kzg_open(c.data(), f.coef.size(), u.value.data(), p.data(), pr.y.value.data(), w));
  pr.w = G1Point::from_wire(w);
  return pr;
}

struct BatchProofKZG { std::vector<FqOrder> ys; G1Point w; };  // kzg.rs:20-23
using ProofDegreeBound = G1Point;                              // kzg.rs:25
inline BatchProofKZG batch_open_kzg(const Polynomial<FqOrder>& f, const std::vector<FqOrder>& us, const PublicKeyKZG& pk) {  // kzg.rs:74-88
  const size_t nq = f.coef.size() > us.size() ? f.coef.size() - us.size() : 0;
  if (pk.powers_1.size() < nq)
    throw Panic(MZK_E_LENGTH, "index out of bounds: the len is " + std::to_string(pk.powers_1.size()) + " but the index is " + std::to_string(pk.powers_1.size()));
  auto c = to_wire(f.coef), u = to_wire(us);
  auto p = points_to_wire(pk.powers_1);
  std::vector<uint64_t> ys(us.size() * 4 + 4);
  uint64_t w[8];
  expect(mzk_kzg_batch_open(c.data(), f.coef.size(), u.data(), us.size(), p.data(), ys.data(), w));
  BatchProofKZG pr;
  pr.ys = from_wire<FqOrder>(ys, us.size());
  pr.w = G1Point::from_wire(w);
  return pr;
}
inline ProofDegreeBound prove_degree_bound(const Polynomial<FqOrder>& f, const PublicKeyKZG& pk, size_t d) {  // kzg.rs:121-134
  auto c = to_wire(f.coef);
  auto p = points_to_wire(pk.powers_1);
  uint64_t w[8];
  expect(mzk_kzg_prove_degree_bound(c.data(), f.coef.size(), p.data(), pk.powers_1.size(), d, w));
  return G1Point::from_wire(w);
}
// ntt::fast_coset_divide (ntt.rs:271-330)
template <class F>
Polynomial<F> fast_coset_divide(const Polynomial<F>& lhs, const Polynomial<F>& rhs, const F& offset, const F& primitive_root, size_t root_order) {
  auto a = to_wire(lhs.coef), b = to_wire(rhs.coef);
  std::vector<uint64_t> out((lhs.coef.size() + 1) * F().value.size());
  size_t len = 0;
  expect(mzk_fast_coset_divide(Polynomial<F>::field_id(), a.data(), lhs.coef.size(), b.data(), rhs.coef.size(), offset.value.data(),
                               primitive_root.value.data(), root_order, out.data(), &len));
  return Polynomial<F>{from_wire<F>(out, len)};
}
// one round of the split-and-fold in FRI::commit (zkstark/fri.rs:182-193)
template <class F>
std::vector<F> fri_split_and_fold(const std::vector<F>& codeword, const F& alpha, const F& offset, const F& omega) {
  auto c = to_wire(codeword);
  std::vector<uint64_t> out((codeword.size() / 2 + 1) * F().value.size());
  expect(mzk_fri_fold(Polynomial<F>::field_id(), c.data(), codeword.size(), alpha.value.data(), offset.value.data(), omega.value.data(), out.data()));
  return from_wire<F>(out, codeword.size() / 2);
}

// ---- MPolynomial<F> (algebra/mpolynomials.rs:9-12): exponent vector -> coefficient --------------------------
// An ordered map stands in for the HashMap (the iteration order of evaluate_symbolic's sum does not matter in a field).
template <class F> struct MPolynomial {
  std::map<std::vector<size_t>, F> dictionary;

  // the flat term table of mzk_mpoly_compose for a set of polynomials over n_vars variables (shorter keys are padded with zeros,
  // as Add / Mul pad them, mpolynomials.rs:219-230)
  static void term_table(const std::vector<MPolynomial>& ms, size_t n_vars, std::vector<uint64_t>& coefs, std::vector<uint32_t>& exps, std::vector<size_t>& offsets) {
    offsets.assign(1, 0);
    for (const MPolynomial& m : ms) {
      for (const auto& kv : m.dictionary) {
        if (kv.first.size() > n_vars) throw Panic(MZK_E_LENGTH, "index out of bounds: the len is " + std::to_string(n_vars) + " but the index is " + std::to_string(n_vars));
        for (size_t i = 0; i < n_vars; i++) {
          const size_t e = i < kv.first.size() ? kv.first[i] : 0;
          if (e > 0xffffffffu) throw Panic(MZK_E_LENGTH, "exponent above 2^32 - 1");
          exps.push_back((uint32_t)e);
        }
        coefs.insert(coefs.end(), kv.second.value.begin(), kv.second.value.end());
      }
      offsets.push_back(coefs.size() / F().value.size());
    }
  }
  // mpolynomials.rs:125-141
  Polynomial<F> evaluate_symbolic(const std::vector<Polynomial<F>>& point) const { return evaluate_symbolic_many({*this}, point)[0]; }
  // every constraint of an AIR over one point in one call (fast_stark.rs:246-259 loops over them)
  static std::vector<Polynomial<F>> evaluate_symbolic_many(const std::vector<MPolynomial>& ms, const std::vector<Polynomial<F>>& point) {
    const size_t nl = F().value.size(), nv = point.size();
    std::vector<uint64_t> coefs, pt;
    std::vector<uint32_t> exps;
    std::vector<size_t> toff, poff(1, 0);
    term_table(ms, nv, coefs, exps, toff);
    for (const Polynomial<F>& q : point) {
      auto w = to_wire(q.coef);
      pt.insert(pt.end(), w.begin(), w.end());
      poff.push_back(pt.size() / nl);
    }
    size_t n = 0, stride = 0;
    expect(mzk_mpoly_compose_plan(Polynomial<F>::field_id(), exps.data(), toff.data(), ms.size(), nv, poff.data(), &n, &stride, nullptr));
    std::vector<uint64_t> out((ms.size() * stride + 1) * nl);
    std::vector<size_t> lens(ms.size() + 1);
    expect(mzk_mpoly_compose(Polynomial<F>::field_id(), coefs.data(), exps.data(), toff.data(), ms.size(), nv, pt.data(), poff.data(), out.data(), stride,
                             lens.data()));
    std::vector<Polynomial<F>> res(ms.size());
    for (size_t a = 0; a < ms.size(); a++) {
      res[a].coef.resize(lens[a]);
      for (size_t i = 0; i < lens[a]; i++) std::memcpy(res[a].coef[i].value.data(), &out[(a * stride + i) * nl], 8 * nl);
    }
    return res;
  }
};
// the weighted sum of FastStark::prove (fast_stark.rs:301-326): sum_i weights[i] * X^shifts[i] * terms[i]
template <class F>
Polynomial<F> weighted_combination(const std::vector<Polynomial<F>>& terms, const std::vector<F>& weights, const std::vector<size_t>& shifts) {
  if (weights.size() != terms.size() || shifts.size() != terms.size()) throw Panic(MZK_E_LENGTH, "index out of bounds: weights / shifts / terms differ in length");
  const size_t nl = F().value.size();
  std::vector<uint64_t> flat;
  std::vector<size_t> off(1, 0);
  size_t cap = 0;
  for (size_t i = 0; i < terms.size(); i++) {
    auto w = to_wire(terms[i].coef);
    flat.insert(flat.end(), w.begin(), w.end());
    off.push_back(flat.size() / nl);
    cap = std::max(cap, terms[i].coef.size() + shifts[i]);
  }
  auto w = to_wire(weights);
  std::vector<uint64_t> out((cap + 1) * nl);
  size_t len = 0;
  expect(mzk_poly_lincomb(Polynomial<F>::field_id(), flat.data(), off.data(), terms.size(), w.data(), shifts.data(), out.data(), cap, &len));
  return Polynomial<F>{from_wire<F>(out, len)};
}

// the boundary quotients of FastStark::prove (fast_stark.rs:217-224): (trace_polynomials[s] - interpolant_s) / zerofier_s with zerofier_s =
// from_monomials(zerofier_roots[s]).  The interpolant has a lower degree than the zerofier, so the quotient of the long division
// (polynomial.rs:371-405) does not depend on it and it is not an argument; an inexact division drops its remainder as the reference does.
template <class F>
std::vector<Polynomial<F>> boundary_quotients(const std::vector<Polynomial<F>>& trace_polynomials, const std::vector<std::vector<F>>& zerofier_roots) {
  if (zerofier_roots.size() != trace_polynomials.size()) throw Panic(MZK_E_LENGTH, "index out of bounds: one list of zerofier roots per trace polynomial");
  const size_t nl = F().value.size(), m = trace_polynomials.size();
  size_t stride = 0;
  for (const auto& q : trace_polynomials) stride = std::max(stride, q.coef.size());
  std::vector<uint64_t> flat(std::max<size_t>(m * stride, 1) * nl, 0), out(flat.size(), 0), roots;
  std::vector<size_t> lens(m + 1, 0), off(1, 0), out_lens(m + 1, 0);
  for (size_t s = 0; s < m; s++) {
    auto w = to_wire(trace_polynomials[s].coef);
    std::copy(w.begin(), w.end(), flat.begin() + s * stride * nl);
    lens[s] = trace_polynomials[s].coef.size();
    auto r = to_wire(zerofier_roots[s]);
    roots.insert(roots.end(), r.begin(), r.end());
    off.push_back(roots.size() / nl);
  }
  roots.resize(roots.size() + nl);      // never an empty pointer
  expect(mzk_poly_div_roots(Polynomial<F>::field_id(), flat.data(), stride, lens.data(), m, roots.data(), off.data(), out.data(), out_lens.data()));
  std::vector<Polynomial<F>> res(m);
  for (size_t s = 0; s < m; s++) {
    std::vector<uint64_t> row(out.begin() + s * stride * nl, out.begin() + (s * stride + out_lens[s]) * nl);
    res[s].coef = from_wire<F>(row, out_lens[s]);
  }
  return res;
}
// initialize_fast_stark_m128 and the degree helpers of FastStark (fast_stark.rs:573-616, :77-111, :150-160) as numbers: mzk_stark_plan.
// boundary: (cycle, register) pairs -- the values do not enter the sizes.
template <class F>
mzk_stark_dims fast_stark_dims(size_t expansion_factor, size_t num_colinearity_checks, size_t num_registers, size_t num_cycles,
                               size_t transition_constraints_degree, const std::vector<MPolynomial<F>>& transition_constraints,
                               const std::vector<std::pair<size_t, size_t>>& boundary) {
  std::vector<uint64_t> coefs;
  std::vector<uint32_t> exps;
  std::vector<size_t> toff, cyc(boundary.size() + 1, 0), reg(boundary.size() + 1, 0);
  MPolynomial<F>::term_table(transition_constraints, 1 + 2 * num_registers, coefs, exps, toff);
  exps.push_back(0);                    // never an empty pointer
  for (size_t i = 0; i < boundary.size(); i++) { cyc[i] = boundary[i].first; reg[i] = boundary[i].second; }
  mzk_stark_dims d;
  expect(mzk_stark_plan(Polynomial<F>::field_id(), expansion_factor, num_colinearity_checks, num_registers, num_cycles, transition_constraints_degree,
                        exps.data(), toff.data(), transition_constraints.size(), cyc.data(), reg.data(), boundary.size(), &d));
  return d;
}

// FastStarkProof (fast_stark.rs:22-32).  fri_proof is the packed proof of mzk_fri_prove (mzk_fri_proof_layout) with the top-level
// indices sorted; a Merkle path is its entries bottom-up (the sibling leaf's bytes, then digests).
using StarkPath = std::vector<std::vector<uint8_t>>;
template <class F> struct FastStarkProof {
  std::vector<uint8_t> fri_proof;
  std::vector<std::array<uint8_t, 32>> bqc_roots;
  std::vector<F> bqc_points;
  std::vector<StarkPath> bqc_paths;
  std::array<uint8_t, 32> rdc_root;
  std::vector<F> rdc_points, tzc_points;
  std::vector<StarkPath> rdc_paths, tzc_paths;
  std::vector<size_t> duplicated_indices;      // not in the reference's struct: the verifier recomputes them
};
// FastStark (fast_stark.rs:34-50) over mzk_stark_new / mzk_stark_prove.  preprocess() returns the transition zerofier's Merkle root (the
// zerofier and its codeword stay on the device); prove() takes the trace WITH its random rows appended and the randomizer polynomial's
// max_degree + 1 coefficients -- the reference draws both itself (fast_stark.rs:187-195, :275-282), here the caller does.
template <class F> struct FastStark {
  using Boundary = std::vector<std::tuple<size_t, size_t, F>>;       // (cycle, register, value), stark.rs
  size_t expansion_factor, num_colinearity_checks, num_registers, original_trace_length, transition_constraints_degree;
  std::vector<MPolynomial<F>> transition_constraints;
  mzk_stark* handle = nullptr;
  FastStark(size_t expansion, size_t checks, size_t registers, size_t cycles, size_t degree, const F& generator, const std::vector<MPolynomial<F>>& air)
      : expansion_factor(expansion), num_colinearity_checks(checks), num_registers(registers), original_trace_length(cycles),
        transition_constraints_degree(degree), transition_constraints(air) {
    std::vector<uint64_t> coefs;
    std::vector<uint32_t> exps;
    std::vector<size_t> toff;
    MPolynomial<F>::term_table(air, 1 + 2 * registers, coefs, exps, toff);
    coefs.resize(coefs.size() + 4);
    exps.push_back(0);
    expect(mzk_stark_new(Polynomial<F>::field_id(), expansion, checks, registers, cycles, degree, generator.value.data(), coefs.data(), exps.data(), toff.data(),
                         air.size(), &handle));
  }
  FastStark(const FastStark&) = delete;
  FastStark& operator=(const FastStark&) = delete;
  ~FastStark() { if (handle) mzk_stark_free(handle); }
  std::array<uint8_t, 32> preprocess() const {
    std::array<uint8_t, 32> root;
    expect(mzk_stark_transition_zerofier_root(handle, root.data()));
    return root;
  }
  mzk_stark_dims dims(const Boundary& boundary) const {
    std::vector<std::pair<size_t, size_t>> b;
    for (const auto& e : boundary) b.push_back({std::get<0>(e), std::get<1>(e)});
    return fast_stark_dims<F>(expansion_factor, num_colinearity_checks, num_registers, original_trace_length, transition_constraints_degree,
                              transition_constraints, b);
  }
  FastStarkProof<F> prove(const std::vector<std::vector<F>>& trace, const Boundary& boundary, const Polynomial<F>& randomizer_polynomial) const {
    const size_t nl = F().value.size(), m = num_registers;
    const mzk_stark_dims d = dims(boundary);
    uint64_t off[MZK_STARK_SECTIONS], size[MZK_STARK_SECTIONS], total = 0;
    expect(mzk_stark_proof_layout(&d, Polynomial<F>::field_id(), off, size, &total));
    std::vector<uint64_t> t;
    for (const auto& row : trace) {
      if (row.size() != m) throw Panic(MZK_E_LENGTH, "index out of bounds: a trace row has " + std::to_string(row.size()) + " registers");
      auto w = to_wire(row);
      t.insert(t.end(), w.begin(), w.end());
    }
    t.resize(t.size() + nl);
    std::vector<size_t> bc(boundary.size() + 1, 0), br(boundary.size() + 1, 0);
    std::vector<uint64_t> bv((boundary.size() + 1) * nl, 0);
    for (size_t i = 0; i < boundary.size(); i++) {
      bc[i] = std::get<0>(boundary[i]); br[i] = std::get<1>(boundary[i]);
      std::memcpy(&bv[i * nl], std::get<2>(boundary[i]).value.data(), 8 * nl);
    }
    auto r = to_wire(randomizer_polynomial.coef);
    r.resize(r.size() + nl);
    std::vector<uint8_t> raw(total);
    expect(mzk_stark_prove(handle, t.data(), trace.size(), bc.data(), br.data(), bv.data(), boundary.size(), r.data(), raw.data(), raw.size()));
    FastStarkProof<F> p;
    const size_t k = d.num_indices, esz = 8 * nl;
    size_t depth = 0;
    while (((size_t)1 << depth) < d.fri_domain_length) depth++;
    p.fri_proof.assign(raw.begin() + off[MZK_STARK_FRI], raw.begin() + off[MZK_STARK_FRI] + size[MZK_STARK_FRI]);
    p.duplicated_indices.resize(k);
    for (size_t i = 0; i < k; i++) { uint64_t v; std::memcpy(&v, &raw[off[MZK_STARK_INDICES] + 8 * i], 8); p.duplicated_indices[i] = (size_t)v; }
    p.bqc_roots.resize(m);
    for (size_t s = 0; s < m; s++) std::memcpy(p.bqc_roots[s].data(), &raw[off[MZK_STARK_BQC_ROOTS] + 32 * s], 32);
    std::memcpy(p.rdc_root.data(), &raw[off[MZK_STARK_RDC_ROOT]], 32);
    auto points = [&](int sec, size_t count) {
      std::vector<F> v(count);
      for (size_t i = 0; i < count; i++) std::memcpy(v[i].value.data(), &raw[off[sec] + i * esz], esz);
      return v;
    };
    p.bqc_points = points(MZK_STARK_BQC_POINTS, m * k);
    p.rdc_points = points(MZK_STARK_RDC_POINTS, k);
    p.tzc_points = points(MZK_STARK_TZC_POINTS, k);
    size_t entry = 0;
    auto paths = [&](int sec, size_t count) {
      std::vector<StarkPath> v(count);
      for (size_t q = 0; q < count; q++)
        for (size_t j = 0; j < depth; j++, entry++) {
          uint64_t len;
          std::memcpy(&len, &raw[off[MZK_STARK_PATH_LENS] + 8 * entry], 8);
          const uint8_t* e = &raw[off[sec] + (q * depth + j) * MZK_FRI_PATH_STRIDE];
          v[q].emplace_back(e, e + len);
        }
      return v;
    };
    p.bqc_paths = paths(MZK_STARK_BQC_PATHS, m * k);
    p.rdc_paths = paths(MZK_STARK_RDC_PATHS, k);
    p.tzc_paths = paths(MZK_STARK_TZC_PATHS, k);
    return p;
  }
};


// ---- G2 (bn128.rs:33-49): Fq2 = Fq[u]/(u^2 + 1), G2Point = EllipticCurvePoint<Fq2, BN128Curve> ----------
struct Fq2 {   // ExtendedFieldElement: poly.coef = [c0, c1]
  Fq c0, c1;
  bool operator==(const Fq2& o) const { return c0 == o.c0 && c1 == o.c1; }
};
struct G2Point {
  bool infinity = true;
  Fq2 x, y;
  static G2Point point_at_infinity() { return G2Point(); }
  static G2Point new_point(const Fq2& x, const Fq2& y) { G2Point p; p.infinity = false; p.x = x; p.y = y; return p; }
  bool is_point_at_infinity() const { return infinity; }
  bool operator==(const G2Point& o) const { return infinity == o.infinity && (infinity || (x == o.x && y == o.y)); }
  void to_wire(uint64_t* w) const {
    if (infinity) { std::memset(w, 0, 128); return; }
    std::memcpy(w, x.c0.value.data(), 32); std::memcpy(w + 4, x.c1.value.data(), 32);
    std::memcpy(w + 8, y.c0.value.data(), 32); std::memcpy(w + 12, y.c1.value.data(), 32);
  }
  static G2Point from_wire(const uint64_t* w) {
    bool z = true;
    for (int i = 0; i < 16; i++) z = z && w[i] == 0;
    if (z) return point_at_infinity();
    return new_point(Fq2{Fq::from_limbs(w), Fq::from_limbs(w + 4)}, Fq2{Fq::from_limbs(w + 8), Fq::from_limbs(w + 12)});
  }
};
// Polynomial::eval_with_powers_on_curve over G2 (polynomial.rs:156-165 as called at kzg.rs:114)
inline G2Point eval_with_powers_on_curve_g2(const Polynomial<FqOrder>& f, const std::vector<G2Point>& powers) {
  if (powers.size() < f.coef.size()) throw Panic(MZK_E_LENGTH, "index out of bounds: powers.len() < coef.len() (polynomial.rs:162)");
  auto s = to_wire(f.coef);
  std::vector<uint64_t> p(16 * f.coef.size() + 16), out(16);
  for (size_t i = 0; i < f.coef.size(); i++) powers[i].to_wire(&p[16 * i]);
  expect(mzk_msm_g2_bn254(s.data(), p.data(), f.coef.size(), out.data()));
  return G2Point::from_wire(out.data());
}
// zksnark/utils.rs:83-92 accumulate_curve_points -- the reference's second spelling of the MSM: sum_i g_vec[i] * assignment[i]
// over zip(g_vec, assignment), i.e. the SHORTER of the two lengths (no index panic), G1 or G2 points
inline G1Point accumulate_curve_points(const std::vector<G1Point>& g_vec, const std::vector<FqOrder>& assignment) {
  const size_t n = g_vec.size() < assignment.size() ? g_vec.size() : assignment.size();
  std::vector<uint64_t> s(4 * n + 4), p(8 * n + 8);
  for (size_t i = 0; i < n; i++) { std::memcpy(&s[4 * i], assignment[i].value.data(), 32); g_vec[i].to_wire(&p[8 * i]); }
  uint64_t out[8];
  expect(mzk_msm_g1_bn254(s.data(), p.data(), n, out));
  return G1Point::from_wire(out);
}
inline G2Point accumulate_curve_points(const std::vector<G2Point>& g_vec, const std::vector<FqOrder>& assignment) {
  const size_t n = g_vec.size() < assignment.size() ? g_vec.size() : assignment.size();
  std::vector<uint64_t> s(4 * n + 4), p(16 * n + 16), out(16);
  for (size_t i = 0; i < n; i++) { std::memcpy(&s[4 * i], assignment[i].value.data(), 32); g_vec[i].to_wire(&p[16 * i]); }
  expect(mzk_msm_g2_bn254(s.data(), p.data(), n, out.data()));
  return G2Point::from_wire(out.data());
}
// powers_2 of setup_kzg_with_full_g2 (kzg.rs:42-55) for a caller-supplied alpha
inline std::vector<G2Point> setup_kzg_powers_2_with_alpha(const G2Point& g2, const FqOrder& alpha, size_t max_d) {
  uint64_t g[16];
  g2.to_wire(g);
  std::vector<uint64_t> w(16 * (max_d + 1));
  expect(mzk_kzg_setup_g2(alpha.value.data(), g, max_d, w.data()));
  std::vector<G2Point> out;
  for (size_t i = 0; i <= max_d; i++) out.push_back(G2Point::from_wire(&w[16 * i]));
  return out;
}

// ---- Merkle (algebra/merkle.rs) and the FRI commit phase (zkstark/fri.rs:144-209) ------------------------
typedef std::vector<uint8_t> MerkleRoot;               // merkle.rs:4
typedef std::vector<std::vector<uint8_t>> MerklePath;  // merkle.rs:5
// SHA3-256 (FIPS 202) on the host, portable and byte-order independent: what Merkle::hash and Merkle::verify run on.  Verification stays
// on the host by design: a verifier hashes a handful of nodes.
inline std::array<uint8_t, 32> sha3_256(const uint8_t* data, size_t len) {
  static const uint64_t RC[24] = {
      0x0000000000000001ULL, 0x0000000000008082ULL, 0x800000000000808aULL, 0x8000000080008000ULL, 0x000000000000808bULL, 0x0000000080000001ULL,
      0x8000000080008081ULL, 0x8000000000008009ULL, 0x000000000000008aULL, 0x0000000000000088ULL, 0x0000000080008009ULL, 0x000000008000000aULL,
      0x000000008000808bULL, 0x800000000000008bULL, 0x8000000000008089ULL, 0x8000000000008003ULL, 0x8000000000008002ULL, 0x8000000000000080ULL,
      0x000000000000800aULL, 0x800000008000000aULL, 0x8000000080008081ULL, 0x8000000000008080ULL, 0x0000000080000001ULL, 0x8000000080008008ULL};
  static const int ROT[25] = {0, 1, 62, 28, 27, 36, 44, 6, 55, 20, 3, 10, 43, 25, 39, 41, 45, 15, 21, 8, 18, 2, 61, 56, 14};      // lane x + 5y
  constexpr size_t RATE = 136;
  uint64_t a[25] = {0};
  const auto permute = [&]() {
    for (int rnd = 0; rnd < 24; rnd++) {
      uint64_t c[5], b[25];
      for (int x = 0; x < 5; x++) c[x] = a[x] ^ a[x + 5] ^ a[x + 10] ^ a[x + 15] ^ a[x + 20];
      for (int x = 0; x < 5; x++) {
        const uint64_t r = c[(x + 1) % 5], d = c[(x + 4) % 5] ^ ((r << 1) | (r >> 63));
        for (int y = 0; y < 25; y += 5) a[x + y] ^= d;
      }
      for (int x = 0; x < 5; x++)
        for (int y = 0; y < 5; y++) {
          const uint64_t v = a[x + 5 * y];
          const int s = ROT[x + 5 * y];
          b[y + 5 * ((2 * x + 3 * y) % 5)] = s ? (v << s) | (v >> (64 - s)) : v;
        }
      for (int y = 0; y < 25; y += 5)
        for (int x = 0; x < 5; x++) a[x + y] = b[x + y] ^ (~b[(x + 1) % 5 + y] & b[(x + 2) % 5 + y]);
      a[0] ^= RC[rnd];
    }
  };
  const auto absorb = [&](size_t pos, uint8_t byte) { a[pos / 8] ^= (uint64_t)byte << (8 * (pos % 8)); };
  size_t pos = 0;
  for (size_t i = 0; i < len; i++) {
    absorb(pos, data[i]);
    if (++pos == RATE) { permute(); pos = 0; }
  }
  absorb(pos, 0x06);
  absorb(RATE - 1, 0x80);
  permute();
  std::array<uint8_t, 32> out;
  for (size_t i = 0; i < 32; i++) out[i] = (uint8_t)(a[i / 8] >> (8 * (i % 8)));
  return out;
}
struct Merkle {
  static std::vector<uint8_t> hash(const std::vector<uint8_t>& data) {          // merkle.rs:8-12
    const auto h = sha3_256(data.data(), data.size());
    return std::vector<uint8_t>(h.begin(), h.end());
  }
  // merkle.rs:49-66, as written: left / right are read off the bits of the index, which is the tree's shape when every split is even
  static bool verify(const MerkleRoot& root, size_t index, const MerklePath& path, const std::vector<uint8_t>& leaf) {
    if (path.empty()) throw Panic(MZK_E_LENGTH, "Merkle::verify: empty path (the reference indexes path[0])");
    std::vector<uint8_t> acc(leaf);
    for (size_t k = 0; k < path.size(); k++) {
      const bool last = k + 1 == path.size();
      const bool leaf_first = last ? index == 0 : index % 2 == 0;
      std::vector<uint8_t> msg(leaf_first ? acc : path[k]);
      const std::vector<uint8_t>& second = leaf_first ? path[k] : acc;
      msg.insert(msg.end(), second.begin(), second.end());
      acc = hash(msg);
      index >>= 1;
    }
    return acc == root;
  }
  static void flatten(const std::vector<std::vector<uint8_t>>& leafs, std::vector<uint8_t>& blob, std::vector<uint64_t>& off, size_t& stride) {
    off.assign(1, 0);
    stride = 32;
    for (auto& l : leafs) { blob.insert(blob.end(), l.begin(), l.end()); off.push_back(blob.size()); if (l.size() > stride) stride = l.size(); }
  }
  static MerkleRoot commit(const std::vector<std::vector<uint8_t>>& leafs) {   // merkle.rs:15-25
    std::vector<uint8_t> blob; std::vector<uint64_t> off; size_t stride;
    flatten(leafs, blob, off, stride);
    MerkleRoot root(stride);
    size_t len = 0;
    expect(mzk_merkle_commit_bytes(blob.data(), off.data(), leafs.size(), root.data(), root.size(), &len));
    root.resize(len);
    return root;
  }
  static MerklePath open(size_t index, const std::vector<std::vector<uint8_t>>& leafs) {   // merkle.rs:28-46
    std::vector<uint8_t> blob; std::vector<uint64_t> off; size_t stride;
    flatten(leafs, blob, off, stride);
    mzk_merkle* t = nullptr;
    expect(mzk_merkle_build_bytes(blob.data(), off.data(), leafs.size(), &t));
    std::vector<uint8_t> buf(stride * 64);
    uint64_t lens[64];
    size_t depth = 0;
    const int rc = mzk_merkle_open(t, index, buf.data(), stride, lens, &depth);
    mzk_merkle_free(t);
    expect(rc);
    MerklePath path;
    for (size_t k = 0; k < depth; k++) path.emplace_back(buf.begin() + k * stride, buf.begin() + k * stride + lens[k]);
    return path;
  }
};
// Merkle::commit(&codeword.map(|c| bincode::serialize(&c))) as the provers write it (fri.rs:160-166)
template <class F> MerkleRoot commit_codeword(const std::vector<F>& codeword) {
  auto c = to_wire(codeword);
  MerkleRoot root(48);
  size_t len = 0;
  expect(mzk_merkle_commit_field(Polynomial<F>::field_id(), c.data(), codeword.size(), root.data(), root.size(), &len));
  root.resize(len);
  return root;
}
// FRI::commit (fri.rs:144-209): `challenge(round, last, root) -> alpha` owns the proof stream (push the root;
// sample alpha unless last).  Returns (codewords, roots) like the reference.
template <class F> struct FriCommitment { std::vector<std::vector<F>> codewords; std::vector<MerkleRoot> roots; };
template <class F, class Fn>
FriCommitment<F> fri_commit(const std::vector<F>& initial_codeword, const F& omega, const F& offset, int num_rounds, Fn&& challenge) {
  typedef typename std::remove_reference<Fn>::type Callee;
  // a throwing transcript must not unwind through the C library: report failure (-> MZK_E_CALLBACK), rethrow below
  struct Ctx { Callee* fn; std::exception_ptr err; } cx{&challenge, nullptr};
  auto tramp = [](void* user, int round, int last, const uint8_t* root, size_t root_len, uint64_t* alpha_out) -> int {
    Ctx* c = static_cast<Ctx*>(user);
    try {
      F a = (*c->fn)(round, last != 0, MerkleRoot(root, root + root_len));
      std::memcpy(alpha_out, a.value.data(), 8 * a.value.size());
      return 0;
    } catch (...) {
      c->err = std::current_exception();
      return 1;
    }
  };
  const size_t n = initial_codeword.size(), nl = F().value.size();
  size_t total = 0;
  for (int r = 0; r < num_rounds; r++) total += n >> r;
  auto c = to_wire(initial_codeword);
  std::vector<uint8_t> roots(48 * (size_t)(num_rounds > 0 ? num_rounds : 0) + 1);
  std::vector<uint64_t> lens(num_rounds > 0 ? num_rounds : 1), all((total + 1) * nl);
  const int frc = mzk_fri_commit(Polynomial<F>::field_id(), c.data(), n, omega.value.data(), offset.value.data(), num_rounds, +tramp, &cx, roots.data(),
                                 lens.data(), all.data());
  if (cx.err) std::rethrow_exception(cx.err);
  expect(frc);
  FriCommitment<F> out;
  size_t at = 0;
  for (int r = 0; r < num_rounds; r++) {
    std::vector<uint64_t> w(all.begin() + at * nl, all.begin() + (at + (n >> r)) * nl);
    out.codewords.push_back(from_wire<F>(w, n >> r));
    out.roots.emplace_back(roots.begin() + 48 * r, roots.begin() + 48 * r + lens[r]);
    at += n >> r;
  }
  return out;
}
// FRI::prove (fri.rs:99-143) in one call (mzk_fri_prove; mzk_fri_prove_gl for the Goldilocks tags): commit, the proof stream (started empty, as FRI::prove starts it),
// sample_indices and reveal on the device.  FriProof / FriQueryLayer as fri.rs:71-82; the codeword's elements are canonical here.
template <class F> struct FriQueryLayer {
  std::pair<std::vector<F>, std::vector<MerklePath>> a, b, c;
};
template <class F> struct FriProof {
  std::vector<size_t> top_level_indices;
  std::vector<F> last_codeword;
  std::vector<MerkleRoot> merkle_roots;
  std::vector<FriQueryLayer<F>> revealed_layers;
};
template <class F>
FriProof<F> fri_prove(const std::vector<F>& initial_codeword, const F& omega, const F& offset, size_t expansion_factor, size_t num_colinearity_tests) {
  const int fid = Polynomial<F>::field_id();
  const size_t n = initial_codeword.size(), nl = F().value.size(), T = num_colinearity_tests;
  int rounds = 0;
  uint64_t off[MZK_FRI_SECTIONS], size[MZK_FRI_SECTIONS], total = 0;
  // the Goldilocks tags have entry points and a path stride of their own (mzk_fri_prove_gl: no signs, 64-byte path entries)
  constexpr bool GL = F::FIELD_ID == MZK_FIELD_M64 || F::FIELD_ID == MZK_FIELD_M64X3;
  constexpr uint64_t STRIDE = GL ? MZK_FRI_PATH_STRIDE_GL : MZK_FRI_PATH_STRIDE;
  if constexpr (GL) expect(mzk_fri_proof_layout_gl(fid, n, expansion_factor, T, &rounds, off, size, &total));
  else expect(mzk_fri_proof_layout(fid, n, expansion_factor, T, &rounds, off, size, &total));
  std::vector<uint8_t> buf(total);
  auto c = to_wire(initial_codeword);
  if constexpr (GL) expect(mzk_fri_prove_gl(fid, c.data(), n, omega.value.data(), offset.value.data(), expansion_factor, T, buf.data(), buf.size()));
  else expect(mzk_fri_prove(fid, c.data(), nullptr, n, omega.value.data(), offset.value.data(), expansion_factor, T, buf.data(), buf.size()));
  auto u64_at = [&](uint64_t byte) { uint64_t v; std::memcpy(&v, buf.data() + byte, 8); return v; };
  auto elems = [&](uint64_t byte, size_t count) {
    std::vector<uint64_t> w(count * nl);
    if (count) std::memcpy(w.data(), buf.data() + byte, 8 * w.size());
    return from_wire<F>(w, count);
  };
  FriProof<F> p;
  for (size_t s = 0; s < T; s++) p.top_level_indices.push_back((size_t)u64_at(off[MZK_FRI_TOP_INDICES] + 8 * s));
  for (int r = 0; r < rounds; r++) p.merkle_roots.emplace_back(buf.begin() + off[MZK_FRI_ROOTS] + 32 * r, buf.begin() + off[MZK_FRI_ROOTS] + 32 * r + 32);
  p.last_codeword = elems(off[MZK_FRI_LAST_CODEWORD], n >> (rounds - 1));
  size_t q = 0, e = 0;
  for (int i = 0; i + 1 < rounds; i++) {
    FriQueryLayer<F> L;
    std::pair<std::vector<F>, std::vector<MerklePath>>* parts[3] = {&L.a, &L.b, &L.c};
    for (int k = 0; k < 3; k++) {
      size_t depth = 0;
      while (((size_t)1 << depth) < (n >> (i + (k == 2)))) depth++;
      parts[k]->first = elems(off[MZK_FRI_VALUES] + 8 * nl * q, T);
      for (size_t s = 0; s < T; s++, e += depth) {
        MerklePath path;
        for (size_t l = 0; l < depth; l++) {
          const uint64_t at = off[MZK_FRI_PATHS] + STRIDE * (e + l);
          path.emplace_back(buf.begin() + at, buf.begin() + at + u64_at(off[MZK_FRI_PATH_LENS] + 8 * (e + l)));
        }
        parts[k]->second.push_back(std::move(path));
      }
      q += T;
    }
    p.revealed_layers.push_back(std::move(L));
  }
  return p;
}

// ---- extensions: the reference's per-item loops as one call ------------------------------------------------------
// The reference has no batch forms; its callers loop (fast_stark.rs:231-243 per register, fri.rs:211-260 per query,
// kzg.rs:57-59 per polynomial).  Each function below returns exactly what that loop over the single call returns.
namespace batch {

// PublicKeyKZG.powers_1 kept on the GPU (with its window tables) across commitments
struct SrsHandle {
  mzk_srs* h = nullptr;
  explicit SrsHandle(const PublicKeyKZG& pk) {
    auto p = points_to_wire(pk.powers_1);
    expect(mzk_srs_upload(p.data(), pk.powers_1.size(), &h));
  }
  // every multiple of every window-table row, for batches of short polynomials (mzk_srs_build_direct); returns the width built
  int build_direct(int window_bits = 0, size_t max_bytes = 0) {
    expect(mzk_srs_build_direct(h, window_bits, max_bytes, nullptr));
    return mzk_srs_direct_bits(h);
  }
  SrsHandle(const SrsHandle&) = delete;
  SrsHandle& operator=(const SrsHandle&) = delete;
  ~SrsHandle() { mzk_srs_free(h); }
};
// for f in fs { commit_kzg(f, pk) }   (kzg.rs:57-59); every polynomial padded with zero coefficients to the longest
inline std::vector<CommitmentKZG> commit_kzg(const std::vector<Polynomial<FqOrder>>& fs, const SrsHandle& srs) {
  size_t n = 0;
  for (auto& f : fs) n = f.coef.size() > n ? f.coef.size() : n;
  std::vector<CommitmentKZG> out(fs.size());
  if (fs.empty() || n == 0) return out;
  std::vector<uint64_t> c(fs.size() * n * 4, 0), xy(fs.size() * 8);
  for (size_t i = 0; i < fs.size(); i++)
    for (size_t j = 0; j < fs[i].coef.size(); j++) std::memcpy(&c[(i * n + j) * 4], fs[i].coef[j].value.data(), 32);
  expect(mzk_kzg_commit_srs_batch(srs.h, c.data(), n, fs.size(), xy.data()));
  for (size_t i = 0; i < fs.size(); i++) out[i] = G1Point::from_wire(&xy[8 * i]);
  return out;
}

// for (f, u) in zip(fs, us) { open_kzg(f, u, pk) }   (kzg.rs:61-72; das/avail.rs:132 opens per cell); polynomials padded with zero
// coefficients to the longest -- the quotient of a padded polynomial has zero leading coefficients, the witness is the same point
inline std::vector<ProofKZG> open_kzg(const std::vector<Polynomial<FqOrder>>& fs, const std::vector<FqOrder>& us, const SrsHandle& srs) {
  if (fs.size() != us.size()) throw Panic(MZK_E_ARG, "batch::open_kzg: one point per polynomial");
  size_t n = 0;
  for (auto& f : fs) n = f.coef.size() > n ? f.coef.size() : n;
  std::vector<ProofKZG> out(fs.size());
  if (fs.empty()) return out;
  std::vector<uint64_t> c(fs.size() * n * 4 + 4, 0), u = to_wire(us), ys(fs.size() * 4), ws(fs.size() * 8);
  for (size_t i = 0; i < fs.size(); i++)
    for (size_t j = 0; j < fs[i].coef.size(); j++) std::memcpy(&c[(i * n + j) * 4], fs[i].coef[j].value.data(), 32);
  expect(mzk_kzg_open_srs_batch(srs.h, c.data(), n, fs.size(), u.data(), ys.data(), ws.data()));
  for (size_t i = 0; i < fs.size(); i++) {
    std::memcpy(out[i].y.value.data(), &ys[4 * i], 32);
    out[i].w = G1Point::from_wire(&ws[8 * i]);
  }
  return out;
}

template <class F> static std::vector<uint64_t> rows_to_wire(const std::vector<std::vector<F>>& rows, size_t n) {
  const size_t nl = F().value.size();
  std::vector<uint64_t> w(rows.size() * n * nl, 0);
  for (size_t i = 0; i < rows.size(); i++) {
    if (rows[i].size() > n) throw Panic(MZK_E_ARG, "batch rows must have one length");
    for (size_t j = 0; j < rows[i].size(); j++) std::memcpy(&w[(i * n + j) * nl], rows[i][j].value.data(), 8 * nl);
  }
  return w;
}
template <class F> static std::vector<std::vector<F>> rows_from_wire(const std::vector<uint64_t>& w, size_t rows, size_t n) {
  const size_t nl = F().value.size();
  std::vector<std::vector<F>> out(rows, std::vector<F>(n));
  for (size_t i = 0; i < rows; i++)
    for (size_t j = 0; j < n; j++) std::memcpy(out[i][j].value.data(), &w[(i * n + j) * nl], 8 * nl);
  return out;
}
// for v in rows { ntt(root, v) } / intt   (ntt.rs:7-64); all rows of one power-of-two length
template <class F> std::vector<std::vector<F>> ntt(const F& primitive_root, const std::vector<std::vector<F>>& rows, bool inverse = false) {
  if (rows.empty()) return {};
  const size_t n = rows[0].size();
  for (auto& r : rows) if (r.size() != n) throw Panic(MZK_E_ARG, "batch rows must have one length");
  auto in = rows_to_wire(rows, n);
  std::vector<uint64_t> out(in.size());
  expect(mzk_ntt_batch(Polynomial<F>::field_id(), primitive_root.value.data(), in.data(), out.data(), n, rows.size(), inverse ? 1 : 0));
  return rows_from_wire<F>(out, rows.size(), n);
}
// for p in polys { fast_coset_evaluate(p, offset, generator, order) }   (ntt.rs:254-269); coefficients zero-padded to
// the longest polynomial (a power of two after padding is the caller's business, as in the reference)
template <class F>
std::vector<std::vector<F>> fast_coset_evaluate(const std::vector<Polynomial<F>>& polys, const F& offset, const F& generator, size_t order) {
  if (polys.empty()) return {};
  size_t n = 1;
  for (auto& p : polys) n = p.coef.size() > n ? p.coef.size() : n;
  std::vector<std::vector<F>> rows;
  for (auto& p : polys) rows.push_back(p.coef);
  auto in = rows_to_wire(rows, n);
  std::vector<uint64_t> out(polys.size() * order * F().value.size());
  expect(mzk_coset_lde_batch(Polynomial<F>::field_id(), in.data(), n, offset.value.data(), generator.value.data(), out.data(), order, polys.size()));
  return rows_from_wire<F>(out, polys.size(), order);
}
// for c in codewords { Merkle::commit(c.map(serialize)) }   (fast_stark.rs:231-243); one power-of-two length >= 2
template <class F> std::vector<MerkleRoot> commit_codewords(const std::vector<std::vector<F>>& codewords) {
  if (codewords.empty()) return {};
  const size_t n = codewords[0].size();
  for (auto& r : codewords) if (r.size() != n) throw Panic(MZK_E_ARG, "batch rows must have one length");
  auto in = rows_to_wire(codewords, n);
  std::vector<uint8_t> roots(32 * codewords.size());
  expect(mzk_merkle_commit_field_batch(Polynomial<F>::field_id(), in.data(), n, codewords.size(), roots.data()));
  std::vector<MerkleRoot> out;
  for (size_t i = 0; i < codewords.size(); i++) out.emplace_back(roots.begin() + 32 * i, roots.begin() + 32 * (i + 1));
  return out;
}
// for i in indices { Merkle::open(i, codeword.map(serialize)) }   (fri.rs:211-260): the tree is hashed once
template <class F> std::vector<MerklePath> open_codeword(const std::vector<size_t>& indices, const std::vector<F>& codeword) {
  auto c = to_wire(codeword);
  mzk_merkle* t = nullptr;
  expect(mzk_merkle_build_field(Polynomial<F>::field_id(), c.data(), codeword.size(), &t));
  const size_t stride = 48;
  std::vector<uint64_t> idx(indices.begin(), indices.end()), lens(indices.size() * 64);
  std::vector<uint8_t> buf(indices.size() * 64 * stride);
  size_t depth = 0;
  const int rc = mzk_merkle_open_batch(t, idx.data(), idx.size(), buf.data(), stride, lens.data(), &depth);
  mzk_merkle_free(t);
  expect(rc);
  std::vector<MerklePath> out(indices.size());
  for (size_t q = 0; q < indices.size(); q++)
    for (size_t l = 0; l < depth; l++) {
      const uint8_t* e = &buf[(q * depth + l) * stride];
      out[q].emplace_back(e, e + lens[q * depth + l]);
    }
  return out;
}
// for v in value_rows { fast_interpolate(domain, v, root, root_order) }   (ntt.rs:211-252): one subproduct tree
template <class F>
std::vector<Polynomial<F>> fast_interpolate(const std::vector<F>& domain, const std::vector<std::vector<F>>& value_rows, const F& primitive_root,
                                            size_t root_order) {
  if (value_rows.empty()) return {};
  const size_t n = domain.size(), nl = F().value.size();
  for (auto& r : value_rows) if (r.size() != n) throw Panic(MZK_E_ARG, "batch rows must have one length");
  auto d = to_wire(domain);
  auto v = rows_to_wire(value_rows, n);
  std::vector<uint64_t> out(value_rows.size() * (n ? n : 1) * nl);
  std::vector<size_t> lens(value_rows.size());
  expect(mzk_fast_interpolate_batch(Polynomial<F>::field_id(), d.data(), v.data(), n, value_rows.size(), primitive_root.value.data(), root_order,
                                    out.data(), lens.data()));
  std::vector<Polynomial<F>> res(value_rows.size());
  for (size_t i = 0; i < value_rows.size(); i++) {
    std::vector<uint64_t> w(out.begin() + i * n * nl, out.begin() + (i * n + lens[i]) * nl);
    res[i].coef = from_wire<F>(w, lens[i]);
  }
  return res;
}


// ntt / intt (ntt.rs:7-64) of ONE vector spread over every context of mzk_init_devices (four-step layout, mzk_ntt_multi)
template <class F> std::vector<F> ntt_multi(const F& primitive_root, const std::vector<F>& values, bool inverse = false) {
  auto in = to_wire(values);
  std::vector<uint64_t> out(in.size());
  expect(mzk_ntt_multi(Polynomial<F>::field_id(), primitive_root.value.data(), in.data(), out.data(), values.size(), inverse ? 1 : 0));
  return from_wire<F>(out, values.size());
}

// ---- Gemini and sum-check (algebra/gemini.rs, algebra/sumcheck.rs) over a device-resident SRS -----------------------------
// split_and_fold (gemini.rs:51-100) -> mzk_gemini_split_fold: the el + 1 fold levels, f_0 = coef, last = [mu]
inline std::vector<Polynomial<FqOrder>> split_and_fold(const std::vector<FqOrder>& coef, const std::vector<FqOrder>& rhos) {
  const size_t n = coef.size();
  auto c = to_wire(coef), r = to_wire(rhos);
  std::vector<uint64_t> out((2 * n + 1) * 4);
  expect(mzk_gemini_split_fold(c.data(), n, r.data(), rhos.size(), out.data()));
  std::vector<Polynomial<FqOrder>> fs;
  for (size_t len = n, at = 0; len >= 1; at += len, len /= 2) {
    std::vector<uint64_t> w(out.begin() + 4 * at, out.begin() + 4 * (at + len));
    fs.push_back(Polynomial<FqOrder>{from_wire<FqOrder>(w, len)});
  }
  return fs;
}
static inline std::vector<uint64_t> levels_to_wire(const std::vector<Polynomial<FqOrder>>& polys, size_t* n) {
  *n = polys.empty() ? 0 : polys[0].coef.size();
  std::vector<uint64_t> w;
  size_t len = *n;
  for (auto& p : polys) {             // every level at its full length 2^(el - i) (trailing zeros included)
    if (p.coef.size() > len) throw Panic(MZK_E_ARG, "gemini: the levels of split_and_fold are expected");
    auto c = to_wire(p.coef);
    c.resize(len * 4, 0);
    w.insert(w.end(), c.begin(), c.end());
    len /= 2;
  }
  return w;
}
// commit_gemini (gemini.rs:112-114) -> mzk_gemini_commit_srs
inline std::vector<CommitmentKZG> commit_gemini(const std::vector<Polynomial<FqOrder>>& polys, const SrsHandle& srs) {
  size_t n;
  auto w = levels_to_wire(polys, &n);
  std::vector<uint64_t> xy(8 * polys.size());
  expect(mzk_gemini_commit_srs(srs.h, w.data(), n, xy.data()));
  std::vector<CommitmentKZG> out(polys.size());
  for (size_t i = 0; i < polys.size(); i++) out[i] = G1Point::from_wire(&xy[8 * i]);
  return out;
}
struct ProofGemini { std::vector<BatchProofKZG> es; std::vector<G1Point> degree_proofs; };   // gemini.rs:107-110
static inline ProofGemini gemini_from_wire(size_t el, const std::vector<uint64_t>& ys, const std::vector<uint64_t>& ws, const std::vector<uint64_t>& deg) {
  ProofGemini pr;
  for (size_t i = 0; i < el; i++) {
    BatchProofKZG b;
    for (int k = 0; k < 3; k++) { FqOrder y; std::memcpy(y.value.data(), &ys[12 * i + 4 * k], 32); b.ys.push_back(y); }
    b.w = G1Point::from_wire(&ws[8 * i]);
    pr.es.push_back(b);
  }
  for (size_t i = 0; i <= el; i++) pr.degree_proofs.push_back(G1Point::from_wire(&deg[8 * i]));
  return pr;
}
// open_gemini (gemini.rs:116-144) -> mzk_gemini_open_srs
inline ProofGemini open_gemini(const std::vector<Polynomial<FqOrder>>& polys, const FqOrder& beta, const SrsHandle& srs) {
  size_t n;
  auto w = levels_to_wire(polys, &n);
  const size_t el = polys.empty() ? 0 : polys.size() - 1;
  std::vector<uint64_t> ys(12 * el + 4), ws(8 * el + 8), deg(8 * (el + 1));
  expect(mzk_gemini_open_srs(srs.h, w.data(), n, beta.value.data(), ys.data(), ws.data(), deg.data()));
  return gemini_from_wire(el, ys, ws, deg);
}
// prove_sumcheck (sumcheck.rs:128-167) for a multilinear g given by get_coefs_in_order (sumcheck.rs:97-108) -> mzk_sumcheck_prove_srs.
// challenge(round, g): g = {A_j, B_j} of g_j(X) = A_j + B_j X for round j < el (the caller pushes the MPolynomial it builds from them to
// its FiatShamirTransformer and samples r_j), g = nullptr for round el (beta: the reference samples it right after r_{el-1}).
struct SumCheckProof {                     // sumcheck.rs:110-116, g_j as (A_j, B_j), plus the challenges
  FqOrder h;
  size_t el = 0;
  std::vector<std::pair<FqOrder, FqOrder>> gs;
  std::vector<FqOrder> rs;
  FqOrder beta;
  std::vector<CommitmentKZG> c_g;
  ProofGemini pi;
};
template <class Challenge>
SumCheckProof prove_sumcheck(const std::vector<FqOrder>& coefs, const FqOrder& h, Challenge challenge, const SrsHandle& srs) {
  struct Ctx { Challenge* f; std::exception_ptr err; } cx{&challenge, nullptr};
  auto tramp = [](void* user, int round, const uint64_t* g, uint64_t* r_out) -> int {
    auto* c = static_cast<Ctx*>(user);
    try {
      FqOrder gg[2];
      if (g) { std::memcpy(gg[0].value.data(), g, 32); std::memcpy(gg[1].value.data(), g + 4, 32); }
      const FqOrder r = (*c->f)(round, g ? gg : nullptr);
      std::memcpy(r_out, r.value.data(), 32);
      return 0;
    } catch (...) {
      c->err = std::current_exception();
      return 1;
    }
  };
  const size_t n = coefs.size();
  size_t el = 0;
  while (((size_t)1 << el) < n) el++;
  const size_t k = el ? el : 1;
  auto c = to_wire(coefs);
  std::vector<uint64_t> gs(8 * k), rs(4 * k), beta(4), commits(8 * (el + 1)), ys(12 * k), ws(8 * k), deg(8 * (el + 1));
  const int rc = mzk_sumcheck_prove_srs(srs.h, c.data(), n, +tramp, &cx, gs.data(), rs.data(), beta.data(), commits.data(), ys.data(), ws.data(),
                                        deg.data());
  if (cx.err) std::rethrow_exception(cx.err);
  expect(rc);
  SumCheckProof pr;
  pr.h = h;
  pr.el = el;
  for (size_t j = 0; j < el; j++) {
    FqOrder a, b, r;
    std::memcpy(a.value.data(), &gs[8 * j], 32); std::memcpy(b.value.data(), &gs[8 * j + 4], 32); std::memcpy(r.value.data(), &rs[4 * j], 32);
    pr.gs.emplace_back(a, b);
    pr.rs.push_back(r);
  }
  std::memcpy(pr.beta.value.data(), beta.data(), 32);
  for (size_t i = 0; i <= el; i++) pr.c_g.push_back(G1Point::from_wire(&commits[8 * i]));
  pr.pi = gemini_from_wire(el, ys, ws, deg);
  return pr;
}

}  // namespace batch

// ---- examples/sumcheck: SumCheckProverGPU::prove (prover.rs:79-247) over evaluation tables -----------------------------------
// prove(max_degree, factors, header) takes the reference's MPolynomial factors: their tables over {0,1}^el (variable 0 the most
// significant index bit) are built on the device (mzk_mpoly_hypercube_evals, the reference's eval_all_binary_combinations) and the
// rounds, the transcript and the challenges run behind them in the same call (mzk_sumcheck_product_prove_terms); the tables never
// exist on the host.  The table overload takes tables the caller already has.  The reference pushes the bincode of its factors into
// the proof stream first; that bincode is a HashMap in the iteration order of one process, so the objects pushed before round 0 stay
// the caller's bytes in both overloads.
typedef std::vector<std::vector<uint8_t>> StreamObject;     // one FiatShamirTransformer::push: a Vec<Vec<u8>>
struct SumCheckProverGPU {
  static std::vector<uint8_t> bincode_usize(size_t v) {
    std::vector<uint8_t> b(8);
    for (int i = 0; i < 8; i++) b[i] = (uint8_t)((uint64_t)v >> (8 * i));
    return b;
  }
  // prover.rs:108-122: max_degree, num_factors, num_variables, then bincode(factor) of every factor (the caller's bytes)
  static std::vector<StreamObject> reference_header(size_t max_degree, size_t num_variables, const std::vector<std::vector<uint8_t>>& factor_bytes) {
    std::vector<StreamObject> h = {{bincode_usize(max_degree)}, {bincode_usize(factor_bytes.size())}, {bincode_usize(num_variables)}};
    for (const auto& f : factor_bytes) h.push_back({f});
    return h;
  }
  // the objects in stream form: per object its u64 string count, then u64 length + bytes per string
  static std::vector<uint8_t> frame_header(const std::vector<StreamObject>& objects) {
    std::vector<uint8_t> out;
    auto put = [&](uint64_t v) { for (int i = 0; i < 8; i++) out.push_back((uint8_t)(v >> (8 * i))); };
    for (const auto& obj : objects) {
      put(obj.size());
      for (const auto& s : obj) { put(s.size()); out.insert(out.end(), s.begin(), s.end()); }
    }
    return out;
  }
  // evals_over_boolean_hypercube (utils.rs) of a dense multilinear polynomial: coef[t] multiplies the x_i whose bit (el-1-i) of t is set
  static std::vector<FqOrder> evals_over_boolean_hypercube(const std::vector<FqOrder>& coef) {
    size_t el = 0;
    while (((size_t)1 << el) < coef.size()) el++;
    if (coef.size() != (size_t)1 << el) throw Panic(MZK_E_NOT_POW2, "evals_over_boolean_hypercube: 2^num_vars coefficients");
    auto c = to_wire(coef);
    std::vector<uint64_t> out(c.size() + 4);
    expect(mzk_mle_evals_from_coeffs(c.data(), el, out.data()));
    return from_wire<FqOrder>(out, coef.size());
  }
  // a factor without terms, or el = 0, leaves an empty vector whose data() may be null, which the ABI refuses: one spare element each
  static void pad_term_table(std::vector<uint64_t>& coefs, std::vector<uint32_t>& exps) {
    coefs.resize(coefs.size() + 4);
    exps.resize(exps.size() + 1);
  }
  // evals_over_boolean_hypercube (utils.rs) of a sparse factor over el variables: what eval_all_binary_combinations leaves in its
  // row of the reference's device buffer.  A factor that is not multilinear gives the table of its multilinearisation.
  static std::vector<FqOrder> evals_over_boolean_hypercube(const MPolynomial<FqOrder>& f, size_t el) {
    if (el > 30) throw Panic(MZK_E_LENGTH, "evals_over_boolean_hypercube: at most 30 variables");
    std::vector<uint64_t> coefs;
    std::vector<uint32_t> exps;
    std::vector<size_t> toff;
    MPolynomial<FqOrder>::term_table({f}, el, coefs, exps, toff);
    std::vector<uint64_t> out(4 * ((size_t)1 << el) + 4);
    pad_term_table(coefs, exps);
    expect(mzk_mpoly_hypercube_evals(coefs.data(), exps.data(), toff.data(), 1, el, MZK_HYPER_AUTO, out.data()));
    return from_wire<FqOrder>(out, (size_t)1 << el);
  }
  static std::pair<FqOrder, std::vector<uint8_t>> unpack(const std::vector<uint8_t>& proof, const uint64_t* off) {
    FqOrder sum;
    std::memcpy(sum.value.data(), &proof[off[MZK_SCP_SUM]], 32);
    uint64_t len = 0;
    std::memcpy(&len, &proof[off[MZK_SCP_TRANSCRIPT_LEN]], 8);
    const uint8_t* tx = &proof[off[MZK_SCP_TRANSCRIPT]];
    return {sum, std::vector<uint8_t>(tx, tx + len)};
  }
  // prover.rs:98: (claimed_sum, transcript.serialize()) from the factors themselves; num_variables is the maximum over the factors
  std::pair<FqOrder, std::vector<uint8_t>> prove(size_t max_degree, const std::vector<MPolynomial<FqOrder>>& factors, const std::vector<StreamObject>& header) const {
    size_t el = 0;
    for (const auto& f : factors)
      for (const auto& kv : f.dictionary) el = std::max(el, kv.first.size());
    std::vector<uint64_t> coefs;
    std::vector<uint32_t> exps;
    std::vector<size_t> toff;
    MPolynomial<FqOrder>::term_table(factors, el, coefs, exps, toff);
    pad_term_table(coefs, exps);
    const std::vector<uint8_t> h = frame_header(header);
    uint64_t off[MZK_SCP_SECTIONS], size[MZK_SCP_SECTIONS], total = 0;
    expect(mzk_sumcheck_product_layout(el, factors.size(), max_degree, h.size(), off, size, &total));
    std::vector<uint8_t> proof(total);
    expect(mzk_sumcheck_product_prove_terms(coefs.data(), exps.data(), toff.data(), factors.size(), el, max_degree, h.data(), h.size(), header.size(),
                                            proof.data(), proof.size()));
    return unpack(proof, off);
  }
  // (claimed_sum, transcript.serialize()); tables[f] = factor f's 2^el values
  std::pair<FqOrder, std::vector<uint8_t>> prove(size_t max_degree, const std::vector<std::vector<FqOrder>>& tables, const std::vector<StreamObject>& header) const {
    const size_t k = tables.size(), n = k ? tables[0].size() : 0;
    size_t el = 0;
    while (((size_t)1 << el) < n) el++;
    std::vector<uint64_t> flat;
    for (const auto& t : tables) {
      if (t.size() != n || n != (size_t)1 << el) throw Panic(MZK_E_LENGTH, "SumCheckProverGPU::prove: every factor needs 2^num_vars values");
      for (const auto& v : t) flat.insert(flat.end(), v.value.begin(), v.value.end());
    }
    const std::vector<uint8_t> h = frame_header(header);
    uint64_t off[MZK_SCP_SECTIONS], size[MZK_SCP_SECTIONS], total = 0;
    expect(mzk_sumcheck_product_layout(el, k, max_degree, h.size(), off, size, &total));
    std::vector<uint8_t> proof(total);
    expect(mzk_sumcheck_product_prove(flat.data(), el, k, max_degree, h.data(), h.size(), header.size(), proof.data(), proof.size()));
    return unpack(proof, off);
  }
};

// ---- Reed-Solomon over GF(2^8) (algebra/reedsolomon.rs) ----------------------------------------------------------------------------
// ReedSolomon<GF2to8> / ReedSolomon2D<GF2to8> with g = x (setup_rs1d / setup_rs2d, :396-416); symbols are bytes.  The library works on
// fixed lengths (n symbols per codeword, k per message); encode_rs1d gives the reference's vector -- trailing zero symbols trimmed,
// reedsolomon.rs:76-77 -- and encode_rs1d_fixed, beside it, all n symbols.  A received word shorter than n is the same word with zeros at
// the top, which is what the reference's sums make of it.
struct ReedSolomon {
  size_t n, k, d;
  ReedSolomon(size_t n_, size_t k_) : n(n_), k(k_), d(n_ - k_) {
    if (n_ < k_) throw Panic(MZK_E_ARG, "n must be at least k");                                   // :29
  }
  std::vector<uint8_t> generator_polynomial() const {                                               // :34-37
    std::vector<uint8_t> g(d + 1);
    expect(mzk_rs_generator_poly(n, k, g.data()));
    return g;
  }
};
struct ReedSolomon2D {
  size_t col_n, row_n, message_len;
  ReedSolomon2D(size_t c, size_t r, size_t len) : col_n(c), row_n(r), message_len(len) {}
};
inline ReedSolomon setup_rs1d(size_t codeword_len, size_t message_len) { return ReedSolomon(codeword_len, message_len); }
inline ReedSolomon2D setup_rs2d(size_t col_codeword_len, size_t row_codeword_len, size_t message_len) {
  return ReedSolomon2D(col_codeword_len, row_codeword_len, message_len);
}
inline std::vector<uint8_t> encode_rs1d_fixed(const std::vector<uint8_t>& message, const ReedSolomon& rs) {
  if (message.size() > rs.k) throw Panic(MZK_E_LENGTH, "Received message must be less than or equal to k");      // :55-60
  std::vector<uint8_t> m(message), code(rs.n);
  m.resize(rs.k, 0);
  expect(mzk_rs_encode(rs.n, rs.k, m.data(), 1, code.data()));
  return code;
}
inline std::vector<uint8_t> encode_rs1d(const std::vector<uint8_t>& message, const ReedSolomon& rs) {             // :418-428
  std::vector<uint8_t> code = encode_rs1d_fixed(message, rs);
  while (!code.empty() && code.back() == 0) code.pop_back();
  return code;
}
inline std::optional<std::vector<uint8_t>> decode_rs1d(const std::vector<uint8_t>& code, const ReedSolomon& rs) {  // :430-433
  if (code.size() > rs.n) throw Panic(MZK_E_LENGTH, "Received codeword must have length n");                       // :207-212
  if (code.size() < rs.d) return std::nullopt;                                                                    // :82-84
  std::vector<uint8_t> r(code), message(rs.k);
  r.resize(rs.n, 0);
  uint8_t status = 0;
  expect(mzk_rs_decode(rs.n, rs.k, r.data(), 1, nullptr, message.data(), &status));
  if (status == 255) return std::nullopt;
  message.resize(code.size() - rs.d);                                                                             // corrected[d..] of a word of code.size() symbols
  return message;
}
inline std::vector<std::vector<uint8_t>> encode_rs2d(const std::vector<uint8_t>& message, const ReedSolomon2D& rs) {      // :435-445
  std::vector<uint8_t> flat(rs.col_n * rs.row_n);
  expect(mzk_rs2d_encode(rs.col_n, rs.row_n, message.data(), message.size(), flat.data()));
  std::vector<std::vector<uint8_t>> code(rs.col_n);
  for (size_t r = 0; r < rs.col_n; r++) code[r].assign(flat.begin() + r * rs.row_n, flat.begin() + (r + 1) * rs.row_n);
  return code;
}
inline std::optional<std::vector<uint8_t>> decode_rs2d(const std::vector<std::vector<uint8_t>>& code, const ReedSolomon2D& rs) {      // :447-455
  if (code.size() != rs.col_n) throw Panic(MZK_E_LENGTH, "decode_rs2d: the code must have col_codeword_len rows");
  std::vector<uint8_t> flat;
  for (const auto& row : code) {
    if (row.size() != rs.row_n) throw Panic(MZK_E_LENGTH, "decode_rs2d: every row must have row_codeword_len symbols");
    flat.insert(flat.end(), row.begin(), row.end());
  }
  std::vector<uint8_t> data(rs.message_len);
  int ok = 0;
  expect(mzk_rs2d_decode(rs.col_n, rs.row_n, flat.data(), rs.message_len, data.data(), &ok, nullptr, nullptr));
  if (!ok) return std::nullopt;
  return data;
}

// ---- Celestia (das/celestia.rs) ------------------------------------------------------------------------------------------------------
// The reference's surface: setup, encode, commit, verify, reconstruct.  encode is the 2D code (mzk_rs2d_encode); commit is ONE call that
// hashes every row tree, every column tree and the tree over their roots (mzk_das_grid_build) and keeps the handle, so that verify's
// Merkle::open (:124-135) is a gather from the stored nodes (mzk_das_grid_open) where the reference re-hashes a whole row or column;
// the check itself is Merkle::verify on the host.  Where Merkle::open does not terminate in the reference (a leaf that is the one-leaf
// half of a three-leaf slice: ragged sides only) verify throws Panic(MZK_E_LENGTH), as Merkle::open of this mirror does.
struct SamplePosition { size_t row, col; bool is_row; };          // das/utils.rs
struct PublicParamsCelestia { size_t codeword_size, chunk_size; };
struct EncodedDataCelestia {
  std::vector<std::vector<std::vector<uint8_t>>> codewords;       // codewords[row][col] = vec![symbol]
  size_t data_size;
};
struct DasGridHandle {                                            // the device-resident trees of one commitment
  mzk_das_grid* h = nullptr;
  DasGridHandle() = default;
  explicit DasGridHandle(mzk_das_grid* g) : h(g) {}
  DasGridHandle(const DasGridHandle&) = delete;
  DasGridHandle& operator=(const DasGridHandle&) = delete;
  ~DasGridHandle() { mzk_das_grid_free(h); }
};
struct CommitmentCelestia {
  std::vector<std::vector<uint8_t>> row_roots, col_roots;
  std::vector<uint8_t> data_root;
  std::shared_ptr<DasGridHandle> grid;                            // not part of the commitment: what verify opens through
};
struct ProofCelestia { MerklePath proof; bool is_row; };
struct Celestia {
  typedef EncodedDataCelestia EncodedData;
  typedef CommitmentCelestia Commitment;
  typedef PublicParamsCelestia PublicParams;
  static PublicParams setup(size_t chunk_size, double expansion_factor, size_t /*data_size*/) {                  // :34-41
    size_t up = (size_t)expansion_factor;
    if ((double)up < expansion_factor) up++;                                                                     // expansion_factor.ceil()
    return PublicParams{chunk_size * up, chunk_size};
  }
  static EncodedData encode(const std::vector<uint8_t>& data, const PublicParams& params) {                      // :43-71
    const auto rows = encode_rs2d(data, setup_rs2d(params.codeword_size, params.codeword_size, data.size()));
    EncodedData e;
    e.data_size = data.size();
    for (const auto& row : rows) {
      e.codewords.emplace_back();
      for (uint8_t s : row) e.codewords.back().push_back(std::vector<uint8_t>(1, s));
    }
    return e;
  }
  static std::vector<uint8_t> flat(const EncodedData& encoded, size_t* rows, size_t* cols) {
    *rows = encoded.codewords.size();
    *cols = *rows ? encoded.codewords[0].size() : 0;
    std::vector<uint8_t> m;
    for (const auto& row : encoded.codewords) {
      if (row.size() != *cols) throw Panic(MZK_E_LENGTH, "Celestia: every row must have the same number of symbols");
      for (const auto& leaf : row) {
        if (leaf.size() != 1) throw Panic(MZK_E_LENGTH, "Celestia: a leaf is one symbol");
        m.push_back(leaf[0]);
      }
    }
    return m;
  }
  static Commitment commit(const EncodedData& encoded, const PublicParams& /*params*/) {                         // :73-113
    size_t rows, cols;
    const std::vector<uint8_t> m = flat(encoded, &rows, &cols);
    mzk_das_grid* g = nullptr;
    expect(mzk_das_grid_build(m.data(), rows, cols, 1, &g));
    Commitment c;
    c.grid = std::make_shared<DasGridHandle>(g);
    std::vector<uint8_t> rr(rows * 32), cr(cols * 32);
    c.data_root.resize(32);
    expect(mzk_das_grid_roots(g, rr.data(), cr.data(), c.data_root.data()));
    for (size_t r = 0; r < rows; r++) c.row_roots.emplace_back(rr.begin() + 32 * r, rr.begin() + 32 * (r + 1));
    for (size_t k = 0; k < cols; k++) c.col_roots.emplace_back(cr.begin() + 32 * k, cr.begin() + 32 * (k + 1));
    return c;
  }
  // Merkle::open(position) of the COMMITTED square, from the handle
  static ProofCelestia open(const SamplePosition& position, const Commitment& commitment, uint8_t* leaf = nullptr) {
    if (!commitment.grid || !commitment.grid->h) throw Panic(MZK_E_ARG, "Celestia: the commitment holds no grid handle");
    const uint64_t pos[4] = {0, position.row, position.col, position.is_row ? 1u : 0u};
    uint8_t paths[MZK_DAS_PATH_MAX * 32], lens[MZK_DAS_PATH_MAX], depth = 0, symbol = 0;
    expect(mzk_das_grid_open(commitment.grid->h, pos, 1, paths, lens, &depth, &symbol));
    if (depth == 0) throw Panic(MZK_E_LENGTH, "Merkle::open recurses forever on the one-leaf half of a three-leaf slice (merkle.rs:36-45)");
    ProofCelestia p;
    p.is_row = position.is_row;
    for (size_t k = 0; k < depth; k++) p.proof.emplace_back(paths + 32 * k, paths + 32 * k + lens[k]);
    if (leaf) *leaf = symbol;
    return p;
  }
  // :115-169.  The path is the committed square's (the reference opens `encoded`, which is the committed square in every honest call);
  // the leaf is encoded's, so a square that differs from the commitment at the sampled position fails as it does there.
  static bool verify(const SamplePosition& position, const EncodedData& encoded, const Commitment& commitment, const PublicParams& /*params*/) {
    const ProofCelestia proof = open(position, commitment);
    const std::vector<uint8_t>& leaf = encoded.codewords.at(position.row).at(position.col);
    if (proof.is_row) return Merkle::verify(commitment.row_roots.at(position.row), position.col, proof.proof, leaf);
    return Merkle::verify(commitment.col_roots.at(position.col), position.row, proof.proof, leaf);
  }
  static std::vector<uint8_t> reconstruct(const EncodedData& encoded, const PublicParams& params) {              // :171-185
    std::vector<std::vector<uint8_t>> reshaped;
    for (const auto& row : encoded.codewords) {
      reshaped.emplace_back();
      for (const auto& v : row) reshaped.back().push_back(v.at(0));
    }
    auto out = decode_rs2d(reshaped, setup_rs2d(params.codeword_size, params.codeword_size, encoded.data_size));
    if (!out) throw Panic(MZK_E_ARG, "called `Option::unwrap()` on a `None` value");                            // :184
    return *out;
  }
};

// ---- RescuePrime (zkstark/rescueprime.rs) ----------------------------------------------------------------------------------------------
// Built from the caller's parameters: the mirror holds no constants (the reference's own are data, tests/golden/rescue_prime_m128.json).
// hash (:401-452) and trace (:531-591) go over the host forms of mzk_rescue_*; boundary_constraints (:521-529) is host arithmetic.
// transition_constraints (:486-519) stays with the caller: symbolic MPolynomial arithmetic and Lagrange interpolation on the host; the
// AIR enters FastStark as a term table.
struct RescueHandle {
  mzk_rescue* h = nullptr;
  RescueHandle() = default;
  explicit RescueHandle(mzk_rescue* r) : h(r) {}
  RescueHandle(const RescueHandle&) = delete;
  RescueHandle& operator=(const RescueHandle&) = delete;
  ~RescueHandle() { mzk_rescue_free(h); }
};
template <class F> struct RescuePrime {
  typedef std::vector<std::vector<F>> Trace;                          // stark.rs
  typedef std::vector<std::tuple<size_t, size_t, F>> Boundary;
  size_t m, n;
  uint64_t alpha;
  std::array<uint64_t, 4> alphainv;                                   // little-endian, below 2^256
  std::vector<std::vector<F>> mds;
  std::vector<F> round_constants;
  std::shared_ptr<RescueHandle> handle;
  RescuePrime(size_t m_, size_t n_, uint64_t alpha_, const std::array<uint64_t, 4>& alphainv_, const std::vector<std::vector<F>>& mds_,
              const std::vector<F>& round_constants_)
      : m(m_), n(n_), alpha(alpha_), alphainv(alphainv_), mds(mds_), round_constants(round_constants_) {
    if (mds.size() != m || round_constants.size() != 2 * n * m) throw Panic(MZK_E_LENGTH, "RescuePrime: mds is m x m, round_constants 2 * n * m");
    std::vector<F> flat;
    for (const auto& row : mds) {
      if (row.size() != m) throw Panic(MZK_E_LENGTH, "RescuePrime: mds is m x m, round_constants 2 * n * m");
      flat.insert(flat.end(), row.begin(), row.end());
    }
    mzk_rescue* r = nullptr;
    expect(mzk_rescue_new(F::FIELD_ID, m, n, alpha, alphainv.data(), to_wire(flat).data(), to_wire(round_constants).data(), &r));
    handle = std::make_shared<RescueHandle>(r);
  }
  F hash(const F& input_element) const { return chain(input_element, 1).at(0); }                                  // :401-452
  // the outputs of `links` hashes, link l + 1 absorbing the output of link l
  std::vector<F> chain(const F& input_element, size_t links) const {
    std::vector<uint64_t> out(links * F().value.size());
    expect(mzk_rescue_hash(handle->h, input_element.value.data(), 1, links, out.data()));
    return from_wire<F>(out, links);
  }
  Trace trace(const F& input_element) const {                                                                     // :531-591
    const size_t nl = F().value.size();
    std::vector<uint64_t> w((n + 1) * m * nl);
    expect(mzk_rescue_trace(handle->h, input_element.value.data(), 1, 1, w.data(), (n + 1) * m, nullptr));
    const std::vector<F> flat = from_wire<F>(w, (n + 1) * m);
    Trace t;
    for (size_t r = 0; r <= n; r++) t.emplace_back(flat.begin() + r * m, flat.begin() + (r + 1) * m);
    return t;
  }
  Boundary boundary_constraints(const F& output_element) const {                                                  // :521-529
    Boundary b;
    b.emplace_back((size_t)0, (size_t)1, F::zero());
    b.emplace_back(n, (size_t)0, output_element);
    return b;
  }
};

}  // namespace myzkp
