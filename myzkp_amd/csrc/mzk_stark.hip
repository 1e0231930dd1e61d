// mzk_stark.hip -- FastStark (zkstark/fast_stark.rs): the plan, the handle that keeps what preprocess makes, and prove in one call.
//
// mzk_stark_prove[_dev] runs the stages of fast_stark.rs:177-396 in the reference's order over the entry points of the other translation
// units, with every polynomial and codeword in buffers the handle owns; the weights' transcript (two or three roots) is hashed on the host.
// mzk_stark_plan is host-only arithmetic: initialize_fast_stark_m128 (fast_stark.rs:573-616), the degree helpers (:77-111, :150-160)
// and FRI's round count.  Every `usize` subtraction of the reference that would underflow (a panic in a debug build, a wrapped
// length in release) is MZK_E_LENGTH here.  The stages themselves are the entry points of the other translation units
// (DESIGN.md section 9d lists them in the order of FastStark::prove).
#include "mzk_common.h"
#include "mzk_transcript.h"
#include <algorithm>

namespace mzk {

static unsigned bit_length(uint64_t v) { return v ? 64u - (unsigned)__builtin_clzll(v) : 0u; }

static int stark_plan(int fid, size_t expansion, size_t checks, size_t m, size_t cycles, size_t degree, const uint32_t* term_exps,
                      const size_t* term_offsets, size_t nc, const size_t* b_cycles, const size_t* b_regs, size_t nb, mzk_stark_dims* d, bool with_boundary = true) {
  MZK_TRY(field_check(fid, "stark_plan"));
  if (!d || (nc && !term_offsets) || (nb && (!b_cycles || !b_regs))) { set_error("stark_plan: null pointer"); return MZK_E_ARG; }
  if (m > MZK_STARK_MAX_REGISTERS) {
    set_error("stark_plan: %zu registers need %zu variables, mzk_mpoly_compose takes %d (at most %d registers)", m, 1 + 2 * m, (int)MZK_MPOLY_MAX_VARS,
              (int)MZK_STARK_MAX_REGISTERS);
    return MZK_E_ARG;
  }
  if (nc == 0) { set_error("stark_plan: no transition constraint (max_degree unwraps the maximum of an empty list, fast_stark.rs:106)"); return MZK_E_ARG; }
  if (nc > MZK_STARK_MAX_CONSTRAINTS) { set_error("stark_plan: %zu transition constraints (at most %d)", nc, (int)MZK_STARK_MAX_CONSTRAINTS); return MZK_E_ARG; }
  if (expansion == 0 || (expansion & (expansion - 1))) { set_error("stark_plan: expansion factor %zu is not a power of two", expansion); return MZK_E_NOT_POW2; }
  memset(d, 0, sizeof *d);
  const size_t nv = 1 + 2 * m;
  uint64_t nr, rl, prod;
  if (__builtin_mul_overflow((uint64_t)4, (uint64_t)checks, &nr) || __builtin_add_overflow((uint64_t)cycles, nr, &rl) ||
      __builtin_mul_overflow(rl, (uint64_t)degree, &prod)) {
    set_error("stark_plan: the randomized trace length times the constraint degree overflows");
    return MZK_E_LENGTH;
  }
  if (cycles == 0) { set_error("stark_plan: num_cycles = 0 (original_trace_length - 1, fast_stark.rs:54)"); return MZK_E_LENGTH; }
  const unsigned max_log = field_max_log(fid);
  const unsigned olog = bit_length(prod), elog = bit_length(expansion) - 1;
  if (olog + elog > max_log) {
    set_error("stark_plan: FRI domain of 2^%u elements (omicron domain 2^%u, expansion 2^%u), transforms go up to 2^%u", olog + elog, olog, elog, max_log);
    return MZK_E_LENGTH;
  }
  d->num_randomizers = nr;
  d->randomized_trace_length = rl;
  d->omicron_domain_length = (uint64_t)1 << olog;
  d->fri_domain_length = (uint64_t)1 << (olog + elog);
  d->num_registers = m;
  d->n_vars = nv;
  d->n_constraints = nc;
  // transition_degree_bounds: X has degree 1, every trace polynomial (and its shifted image) original_trace_length + num_randomizers - 1
  uint64_t max_q = 0;
  for (size_t a = 0; a < nc; a++) {
    if (term_offsets[a + 1] < term_offsets[a]) { set_error("stark_plan: term_offsets[%zu] is below term_offsets[%zu]", a + 1, a); return MZK_E_LENGTH; }
    if (term_offsets[a + 1] > term_offsets[a] && !term_exps) { set_error("stark_plan: null pointer"); return MZK_E_ARG; }
    uint64_t best = 0;
    for (size_t t = term_offsets[a]; t < term_offsets[a + 1]; t++) {
      uint64_t sum = term_exps[t * nv];
      for (size_t i = 1; i < nv; i++) {
        uint64_t part;
        if (__builtin_mul_overflow(rl - 1, (uint64_t)term_exps[t * nv + i], &part) || __builtin_add_overflow(sum, part, &sum)) {
          set_error("stark_plan: the degree bound of constraint %zu overflows", a);
          return MZK_E_LENGTH;
        }
      }
      best = sum > best ? sum : best;
    }
    if (best < (uint64_t)cycles - 1) {
      set_error("stark_plan: constraint %zu has degree bound %llu, below the transition zerofier's %zu (fast_stark.rs:99)", a, (unsigned long long)best, cycles - 1);
      return MZK_E_LENGTH;
    }
    d->transition_degree_bounds[a] = best;
    d->transition_quotient_degree_bounds[a] = best - (cycles - 1);
    max_q = d->transition_quotient_degree_bounds[a] > max_q ? d->transition_quotient_degree_bounds[a] : max_q;
  }
  const unsigned qbits = max_q ? bit_length(max_q) : 1;            // format!("{:b}", 0) is "0": one digit (fast_stark.rs:107)
  if (qbits > max_log) { set_error("stark_plan: max_degree of 2^%u - 1", qbits); return MZK_E_LENGTH; }
  d->max_degree = ((uint64_t)1 << qbits) - 1;
  d->randomizer_length = d->max_degree + 1;
  for (size_t a = 0; a < nc; a++) d->transition_shifts[a] = d->max_degree - d->transition_quotient_degree_bounds[a];
  // boundary zerofiers: one linear factor per boundary entry of the register, repeated cells included (from_monomials); an entry of a
  // register that does not exist matches no `if *r == s` and is ignored
  for (size_t j = 0; j < nb; j++)
    if (b_regs[j] < m) d->boundary_counts[b_regs[j]]++;
  for (size_t s = 0; s < m && with_boundary; s++) {
    if (d->boundary_counts[s] > rl - 1) {
      set_error("stark_plan: register %zu has %llu boundary entries, the randomized trace degree is %llu (fast_stark.rs:156)", s,
                (unsigned long long)d->boundary_counts[s], (unsigned long long)(rl - 1));
      return MZK_E_LENGTH;
    }
    d->boundary_quotient_degree_bounds[s] = rl - 1 - d->boundary_counts[s];
    if (d->boundary_quotient_degree_bounds[s] > d->max_degree) {
      set_error("stark_plan: boundary quotient %zu has degree bound %llu above max_degree = %llu (fast_stark.rs:316)", s,
                (unsigned long long)d->boundary_quotient_degree_bounds[s], (unsigned long long)d->max_degree);
      return MZK_E_LENGTH;
    }
    d->boundary_shifts[s] = d->max_degree - d->boundary_quotient_degree_bounds[s];
  }
  d->n_weights = 1 + 2 * nc + 2 * m;
  // FRI over the whole domain (fri.rs:86-97) with the conditions of mzk_fri_prove
  const int rounds = mzk_tx::fri_num_rounds(d->fri_domain_length, expansion, checks);
  if (rounds < 2) {
    set_error("stark_plan: num_rounds = %d for domain length %llu, expansion factor %zu, %zu colinearity checks; FRI::prove reads codewords[1] (fri.rs:117-121)",
              rounds, (unsigned long long)d->fri_domain_length, expansion, checks);
    return MZK_E_LENGTH;
  }
  d->fri_num_rounds = (uint64_t)rounds;
  d->fri_last_length = d->fri_domain_length >> (rounds - 1);
  if (checks > d->fri_last_length) {
    set_error("cannot sample more indices than available in last codeword; requested: %zu, available: %llu", checks, (unsigned long long)d->fri_last_length);
    return MZK_E_ARG;
  }
  d->num_indices = nr;                                             // 4 * checks: the top-level indices, each + expansion_factor, all of them + half
  return MZK_OK;
}


// ---- the proof layout -----------------------------------------------------------------------------------------------------------------
static int stark_layout(const mzk_stark_dims* d, int fid, uint64_t* off, uint64_t* size, uint64_t* total) {
  MZK_TRY(field_check(fid, "stark_proof_layout"));
  if (!d) { set_error("stark_proof_layout: null pointer"); return MZK_E_ARG; }
  if (d->num_indices == 0 || d->fri_domain_length < 2 || (d->fri_domain_length & (d->fri_domain_length - 1)) || d->num_registers > MZK_STARK_MAX_REGISTERS ||
      d->fri_num_rounds < 2) {
    set_error("stark_proof_layout: dims were not filled by mzk_stark_plan");
    return MZK_E_LENGTH;
  }
  const uint64_t esz = field_bytes(fid), m = d->num_registers, k = d->num_indices, depth = bit_length(d->fri_domain_length) - 1;
  mzk_tx::FriLayout L;
  mzk_tx::fri_layout(d->fri_domain_length, d->fri_domain_length / d->omicron_domain_length, d->num_randomizers / 4, field_limbs64(fid), &L);
  const uint64_t entries = (m + 2) * k * depth;
  const uint64_t sz[MZK_STARK_SECTIONS] = {8, L.total, 8 * k, 32 * m, 32, esz * m * k, esz * k, esz * k, (uint64_t)MZK_FRI_PATH_STRIDE * m * k * depth,
                                           (uint64_t)MZK_FRI_PATH_STRIDE * k * depth, (uint64_t)MZK_FRI_PATH_STRIDE * k * depth, 8 * entries};
  uint64_t at = 0;
  for (int i = 0; i < MZK_STARK_SECTIONS; i++) {
    if (off) off[i] = at;
    if (size) size[i] = sz[i];
    at += (sz[i] + 7) & ~(uint64_t)7;
  }
  if (total) *total = at;
  return MZK_OK;
}

// ---- SHAKE256 on the host (the weights' seed: prover_fiat_shamir(32) over the pushed roots, algebra/fiat_shamir.rs) -----------------------
static void keccak_f1600(uint64_t st[25]) {
  static const uint64_t RC[24] = {0x0000000000000001ULL, 0x0000000000008082ULL, 0x800000000000808aULL, 0x8000000080008000ULL, 0x000000000000808bULL,
                                  0x0000000080000001ULL, 0x8000000080008081ULL, 0x8000000000008009ULL, 0x000000000000008aULL, 0x0000000000000088ULL,
                                  0x0000000080008009ULL, 0x000000008000000aULL, 0x000000008000808bULL, 0x800000000000008bULL, 0x8000000000008089ULL,
                                  0x8000000000008003ULL, 0x8000000000008002ULL, 0x8000000000000080ULL, 0x000000000000800aULL, 0x800000008000000aULL,
                                  0x8000000080008081ULL, 0x8000000000008080ULL, 0x0000000080000001ULL, 0x8000000080008008ULL};
  static const int ROT[24] = {1, 3, 6, 10, 15, 21, 28, 36, 45, 55, 2, 14, 27, 41, 56, 8, 25, 43, 62, 18, 39, 61, 20, 44};
  static const int PIL[24] = {10, 7, 11, 17, 18, 3, 5, 16, 8, 21, 24, 4, 15, 23, 19, 13, 12, 2, 20, 14, 22, 9, 6, 1};
  for (int r = 0; r < 24; r++) {
    uint64_t bc[5];
    for (int i = 0; i < 5; i++) bc[i] = st[i] ^ st[i + 5] ^ st[i + 10] ^ st[i + 15] ^ st[i + 20];
    for (int i = 0; i < 5; i++) {
      const uint64_t t = bc[(i + 4) % 5] ^ ((bc[(i + 1) % 5] << 1) | (bc[(i + 1) % 5] >> 63));
      for (int j = 0; j < 25; j += 5) st[j + i] ^= t;
    }
    uint64_t t = st[1];
    for (int i = 0; i < 24; i++) {
      const int j = PIL[i];
      const uint64_t b = st[j];
      st[j] = (t << ROT[i]) | (t >> (64 - ROT[i]));
      t = b;
    }
    for (int j = 0; j < 25; j += 5) {
      for (int i = 0; i < 5; i++) bc[i] = st[j + i];
      for (int i = 0; i < 5; i++) st[j + i] ^= (~bc[(i + 1) % 5]) & bc[(i + 2) % 5];
    }
    st[0] ^= RC[r];
  }
}
static void shake256_32(const std::vector<uint8_t>& msg, uint8_t out[32]) {
  std::vector<uint8_t> padded(msg);
  padded.resize((msg.size() / mzk_tx::SHAKE_RATE + 1) * mzk_tx::SHAKE_RATE, 0);
  padded[msg.size()] ^= 0x1F;
  padded[padded.size() - 1] ^= 0x80;
  uint64_t st[25] = {0};
  for (size_t b = 0; b < padded.size(); b += mzk_tx::SHAKE_RATE) {
    for (int w = 0; w < mzk_tx::SHAKE_RATE / 8; w++) {
      uint64_t v;
      memcpy(&v, &padded[b + 8 * w], 8);
      st[w] ^= v;
    }
    keccak_f1600(st);
  }
  memcpy(out, st, 32);
}
// sample_weights (fast_stark.rs:162-175) over the pushes root_0 .. root_{k-1} (each vec![root]): nl-limb canonical elements
static void stark_weights(int fid, const uint8_t* roots, size_t k, size_t number, std::vector<uint64_t>& out) {
  std::vector<uint8_t> ser;
  auto put64 = [&](uint64_t v) { for (int i = 0; i < 8; i++) ser.push_back((uint8_t)(v >> (8 * i))); };
  put64(k);
  for (size_t i = 0; i < k; i++) { put64(1); put64(32); ser.insert(ser.end(), roots + 32 * i, roots + 32 * i + 32); }
  uint8_t seed[32];
  shake256_32(ser, seed);
  const HostField* hf = host_field(fid);
  out.assign(number * hf->nl, 0);
  for (size_t i = 0; i < number; i++) {
    uint8_t msg[40];
    memcpy(msg, seed, 32);
    for (int j = 0; j < 8; j++) msg[32 + j] = (uint8_t)((uint64_t)i >> (8 * j));
    uint64_t dg[4];
    mzk_tx::blake2b256(msg, 40, dg);
    out[i * hf->nl] = mzk_tx::sample_digest_word3(dg[3]);      // F::sample wraps at 2^64: below either modulus, already canonical
  }
}

}  // namespace mzk

// FastStark with what preprocess (fast_stark.rs:52-75) makes, and the buffers one prove needs
struct mzk_stark {
  int fid, ctx_index;
  size_t e, checks, m, cycles, degree, nc, nv, rl, olen, flen, cstride, tz_len;
  uint64_t g[4], omega[4], omicron[4];
  std::vector<uint64_t> coefs, domain;
  std::vector<uint32_t> exps;
  std::vector<size_t> toff;
  mzk_stark_dims dims;                   // without a boundary
  struct Buf : mzk::DevMem { operator char*() const { return as<char>(); } };       // read as the char* it owns
  Buf d_tz, d_tz_cw, d_vals, d_point, d_bq, d_cw, d_tpoly, d_tq, d_lin, d_comb, d_comb_cw, d_fri, d_stage;
  size_t stage_bytes = 0;
  mzk_merkle* tz_tree = nullptr;
  uint8_t tz_root[32];
  ~mzk_stark() { if (tz_tree) mzk_merkle_free(tz_tree); }
};

namespace mzk {
#define STARK_TRY(x) do { int _rc = (x); if (_rc != MZK_OK) return fail(_rc); } while (0)
#define STARK_HIP(x) do { if ((x) != hipSuccess) { set_error("stark_prove: %s failed", #x); return fail(MZK_E_HIP); } } while (0)

static int stark_prove_dev(mzk_stark* h, const void* d_trace, const size_t* b_cycles, const size_t* b_regs, const uint64_t* b_values, size_t nb,
                           const void* d_randomizer, void* d_proof, hipStream_t s) {
  (void)b_values;        // the interpolant never enters the quotient (mzk_poly_div_roots)
  const int fid = h->fid;
  const HostField* hf = host_field(fid);
  const size_t esz = field_bytes(fid), nl = hf->nl, m = h->m, nc = h->nc, rl = h->rl, flen = h->flen;
  mzk_stark_dims d;
  MZK_TRY(stark_plan(fid, h->e, h->checks, m, h->cycles, h->degree, h->exps.data(), h->toff.data(), nc, b_cycles, b_regs, nb, &d));
  uint64_t off[MZK_STARK_SECTIONS], size[MZK_STARK_SECTIONS], total;
  MZK_TRY(stark_layout(&d, fid, off, size, &total));
  std::vector<mzk_merkle*> trees;
  auto fail = [&](int rc) { (void)hipStreamSynchronize(s); for (mzk_merkle* t : trees) mzk_merkle_free(t); return rc; };
  // interpolate every register (:197-215): registers as rows, rows of rl coefficients with zero tails
  STARK_TRY(transpose_elems_dev_impl(fid, d_trace, h->d_vals, rl, m, s));
  char* d_tp = h->d_point + 2 * esz;
  std::vector<size_t> tp_lens(m + 1);
  STARK_TRY(mzk_fast_interpolate_batch_dev(fid, h->domain.data(), h->d_vals, rl, m, h->omicron, h->olen, d_tp, tp_lens.data(), s));
  for (size_t r = 0; r < m; r++)
    if (tp_lens[r] < rl) STARK_HIP(hipMemsetAsync(d_tp + (r * rl + tp_lens[r]) * esz, 0, (rl - tp_lens[r]) * esz, s));
  // boundary quotients (:217-224): the roots omicron^cycle of each register's entries, in the boundary's order
  std::vector<uint64_t> roots;
  std::vector<size_t> roff(1, 0), bq_lens(m + 1);
  for (size_t r = 0; r < m; r++) {
    for (size_t j = 0; j < nb; j++)
      if (b_regs[j] == r) { uint64_t w[4] = {0, 0, 0, 0}; h_powmod_u64(hf, w, h->omicron, b_cycles[j]); roots.insert(roots.end(), w, w + nl); }
    roff.push_back(roots.size() / nl);
  }
  roots.resize(roots.size() + nl);
  STARK_TRY(poly_div_roots_dev_impl(fid, d_tp, rl, tp_lens.data(), m, roots.data(), roff.data(), h->d_bq, bq_lens.data(), s));
  // extend, commit (:228-244); the randomizer codeword behind them (:275-299)
  STARK_TRY(coset_lde_dev_impl(fid, h->d_bq, rl, h->g, h->omega, h->d_cw, flen, s, m));
  STARK_TRY(coset_lde_dev_impl(fid, d_randomizer, d.randomizer_length, h->g, h->omega, h->d_cw + m * flen * esz, flen, s));
  std::vector<uint8_t> roots32(32 * (m + 1));
  for (size_t r = 0; r <= m; r++) {
    mzk_merkle* t = nullptr;
    STARK_TRY(mzk_merkle_build_field_dev(fid, h->d_cw + r * flen * esz, flen, &t, s));
    trees.push_back(t);
  }
  // evaluate_symbolic over (X, tp, tp.scale(omicron)) (:246-259) and the division by the transition zerofier (:261-273): nothing here
  // depends on the weights, so it is enqueued before the roots are waited for
  for (size_t r = 0; r < m; r++) STARK_TRY(poly_scale_dev_impl(fid, d_tp + r * rl * esz, rl, h->omicron, nullptr, d_tp + (m + r) * rl * esz, s));
  std::vector<size_t> poff(h->nv + 1), t_lens(nc + 1), q_lens(nc + 1);
  poff[0] = 0;
  for (size_t i = 1; i <= h->nv; i++) poff[i] = 2 + (i - 1) * rl;
  STARK_TRY(mzk_mpoly_compose_dev(fid, h->coefs.data(), h->exps.data(), h->toff.data(), nc, h->nv, h->d_point, poff.data(), h->d_tpoly, h->cstride, t_lens.data(), s));
  STARK_TRY(mzk_fast_coset_divide_batch_dev(fid, h->d_tpoly, h->cstride, t_lens.data(), nc, h->d_tz, h->tz_len, h->g, h->omicron, h->olen, h->d_tq, h->cstride,
                                            q_lens.data(), s));
  for (size_t r = 0; r <= m; r++) {
    size_t len = 0;
    STARK_TRY(mzk_merkle_root(trees[r], &roots32[32 * r], 32, &len));
    if (len != 32) { set_error("stark_prove: a codeword of one element"); return fail(MZK_E_LENGTH); }
  }
  std::vector<uint64_t> weights;
  stark_weights(fid, roots32.data(), m + 1, d.n_weights, weights);
  // the weighted sum (:301-326): randomizer, each transition quotient plain and shifted, each boundary quotient plain and shifted
  std::vector<size_t> loff(1, 0), shifts;
  auto add = [&](const void* src, size_t len, size_t shift) -> int {
    if (len && hipMemcpyAsync(h->d_lin + loff.back() * esz, src, len * esz, hipMemcpyDeviceToDevice, s) != hipSuccess) return MZK_E_HIP;
    loff.push_back(loff.back() + len);
    shifts.push_back(shift);
    return MZK_OK;
  };
  STARK_TRY(add(d_randomizer, d.randomizer_length, 0));
  for (size_t a = 0; a < nc; a++) {
    if (q_lens[a] > d.transition_quotient_degree_bounds[a] + 1) { set_error("stark_prove: transition quotient %zu exceeds its degree bound", a); return fail(MZK_E_LENGTH); }
    STARK_TRY(add(h->d_tq + a * h->cstride * esz, q_lens[a], 0));
    STARK_TRY(add(h->d_tq + a * h->cstride * esz, q_lens[a], d.transition_shifts[a]));
  }
  for (size_t r = 0; r < m; r++) {
    STARK_TRY(add(h->d_bq + r * rl * esz, bq_lens[r], 0));
    STARK_TRY(add(h->d_bq + r * rl * esz, bq_lens[r], d.boundary_shifts[r]));
  }
  size_t comb_len = 0;
  STARK_TRY(mzk_poly_lincomb_dev(fid, h->d_lin, loff.data(), shifts.size(), weights.data(), shifts.data(), h->d_comb, d.max_degree + 1, &comb_len, s));
  STARK_TRY(coset_lde_dev_impl(fid, h->d_comb, comb_len, h->g, h->omega, h->d_comb_cw, flen, s));
  // FRI::prove on its own empty proof stream (:337), then the sorted indices (:338) back into its section
  char* dp = (char*)d_proof;
  // (into a buffer of the handle's: the packed FRI proof sits 8 bytes into the STARK proof, its kernels were written for an allocation's start)
  STARK_TRY(mzk_fri_prove_dev(fid, h->d_comb_cw, nullptr, flen, h->omega, h->g, h->e, h->checks, h->d_fri, size[MZK_STARK_FRI], s));
  STARK_HIP(hipMemcpyAsync(dp + off[MZK_STARK_FRI], h->d_fri, size[MZK_STARK_FRI], hipMemcpyDeviceToDevice, s));
  uint64_t foff[MZK_FRI_SECTIONS];
  STARK_TRY(mzk_fri_proof_layout(fid, flen, h->e, h->checks, nullptr, foff, nullptr, nullptr));
  std::vector<uint64_t> head(1 + h->checks);
  STARK_TRY(d2h_sync(head.data(), dp + off[MZK_STARK_FRI] + foff[MZK_FRI_STATUS], 8, s));
  STARK_TRY(d2h_sync(head.data() + 1, dp + off[MZK_STARK_FRI] + foff[MZK_FRI_TOP_INDICES], 8 * h->checks, s));
  const uint64_t status = head[0];
  std::vector<uint64_t> top(head.begin() + 1, head.end());
  std::sort(top.begin(), top.end());
  std::vector<uint64_t> dup(top);
  for (uint64_t i : top) dup.push_back((i + h->e) % flen);
  const size_t half = dup.size();
  for (size_t i = 0; i < half; i++) dup.push_back((dup[i] + flen / 2) % flen);
  std::sort(dup.begin(), dup.end());
  // open all m + 2 trees at the duplicated indices in one pass (:338-383); the points come from the trees
  const size_t k = dup.size(), depth = bit_length(flen) - 1, nt = m + 2;
  std::vector<const mzk_merkle*> tp(trees.begin(), trees.end());
  tp.push_back(h->tz_tree);
  std::vector<uint64_t> idx;
  std::vector<size_t> counts(nt, k), depths(nt);
  for (size_t t = 0; t < nt; t++) idx.insert(idx.end(), dup.begin(), dup.end());
  std::vector<uint8_t> tailbuf(total - off[MZK_STARK_INDICES], 0);
  auto sec = [&](int id) { return tailbuf.data() + (off[id] - off[MZK_STARK_INDICES]); };
  // the paths sections are contiguous and 8-byte sized, in the order of the trees: bqc (m trees), rdc, tzc
  STARK_TRY(mzk_merkle_open_multi(tp.data(), nt, idx.data(), counts.data(), sec(MZK_STARK_BQC_PATHS), MZK_FRI_PATH_STRIDE, (uint64_t*)sec(MZK_STARK_PATH_LENS),
                                  depths.data()));
  for (size_t t = 0; t < nt; t++)
    if (depths[t] != depth) { set_error("stark_prove: a tree of depth %zu, expected %zu", depths[t], depth); return fail(MZK_E_LENGTH); }
  for (size_t t = 0; t < nt; t++)
    STARK_TRY(mzk_merkle_leaves(tp[t], dup.data(), k, (uint64_t*)(sec(MZK_STARK_BQC_POINTS) + t * k * esz), nullptr));
  memcpy(sec(MZK_STARK_INDICES), dup.data(), 8 * k);
  memcpy(sec(MZK_STARK_BQC_ROOTS), roots32.data(), 32 * m);
  memcpy(sec(MZK_STARK_RDC_ROOT), roots32.data() + 32 * m, 32);
  STARK_HIP(hipMemcpyAsync(dp + off[MZK_STARK_INDICES], tailbuf.data(), tailbuf.size(), hipMemcpyHostToDevice, s));
  STARK_HIP(hipMemcpyAsync(dp + off[MZK_STARK_FRI] + foff[MZK_FRI_TOP_INDICES], top.data(), 8 * h->checks, hipMemcpyHostToDevice, s));
  STARK_HIP(hipMemcpyAsync(dp + off[MZK_STARK_STATUS], &status, 8, hipMemcpyHostToDevice, s));
  STARK_HIP(hipStreamSynchronize(s));
  for (mzk_merkle* t : trees) mzk_merkle_free(t);
  trees.clear();
  if (status != 0) { set_error("stark_prove: sample_indices gave up (status %llu)", (unsigned long long)status); return MZK_E_RANGE; }
  return MZK_OK;
}
}  // namespace mzk

using namespace mzk;

extern "C" {

int mzk_stark_plan(int field_id, size_t expansion_factor, size_t num_colinearity_checks, size_t num_registers, size_t num_cycles,
                   size_t transition_constraints_degree, const uint32_t* term_exps, const size_t* term_offsets, size_t n_constraints,
                   const size_t* boundary_cycles, const size_t* boundary_registers, size_t n_boundary, mzk_stark_dims* out) {
  return stark_plan(field_id, expansion_factor, num_colinearity_checks, num_registers, num_cycles, transition_constraints_degree, term_exps, term_offsets,
                    n_constraints, boundary_cycles, boundary_registers, n_boundary, out);
}

int mzk_stark_proof_layout(const mzk_stark_dims* dims, int field_id, uint64_t* offsets, uint64_t* sizes, uint64_t* total_bytes) {
  return stark_layout(dims, field_id, offsets, sizes, total_bytes);
}

int mzk_stark_new(int field_id, size_t expansion_factor, size_t num_colinearity_checks, size_t num_registers, size_t num_cycles,
                  size_t transition_constraints_degree, const uint64_t* generator, const uint64_t* term_coefs, const uint32_t* term_exps,
                  const size_t* term_offsets, size_t n_constraints, mzk_stark** out) {
  MZK_ENTER();
  if (!out || !generator) { set_error("stark_new: null pointer"); return MZK_E_ARG; }
  *out = nullptr;
  mzk_stark_dims d;
  MZK_TRY(stark_plan(field_id, expansion_factor, num_colinearity_checks, num_registers, num_cycles, transition_constraints_degree, term_exps, term_offsets,
                     n_constraints, nullptr, nullptr, 0, &d, false));
  const HostField* hf = host_field(field_id);
  const size_t nl = hf->nl, esz = field_bytes(field_id), nterms = term_offsets[n_constraints] - term_offsets[0];
  if (nterms && !term_coefs) { set_error("stark_new: null pointer"); return MZK_E_ARG; }
  if (!h_is_canonical(hf, generator)) { set_error("stark_new: generator not canonical"); return MZK_E_RANGE; }
  if (num_cycles < 2) { set_error("stark_new: a trace of one cycle has no transition"); return MZK_E_LENGTH; }
  std::unique_ptr<mzk_stark> h(new mzk_stark());
  h->fid = field_id; h->ctx_index = ctx().index;
  h->e = expansion_factor; h->checks = num_colinearity_checks; h->m = num_registers; h->cycles = num_cycles; h->degree = transition_constraints_degree;
  h->nc = n_constraints; h->nv = d.n_vars; h->rl = d.randomized_trace_length; h->olen = d.omicron_domain_length; h->flen = d.fri_domain_length;
  h->dims = d;
  memset(h->g, 0, sizeof h->g); memset(h->omega, 0, sizeof h->omega); memset(h->omicron, 0, sizeof h->omicron);
  memcpy(h->g, generator, 8 * nl);
  MZK_TRY(mzk_root_of_unity(field_id, bit_length(h->flen) - 1, h->omega));
  MZK_TRY(mzk_root_of_unity(field_id, bit_length(h->olen) - 1, h->omicron));
  h->toff.assign(term_offsets, term_offsets + n_constraints + 1);
  for (size_t& o : h->toff) o -= term_offsets[0];
  h->coefs.assign(term_coefs + term_offsets[0] * nl, term_coefs + term_offsets[n_constraints] * nl);
  h->coefs.resize(h->coefs.size() + nl);
  h->exps.assign(term_exps + term_offsets[0] * h->nv, term_exps + term_offsets[n_constraints] * h->nv);
  h->exps.resize(h->exps.size() + 1);
  h->domain.assign(h->rl * nl, 0);
  h->domain[0] = 1;
  for (size_t i = 1; i < h->rl; i++) h_mulmod(hf, &h->domain[i * nl], &h->domain[(i - 1) * nl], h->omicron);
  // the composed constraints' row stride, from the untrimmed point lengths (2, rl, rl, ..)
  std::vector<size_t> poff(h->nv + 1, 0);
  for (size_t i = 1; i <= h->nv; i++) poff[i] = 2 + (i - 1) * h->rl;
  size_t ntr = 0;
  MZK_TRY(mzk_mpoly_compose_plan(field_id, h->exps.data(), h->toff.data(), h->nc, h->nv, poff.data(), &ntr, &h->cstride, nullptr));
  if (h->cstride == 0) h->cstride = 1;
  // preprocess (:52-75): fast_zerofier over omicron^0 .. omicron^(T-2), its codeword, its tree
  const size_t nz = h->cycles - 1;
  size_t cap = 1;
  while (cap < nz + 1) cap <<= 1;
  std::vector<uint64_t> tz((cap + 1) * nl, 0);
  MZK_TRY(mzk_fast_zerofier(field_id, h->domain.data(), nz, h->omicron, h->olen, tz.data(), &h->tz_len));
  const size_t lin = d.randomizer_length + 2 * h->nc * h->cstride + 2 * h->m * h->rl;
  struct { mzk_stark::Buf* p; size_t bytes; } bufs[] = {{&h->d_tz, (h->tz_len + 1) * esz}, {&h->d_tz_cw, h->flen * esz}, {&h->d_vals, (h->m * h->rl + 1) * esz},
                                               {&h->d_point, (2 + 2 * h->m * h->rl) * esz}, {&h->d_bq, (h->m * h->rl + 1) * esz},
                                               {&h->d_cw, (h->m + 1) * h->flen * esz}, {&h->d_tpoly, h->nc * h->cstride * esz},
                                               {&h->d_tq, h->nc * h->cstride * esz}, {&h->d_lin, lin * esz}, {&h->d_comb, (d.max_degree + 1) * esz},
                                               {&h->d_comb_cw, h->flen * esz}, {&h->d_fri, 0}};
  {
    mzk_tx::FriLayout L;
    mzk_tx::fri_layout(h->flen, h->e, h->checks, (int)nl, &L);
    bufs[sizeof bufs / sizeof bufs[0] - 1].bytes = L.total + 64;
  }
  for (auto& b : bufs) MZK_TRY(b.p->alloc(b.bytes, "stark handle"));
  hipStream_t s = ctx().stream;
  WsGuard wsg(s);
  uint64_t x[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  x[nl] = 1;                                               // the polynomial X
  if (hipMemcpyAsync(h->d_point, x, 2 * esz, hipMemcpyHostToDevice, s) != hipSuccess ||
      hipMemcpyAsync(h->d_tz, tz.data(), h->tz_len * esz, hipMemcpyHostToDevice, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess) {
    set_error("stark_new: upload failed");
    return MZK_E_HIP;
  }
  MZK_TRY(coset_lde_dev_impl(field_id, h->d_tz, h->tz_len, h->g, h->omega, h->d_tz_cw, h->flen, s));
  MZK_TRY(mzk_merkle_build_field_dev(field_id, h->d_tz_cw, h->flen, &h->tz_tree, s));
  size_t len = 0;
  MZK_TRY(mzk_merkle_root(h->tz_tree, h->tz_root, 32, &len));
  *out = h.release();
  return MZK_OK;
}
void mzk_stark_free(mzk_stark* h) { delete h; }
int mzk_stark_transition_zerofier_root(const mzk_stark* h, uint8_t root[32]) {
  if (!h || !root) { set_error("stark: null pointer"); return MZK_E_ARG; }
  memcpy(root, h->tz_root, 32);
  return MZK_OK;
}
int mzk_stark_dims_of(const mzk_stark* h, mzk_stark_dims* out) {
  if (!h || !out) { set_error("stark: null pointer"); return MZK_E_ARG; }
  *out = h->dims;
  return MZK_OK;
}
static int stark_prove_check(const mzk_stark* h, const void* trace, size_t n_rows, const size_t* bc, const size_t* br, const uint64_t* bv, size_t nb,
                             const void* randomizer, const void* proof, size_t cap, uint64_t* total) {
  if (!h || !trace || !randomizer || !proof || (nb && (!bc || !br || !bv))) { set_error("stark_prove: null pointer"); return MZK_E_ARG; }
  if (n_rows != h->rl) { set_error("stark_prove: %zu trace rows, num_cycles + num_randomizers = %zu", n_rows, h->rl); return MZK_E_LENGTH; }
  mzk_stark_dims d;
  MZK_TRY(stark_plan(h->fid, h->e, h->checks, h->m, h->cycles, h->degree, h->exps.data(), h->toff.data(), h->nc, bc, br, nb, &d));
  MZK_TRY(stark_layout(&d, h->fid, nullptr, nullptr, total));
  if (cap < *total) { set_error("stark_prove: proof buffer of %zu bytes, the layout needs %llu", cap, (unsigned long long)*total); return MZK_E_LENGTH; }
  return MZK_OK;
}
int mzk_stark_prove_dev(mzk_stark* h, const void* d_trace, size_t n_rows, const size_t* boundary_cycles, const size_t* boundary_registers,
                        const uint64_t* boundary_values, size_t n_boundary, const void* d_randomizer, void* d_proof, size_t proof_cap, void* stream) {
  MZK_ENTER();
  uint64_t total = 0;
  MZK_TRY(stark_prove_check(h, d_trace, n_rows, boundary_cycles, boundary_registers, boundary_values, n_boundary, d_randomizer, d_proof, proof_cap, &total));
  WsGuard wsg((hipStream_t)stream);
  return stark_prove_dev(h, d_trace, boundary_cycles, boundary_registers, boundary_values, n_boundary, d_randomizer, d_proof, (hipStream_t)stream);
}
int mzk_stark_prove(mzk_stark* h, const uint64_t* trace, size_t n_rows, const size_t* boundary_cycles, const size_t* boundary_registers,
                    const uint64_t* boundary_values, size_t n_boundary, const uint64_t* randomizer, uint8_t* proof_out, size_t proof_cap) {
  MZK_ENTER();
  uint64_t total = 0;
  MZK_TRY(stark_prove_check(h, trace, n_rows, boundary_cycles, boundary_registers, boundary_values, n_boundary, randomizer, proof_out, proof_cap, &total));
  const HostField* hf = host_field(h->fid);
  const size_t nl = hf->nl, esz = field_bytes(h->fid), nt = h->rl * h->m, nr = h->dims.randomizer_length;
  for (size_t i = 0; i < nt; i++) if (!h_is_canonical(hf, trace + i * nl)) { set_error("stark_prove: trace element %zu not canonical", i); return MZK_E_RANGE; }
  for (size_t i = 0; i < nr; i++) if (!h_is_canonical(hf, randomizer + i * nl)) { set_error("stark_prove: randomizer[%zu] not canonical", i); return MZK_E_RANGE; }
  for (size_t i = 0; i < n_boundary; i++) if (!h_is_canonical(hf, boundary_values + i * nl)) { set_error("stark_prove: boundary value %zu not canonical", i); return MZK_E_RANGE; }
  const size_t need = (nt + nr + 2) * esz + total + 64;
  if (need > h->stage_bytes) {
    if (h->d_stage) (void)hipDeviceSynchronize();      // an earlier call's enqueued work may still read the old buffer
    h->stage_bytes = 0;
    MZK_TRY(h->d_stage.alloc(need, "stark staging"));
    h->stage_bytes = need;
  }
  hipStream_t s = ctx().stream;
  WsGuard wsg(s);
  char *d_t = h->d_stage, *d_r = d_t + (nt + 1) * esz, *d_p = d_r + (((nr + 1) * esz + 63) & ~(size_t)63);
  MZK_HIP(hipMemcpyAsync(d_t, trace, nt * esz, hipMemcpyHostToDevice, s));
  MZK_HIP(hipMemcpyAsync(d_r, randomizer, nr * esz, hipMemcpyHostToDevice, s));
  const int rc = stark_prove_dev(h, d_t, boundary_cycles, boundary_registers, boundary_values, n_boundary, d_r, d_p, s);
  const int rc2 = d2h_sync(proof_out, d_p, total, s);       // the status word travels with a refused proof too
  return rc != MZK_OK ? rc : rc2;
}

}  // extern "C"
