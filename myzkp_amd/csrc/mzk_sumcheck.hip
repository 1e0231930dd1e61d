// mzk_sumcheck.hip -- the product sum-check prover over evaluation tables (examples/sumcheck/src/prover.rs:98-247, the
// `*_cpu` twins of examples/sumcheck/src/utils.rs) with its Fiat-Shamir transcript on the device, the subset-sum butterfly that
// turns dense multilinear coefficients into such a table (evals_over_boolean_hypercube), and the tables of sparse MPolynomial factors
// from their term table (the reference prover's eval_all_binary_combinations), with the prover behind them in one call.
//
// k factors as tables of n = 2^el canonical Fr values, variable 0 the most significant index bit.  Round j (m = n >> j live entries,
// h = m / 2):  s_j(c) = sum_{i<h} prod_f (T_f[i] + c (T_f[i+h] - T_f[i])), c = 0..=d, pushed as d + 1 objects vec![bincode(s_j(c))];
// r_j = F::sample(SHAKE256(stream)[0..32)); T_f[i] <- T_f[i] + r_j (T_f[i+h] - T_f[i]).  The reference's `sum` kernel reduces one
// buffer in place from several blocks; here the mathematical definition is followed.
// bincode(FiniteFieldElement) is the library's restatement (mzk_sumcheck_tx.h), not pinned against a Rust vector.
//
// Form of the tables: canonical, standard form, everywhere ("Product sum-check").  A product of k standard-form values by
// k - 1 Montgomery products is prod / R^(k-1); the factor R^(k-1) is put back ONCE per round and point, on the reduced sum (one
// product by R^k mod p in the round-end step), so no table is ever converted and the inner loop has exactly (k-1)(d+1) products.
//
// Kernels:
//   k_sc_round<K>     one pass per round: folds round j-1's tables with r_(j-1) (read from the proof's CHALLENGES section, where the
//                     transcript step left it), writes the folded tables and accumulates s_j(0..=d) of them in the same pass
//                     (four inputs per factor and output pair); round 0 has no fold and writes nothing.  Per-workgroup partials.
//   k_sc_round_end    one workgroup: reduces the partials, writes s_j(c) to the proof, appends the d + 1 objects to the stream,
//                     rehashes the whole stream (the leading object count changed: no hash state can be kept) and writes r_j.
//   k_sc_tail         one wave: every round from SC_TAIL_M live entries per factor down, the tables in LDS, the transcript step
//                     between the rounds inside the kernel; FINALS, TRANSCRIPT_LEN and STATUS at the end.
//   k_mle_pass        the subset-sum butterfly, up to MLE_TILE_LOG index bits per pass in LDS.
//   k_hyper_tile      a sparse factor's evaluation table tile by tile: the support masks that fit a tile's high bits go into LDS, the
//                     butterfly's stages run there, the tile is written once (eval_all_binary_combinations, MZK_HYPER_TILE).
//   k_hyper_scatter   merged coefficients to table[mask] of zero-filled tables, k_mle_pass after it (MZK_HYPER_SCATTER).
#include <utility>
#include "mzk_common.h"
#include "mzk_elem.h"
#include "mzk_keccak_pair.h"
#include "mzk_sumcheck_tx.h"
#include "mzk_hypercube_plan.h"

namespace mzk {

typedef FrParams SP;
typedef Fe<SP> SE;

// a + r (b - a), canonical; a, b canonical, r_mont = r R normalised
__device__ __forceinline__ SE sc_fold1(const SE& a, const SE& b, const SE& r_mont) {
  return fe_reduce<SP>(fe_add<SP>(a, fe_mul<SP>(fe_sub_carry<SP, 2>(b, a), r_mont)));
}
// x + y for normalised x, y below 3 p each: normalised, below 3 p
__device__ __forceinline__ SE sc_add(const SE& x, const SE& y) { return fe_weak_reduce<SP>(fe_add<SP>(x, y)); }
// the sum of v over the 64 lanes of the wave, in every lane (all lanes active).  Modular addition is exact: any order, same residue.
__device__ __forceinline__ SE sc_wave_sum(SE v) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    SE o;
#pragma unroll
    for (int i = 0; i < SP::L; i++) o.l[i] = (u32)__shfl_xor((int)v.l[i], d, 64);
    v = sc_add(v, o);
  }
  return v;
}
// the challenge as the folds use it: r R mod p from the canonical r
__device__ __forceinline__ SE sc_challenge_mont(const u64* __restrict__ r) {
  u32 w[8];
#pragma unroll
  for (int i = 0; i < 4; i++) { w[2 * i] = (u32)r[i]; w[2 * i + 1] = (u32)(r[i] >> 32); }
  return fe_to_mont<SP>(fe_unpack<SP>(w));
}

// f(integral_constant<int, 0>) ... f(integral_constant<int, N - 1>): unrolled by the front end.  `#pragma unroll` gives up above the
// optimizer's size limit for pragma-unrolled loops (about ten field products), and an array indexed by a loop counter then lives in scratch.
template <int... Is, class F> __device__ __forceinline__ void sc_static_for_seq(std::integer_sequence<int, Is...>, F&& f) {
  (f(std::integral_constant<int, Is>()), ...);
}
template <int N, class F> __device__ __forceinline__ void sc_static_for(F&& f) { sc_static_for_seq(std::make_integer_sequence<int, N>(), f); }

// ---- the grid rounds --------------------------------------------------------------------------------------------------------
constexpr int SC_THREADS = 128;
constexpr int SC_WAVES = SC_THREADS / 64;
constexpr int SC_MAX_WG = 2048;
constexpr int SC_END_THREADS = 256;
constexpr int SC_END_WAVES = SC_END_THREADS / 64;
// src: factor f at src + f * src_stride elements.  chal == null (round 0): the live table is src itself, m = 2 h entries.
// Otherwise src holds 4 h entries per factor and out[i] = fold(src[i], src[i + 2 h]) for i < 2 h goes to dst (stride 2 h).
// partials: (D + 1) canonical values per workgroup, prod / R^(K-1) summed.
// K is a template parameter: the 2 K operands (point and difference per factor, 9 limbs each) stay in registers through the loop over
// the points.  D is not: the D + 1 accumulators are a column of LDS per lane (dynamic, (D + 1) * 9 * SC_THREADS words), read and
// written once per point and index -- 18 LDS words against K - 1 field products -- so that the loop over c stays a loop.  With both as
// template parameters and everything unrolled the 64 kernels took over ten minutes to compile and k = d = 8 needed 81 more registers.
template <int K>
__global__ __launch_bounds__(SC_THREADS) void k_sc_round(const u32* __restrict__ src, size_t src_stride, size_t h, const u64* __restrict__ chal,
                                                          u32* __restrict__ dst, u32* __restrict__ partials, int D) {
  extern __shared__ u32 sc_acc[];                       // [D + 1][L][SC_THREADS]
  __shared__ u32 S[SC_WAVES][mzk_tx::SCP_MAX_DEGREE + 1][SP::L];
  const int tid = threadIdx.x;
  for (int q = 0; q < (D + 1) * SP::L; q++) sc_acc[q * SC_THREADS + tid] = 0;
  SE rm = fe_zero<SP>();
  if (chal) rm = sc_challenge_mont(chal);
  for (size_t i = (size_t)blockIdx.x * SC_THREADS + tid; i < h; i += (size_t)gridDim.x * SC_THREADS) {
    SE pt[K], df[K];
    sc_static_for<K>([&](auto fc) __attribute__((always_inline)) {
      constexpr int f = decltype(fc)::value;
      const u32* t = src + 8 * (size_t)f * src_stride;
      SE a, b;
      if (chal) {
        a = sc_fold1(fe_gload<SP>(t, i), fe_gload<SP>(t, i + 2 * h), rm);
        b = sc_fold1(fe_gload<SP>(t, i + h), fe_gload<SP>(t, i + 3 * h), rm);
        u32* o = dst + 8 * (size_t)f * 2 * h;
        fe_gstore<SP>(o, i, a);
        fe_gstore<SP>(o, i + h, b);
      } else {
        a = fe_gload<SP>(t, i);
        b = fe_gload<SP>(t, i + h);
      }
      pt[f] = a;
      df[f] = fe_sub_carry<SP, 2>(b, a);          // b - a + 2 p: the c-points are a, a + df, a + 2 df, ... by repeated addition
    });
#pragma unroll 1
    for (int c = 0; c <= D; c++) {
      SE prod = pt[0];
      sc_static_for<K - 1>([&](auto fc) __attribute__((always_inline)) { prod = fe_mul<SP>(prod, pt[decltype(fc)::value + 1]); });
      u32* col = sc_acc + (size_t)c * SP::L * SC_THREADS + tid;
      SE a;
#pragma unroll
      for (int q = 0; q < SP::L; q++) a.l[q] = col[q * SC_THREADS];
      a = sc_add(a, prod);
#pragma unroll
      for (int q = 0; q < SP::L; q++) col[q * SC_THREADS] = a.l[q];
      if (c < D) sc_static_for<K>([&](auto fc) __attribute__((always_inline)) { pt[decltype(fc)::value] = sc_add(pt[decltype(fc)::value], df[decltype(fc)::value]); });
    }
  }
  const int wave = tid >> 6, lane = tid & 63;
  for (int c = 0; c <= D; c++) {
    const u32* col = sc_acc + (size_t)c * SP::L * SC_THREADS + tid;
    SE a;
#pragma unroll
    for (int q = 0; q < SP::L; q++) a.l[q] = col[q * SC_THREADS];
    const SE v = sc_wave_sum(a);
    if (lane == 0) {
#pragma unroll
      for (int q = 0; q < SP::L; q++) S[wave][c][q] = v.l[q];
    }
  }
  __syncthreads();
  if (tid <= D) {
    SE v;
#pragma unroll
    for (int q = 0; q < SP::L; q++) v.l[q] = S[0][tid][q];
    for (int w = 1; w < SC_WAVES; w++) {
      SE o;
#pragma unroll
      for (int q = 0; q < SP::L; q++) o.l[q] = S[w][tid][q];
      v = sc_add(v, o);
    }
    fe_gstore<SP>(partials, (size_t)blockIdx.x * (D + 1) + tid, fe_reduce<SP>(v));
  }
}

// ---- the transcript step ----------------------------------------------------------------------------------------------------
struct ScProof {
  u8* base;                      // the packed proof (device)
  u64 off[mzk_tx::SCP_COUNT];
  u64 header_objects, pos0;      // objects of the caller's header; stream bytes before round 0 (8 + header_len)
  int el, D;
  Words8 rk;                     // R^k mod p, standard form: sum / R^(k-1) times it, Montgomery-reduced, is the sum
};
// Every thread of the workgroup calls.  sw: the d + 1 canonical values of round j (LDS, 8 words each); pos: stream bytes so far.
// Writes s_j to EVALS (and C = s_0(0) + s_0(1) to SUM), appends the d + 1 objects, sets the object count, hashes the stream and
// writes r_j to CHALLENGES.  Returns the new stream length.  dig, s_len: LDS scratch.
__device__ u64 sc_tx_step(const ScProof& P, int j, u64 pos, const u32 (*sw)[8], u32* dig, u64* s_len) {
  const int tid = threadIdx.x, nt = blockDim.x;
  const int D = P.D;
  u8* tx = P.base + P.off[mzk_tx::SCP_TRANSCRIPT];
  u32* evals = reinterpret_cast<u32*>(P.base + P.off[mzk_tx::SCP_EVALS]) + 8 * (size_t)j * (D + 1);
  for (int q = tid; q < 8 * (D + 1); q += nt) evals[q] = sw[q >> 3][q & 7];
  if (tid == 0) {
    if (j == 0) {
      const SE c = fe_reduce<SP>(fe_add<SP>(fe_unpack<SP>(sw[0]), fe_unpack<SP>(sw[1])));
      u32 w[8];
      fe_pack<SP>(c, w);
      u32* sum = reinterpret_cast<u32*>(P.base + P.off[mzk_tx::SCP_SUM]);
      for (int q = 0; q < 8; q++) sum[q] = w[q];
    }
    u64 at = pos;
    for (int c = 0; c <= D; c++) at += mzk_tx::scp_write_record(tx + at, sw[c]);
    *reinterpret_cast<u64*>(tx) = P.header_objects + (u64)(j + 1) * (u64)(D + 1);
    *s_len = at;
  }
  __syncthreads();
  const u64 len = *s_len;
  if (tid < 2) fri_shake256_pair(tx, len, tid, dig);
  __syncthreads();
  if (tid < 4) {
    u64* chal = reinterpret_cast<u64*>(P.base + P.off[mzk_tx::SCP_CHALLENGES]) + 4 * (size_t)j;
    chal[tid] = tid == 0 ? mzk_tx::sample_digest_word3(((u64)dig[7] << 32) | dig[6]) : 0;
  }
  __syncthreads();
  return len;
}

// One workgroup: partials of round j -> s_j -> transcript -> r_j.  state[0]: stream bytes so far (written here; read unless j == 0).
__global__ __launch_bounds__(SC_END_THREADS) void k_sc_round_end(const u32* __restrict__ partials, int nparts, int j, ScProof P, u64* __restrict__ state) {
  __shared__ u32 S[SC_END_WAVES][SP::L];
  __shared__ u32 sw[mzk_tx::SCP_MAX_DEGREE + 1][8];
  __shared__ u32 dig[8];
  __shared__ u64 s_len;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int D = P.D;
  for (int c = 0; c <= D; c++) {
    SE acc = fe_zero<SP>();
    for (int p = tid; p < nparts; p += SC_END_THREADS) acc = sc_add(acc, fe_gload<SP>(partials, (size_t)p * (D + 1) + c));
    acc = sc_wave_sum(acc);
    if (lane == 0) {
#pragma unroll
      for (int i = 0; i < SP::L; i++) S[wave][i] = acc.l[i];
    }
    __syncthreads();
    if (tid == 0) {
      SE v = acc;
      for (int w = 1; w < SC_END_WAVES; w++) {
        SE o;
#pragma unroll
        for (int i = 0; i < SP::L; i++) o.l[i] = S[w][i];
        v = sc_add(v, o);
      }
      fe_pack<SP>(fe_reduce<SP>(fe_mul<SP>(v, fe_unpack<SP>(P.rk.w))), sw[c]);
    }
    __syncthreads();
  }
  const u64 pos = j == 0 ? P.pos0 : state[0];
  const u64 len = sc_tx_step(P, j, pos, sw, dig, &s_len);
  if (tid == 0) state[0] = len;
}

// ---- the tail ---------------------------------------------------------------------------------------------------------------
// LDS holds K tables of at most SC_TAIL_M entries: 8 x 128 x 32 bytes = 32 KiB at the largest K, half of what a workgroup may
// declare statically.  One wave: h <= 64, one lane per index pair, and every reduction is a wave reduction.
constexpr int SC_TAIL_M = 128;
constexpr int SC_TAIL_LOG = 7;
// Rounds j0 .. el-1.  fold == 0 (j0 == 0): src is the input, m entries per factor.  fold != 0: src holds 2 m entries per factor, to be
// folded with r_(j0-1) on the way in.
__global__ __launch_bounds__(64) void k_sc_tail(const u32* __restrict__ src, size_t src_stride, int fold, int m, int j0, int K, ScProof P,
                                                 const u64* __restrict__ state) {
  __shared__ u32 T[mzk_tx::SCP_MAX_FACTORS][SC_TAIL_M][8];
  __shared__ u32 sw[mzk_tx::SCP_MAX_DEGREE + 1][8];
  __shared__ u32 dig[8];
  __shared__ u64 s_len;
  const int tid = threadIdx.x;
  const int D = P.D;
  const u64* chal = reinterpret_cast<const u64*>(P.base + P.off[mzk_tx::SCP_CHALLENGES]);
  {
    SE rm = fe_zero<SP>();
    if (fold) rm = sc_challenge_mont(chal + 4 * (size_t)(j0 - 1));
    for (int f = 0; f < K; f++) {
      const u32* t = src + 8 * (size_t)f * src_stride;
      for (int i = tid; i < m; i += 64) {
        const SE v = fold ? sc_fold1(fe_gload<SP>(t, i), fe_gload<SP>(t, (size_t)i + m), rm) : fe_gload<SP>(t, i);
        fe_pack<SP>(v, T[f][i]);
      }
    }
  }
  __syncthreads();
  u64 pos = j0 == 0 ? P.pos0 : state[0];
  const SE rk = fe_unpack<SP>(P.rk.w);
  for (int j = j0; j < P.el; j++) {
    const int h = m >> 1;
    for (int c = 0; c <= D; c++) {
      SE prod = fe_zero<SP>();
      if (tid < h) {
        for (int f = 0; f < K; f++) {
          const SE a = fe_unpack<SP>(T[f][tid]);
          const SE df = fe_sub_carry<SP, 2>(fe_unpack<SP>(T[f][tid + h]), a);
          SE pt = a;
          for (int t = 0; t < c; t++) pt = sc_add(pt, df);
          prod = f == 0 ? pt : fe_mul<SP>(prod, pt);
        }
      }
      const SE total = sc_wave_sum(prod);
      if (tid == 0) fe_pack<SP>(fe_reduce<SP>(fe_mul<SP>(total, rk)), sw[c]);
    }
    __syncthreads();
    pos = sc_tx_step(P, j, pos, sw, dig, &s_len);
    const SE rm = sc_challenge_mont(chal + 4 * (size_t)j);
    if (tid < h) {
      for (int f = 0; f < K; f++) {
        const SE v = sc_fold1(fe_unpack<SP>(T[f][tid]), fe_unpack<SP>(T[f][tid + h]), rm);
        fe_pack<SP>(v, T[f][tid]);                 // in place: entry i is read by lane i alone, entry i + h is never written
      }
    }
    __syncthreads();
    m = h;
  }
  u32* fin = reinterpret_cast<u32*>(P.base + P.off[mzk_tx::SCP_FINALS]);
  for (int q = tid; q < 8 * K; q += 64) fin[q] = T[q >> 3][0][q & 7];
  if (tid == 0) {
    *reinterpret_cast<u64*>(P.base + P.off[mzk_tx::SCP_TRANSCRIPT_LEN]) = pos;
    *reinterpret_cast<u64*>(P.base + P.off[mzk_tx::SCP_STATUS]) = 0;
  }
}

// ---- host side --------------------------------------------------------------------------------------------------------------
typedef void (*ScRoundFn)(const u32*, size_t, size_t, const u64*, u32*, u32*, int);
template <int... Ks> static ScRoundFn sc_round_pick(int k, std::integer_sequence<int, Ks...>) {
  static const ScRoundFn col[] = {k_sc_round<Ks + 1>...};
  return col[k - 1];
}
static ScRoundFn sc_round_kernel(int k) { return sc_round_pick(k, std::make_integer_sequence<int, mzk_tx::SCP_MAX_FACTORS>()); }

static int scp_check(size_t el, size_t k, size_t d, size_t header_len, mzk_tx::ScpLayout* L) {
  if (k < 1 || k > (size_t)mzk_tx::SCP_MAX_FACTORS) { set_error("sumcheck_product: %zu factors (1 to %d)", k, mzk_tx::SCP_MAX_FACTORS); return MZK_E_ARG; }
  if (d < 1 || d > (size_t)mzk_tx::SCP_MAX_DEGREE) { set_error("sumcheck_product: max_degree %zu (1 to %d)", d, mzk_tx::SCP_MAX_DEGREE); return MZK_E_ARG; }
  if (el == 0) { set_error("sumcheck_product: no variable, the prover has no round to run"); return MZK_E_LENGTH; }
  if (el > (size_t)mzk_tx::SCP_MAX_VARS) { set_error("sumcheck_product: %zu variables (at most %d)", el, mzk_tx::SCP_MAX_VARS); return MZK_E_LENGTH; }
  // the layout's sizes are sums over header_len: keep them far from wrapping (no stream this long is hashed el times anyway)
  if (header_len > ((size_t)1 << 40)) { set_error("sumcheck_product: header of %zu bytes (at most 2^40)", header_len); return MZK_E_LENGTH; }
  mzk_tx::scp_layout(el, k, d, header_len, L);
  return MZK_OK;
}

// every refusal of the prover that does not read a table value, in the prover's order; sets the layout
static int scp_args_check(const void* tables, bool on_device, size_t el, size_t k, size_t d, const uint8_t* header, size_t header_len,
                          size_t header_objects, const void* proof_out, size_t proof_cap, mzk_tx::ScpLayout* Lp) {
  if (!tables || !proof_out || (header_len && !header)) { set_error("sumcheck_product_prove: null pointer"); return MZK_E_ARG; }
  mzk_tx::ScpLayout& L = *Lp;
  MZK_TRY(scp_check(el, k, d, header_len, &L));
  if (proof_cap < L.total) { set_error("sumcheck_product_prove: proof buffer of %zu bytes, the layout needs %llu", proof_cap, (unsigned long long)L.total); return MZK_E_LENGTH; }
  if (!mzk_tx::scp_header_ok(header, header_len, header_objects)) {
    set_error("sumcheck_product_prove: the header does not parse to %zu objects over %zu bytes", header_objects, header_len);
    return MZK_E_ARG;
  }
  if (on_device && (((uintptr_t)tables & 15) || ((uintptr_t)proof_out & 7))) { set_error("sumcheck_product_prove: tables need 16-byte, the proof 8-byte alignment"); return MZK_E_ARG; }
  return MZK_OK;
}

static int scp_prove_impl(const void* tables, bool on_device, size_t el, size_t k, size_t d, const uint8_t* header, size_t header_len,
                          size_t header_objects, void* proof_out, size_t proof_cap, hipStream_t s_in) {
  mzk_tx::ScpLayout L;
  MZK_TRY(scp_args_check(tables, on_device, el, k, d, header, header_len, header_objects, proof_out, proof_cap, &L));
  const size_t n = (size_t)1 << el;
  const HostField* fr = host_field(MZK_FIELD_FR);
  if (!on_device) {
    const uint64_t* t = (const uint64_t*)tables;
    for (size_t i = 0; i < k * n; i++)
      if (!h_is_canonical(fr, t + 4 * i)) { set_error("sumcheck_product_prove: table value %zu of factor %zu not canonical", i % n, i / n); return MZK_E_RANGE; }
  }
  MZK_ENTER();
  WsFrame ws("scp_prove_impl");
  hipStream_t s = on_device ? s_in : ctx().stream;
  WsGuard wsg(s);
  auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
  // rounds 0 .. j0-1 on the grid, the tail from j0 on: its first live size n >> j0 is at most SC_TAIL_M
  const int j0 = el > (size_t)SC_TAIL_LOG ? (int)el - SC_TAIL_LOG : 0;
  // one workspace block: the tables (host form) | folded tables of odd rounds | of even rounds | partials | state | the proof (host form)
  const size_t o_a = on_device ? 0 : al(k * n * 32), o_b = o_a + (j0 > 1 ? al(k * (n / 2) * 32) : 0), o_part = o_b + (j0 > 2 ? al(k * (n / 4) * 32) : 0);
  const size_t o_state = o_part + al((size_t)SC_MAX_WG * (d + 1) * 32), o_proof = o_state + 256, total = o_proof + (on_device ? 0 : al(L.total));
  uint8_t* blk;
  MZK_TRY(ws.get(WS_MISC_F, total, (void**)&blk));
  const u32* d_tab = (const u32*)tables;
  if (!on_device) {
    MZK_HIP(hipMemcpyAsync(blk, tables, k * n * 32, hipMemcpyHostToDevice, s));
    d_tab = (const u32*)blk;
  }
  ScProof P;
  P.base = on_device ? (u8*)proof_out : blk + o_proof;
  for (int q = 0; q < mzk_tx::SCP_COUNT; q++) P.off[q] = L.off[q];
  P.header_objects = header_objects;
  P.pos0 = 8 + header_len;
  P.el = (int)el;
  P.D = (int)d;
  {
    uint64_t rmod[4], rk[4];
    h_rmod(fr, rmod);
    memcpy(rk, rmod, 32);
    for (size_t q = 1; q < k; q++) { uint64_t t[4]; h_mulmod(fr, t, rk, rmod); memcpy(rk, t, 32); }
    h_words(rk, 4, P.rk.w);
  }
  if (header_len) MZK_HIP(hipMemcpyAsync(P.base + L.off[mzk_tx::SCP_TRANSCRIPT] + 8, header, header_len, hipMemcpyHostToDevice, s));
  u32* partials = (u32*)(blk + o_part);
  u64* state = (u64*)(blk + o_state);
  const u64* chal = (const u64*)(P.base + L.off[mzk_tx::SCP_CHALLENGES]);
  const ScRoundFn round = sc_round_kernel((int)k);
  const size_t acc_bytes = (d + 1) * SP::L * SC_THREADS * sizeof(u32);
  const u32* cur = d_tab;            // round j-1's tables, stride n >> (j-1) (round 0: the input)
  size_t cur_stride = n;
  for (int j = 0; j < j0; j++) {
    const size_t h = n >> (j + 1);
    const size_t need = (h + SC_THREADS - 1) / SC_THREADS;
    const int nwg = (int)(need < (size_t)SC_MAX_WG ? need : SC_MAX_WG);
    u32* dst = j == 0 ? nullptr : (u32*)(blk + ((j & 1) ? o_a : o_b));
    prof_begin(s, j == 0 ? MZK_PH_SCP_ROUND0 : MZK_PH_SCP_ROUND);
    hipLaunchKernelGGL(round, dim3(nwg), dim3(SC_THREADS), acc_bytes, s, cur, cur_stride, h, j == 0 ? (const u64*)nullptr : chal + 4 * (size_t)(j - 1), dst, partials, (int)d);
    prof_end(s, j == 0 ? MZK_PH_SCP_ROUND0 : MZK_PH_SCP_ROUND);
    ProfScope pe(s, MZK_PH_SCP_ROUND_END);
    hipLaunchKernelGGL(k_sc_round_end, dim3(1), dim3(SC_END_THREADS), 0, s, (const u32*)partials, nwg, j, P, state);
    if (j > 0) { cur = dst; cur_stride = 2 * h; }
  }
  prof_begin(s, MZK_PH_SCP_TAIL);
  hipLaunchKernelGGL(k_sc_tail, dim3(1), dim3(64), 0, s, cur, cur_stride, j0 > 0 ? 1 : 0, (int)(n >> j0), j0, (int)k, P, (const u64*)state);
  prof_end(s, MZK_PH_SCP_TAIL);
  MZK_HIP(hipGetLastError());
  if (on_device) return MZK_OK;
  MZK_TRY(d2h_sync(proof_out, P.base, L.total, s));
  uint64_t status;
  memcpy(&status, (const uint8_t*)proof_out + L.off[mzk_tx::SCP_STATUS], 8);
  if (status != 0) { set_error("sumcheck_product_prove: status word %llu", (unsigned long long)status); return MZK_E_RANGE; }
  return MZK_OK;
}

// ---- dense multilinear coefficients -> evaluation table ---------------------------------------------------------------------
// evals[b] = sum over t subset of b of coef[t]: for every index bit, x[i | bit] += x[i].  One pass handles the g bits
// [lo, lo + g) of a tile of 2^(g + cb) elements in LDS: 2^g rows 2^lo apart, 2^cb consecutive elements (cb = min(lo, 2): 128-byte
// runs) per row.  The first pass takes bits [0, MLE_TILE_LOG) of consecutive tiles; every tile is read and written by one workgroup,
// so a pass may run in place.
constexpr int MLE_TILE_LOG = 10;
constexpr int MLE_THREADS = 256;
// x <- x + y mod p on canonical 32-bit words, BOTH operands below p: one carry chain, one borrow chain, one select -- the words that
// fe_pack(fe_reduce(fe_add(fe_unpack(x), fe_unpack(y)))) leaves, at a tenth of its instructions.  An operand of p or more is outside
// its contract (the limb form reduces any value), so only code whose operands are canonical by construction may use it.
__device__ __forceinline__ void mle_addmod_words(u32* x, const u32* y) {
  u32 s[8], t[8];
  u64 c = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) { c += (u64)x[i] + y[i]; s[i] = (u32)c; c >>= 32; }          // x + y < 2 p < 2^255: nothing is carried out
  int64_t b = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) { b += (int64_t)s[i] - (int64_t)SP::PW[i]; t[i] = (u32)b; b >>= 32; }
  const bool below = b < 0;                                                                  // the borrow out: x + y < p
#pragma unroll
  for (int i = 0; i < 8; i++) x[i] = below ? s[i] : t[i];
}
// The g subset-sum stages over the element-index bits [cb, cb + g) of a tile of `elems` canonical values in LDS; every stage starts
// with a barrier, none follows the last.  Shared by k_mle_pass (WORDS = false: the limb form it always had, which also reduces a caller's
// value that is not canonical) and k_hyper_tile (WORDS = true: its tile holds sums of host-checked coefficients only).
template <bool WORDS> __device__ __forceinline__ void mle_tile_stages(u32 (*X)[8], int tid, int elems, int cb, int g) {
  for (int st = 0; st < g; st++) {
    __syncthreads();
    const int bit = 1 << (cb + st);
    for (int q = tid; q < elems / 2; q += MLE_THREADS) {
      const int e0 = ((q & ~(bit - 1)) << 1) | (q & (bit - 1)), e1 = e0 | bit;
      if constexpr (WORDS) {
        mle_addmod_words(X[e1], X[e0]);
      } else {
        const SE v = fe_reduce<SP>(fe_add<SP>(fe_unpack<SP>(X[e0]), fe_unpack<SP>(X[e1])));
        fe_pack<SP>(v, X[e1]);
      }
    }
  }
}
// one 32-byte element as two 16-byte stores: four neighbouring lanes fill a 128-byte row
__device__ __forceinline__ void mle_store32(u32* out, size_t idx, const u32* x) {
  uint4* p = reinterpret_cast<uint4*>(out + 8 * idx);
  p[0] = make_uint4(x[0], x[1], x[2], x[3]);
  p[1] = make_uint4(x[4], x[5], x[6], x[7]);
}
__global__ __launch_bounds__(MLE_THREADS) void k_mle_pass(const u32* in, u32* out, int lo, int g, int cb) {
  __shared__ u32 X[1 << MLE_TILE_LOG][8];
  const int tid = threadIdx.x;
  const int elems = 1 << (g + cb);
  const size_t tile = blockIdx.x;
  const size_t t_low = tile & (((size_t)1 << (lo - cb)) - 1), t_high = tile >> (lo - cb);
  const size_t base = (t_high << (lo + g)) | (t_low << cb);
  for (int e = tid; e < elems; e += MLE_THREADS) {
    const size_t idx = base | ((size_t)(e >> cb) << lo) | (size_t)(e & ((1 << cb) - 1));
    gload_words<8>(in, idx, X[e]);
  }
  mle_tile_stages<false>(X, tid, elems, cb, g);
  __syncthreads();
  for (int e = tid; e < elems; e += MLE_THREADS) {
    const size_t idx = base | ((size_t)(e >> cb) << lo) | (size_t)(e & ((1 << cb) - 1));
    mle_store32(out, idx, X[e]);
  }
}

static int mle_check(size_t el) {
  if (el > (size_t)mzk_tx::SCP_MAX_VARS) { set_error("mle_evals_from_coeffs: %zu variables (at most %d)", el, mzk_tx::SCP_MAX_VARS); return MZK_E_LENGTH; }
  return MZK_OK;
}
static int mle_dev_impl(const void* d_coef, size_t el, void* d_evals, hipStream_t s) {
  const size_t n = (size_t)1 << el;
  if (el == 0) {
    if (d_coef != d_evals) MZK_HIP(hipMemcpyAsync(d_evals, d_coef, 32, hipMemcpyDeviceToDevice, s));
    return MZK_OK;
  }
  const u32* in = (const u32*)d_coef;
  for (int lo = 0; lo < (int)el;) {
    const int cb = lo < 2 ? lo : 2;
    const int g = (int)el - lo < MLE_TILE_LOG - cb ? (int)el - lo : MLE_TILE_LOG - cb;
    hipLaunchKernelGGL(k_mle_pass, dim3((unsigned)(n >> (g + cb))), dim3(MLE_THREADS), 0, s, in, (u32*)d_evals, lo, g, cb);
    in = (const u32*)d_evals;
    lo += g;
  }
  MZK_HIP(hipGetLastError());
  return MZK_OK;
}

// ---- sparse MPolynomial factors -> evaluation tables (eval_all_binary_combinations of the reference's prover) ------------------
// The host plan (mzk_hypercube_plan.h) leaves, per factor, the distinct support masks in ascending order with the coefficients of
// equal masks already added (on the host), and the groups of masks with one high part mask >> g.  evals[b] = sum of the
// coefficients whose mask is a subset of b.
//
// k_hyper_tile: workgroup (x, f) owns the 2^g consecutive entries of factor f whose high index bits are x.  A mask contributes to the
// tile iff its high part is a subset of x -- one test per GROUP, the same for every lane (group heads and ranges are read at uniform
// addresses) -- and then lands on slot (mask & (2^g - 1)) of the tile.  Low masks within a group are distinct, so the lanes of one
// group write different slots; a barrier orders the groups.  The g subset-sum stages in LDS then finish the tile, which is written
// once.  Nothing of size 2^el is read.
__global__ __launch_bounds__(HC_THREADS) void k_hyper_tile(const u32* __restrict__ grp_off, const u32* __restrict__ grp_hi, const u32* __restrict__ grp_begin,
                                                           const u32* __restrict__ mask, const u32* __restrict__ coef, int g, size_t n,
                                                           u32* __restrict__ tables) {
  __shared__ u32 X[1 << MLE_TILE_LOG][8];
  static_assert(HC_TILE_LOG == MLE_TILE_LOG && HC_THREADS == MLE_THREADS, "the tile of k_hyper_tile is the tile of k_mle_pass");
  const int tid = threadIdx.x;
  const int elems = 1 << g;
  const u32 hi = blockIdx.x, f = blockIdx.y;
  for (int e = tid; e < elems; e += HC_THREADS) {
    uint4* x = reinterpret_cast<uint4*>(X[e]);
    x[0] = make_uint4(0, 0, 0, 0);
    x[1] = make_uint4(0, 0, 0, 0);
  }
  __syncthreads();
  const u32 j1 = grp_off[f + 1];
  for (u32 j = grp_off[f]; j < j1; j++) {
    if (grp_hi[j] & ~hi) continue;
    const u32 q1 = grp_begin[j + 1];
    for (u32 q = grp_begin[j] + tid; q < q1; q += HC_THREADS) {
      u32 w[8];
      gload_words<8>(coef, q, w);
      mle_addmod_words(X[mask[q] & (u32)(elems - 1)], w);
    }
    __syncthreads();
  }
  mle_tile_stages<true>(X, tid, elems, 0, g);
  __syncthreads();
  u32* out = tables + 8 * ((size_t)f * n + ((size_t)hi << g));
  // the loop vectoriser would turn this into word-by-word stores 32 bytes apart per lane: keep one element, two 16-byte stores, per trip
#pragma clang loop vectorize(disable) interleave(disable)
  for (int e = tid; e < elems; e += HC_THREADS) mle_store32(out, e, X[e]);
}
// k_hyper_scatter: entry q of factor f -> table_f[mask[q]] of the zero-filled tables; masks within a factor are distinct and below n
__global__ __launch_bounds__(HC_THREADS) void k_hyper_scatter(const u32* __restrict__ ent_off, const u32* __restrict__ mask, const u32* __restrict__ coef, size_t n,
                                                              u32* __restrict__ tables) {
  const u32 f = blockIdx.y;
  const u32 q = ent_off[f] + blockIdx.x * HC_THREADS + threadIdx.x;
  if (q >= ent_off[f + 1]) return;
  u32 w[8];
  gload_words<8>(coef, q, w);
  mle_store32(tables, (size_t)f * n + mask[q], w);
}

// the plan and the words that go to the device: head (hc_plan's order) | merged coefficients
struct HcStaged { HcPlan pl; std::vector<u32> blob; };
// every refusal of mzk_mpoly_hypercube_evals* that needs no device, then the host merge
static int hc_prepare(const uint64_t* term_coefs, const uint32_t* term_exps, const size_t* term_offsets, size_t k, size_t el, int form, HcStaged* st) {
  HcPlan& pl = st->pl;
  const int rc = hc_plan(term_exps, term_offsets, k, el, form, &pl);
  if (rc != MZK_OK) { set_error("%s", pl.msg); return rc; }
  if (pl.terms && !term_coefs) { set_error("mpoly_hypercube: null pointer"); return MZK_E_ARG; }
  const HostField* fr = host_field(MZK_FIELD_FR);
  const size_t t0 = k ? term_offsets[0] : 0;
  for (size_t t = 0; t < pl.terms; t++)
    if (!h_is_canonical(fr, term_coefs + 4 * (t0 + t))) { set_error("mpoly_hypercube: term_coefs[%zu] not canonical", t0 + t); return MZK_E_RANGE; }
  if (k == 0) return MZK_OK;
  st->blob.assign(pl.upload_bytes / 4, 0);
  u32* w = st->blob.data();
  if (pl.form == MZK_HYPER_TILE) {
    w = std::copy(pl.grp_off.begin(), pl.grp_off.end(), w);
    w = std::copy(pl.grp_hi.begin(), pl.grp_hi.end(), w);
    w = std::copy(pl.grp_begin.begin(), pl.grp_begin.end(), w);
  } else {
    w = std::copy(pl.ent_off.begin(), pl.ent_off.end(), w);
  }
  std::copy(pl.mask.begin(), pl.mask.end(), w);
  hc_merge_coefs(pl, term_coefs, t0, st->blob.data() + pl.upload_words_head);
  return MZK_OK;
}
// Uploads the staged words and enqueues the form.  The words are host memory of the caller's frame: the stream is waited for right
// behind the copy (it has only earlier work and the copy on it), so the kernels below are enqueued and not waited for.
static int hc_enqueue(const HcStaged& st, WsFrame& ws, void* d_tables, hipStream_t s) {
  const HcPlan& pl = st.pl;
  if (pl.k == 0) return MZK_OK;
  const size_t n = (size_t)1 << pl.el, E = pl.mask.size(), G = pl.grp_hi.size(), k = pl.k;
  u32* d_blob;
  MZK_TRY(ws.get(WS_MISC_C, pl.workspace_bytes, (void**)&d_blob));
  MZK_HIP(hipMemcpyAsync(d_blob, st.blob.data(), pl.upload_bytes, hipMemcpyHostToDevice, s));
  MZK_HIP(hipStreamSynchronize(s));
  const u32* d_coef = d_blob + pl.upload_words_head;
  ProfScope ph(s, MZK_PH_HYPERCUBE);
  if (pl.form == MZK_HYPER_TILE) {
    const u32 *d_goff = d_blob, *d_ghi = d_goff + (k + 1), *d_gbeg = d_ghi + G, *d_mask = d_gbeg + (G + 1);
    hipLaunchKernelGGL(k_hyper_tile, dim3((unsigned)pl.grid_x, (unsigned)pl.grid_y), dim3(HC_THREADS), 0, s, d_goff, d_ghi, d_gbeg, d_mask, d_coef, pl.g, n,
                       (u32*)d_tables);
    MZK_HIP(hipGetLastError());
    return MZK_OK;
  }
  MZK_HIP(hipMemsetAsync(d_tables, 0, pl.table_bytes, s));
  if (E == 0) return MZK_OK;
  const u32 *d_eoff = d_blob, *d_mask = d_eoff + (k + 1);
  hipLaunchKernelGGL(k_hyper_scatter, dim3((unsigned)pl.grid_x, (unsigned)pl.grid_y), dim3(HC_THREADS), 0, s, d_eoff, d_mask, d_coef, n, (u32*)d_tables);
  MZK_HIP(hipGetLastError());
  for (size_t f = 0; f < k; f++) {
    void* t = (char*)d_tables + f * n * 32;
    MZK_TRY(mle_dev_impl(t, pl.el, t, s));
  }
  return MZK_OK;
}

static int hc_prove_terms_impl(const uint64_t* term_coefs, const uint32_t* term_exps, const size_t* term_offsets, size_t k, size_t el, size_t d,
                               const uint8_t* header, size_t header_len, size_t header_objects, void* proof_out, size_t proof_cap, bool on_device,
                               hipStream_t s_in) {
  mzk_tx::ScpLayout L;
  // the prover's refusals first (the tables are this call's own: any aligned non-null value stands in for them)
  MZK_TRY(scp_args_check((const void*)(uintptr_t)16, on_device, el, k, d, header, header_len, header_objects, proof_out, proof_cap, &L));
  HcStaged st;
  MZK_TRY(hc_prepare(term_coefs, term_exps, term_offsets, k, el, MZK_HYPER_AUTO, &st));
  MZK_ENTER();
  WsFrame ws("mzk_sumcheck_product_prove_terms");
  hipStream_t s = on_device ? s_in : ctx().stream;
  WsGuard wsg(s);
  void *d_tab, *d_proof = proof_out;
  MZK_TRY(ws.get(WS_MISC_E, st.pl.table_bytes, &d_tab));
  if (!on_device) MZK_TRY(ws.get(WS_MISC_D, L.total, &d_proof));
  MZK_TRY(hc_enqueue(st, ws, d_tab, s));
  MZK_TRY(scp_prove_impl(d_tab, true, el, k, d, header, header_len, header_objects, d_proof, L.total, s));
  if (on_device) return MZK_OK;
  MZK_TRY(d2h_sync(proof_out, d_proof, L.total, s));
  uint64_t status;
  memcpy(&status, (const uint8_t*)proof_out + L.off[mzk_tx::SCP_STATUS], 8);
  if (status != 0) { set_error("sumcheck_product_prove_terms: status word %llu", (unsigned long long)status); return MZK_E_RANGE; }
  return MZK_OK;
}

}  // namespace mzk

extern "C" {

int mzk_sumcheck_product_layout(size_t num_vars, size_t num_factors, size_t max_degree, size_t header_len, uint64_t* offsets, uint64_t* sizes,
                                uint64_t* total_bytes) {
  mzk_tx::ScpLayout L;
  MZK_TRY(mzk::scp_check(num_vars, num_factors, max_degree, header_len, &L));
  for (int q = 0; q < mzk_tx::SCP_COUNT; q++) {
    if (offsets) offsets[q] = L.off[q];
    if (sizes) sizes[q] = L.size[q];
  }
  if (total_bytes) *total_bytes = L.total;
  return MZK_OK;
}
int mzk_sumcheck_product_prove(const uint64_t* tables, size_t num_vars, size_t num_factors, size_t max_degree, const uint8_t* header, size_t header_len,
                               size_t header_objects, uint8_t* proof_out, size_t proof_cap) {
  return mzk::scp_prove_impl(tables, false, num_vars, num_factors, max_degree, header, header_len, header_objects, proof_out, proof_cap, nullptr);
}
int mzk_sumcheck_product_prove_dev(const void* d_tables, size_t num_vars, size_t num_factors, size_t max_degree, const uint8_t* header, size_t header_len,
                                   size_t header_objects, void* d_proof, size_t proof_cap, void* stream) {
  return mzk::scp_prove_impl(d_tables, true, num_vars, num_factors, max_degree, header, header_len, header_objects, d_proof, proof_cap,
                             (hipStream_t)stream);
}
int mzk_mle_evals_from_coeffs(const uint64_t* coef, size_t num_vars, uint64_t* evals) {
  using namespace mzk;
  if (!coef || !evals) { set_error("mle_evals_from_coeffs: null pointer"); return MZK_E_ARG; }
  MZK_TRY(mle_check(num_vars));
  const size_t n = (size_t)1 << num_vars;
  const HostField* fr = host_field(MZK_FIELD_FR);
  for (size_t i = 0; i < n; i++)
    if (!h_is_canonical(fr, coef + 4 * i)) { set_error("mle_evals_from_coeffs: coefficient %zu not canonical", i); return MZK_E_RANGE; }
  MZK_ENTER();
  WsFrame ws("mzk_mle_evals_from_coeffs");
  hipStream_t s = ctx().stream;
  WsGuard wsg(s);
  void* buf;
  MZK_TRY(ws.get(WS_MISC_F, n * 32, &buf));
  MZK_HIP(hipMemcpyAsync(buf, coef, n * 32, hipMemcpyHostToDevice, s));
  MZK_TRY(mle_dev_impl(buf, num_vars, buf, s));
  return d2h_sync(evals, buf, n * 32, s);
}
int mzk_mle_evals_from_coeffs_dev(const void* d_coef, size_t num_vars, void* d_evals, void* stream) {
  using namespace mzk;
  if (!d_coef || !d_evals) { set_error("mle_evals_from_coeffs: null pointer"); return MZK_E_ARG; }
  MZK_TRY(mle_check(num_vars));
  if (((uintptr_t)d_coef & 15) || ((uintptr_t)d_evals & 15)) { set_error("mle_evals_from_coeffs: buffers need 16-byte alignment"); return MZK_E_ARG; }
  MZK_ENTER();
  return mle_dev_impl(d_coef, num_vars, d_evals, (hipStream_t)stream);
}

int mzk_mpoly_hypercube_plan(const uint32_t* term_exps, const size_t* term_offsets, size_t n_factors, size_t num_vars, int form, mzk_hypercube_plan* out) {
  using namespace mzk;
  if (!out) { set_error("mpoly_hypercube_plan: null pointer"); return MZK_E_ARG; }
  HcPlan pl;
  const int rc = hc_plan(term_exps, term_offsets, n_factors, num_vars, form, &pl);
  if (rc != MZK_OK) { set_error("%s", pl.msg); return rc; }
  memset(out, 0, sizeof *out);
  out->form = (uint64_t)pl.form; out->tile_log = (uint64_t)pl.g; out->terms = pl.terms; out->masks = pl.mask.size(); out->groups = pl.grp_hi.size();
  out->max_masks = pl.max_masks; out->max_groups = pl.max_groups;
  out->launches = pl.launches; out->memsets = pl.memsets; out->grid_x = pl.grid_x; out->grid_y = pl.grid_y; out->mle_passes = pl.mle_passes;
  out->upload_bytes = pl.upload_bytes; out->workspace_bytes = pl.workspace_bytes; out->table_bytes = pl.table_bytes;
  for (size_t f = 0; f < n_factors && f < (size_t)MZK_HYPER_PLAN_FACTORS; f++) {
    out->factor_masks[f] = pl.ent_off[f + 1] - pl.ent_off[f];
    out->factor_groups[f] = pl.grp_off[f + 1] - pl.grp_off[f];
  }
  return MZK_OK;
}
int mzk_mpoly_hypercube_evals(const uint64_t* term_coefs, const uint32_t* term_exps, const size_t* term_offsets, size_t n_factors, size_t num_vars, int form,
                              uint64_t* tables) {
  using namespace mzk;
  if (n_factors && !tables) { set_error("mpoly_hypercube_evals: null pointer"); return MZK_E_ARG; }
  HcStaged st;
  MZK_TRY(hc_prepare(term_coefs, term_exps, term_offsets, n_factors, num_vars, form, &st));
  if (n_factors == 0) return MZK_OK;
  MZK_ENTER();
  WsFrame ws("mzk_mpoly_hypercube_evals");
  hipStream_t s = ctx().stream;
  WsGuard wsg(s);
  void* d_tab;
  MZK_TRY(ws.get(WS_MISC_E, st.pl.table_bytes, &d_tab));
  MZK_TRY(hc_enqueue(st, ws, d_tab, s));
  return d2h_sync(tables, d_tab, st.pl.table_bytes, s);
}
int mzk_mpoly_hypercube_evals_dev(const uint64_t* term_coefs, const uint32_t* term_exps, const size_t* term_offsets, size_t n_factors, size_t num_vars,
                                  int form, void* d_tables, void* stream) {
  using namespace mzk;
  if (n_factors && !d_tables) { set_error("mpoly_hypercube_evals: null pointer"); return MZK_E_ARG; }
  if ((uintptr_t)d_tables & 15) { set_error("mpoly_hypercube_evals: the tables need 16-byte alignment"); return MZK_E_ARG; }
  HcStaged st;
  MZK_TRY(hc_prepare(term_coefs, term_exps, term_offsets, n_factors, num_vars, form, &st));
  if (n_factors == 0) return MZK_OK;
  MZK_ENTER();
  WsFrame ws("mzk_mpoly_hypercube_evals_dev");
  WsGuard wsg((hipStream_t)stream);
  return hc_enqueue(st, ws, d_tables, (hipStream_t)stream);
}
int mzk_sumcheck_product_prove_terms(const uint64_t* term_coefs, const uint32_t* term_exps, const size_t* term_offsets, size_t n_factors, size_t num_vars,
                                     size_t max_degree, const uint8_t* header, size_t header_len, size_t header_objects, uint8_t* proof_out,
                                     size_t proof_cap) {
  return mzk::hc_prove_terms_impl(term_coefs, term_exps, term_offsets, n_factors, num_vars, max_degree, header, header_len, header_objects, proof_out,
                                  proof_cap, false, nullptr);
}
int mzk_sumcheck_product_prove_terms_dev(const uint64_t* term_coefs, const uint32_t* term_exps, const size_t* term_offsets, size_t n_factors, size_t num_vars,
                                         size_t max_degree, const uint8_t* header, size_t header_len, size_t header_objects, void* d_proof,
                                         size_t proof_cap, void* stream) {
  return mzk::hc_prove_terms_impl(term_coefs, term_exps, term_offsets, n_factors, num_vars, max_degree, header, header_len, header_objects, d_proof, proof_cap,
                                  true, (hipStream_t)stream);
}

}  // extern "C"
