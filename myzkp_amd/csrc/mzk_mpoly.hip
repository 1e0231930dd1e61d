// mzk_mpoly.hip -- the polynomial algebra between the transforms of FastStark::prove (zkstark/fast_stark.rs:177-396) on gfx950:
//   * MPolynomial::evaluate_symbolic (algebra/mpolynomials.rs:125-141; fast_stark.rs:246-259, stark.rs:214): univariate polynomials
//     substituted for the variables of sparse multivariate constraints, several constraints over one point in one call;
//   * the weighted, shifted combination of the quotients (fast_stark.rs:301-326).
//
// evaluate_symbolic is a polynomial identity, out_a = sum_t c_t prod_i point[i]^k[t][i], and field arithmetic is exact: computed in
// EVALUATION form over a subgroup of N > deg(out_a) points it gives the canonical coefficients the reference's term-by-term schoolbook
// products give.  A call is
//   k_mp_pad      the n_vars point polynomials, zero-padded to N, as rows of one matrix;
//   ONE batched forward transform of n_vars rows (mzk_ntt.hip);
//   k_mp_terms    V[a][j] = sum_t c_t prod_i E[i][j]^k[t][i] for every domain point j and constraint a (below);
//   ONE batched inverse transform of n_constraints rows;
//   k_mp_rows     rows copied to the caller's stride (zeros behind them) and every row's trimmed length (polynomial.rs:214-228 trims
//                 after every + and *), so that only the lengths travel to the host.
//
// k_mp_terms runs a TERM PROGRAM the host compiles per constraint (mp_compile, mzk_mpoly_plan.h).  The terms are sorted so that those sharing the monomial of
// every variable but one (the Horner variable h: the one with the largest exponent in the constraint) form a run -- the shape
// MPolynomial::lift produces (rescueprime.rs:454-484: a univariate in the cycle variable times a monomial of the state variables) -- and a
// run sum_j c_j x_h^(d_j) m, d_0 > d_1 > ..., is evaluated as (((c_0 x_h^(d_0-d_1) + c_1) x_h^(d_1-d_2) + ...) x_h^(d_k)) m: about one
// product per term.  Exponents of at most MP_TABLE come from per-variable power tables, 4 .. 2 MP_TABLE from two table products, larger
// ones from square-and-multiply (uniform over the wave: the exponent is part of the program).
//
// Launch shape: one wave per workgroup, one domain point per lane, grid = (N / 64, n_constraints).  The program and the coefficients are
// the same for every lane and are read with wave-uniform loads; a lane's state is the Horner accumulator, the constraint's sum and the
// operand of the running product.  The power tables x_i, x_i^2, x_i^3 (Montgomery form) live in LDS as [slot][limb][lane] -- the slot is a
// run-time value of the program, and a register array indexed by it would go to scratch memory; lane-minor order makes every read
// conflict-free.  Variables that never need a power above 1 or 2 get fewer slots (mp_compile: depth), unused ones none.
// Values: E and the coefficients are plain (canonical), the tables are Montgomery form, and plain * Montgomery / R = plain: the
// accumulator never changes form and the sum is reduced and stored as it stands.
#include <algorithm>
#include <vector>
#include "mzk_common.h"
#include "mzk_elem.h"
#include "mzk_field_asm.h"
#include "mzk_mpoly_plan.h"

namespace mzk {

struct MpRows { size_t off[MP_MAX_VARS + 1]; };

// the same element for every lane: word loads at a wave-uniform address
template <class P> __device__ __forceinline__ Fe<P> mp_uload(const u32* __restrict__ g, u32 idx) {
  u32 w[P::NW];
#pragma unroll
  for (int k = 0; k < P::NW; k++) w[k] = g[(size_t)idx * P::NW + k];
  return fe_unpack<P>(w);
}
template <class P> __device__ __forceinline__ Fe<P> mp_lds_load(const u32* lds, u32 slot, int lane) {
  Fe<P> r;
#pragma unroll
  for (int i = 0; i < P::L; i++) r.l[i] = lds[(slot * P::L + i) * MP_LANES + lane];
  return r;
}
template <class P> __device__ __forceinline__ void mp_lds_store(u32* lds, u32 slot, int lane, const Fe<P>& v) {
#pragma unroll
  for (int i = 0; i < P::L; i++) lds[(slot * P::L + i) * MP_LANES + lane] = v.l[i];
}

// row i of dst (n elements) = point i, zero-padded
template <class P>
__global__ __launch_bounds__(256) void k_mp_pad(const u32* __restrict__ point, MpRows R, size_t n, u32* __restrict__ dst) {
  const size_t j = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  const int i = blockIdx.y;
  const size_t len = R.off[i + 1] - R.off[i];
  uint4* o = reinterpret_cast<uint4*>(dst + ((size_t)i * n + j) * P::NW);
  const uint4* s = reinterpret_cast<const uint4*>(point + (R.off[i] + j) * P::NW);
#pragma unroll
  for (int q = 0; q < P::NW / 4; q++) o[q] = j < len ? s[q] : make_uint4(0, 0, 0, 0);
}

// E: n_vars rows of n evaluations (canonical).  prog_off[a] .. prog_off[a + 1]: the ops of constraint a = blockIdx.y.  V: row a.
template <class P>
__global__ __launch_bounds__(MP_LANES) void k_mp_terms(const u32* __restrict__ E, size_t n, int n_vars, MpVars vars, const MpOp* __restrict__ prog,
                                                       const u32* __restrict__ prog_off, const u32* __restrict__ coefs, u32* __restrict__ V) {
  static_assert(P::L <= MP_MAX_LIMBS, "the LDS bound of mzk_mpoly_plan.h is stated for at most MP_MAX_LIMBS limbs");
  extern __shared__ u32 mp_lds[];
  const int lane = threadIdx.x;
  const size_t j = (size_t)blockIdx.x * MP_LANES + lane;
  const size_t jj = j < n ? j : n - 1;             // lanes past the end compute point n - 1 again and store nothing
  for (int i = 0; i < n_vars; i++) {
    const u32 depth = vars.depth[i], s0 = vars.first_slot[i];
    if (depth == 0) continue;
    const Fe<P> x = FeAsm<P>::mul(fe_gload<P>(E, (size_t)i * n + jj), fe_r2<P>());
    mp_lds_store<P>(mp_lds, s0, lane, x);
    if (depth > 1) {
      const Fe<P> x2 = FeAsm<P>::sqr(x);
      mp_lds_store<P>(mp_lds, s0 + 1, lane, x2);
      if (depth > 2) mp_lds_store<P>(mp_lds, s0 + 2, lane, FeAsm<P>::mul(x2, x));
    }
  }
  // a lane reads back only what it wrote itself: no barrier
  const int a = blockIdx.y;
  const u32 pc0 = prog_off[a], pc1 = prog_off[a + 1];
  Fe<P> acc = fe_zero<P>(), sum = fe_zero<P>();
  for (u32 pc = pc0; pc < pc1; pc++) {
    const u32 w = __builtin_amdgcn_readfirstlane(prog[pc].op), arg = __builtin_amdgcn_readfirstlane(prog[pc].arg);
    const u32 op = w & 0xffu, slot = (w >> 8) & 0xffffu;
    if (op == MP_LOADC) {
      acc = mp_uload<P>(coefs, arg);
    } else if (op == MP_ADDC) {
      acc = fe_reduce<P>(fe_add<P>(acc, mp_uload<P>(coefs, arg)));
    } else if (op == MP_POW) {
      // acc *= x^arg, arg > 2 MP_TABLE: square-and-multiply from the top bit down
      const Fe<P> x = mp_lds_load<P>(mp_lds, slot, lane);
      Fe<P> y = x;
      for (int bit = 30 - __builtin_clz(arg); bit >= 0; bit--) {
        y = FeAsm<P>::sqr(y);
        if ((arg >> bit) & 1u) y = FeAsm<P>::mul(y, x);
      }
      acc = FeAsm<P>::mul(acc, y);
    } else {
      // MULT / HORNER: acc < 3p with limbs below 2^30 times a normalised table entry; the sum of a product (< p + 1) and a canonical
      // coefficient needs no reduction before the next product
      acc = FeAsm<P>::mul(acc, mp_lds_load<P>(mp_lds, slot, lane));
      if (op == MP_HORNER) acc = fe_add<P>(acc, mp_uload<P>(coefs, arg));
    }
    if (w & MP_FLUSH) sum = fe_reduce<P>(fe_add<P>(sum, acc));
  }
  if (j < n) fe_gstore<P>(V, (size_t)a * n + j, sum);
}

// out row a (stride elements) = the first min(n, stride) elements of V's row a, zeros behind them; lens[a] = max(lens[a], 1 + index of the
// last non-zero element) -- lens zeroed before the launch
template <class P>
__global__ __launch_bounds__(256) void k_mp_rows(const u32* __restrict__ V, size_t n, u32* __restrict__ out, size_t stride, unsigned long long* __restrict__ lens) {
  __shared__ unsigned long long sh[256];
  const size_t j = (size_t)blockIdx.x * 256 + threadIdx.x;
  const int a = blockIdx.y;
  unsigned long long best = 0;
  if (j < stride) {
    uint4 v[P::NW / 4];
    u32 nz = 0;
#pragma unroll
    for (int q = 0; q < P::NW / 4; q++) {
      v[q] = j < n ? reinterpret_cast<const uint4*>(V + ((size_t)a * n + j) * P::NW)[q] : make_uint4(0, 0, 0, 0);
      nz |= v[q].x | v[q].y | v[q].z | v[q].w;
      reinterpret_cast<uint4*>(out + ((size_t)a * stride + j) * P::NW)[q] = v[q];
    }
    if (nz) best = j + 1;
  }
  sh[threadIdx.x] = best;
  __syncthreads();
  for (int off = 128; off >= 1; off >>= 1) {
    if ((int)threadIdx.x < off && sh[threadIdx.x + off] > sh[threadIdx.x]) sh[threadIdx.x] = sh[threadIdx.x + off];
    __syncthreads();
  }
  if (threadIdx.x == 0 && sh[0]) atomicMax(&lens[a], sh[0]);
}

// ---- the weighted combination (fast_stark.rs:301-326) ------------------------------------------------------------------------------
// out[j] = sum_i w_i p_i[j - s_i]: one output coefficient per lane, the table (offset, length, shift, weight in Montgomery form) wave-uniform
struct MpLcItem { unsigned long long off, len, shift; u32 w[8]; u32 pad[2]; };
template <class P>
__global__ __launch_bounds__(256) void k_mp_lincomb(const u32* __restrict__ polys, const MpLcItem* __restrict__ items, u32 count, u32* __restrict__ out,
                                                    size_t cap, unsigned long long* __restrict__ len) {
  __shared__ unsigned long long sh[256];
  const size_t j = (size_t)blockIdx.x * 256 + threadIdx.x;
  Fe<P> acc = fe_zero<P>();
  for (u32 i = 0; i < count; i++) {
    const unsigned long long off = items[i].off, ln = items[i].len, sft = items[i].shift;
    if (j < sft || j - sft >= ln || j >= cap) continue;
    u32 w[P::NW];
#pragma unroll
    for (int k = 0; k < P::NW; k++) w[k] = items[i].w[k];
    acc = fe_reduce<P>(fe_add<P>(acc, FeAsm<P>::mul(fe_gload<P>(polys, off + (j - sft)), fe_unpack<P>(w))));
  }
  unsigned long long best = 0;
  if (j < cap) {
    fe_gstore<P>(out, j, acc);
    if (!fe_is_zero_canon<P>(acc)) best = j + 1;
  }
  sh[threadIdx.x] = best;
  __syncthreads();
  for (int off = 128; off >= 1; off >>= 1) {
    if ((int)threadIdx.x < off && sh[threadIdx.x + off] > sh[threadIdx.x]) sh[threadIdx.x] = sh[threadIdx.x + off];
    __syncthreads();
  }
  if (threadIdx.x == 0 && sh[0]) atomicMax(len, sh[0]);
}

// ---- host plan and term programs: mzk_mpoly_plan.h (mp_plan, mp_compile) -------------------------------------------------------------
static int mp_plan_of(int fid, const uint32_t* term_exps, const size_t* term_offsets, size_t nc, size_t nv, const size_t* point_offsets, MpPlan* pl) {
  MZK_TRY(field_check(fid, "mpoly_compose"));
  const int rc = mp_plan(field_max_log(fid), term_exps, term_offsets, nc, nv, point_offsets, pl);
  if (rc != MZK_OK) set_error("%s", pl->msg);
  return rc;
}

static inline unsigned mp_grid(size_t n, unsigned per) { return (unsigned)((n + per - 1) / per); }

template <class P>
static int mp_compose_dev(int fid, const uint64_t* term_coefs, const uint32_t* term_exps, const size_t* term_offsets, size_t nc, size_t nv,
                          const void* d_point, const size_t* point_offsets, void* d_out, size_t out_stride, size_t* out_lens, hipStream_t s) {
  WsFrame ws("mp_compose_dev");
  MpPlan pl;
  MZK_TRY(mp_plan_of(fid, term_exps, term_offsets, nc, nv, point_offsets, &pl));
  if (nc == 0) return MZK_OK;
  if (!out_lens || (out_stride && !d_out)) { set_error("mpoly_compose: null pointer"); return MZK_E_ARG; }
  const size_t t0 = term_offsets[0], nt = term_offsets[nc] - t0;
  if (nt && !term_coefs) { set_error("mpoly_compose: null pointer"); return MZK_E_ARG; }
  if (nv && point_offsets[nv] > point_offsets[0] && !d_point) { set_error("mpoly_compose: null pointer"); return MZK_E_ARG; }
  if (nt >= ((size_t)1 << 28)) { set_error("mpoly_compose: %zu terms (at most 2^28 - 1)", nt); return MZK_E_LENGTH; }     // op counters are 32 bits
  const HostField* hf = host_field(fid);
  const int nl = hf->nl;
  for (size_t t = 0; t < nt; t++)
    if (!h_is_canonical(hf, term_coefs + (t0 + t) * nl)) { set_error("mpoly_compose: term_coefs[%zu] not canonical", t0 + t); return MZK_E_RANGE; }
  if (out_stride < pl.stride_min) { set_error("mpoly_compose: out_stride %zu is below the degree bound + 1 = %zu", out_stride, pl.stride_min); return MZK_E_LENGTH; }
  if (out_stride == 0) { for (size_t a = 0; a < nc; a++) out_lens[a] = 0; return MZK_OK; }      // every constraint is empty or vanishes
  MpProgram pg;
  mp_compile(term_exps, term_offsets, nc, nv, point_offsets, &pg);
  const size_t N = pl.n, esz = field_bytes(fid);
  uint64_t root[4] = {0, 0, 0, 0};
  unsigned lg = 0;
  while (((size_t)1 << lg) < N) lg++;
  MZK_TRY(mzk_root_of_unity(fid, lg, root));
  // one blob: ops | offsets | coefficients | lengths
  const size_t b_ops = (pg.ops.size() * sizeof(MpOp) + 15) & ~(size_t)15, b_off = (pg.off.size() * 4 + 15) & ~(size_t)15, b_coef = (nt * esz + 15) & ~(size_t)15;
  const size_t b_tab = b_ops + b_off + b_coef;
  char *d_tab, *d_E, *d_V;
  unsigned long long* d_lens;
  MZK_TRY(ws.get(WS_MISC_C, b_tab ? b_tab : 16, (void**)&d_tab));
  MZK_TRY(ws.get(WS_MISC_D, nc * 8, (void**)&d_lens));
  MZK_TRY(ws.get(WS_MISC_A, (nv ? nv : 1) * N * esz, (void**)&d_E));
  MZK_TRY(ws.get(WS_MISC_B, nc * N * esz, (void**)&d_V));
  std::vector<char> tab(b_tab);
  if (!pg.ops.empty()) memcpy(tab.data(), pg.ops.data(), pg.ops.size() * sizeof(MpOp));
  memcpy(tab.data() + b_ops, pg.off.data(), pg.off.size() * 4);
  if (nt) memcpy(tab.data() + b_ops + b_off, term_coefs + t0 * nl, nt * esz);
  auto fail = [&](int rc) { (void)hipStreamSynchronize(s); return rc; };       // nothing stays enqueued behind an error
  // the blob is host memory of this call: every path below waits for the stream before it returns
  MZK_HIP(hipMemcpyAsync(d_tab, tab.data(), b_tab, hipMemcpyHostToDevice, s));
  if (hipMemsetAsync(d_lens, 0, nc * 8, s) != hipSuccess) return fail(MZK_E_HIP);
  if (nv) {
    MpRows R;
    for (size_t i = 0; i <= (size_t)MP_MAX_VARS; i++) R.off[i] = point_offsets[i < nv ? i : nv] - point_offsets[0];
    const char* pt = (const char*)d_point + point_offsets[0] * esz;
    hipLaunchKernelGGL((k_mp_pad<P>), dim3(mp_grid(N, 256), (unsigned)nv), dim3(256), 0, s, (const u32*)pt, R, N, (u32*)d_E);
    int rc = ntt_batch_dev_impl(fid, root, d_E, d_E, N, nv, 0, s);
    if (rc != MZK_OK) return fail(rc);
  }
  hipLaunchKernelGGL((k_mp_terms<P>), dim3(mp_grid(N, MP_LANES), (unsigned)nc), dim3(MP_LANES), (size_t)pg.slots * P::L * MP_LANES * 4, s, (const u32*)d_E, N,
                     (int)nv, pg.vars, (const MpOp*)d_tab, (const u32*)(d_tab + b_ops), (const u32*)(d_tab + b_ops + b_off), (u32*)d_V);
  if (hipGetLastError() != hipSuccess) { set_error("mpoly_compose: launch failed"); return fail(MZK_E_HIP); }
  int rc = ntt_batch_dev_impl(fid, root, d_V, d_V, N, nc, 1, s);
  if (rc != MZK_OK) return fail(rc);
  hipLaunchKernelGGL((k_mp_rows<P>), dim3(mp_grid(out_stride, 256), (unsigned)nc), dim3(256), 0, s, (const u32*)d_V, N, (u32*)d_out, out_stride, d_lens);
  if (hipGetLastError() != hipSuccess) { set_error("mpoly_compose: launch failed"); return fail(MZK_E_HIP); }
  std::vector<unsigned long long> lens(nc);
  rc = d2h_sync(lens.data(), d_lens, nc * 8, s);
  if (rc != MZK_OK) return fail(rc);
  for (size_t a = 0; a < nc; a++) out_lens[a] = (size_t)lens[a];
  return MZK_OK;
}

static int mp_lincomb_check(int fid, const size_t* offsets, size_t count, const uint64_t* weights, const size_t* shifts, size_t out_cap, const void* out,
                            const size_t* out_len) {
  MZK_TRY(field_check(fid, "poly_lincomb"));
  if (!out_len || (out_cap && !out) || (count && (!offsets || !weights || !shifts))) { set_error("poly_lincomb: null pointer"); return MZK_E_ARG; }
  if (count >= ((size_t)1 << 31)) { set_error("poly_lincomb: %zu polynomials (at most 2^31 - 1)", count); return MZK_E_LENGTH; }
  const HostField* hf = host_field(fid);
  for (size_t i = 0; i < count; i++) {
    if (offsets[i + 1] < offsets[i]) { set_error("poly_lincomb: offsets[%zu] = %zu is below offsets[%zu] = %zu", i + 1, offsets[i + 1], i, offsets[i]); return MZK_E_LENGTH; }
    if (!h_is_canonical(hf, weights + i * hf->nl)) { set_error("poly_lincomb: weights[%zu] not canonical", i); return MZK_E_RANGE; }
    size_t end;
    if (__builtin_add_overflow(offsets[i + 1] - offsets[i], shifts[i], &end) || end > out_cap) {
      set_error("poly_lincomb: polynomial %zu (%zu coefficients, shift %zu) does not fit out_cap = %zu", i, offsets[i + 1] - offsets[i], shifts[i], out_cap);
      return MZK_E_LENGTH;
    }
  }
  return MZK_OK;
}
// validated arguments
template <class P>
static int mp_lincomb_dev(int fid, const void* d_polys, const size_t* offsets, size_t count, const uint64_t* weights, const size_t* shifts, void* d_out,
                          size_t out_cap, size_t* out_len, hipStream_t s) {
  WsFrame ws("mp_lincomb_dev");
  *out_len = 0;
  if (out_cap == 0) return MZK_OK;
  std::vector<MpLcItem> items(count);
  const HostField* hf = host_field(fid);
  for (size_t i = 0; i < count; i++) {
    items[i].off = offsets[i] - offsets[0]; items[i].len = offsets[i + 1] - offsets[i]; items[i].shift = shifts[i];
    h_mont_words(hf, weights + i * hf->nl, items[i].w);
    items[i].pad[0] = items[i].pad[1] = 0;
  }
  char* d_tab;
  MZK_TRY(ws.get(WS_MISC_C, (count ? count : 1) * sizeof(MpLcItem) + 16, (void**)&d_tab));
  unsigned long long* d_len = (unsigned long long*)d_tab;
  MpLcItem* d_items = (MpLcItem*)(d_tab + 16);
  auto fail = [&](int rc) { (void)hipStreamSynchronize(s); return rc; };
  MZK_HIP(hipMemsetAsync(d_len, 0, 16, s));
  if (count && hipMemcpyAsync(d_items, items.data(), count * sizeof(MpLcItem), hipMemcpyHostToDevice, s) != hipSuccess) return fail(MZK_E_HIP);
  const char* base = (const char*)d_polys + (count ? offsets[0] : 0) * field_bytes(fid);
  hipLaunchKernelGGL((k_mp_lincomb<P>), dim3(mp_grid(out_cap, 256)), dim3(256), 0, s, (const u32*)base, (const MpLcItem*)d_items, (u32)count, (u32*)d_out, out_cap,
                     d_len);
  if (hipGetLastError() != hipSuccess) { set_error("poly_lincomb: launch failed"); return fail(MZK_E_HIP); }
  unsigned long long len = 0;
  const int rc = d2h_sync(&len, d_len, 8, s);
  if (rc != MZK_OK) return fail(rc);
  *out_len = (size_t)len;
  return MZK_OK;
}

}  // namespace mzk

using namespace mzk;

extern "C" {

int mzk_mpoly_compose_plan(int field_id, const uint32_t* term_exps, const size_t* term_offsets, size_t n_constraints, size_t n_vars,
                           const size_t* point_offsets, size_t* n_transform, size_t* out_stride_min, size_t* bounds) {
  if (!n_transform || !out_stride_min) { set_error("mpoly_compose_plan: null pointer"); return MZK_E_ARG; }
  MpPlan pl;
  MZK_TRY(mp_plan_of(field_id, term_exps, term_offsets, n_constraints, n_vars, point_offsets, &pl));
  *n_transform = pl.n;
  *out_stride_min = pl.stride_min;
  if (bounds) for (size_t a = 0; a < n_constraints; a++) bounds[a] = pl.bounds[a];
  return MZK_OK;
}

int mzk_mpoly_compose_dev(int field_id, const uint64_t* term_coefs, const uint32_t* term_exps, const size_t* term_offsets, size_t n_constraints,
                          size_t n_vars, const void* d_point, const size_t* point_offsets, void* d_out, size_t out_stride, size_t* out_lens,
                          void* stream) {
  MZK_ENTER();
  MZK_TRY(field_check(field_id, "mpoly_compose"));
  WsGuard wsg((hipStream_t)stream);
  return with_field(field_id, [&](auto tag) {
    return mp_compose_dev<typename decltype(tag)::P>(field_id, term_coefs, term_exps, term_offsets, n_constraints, n_vars, d_point, point_offsets, d_out, out_stride, out_lens, (hipStream_t)stream);
  });
}

int mzk_mpoly_compose(int field_id, const uint64_t* term_coefs, const uint32_t* term_exps, const size_t* term_offsets, size_t n_constraints,
                      size_t n_vars, const uint64_t* point, const size_t* point_offsets, uint64_t* out, size_t out_stride, size_t* out_lens) {
  MZK_ENTER();
  WsFrame ws("mzk_mpoly_compose");
  MpPlan pl;
  MZK_TRY(mp_plan_of(field_id, term_exps, term_offsets, n_constraints, n_vars, point_offsets, &pl));
  if (n_constraints == 0) return MZK_OK;
  if (!out_lens || (out_stride && !out)) { set_error("mpoly_compose: null pointer"); return MZK_E_ARG; }
  const HostField* hf = host_field(field_id);
  const size_t esz = field_bytes(field_id), p0 = n_vars ? point_offsets[0] : 0, np = n_vars ? point_offsets[n_vars] - p0 : 0;
  if (np && !point) { set_error("mpoly_compose: null pointer"); return MZK_E_ARG; }
  for (size_t i = 0; i < np; i++)
    if (!h_is_canonical(hf, point + (p0 + i) * hf->nl)) { set_error("mpoly_compose: point[%zu] not canonical", p0 + i); return MZK_E_RANGE; }
  if (out_stride > ((size_t)1 << 40) / n_constraints) { set_error("mpoly_compose: out_stride too large"); return MZK_E_LENGTH; }
  hipStream_t s = ctx().stream;
  WsGuard wsg(s);
  char *d_p, *d_o;
  MZK_TRY(ws.get(WS_MISC_E, (np ? np : 1) * esz, (void**)&d_p));
  MZK_TRY(ws.get(WS_MISC_F, (n_constraints * out_stride + 1) * esz, (void**)&d_o));
  // offsets relative to the staged copy
  std::vector<size_t> rel(n_vars + 1, 0);
  for (size_t i = 0; i <= n_vars && n_vars; i++) rel[i] = point_offsets[i] - p0;
  if (np) MZK_HIP(hipMemcpyAsync(d_p, point + p0 * hf->nl, np * esz, hipMemcpyHostToDevice, s));
  const int rc = with_field(field_id, [&](auto tag) {
    return mp_compose_dev<typename decltype(tag)::P>(field_id, term_coefs, term_exps, term_offsets, n_constraints, n_vars, d_p, rel.data(), d_o, out_stride, out_lens, s);
  });
  if (rc != MZK_OK) { (void)hipStreamSynchronize(s); return rc; }
  if (out_stride == 0) return MZK_OK;
  return d2h_sync(out, d_o, n_constraints * out_stride * esz, s);
}

int mzk_poly_lincomb_dev(int field_id, const void* d_polys, const size_t* offsets, size_t count, const uint64_t* weights, const size_t* shifts,
                         void* d_out, size_t out_cap, size_t* out_len, void* stream) {
  MZK_ENTER();
  MZK_TRY(mp_lincomb_check(field_id, offsets, count, weights, shifts, out_cap, d_out, out_len));
  if (count && offsets[count] > offsets[0] && !d_polys) { set_error("poly_lincomb: null pointer"); return MZK_E_ARG; }
  WsGuard wsg((hipStream_t)stream);
  return with_field(field_id, [&](auto tag) { return mp_lincomb_dev<typename decltype(tag)::P>(field_id, d_polys, offsets, count, weights, shifts, d_out, out_cap, out_len, (hipStream_t)stream); });
}

int mzk_poly_lincomb(int field_id, const uint64_t* polys, const size_t* offsets, size_t count, const uint64_t* weights, const size_t* shifts,
                     uint64_t* out, size_t out_cap, size_t* out_len) {
  MZK_ENTER();
  WsFrame ws("mzk_poly_lincomb");
  MZK_TRY(mp_lincomb_check(field_id, offsets, count, weights, shifts, out_cap, out, out_len));
  const HostField* hf = host_field(field_id);
  const size_t esz = field_bytes(field_id), p0 = count ? offsets[0] : 0, np = count ? offsets[count] - p0 : 0;
  if (np && !polys) { set_error("poly_lincomb: null pointer"); return MZK_E_ARG; }
  for (size_t i = 0; i < np; i++)
    if (!h_is_canonical(hf, polys + (p0 + i) * hf->nl)) { set_error("poly_lincomb: polys[%zu] not canonical", p0 + i); return MZK_E_RANGE; }
  hipStream_t s = ctx().stream;
  WsGuard wsg(s);
  char *d_p, *d_o;
  MZK_TRY(ws.get(WS_MISC_E, (np ? np : 1) * esz, (void**)&d_p));
  MZK_TRY(ws.get(WS_MISC_F, (out_cap ? out_cap : 1) * esz, (void**)&d_o));
  std::vector<size_t> rel(count + 1, 0);
  for (size_t i = 0; i <= count; i++) rel[i] = count ? offsets[i] - p0 : 0;
  if (np) MZK_HIP(hipMemcpyAsync(d_p, polys + p0 * hf->nl, np * esz, hipMemcpyHostToDevice, s));
  const int rc = with_field(field_id, [&](auto tag) { return mp_lincomb_dev<typename decltype(tag)::P>(field_id, d_p, rel.data(), count, weights, shifts, d_o, out_cap, out_len, s); });
  if (rc != MZK_OK) { (void)hipStreamSynchronize(s); return rc; }
  if (out_cap == 0) return MZK_OK;
  return d2h_sync(out, d_o, out_cap * esz, s);
}

}  // extern "C"
