// mzk_gemini.hip -- the multilinear half of the prover path on gfx950: Gemini split-and-fold, commit and open
// (myzkp/src/modules/algebra/gemini.rs:51-144) and the sum-check prover (algebra/sumcheck.rs:57-166).
//
// All values are BN254 Fr in standard form.  A multilinear g with coefficient c[t] at index t (bit i of t = exponent of
// variable i, get_coefs_in_order, sumcheck.rs:97-108) folds as f_{i+1}[k] = f_i[2k] + rho_i f_i[2k+1]; level el is the
// constant mu.  rho is turned into Montgomery form (rho R) once on the host, so one Montgomery product c * (rho R) / R
// returns c rho in standard form.
//
// Kernels:
//   k_gm_fold        one memory-bound pass per large level;
//   k_gm_fold_lds    every level from FOLD_LDS_IN elements down, in LDS, in one launch;
//   k_gm_sums        weighted sums over a level (sum_over_boolean_hypercube, and the sum-check round messages A_j / B_j),
//                    optionally fused with the fold that produces the level (one pass over the data per round);
// Gemini's evaluations at beta, -beta, beta^2 and its quotients by (X - beta)(X + beta)(X - beta^2) of every level are three rounds
// of the library's synthetic division (synth_div_dev, mzk_kzg.hip).
// The MSMs run on the SRS handle's tables (mzk_msm.hip); the degree-bound MSMs of prove_degree_bound (kzg.rs:121-134) on the
// handle entered max_d - d rows further on (see gemini_open_impl).
#include "mzk_common.h"
#include "mzk_srs.h"
#include "mzk_elem.h"

namespace mzk {

typedef FrParams GP;
typedef Fe<GP> GE;

// canonical a + b * (r R) / R = a + b r
__device__ __forceinline__ GE gm_fold1(const GE& a, const GE& b, const GE& r_mont) {
  return fe_reduce<GP>(fe_add<GP>(a, fe_mul<GP>(b, r_mont)));
}

// ---- host parameter math ------------------------------------------------------------------------------------------
constexpr int GM_MAX_LOG = 30;
static int gm_check_n(size_t n, int* el, const char* who) {
  if (!is_pow2(n)) { set_error("%s: coefs.len() must be a power of two, but got %zu", who, n); return MZK_E_NOT_POW2; }
  *el = (int)ilog2(n);
  if (*el > GM_MAX_LOG) { set_error("%s: 2^%d coefficients (at most 2^%d)", who, *el, GM_MAX_LOG); return MZK_E_ARG; }
  return MZK_OK;
}
// 2^k R for k = 0..31: the weights of the hypercube sums
struct GmPow2 { u32 w[32][8]; };
static GmPow2 gm_pow2() {
  GmPow2 p;
  for (int k = 0; k < 32; k++) {
    uint64_t v[4] = {(uint64_t)1 << k, 0, 0, 0};
    h_mont_words(host_field(MZK_FIELD_FR), v, p.w[k]);
  }
  return p;
}

// ---- split-and-fold (gemini.rs:51-100) ----------------------------------------------------------------------------
constexpr size_t FOLD_LDS_IN = 2048;       // levels of at most this many elements fold in LDS, all in one launch
constexpr int FOLD_THREADS = 256;
struct GmRho16 { u32 w[16][8]; };

__global__ __launch_bounds__(FOLD_THREADS) void k_gm_fold(const u32* __restrict__ in, size_t n_out, Words8 rho, u32* __restrict__ out) {
  const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n_out) return;
  fe_gstore<GP>(out, k, gm_fold1(fe_gload<GP>(in, 2 * k), fe_gload<GP>(in, 2 * k + 1), fe_unpack<GP>(rho.w)));
}
// in: one level of len0 <= FOLD_LDS_IN elements (global); writes the nfold levels below it back to back from `out`
__global__ __launch_bounds__(FOLD_THREADS) void k_gm_fold_lds(const u32* __restrict__ in, int len0, GmRho16 rho, int nfold, u32* __restrict__ out) {
  __shared__ u32 A[FOLD_LDS_IN / 2][8];
  __shared__ u32 B[FOLD_LDS_IN / 4][8];
  const int tid = threadIdx.x;
  int len = len0 >> 1;
  {
    const GE r = fe_unpack<GP>(rho.w[0]);
    for (int k = tid; k < len; k += FOLD_THREADS) {
      const GE v = gm_fold1(fe_gload<GP>(in, 2 * k), fe_gload<GP>(in, 2 * k + 1), r);
      fe_pack<GP>(v, A[k]);
      fe_gstore<GP>(out, k, v);
    }
  }
  u32* o = out + 8 * (size_t)len;
  for (int f = 1; f < nfold; f++) {
    __syncthreads();
    u32 (*src)[8] = (f & 1) ? A : B;
    u32 (*dst)[8] = (f & 1) ? B : A;
    const GE r = fe_unpack<GP>(rho.w[f]);
    const int nl = len >> 1;
    for (int k = tid; k < nl; k += FOLD_THREADS) {
      const GE v = gm_fold1(fe_unpack<GP>(src[2 * k]), fe_unpack<GP>(src[2 * k + 1]), r);
      fe_pack<GP>(v, dst[k]);
      fe_gstore<GP>(o, k, v);
    }
    o += 8 * (size_t)nl;
    len = nl;
  }
}

// levels: 2n - 1 elements, level 0 first.  rhos: el host values (canonical).  d_levels may hold level 0 already.
static int split_fold_impl(const void* d_coef, size_t n, const uint64_t* rhos, size_t n_rhos, void* d_levels, hipStream_t s) {
  if (!d_levels || (!d_coef && n)) { set_error("split_fold: null pointer"); return MZK_E_ARG; }
  int el;
  MZK_TRY(gm_check_n(n, &el, "split_fold"));
  if (n_rhos != (size_t)el) { set_error("points.len() must be %d, but got %zu", el, n_rhos); return MZK_E_LENGTH; }
  if (el && !rhos) { set_error("split_fold: null pointer"); return MZK_E_ARG; }
  const HostField* fr = host_field(MZK_FIELD_FR);
  for (int i = 0; i < el; i++) if (!h_is_canonical(fr, rhos + 4 * i)) { set_error("split_fold: rho_%d not canonical", i); return MZK_E_RANGE; }
  if (d_coef != d_levels) MZK_HIP(hipMemcpyAsync(d_levels, d_coef, n * 32, hipMemcpyDeviceToDevice, s));
  const u32* cur = (const u32*)d_levels;
  size_t len = n;
  int i = 0;
  while (len > FOLD_LDS_IN) {
    Words8 r;
    h_mont_words(fr, rhos + 4 * i, r.w);
    u32* next = (u32*)cur + 8 * len;
    const size_t nout = len / 2;
    hipLaunchKernelGGL(k_gm_fold, dim3((unsigned)((nout + FOLD_THREADS - 1) / FOLD_THREADS)), dim3(FOLD_THREADS), 0, s, cur, nout, r, next);
    cur = next; len = nout; i++;
  }
  if (len > 1) {
    GmRho16 rr;
    for (int f = 0; f < el - i; f++) h_mont_words(fr, rhos + 4 * (i + f), rr.w[f]);
    hipLaunchKernelGGL(k_gm_fold_lds, dim3(1), dim3(FOLD_THREADS), 0, s, cur, (int)len, rr, el - i, (u32*)cur + 8 * len);
  }
  MZK_HIP(hipGetLastError());
  return MZK_OK;
}

// ---- hypercube sums ------------------------------------------------------------------------------------------------
// Element t of the visited level (FOLD: t of the level being produced, v_t = f[2t] + r f[2t+1], stored to out) enters slot
// (split ? t & 1 : 0) with weight 2^(base - popcount(t >> shift)); base < 0: no sums.  One partial per (workgroup, slot).
constexpr int SUM_THREADS = 256;
constexpr int SUM_MAX_WG = 1024;
template <bool FOLD>
__global__ __launch_bounds__(SUM_THREADS) void k_gm_sums(const u32* __restrict__ f, size_t count, Words8 r, u32* __restrict__ out, int base, int shift,
                                                          int split, GmPow2 pw, u32* __restrict__ partials) {
  __shared__ u32 S[2][SUM_THREADS][GP::L];
  const int tid = threadIdx.x;
  GE acc[2] = {fe_zero<GP>(), fe_zero<GP>()};
  const GE rm = fe_unpack<GP>(r.w);
  for (size_t t = (size_t)blockIdx.x * SUM_THREADS + tid; t < count; t += (size_t)gridDim.x * SUM_THREADS) {
    GE v;
    if (FOLD) {
      v = gm_fold1(fe_gload<GP>(f, 2 * t), fe_gload<GP>(f, 2 * t + 1), rm);
      fe_gstore<GP>(out, t, v);
    } else {
      v = fe_gload<GP>(f, t);
    }
    if (base < 0) continue;
    const int e = base - __popcll((unsigned long long)(t >> shift));
    const GE term = fe_mul<GP>(v, fe_unpack<GP>(pw.w[e]));
    const int slot = split ? (int)(t & 1) : 0;
    acc[slot] = fe_reduce<GP>(fe_add<GP>(acc[slot], term));
  }
  if (base < 0) return;
#pragma unroll
  for (int q = 0; q < 2; q++)
#pragma unroll
    for (int i = 0; i < GP::L; i++) S[q][tid][i] = acc[q].l[i];
  for (int d = SUM_THREADS / 2; d > 0; d >>= 1) {
    __syncthreads();
    if (tid < d) {
#pragma unroll
      for (int q = 0; q < 2; q++) {
        GE a, b;
#pragma unroll
        for (int i = 0; i < GP::L; i++) { a.l[i] = S[q][tid][i]; b.l[i] = S[q][tid + d][i]; }
        a = fe_reduce<GP>(fe_add<GP>(a, b));
#pragma unroll
        for (int i = 0; i < GP::L; i++) S[q][tid][i] = a.l[i];
      }
    }
  }
  __syncthreads();                 // lane 1 reads S[1][0], which lane 0 wrote in the last step
  if (tid < 2) {
    GE a;
#pragma unroll
    for (int i = 0; i < GP::L; i++) a.l[i] = S[tid][0][i];
    fe_gstore<GP>(partials, 2 * (size_t)blockIdx.x + tid, a);
  }
}
// out[0..2) = the two slots summed over nparts workgroups
__global__ __launch_bounds__(SUM_THREADS) void k_gm_sums_final(const u32* __restrict__ partials, int nparts, u32* __restrict__ out) {
  __shared__ u32 S[2][SUM_THREADS][GP::L];
  const int tid = threadIdx.x;
  GE acc[2] = {fe_zero<GP>(), fe_zero<GP>()};
  for (int p = tid; p < nparts; p += SUM_THREADS)
#pragma unroll
    for (int q = 0; q < 2; q++) acc[q] = fe_reduce<GP>(fe_add<GP>(acc[q], fe_gload<GP>(partials, 2 * (size_t)p + q)));
#pragma unroll
  for (int q = 0; q < 2; q++)
#pragma unroll
    for (int i = 0; i < GP::L; i++) S[q][tid][i] = acc[q].l[i];
  for (int d = SUM_THREADS / 2; d > 0; d >>= 1) {
    __syncthreads();
    if (tid < d) {
#pragma unroll
      for (int q = 0; q < 2; q++) {
        GE a, b;
#pragma unroll
        for (int i = 0; i < GP::L; i++) { a.l[i] = S[q][tid][i]; b.l[i] = S[q][tid + d][i]; }
        a = fe_reduce<GP>(fe_add<GP>(a, b));
#pragma unroll
        for (int i = 0; i < GP::L; i++) S[q][tid][i] = a.l[i];
      }
    }
  }
  __syncthreads();                 // lane 1 reads S[1][0], which lane 0 wrote in the last step
  if (tid < 2) {
    GE a;
#pragma unroll
    for (int i = 0; i < GP::L; i++) a.l[i] = S[tid][0][i];
    fe_gstore<GP>(out, tid, a);
  }
}
// d_out2: 2 elements (slot 0, slot 1).  Workspace: WS_NTT_IO_A (partials).
static int gm_sums(const void* d_f, size_t count, const uint64_t* r_host, void* d_fold_out, int base, int shift, int split, void* d_out2, hipStream_t s) {
  WsFrame ws("gm_sums");
  static const GmPow2 pw = gm_pow2();
  Words8 r = {};
  if (r_host) h_mont_words(host_field(MZK_FIELD_FR), r_host, r.w);
  const size_t wg_need = (count + SUM_THREADS - 1) / SUM_THREADS;
  const int nwg = (int)(wg_need < (size_t)SUM_MAX_WG ? (wg_need ? wg_need : 1) : SUM_MAX_WG);
  u32* partials = nullptr;
  MZK_TRY(ws.get(WS_NTT_IO_A, (size_t)nwg * 64, (void**)&partials));
  if (d_fold_out)
    hipLaunchKernelGGL(k_gm_sums<true>, dim3(nwg), dim3(SUM_THREADS), 0, s, (const u32*)d_f, count, r, (u32*)d_fold_out, base, shift, split, pw, partials);
  else
    hipLaunchKernelGGL(k_gm_sums<false>, dim3(nwg), dim3(SUM_THREADS), 0, s, (const u32*)d_f, count, r, (u32*)nullptr, base, shift, split, pw, partials);
  if (base >= 0) hipLaunchKernelGGL(k_gm_sums_final, dim3(1), dim3(SUM_THREADS), 0, s, (const u32*)partials, nwg, (u32*)d_out2);
  MZK_HIP(hipGetLastError());
  return MZK_OK;
}

// ---- MSM schedule ---------------------------------------------------------------------------------------------------
// Levels of at most GM_SMALL coefficients go through ONE grid-batched pass per kind (commitments, quotients, degree bounds)
// when the handle has a grid-batched path (srs_many_capable: direct tables, or narrow 8 / 10..13-bit tables with one bucket
// set); rows are zero-padded to the longest small level (zero coefficients add nothing).  Larger levels -- and every level on
// handles without that path (wide default tables of large SRS, degraded bucket sets, the no-table layout) -- take one MSM each.
constexpr size_t GM_SMALL = (size_t)1 << 12;
constexpr int GM_ROWS_MAX = 32;
struct GmRows { const u32* src[GM_ROWS_MAX]; u32 len[GM_ROWS_MAX]; u32 pad[GM_ROWS_MAX]; };
// row r of dst (width w): pad[r] zeros, src[r][0 .. len[r]), zeros
__global__ __launch_bounds__(256) void k_gm_pack(GmRows R, u32 w, u32* __restrict__ dst) {
  const u32 t = blockIdx.x * blockDim.x + threadIdx.x;
  const int r = blockIdx.y;
  if (t >= w) return;
  uint4* p = reinterpret_cast<uint4*>(dst + 8 * ((size_t)r * w + t));
  if (t >= R.pad[r] && t - R.pad[r] < R.len[r]) {
    const uint4* q = reinterpret_cast<const uint4*>(R.src[r] + 8 * (size_t)(t - R.pad[r]));
    p[0] = q[0]; p[1] = q[1];
  } else {
    p[0] = make_uint4(0, 0, 0, 0); p[1] = p[0];
  }
}
int msm_points_to_plain(const void* d_points_mont, size_t n, void* d_points_plain, hipStream_t s);   // mzk_msm.hip
// On handles without that path a table MSM pays its bucket pass whatever n is (about 0.9 ms at 17-bit windows, also for 16
// coefficients), so levels of at most GM_PLAIN_MAX coefficients run as generic MSMs over a plain copy of the points they use:
// row 0 of every layout holds the prepared points P_i themselves.
constexpr size_t GM_PLAIN_MAX = (size_t)1 << 16;
struct GmMsm { const void* src; size_t len; size_t shift; };
// out[k] (64 bytes each) = MSM(items[k].src, points [shift_k, shift_k + len_k)).  Items i0.. (the small ones) may go as one pass:
// then `front` pads at the front (all windows end at the same point, base = that end - width) instead of at the back.
static int gm_msms(const mzk_srs* srs, const GmMsm* items, int count, int i0, bool front, u32* d_out, hipStream_t s) {
  WsFrame ws("gm_msms");
  const bool capable = srs_many_capable(srs);
  const bool many = capable && count - i0 >= 2;
  const int single_to = many ? i0 : count;
  size_t plain_max = 0;
  for (int k = 0; k < single_to && !capable; k++)
    if (items[k].len <= GM_PLAIN_MAX && items[k].len > plain_max) plain_max = items[k].len;
  u32* plain = nullptr;
  if (plain_max) MZK_TRY(ws.get(WS_NTT_TMP, plain_max * 64, (void**)&plain));
  for (int k = 0; k < single_to; k++) {
    const MsmPoints pts = srs->points(items[k].shift);
    if (plain && items[k].len <= plain_max && items[k].len > 0) {
      MZK_TRY(msm_points_to_plain(pts.d, items[k].len, plain, s));
      MZK_TRY(msm_dev_impl(items[k].src, MsmPoints::plain(plain), items[k].len, d_out + 16 * k, false, s));
    } else {
      MZK_TRY(msm_dev_impl(items[k].src, pts, items[k].len, d_out + 16 * k, false, s));
    }
  }
  if (!many) return MZK_OK;
  GmRows R;
  size_t w = 0;
  const int rows = count - i0;
  for (int k = i0; k < count; k++) w = items[k].len > w ? items[k].len : w;
  if (w == 0) { MZK_HIP(hipMemsetAsync(d_out + 16 * i0, 0, (size_t)rows * 64, s)); return MZK_OK; }
  for (int r = 0; r < rows; r++) {
    R.src[r] = (const u32*)items[i0 + r].src;
    R.len[r] = (u32)items[i0 + r].len;
    R.pad[r] = front ? (u32)(w - items[i0 + r].len) : 0;
  }
  u32* mat;
  MZK_TRY(ws.get(WS_MISC_F, (size_t)rows * w * 32, (void**)&mat));
  hipLaunchKernelGGL(k_gm_pack, dim3((unsigned)((w + 255) / 256), (unsigned)rows), dim3(256), 0, s, R, (u32)w, mat);
  MZK_HIP(hipGetLastError());
  // front-padded rows: every window ends at shift_k + len_k = the same point; the padded row starts w earlier
  const size_t shift = front ? items[i0].shift + items[i0].len - w : 0;
  return msm_many_srs(srs, mat, w, w, (size_t)rows, d_out + 16 * i0, s, shift);
}

static int gm_srs_ok(const mzk_srs* srs, size_t n, int* el, const char* who) {
  MZK_TRY(gm_check_n(n, el, who));
  return srs_check_ctx(srs);
}
static inline size_t gm_level_off(size_t n, int i) { return 2 * n - (n >> i) * 2; }     // sum_{j < i} n / 2^j

// commit_gemini (gemini.rs:112-114): el + 1 commitments of the packed levels.  d_out: (el + 1) * 16 words.
static int gemini_commit_impl(const mzk_srs* srs, const void* d_levels, size_t n, void* d_out, hipStream_t s) {
  if (!srs || !d_levels || !d_out) { set_error("gemini_commit: null pointer"); return MZK_E_ARG; }
  int el;
  MZK_TRY(gm_srs_ok(srs, n, &el, "gemini_commit"));
  if (n > srs->n) { set_error("index out of bounds: the len is %zu but the index is %zu", srs->n, srs->n); return MZK_E_LENGTH; }
  GmMsm it[GM_MAX_LOG + 1];
  int i0 = el + 1;
  for (int i = 0; i <= el; i++) {
    it[i] = {(const char*)d_levels + gm_level_off(n, i) * 32, n >> i, 0};
    if ((n >> i) <= GM_SMALL && i0 > i) i0 = i;
  }
  return gm_msms(srs, it, el + 1, i0, false, (u32*)d_out, s);
}

// open_gemini (gemini.rs:116-144).  d_ys: el * 3 values (f_i(beta), f_i(-beta), f_i(beta^2)); d_ws: el points; d_deg: el + 1 points.
static int gemini_open_impl(const mzk_srs* srs, const void* d_levels, size_t n, const uint64_t* beta, void* d_ys, void* d_ws, void* d_deg, hipStream_t s) {
  WsFrame ws("gemini_open_impl");
  if (!srs || !d_levels || !beta || !d_deg || ((!d_ys || !d_ws) && n > 1)) { set_error("gemini_open: null pointer"); return MZK_E_ARG; }
  int el;
  MZK_TRY(gm_srs_ok(srs, n, &el, "gemini_open"));
  const HostField* fr = host_field(MZK_FIELD_FR);
  if (!h_is_canonical(fr, beta)) { set_error("gemini_open: beta not canonical"); return MZK_E_RANGE; }
  // prove_degree_bound(f_0, pk, n): max_d - n underflows when max_d < n (kzg.rs:126)
  const size_t max_d = srs->n - 1;
  if (srs->n == 0 || max_d < n) { set_error("attempt to subtract with overflow (max_d %zu - d %zu): the SRS needs n + 1 powers", srs->n ? max_d : 0, n); return MZK_E_LENGTH; }
  uint64_t nb[4] = {0, 0, 0, 0}, b2[4];
  h_negmod(fr, nb, beta);                                 // (0 - beta).sanitize()
  h_mulmod(fr, b2, beta, beta);
  if (el > 0 && (!memcmp(beta, nb, 32) || !memcmp(beta, b2, 32) || !memcmp(nb, b2, 32))) {
    set_error("gemini_open: beta, -beta and beta^2 must be distinct (beta in {0, 1, -1}: interpolate divides by zero)");
    return MZK_E_ARG;
  }
  // evaluations and quotients: three rounds of synthetic division over every level i < el
  size_t qtot = 0;
  for (int i = 0; i < el; i++) qtot += n >> i;
  u32 *qa = nullptr, *qb = nullptr;
  if (el > 0) {
    MZK_TRY(ws.get(WS_MISC_A, qtot * 32, (void**)&qa));
    MZK_TRY(ws.get(WS_MISC_B, qtot * 32, (void**)&qb));
    // round A: every level at beta (quotient q1 kept), at -beta and at beta^2 (values); round B: q2 = q1 / (X + beta); round C:
    // q3 = q2 / (X - beta^2), len - 3 elements.  Grouped by point: the engine's host powers of u are per run of equal points.
    std::vector<SdJob> jobs;
    for (int p = 0; p < 5; p++) {
      size_t qoff = 0;
      for (int i = 0; i < el; i++) {
        const size_t len = n >> i;
        const char* f = (const char*)d_levels + gm_level_off(n, i) * 32;
        char* y = (char*)d_ys + (size_t)i * 96;
        u32 *q1 = qa + 8 * qoff, *q2 = qb + 8 * qoff;
        switch (p) {
          case 0: jobs.push_back({f, len, beta, nullptr, y, q1}); break;
          case 1: jobs.push_back({f, len, nb, nullptr, y + 32, nullptr}); break;
          case 2: jobs.push_back({f, len, b2, nullptr, y + 64, nullptr}); break;
          case 3: jobs.push_back({q1, len - 1, nb, nullptr, nullptr, q2}); break;
          default: jobs.push_back({q2, len - 2, b2, nullptr, nullptr, q1}); break;
        }
        qoff += len;
      }
    }
    const size_t rounds[3] = {3 * (size_t)el, (size_t)el, (size_t)el};
    MZK_TRY(synth_div_dev(jobs.data(), rounds, 3, s));
  }
  // w_i = MSM(q3_i, powers[0, len - 3))
  GmMsm it[GM_MAX_LOG + 1];
  int i0 = el;
  size_t qoff = 0;
  for (int i = 0; i < el; i++) {
    const size_t len = n >> i;
    it[i] = {qa + 8 * qoff, len >= 3 ? len - 3 : 0, 0};
    if (len <= GM_SMALL && i0 > i) i0 = i;
    qoff += len;
  }
  if (el > 0) MZK_TRY(gm_msms(srs, it, el, i0, false, (u32*)d_ws, s));
  // deg_i = MSM(f_i * X^(max_d - d_i), powers) = MSM(f_i, powers[max_d - d_i, max_d)), d_i = len(f_i) = 2^(el - i)
  i0 = el + 1;
  for (int i = 0; i <= el; i++) {
    const size_t len = n >> i;
    it[i] = {(const char*)d_levels + gm_level_off(n, i) * 32, len, max_d - len};
    if (len <= GM_SMALL && i0 > i) i0 = i;
  }
  return gm_msms(srs, it, el + 1, i0, true, (u32*)d_deg, s);
}

}  // namespace mzk

using namespace mzk;

extern "C" {

int mzk_gemini_split_fold_dev(const void* d_coef, size_t n, const uint64_t* rhos, size_t n_rhos, void* d_out, void* stream) {
  MZK_ENTER();
  WsGuard wsg((hipStream_t)stream);
  return split_fold_impl(d_coef, n, rhos, n_rhos, d_out, (hipStream_t)stream);
}

int mzk_gemini_split_fold(const uint64_t* coef, size_t n, const uint64_t* rhos, size_t n_rhos, uint64_t* out) {
  MZK_ENTER();
  WsFrame ws("mzk_gemini_split_fold");
  if (!out || (!coef && n)) { set_error("split_fold: null pointer"); return MZK_E_ARG; }
  int el;
  MZK_TRY(gm_check_n(n, &el, "split_fold"));
  if (n_rhos != (size_t)el) { set_error("points.len() must be %d, but got %zu", el, n_rhos); return MZK_E_LENGTH; }
  if (el && !rhos) { set_error("split_fold: null pointer"); return MZK_E_ARG; }
  for (int i = 0; i < el; i++)
    if (!h_is_canonical(host_field(MZK_FIELD_FR), rhos + 4 * i)) { set_error("split_fold: rho_%d not canonical", i); return MZK_E_RANGE; }
  hipStream_t s = ctx().stream;
  WsGuard wsg(s);
  void* d;
  MZK_TRY(ws.get(WS_MISC_E, (2 * n - 1) * 32, &d));
  MZK_HIP(hipMemcpyAsync(d, coef, n * 32, hipMemcpyHostToDevice, s));
  MZK_TRY(split_fold_impl(d, n, rhos, n_rhos, d, s));
  return d2h_sync(out, d, (2 * n - 1) * 32, s);
}

int mzk_gemini_commit_srs_dev(const mzk_srs* srs, const void* d_levels, size_t n, void* d_out_xy, void* stream) {
  MZK_ENTER();
  WsGuard wsg((hipStream_t)stream);
  return gemini_commit_impl(srs, d_levels, n, d_out_xy, (hipStream_t)stream);
}

int mzk_gemini_commit_srs(const mzk_srs* srs, const uint64_t* levels, size_t n, uint64_t* out_xy) {
  MZK_ENTER();
  WsFrame ws("mzk_gemini_commit_srs");
  if (!srs || !levels || !out_xy) { set_error("gemini_commit: null pointer"); return MZK_E_ARG; }
  int el;
  MZK_TRY(gm_srs_ok(srs, n, &el, "gemini_commit"));
  hipStream_t s = ctx().stream;
  WsGuard wsg(s);
  void *d, *d_o;
  MZK_TRY(ws.get(WS_MISC_E, (2 * n - 1) * 32, &d));
  MZK_TRY(ws.get(WS_NTT_IO_B, (size_t)(el + 1) * 64, &d_o));
  MZK_HIP(hipMemcpyAsync(d, levels, (2 * n - 1) * 32, hipMemcpyHostToDevice, s));
  const int rc = gemini_commit_impl(srs, d, n, d_o, s);
  if (rc != MZK_OK) { (void)hipStreamSynchronize(s); return rc; }
  return d2h_sync(out_xy, d_o, (size_t)(el + 1) * 64, s);
}

int mzk_gemini_open_srs_dev(const mzk_srs* srs, const void* d_levels, size_t n, const uint64_t beta[4], void* d_ys, void* d_ws_xy, void* d_deg_xy,
                            void* stream) {
  MZK_ENTER();
  WsGuard wsg((hipStream_t)stream);
  return gemini_open_impl(srs, d_levels, n, beta, d_ys, d_ws_xy, d_deg_xy, (hipStream_t)stream);
}

// results of the host forms in one device block: ys (el * 3 * 32 B), ws (el * 64 B), deg ((el + 1) * 64 B)
static int gm_open_host(const mzk_srs* srs, const void* d_levels, size_t n, int el, const uint64_t* beta, uint64_t* ys, uint64_t* ws_xy, uint64_t* deg_xy,
                        hipStream_t s) {
  WsFrame ws("gm_open_host");
  const size_t by = (size_t)el * 96, bw = (size_t)el * 64, bd = (size_t)(el + 1) * 64;
  char* d_o;
  MZK_TRY(ws.get(WS_NTT_IO_B, by + bw + bd, (void**)&d_o));
  const int rc = gemini_open_impl(srs, d_levels, n, beta, d_o, d_o + by, d_o + by + bw, s);
  if (rc != MZK_OK) { (void)hipStreamSynchronize(s); return rc; }
  std::vector<uint64_t> tmp((by + bw + bd) / 8);
  MZK_TRY(d2h_sync(tmp.data(), d_o, by + bw + bd, s));
  if (el) { memcpy(ys, tmp.data(), by); memcpy(ws_xy, (char*)tmp.data() + by, bw); }
  memcpy(deg_xy, (char*)tmp.data() + by + bw, bd);
  return MZK_OK;
}

int mzk_gemini_open_srs(const mzk_srs* srs, const uint64_t* levels, size_t n, const uint64_t beta[4], uint64_t* ys, uint64_t* ws_xy, uint64_t* deg_xy) {
  MZK_ENTER();
  WsFrame ws("mzk_gemini_open_srs");
  if (!srs || !levels || !beta || !deg_xy || ((!ys || !ws_xy) && n > 1)) { set_error("gemini_open: null pointer"); return MZK_E_ARG; }
  int el;
  MZK_TRY(gm_srs_ok(srs, n, &el, "gemini_open"));
  hipStream_t s = ctx().stream;
  WsGuard wsg(s);
  void* d;
  MZK_TRY(ws.get(WS_MISC_E, (2 * n - 1) * 32, &d));
  MZK_HIP(hipMemcpyAsync(d, levels, (2 * n - 1) * 32, hipMemcpyHostToDevice, s));
  return gm_open_host(srs, d, n, el, beta, ys, ws_xy, deg_xy, s);
}

int mzk_sumcheck_sum(const uint64_t* coef, size_t n, uint64_t h[4]) {
  MZK_ENTER();
  WsFrame ws("mzk_sumcheck_sum");
  if (!h || (!coef && n)) { set_error("sumcheck_sum: null pointer"); return MZK_E_ARG; }
  int el;
  MZK_TRY(gm_check_n(n, &el, "sumcheck_sum"));
  hipStream_t s = ctx().stream;
  WsGuard wsg(s);
  void *d, *d_o;
  MZK_TRY(ws.get(WS_MISC_E, n * 32, &d));
  MZK_TRY(ws.get(WS_NTT_IO_B, 64, &d_o));
  MZK_HIP(hipMemcpyAsync(d, coef, n * 32, hipMemcpyHostToDevice, s));
  // h = sum_t c[t] 2^(el - popcount t): variable i contributes g(..0..) + g(..1..), a factor 2 where its exponent is 0
  MZK_TRY(gm_sums(d, n, nullptr, nullptr, el, 0, 0, d_o, s));
  uint64_t out[8];
  MZK_TRY(d2h_sync(out, d_o, 64, s));
  memcpy(h, out, 32);
  return MZK_OK;
}

int mzk_sumcheck_prove_srs(const mzk_srs* srs, const uint64_t* coef, size_t n, mzk_sumcheck_challenge_fn cb, void* user, uint64_t* gs, uint64_t* rs,
                           uint64_t beta[4], uint64_t* commits_xy, uint64_t* ys, uint64_t* ws_xy, uint64_t* deg_xy) {
  MZK_ENTER();
  WsFrame ws("mzk_sumcheck_prove_srs");
  if (!srs || !coef || !cb || !gs || !rs || !beta || !commits_xy || !ys || !ws_xy || !deg_xy) { set_error("sumcheck_prove: null pointer"); return MZK_E_ARG; }
  int el;
  MZK_TRY(gm_srs_ok(srs, n, &el, "sumcheck_prove"));
  if (el == 0) { set_error("invalid sizes for sum-check round (el = 0)"); return MZK_E_LENGTH; }
  if (srs->n < n + 1) { set_error("attempt to subtract with overflow (max_d %zu - d %zu): the SRS needs n + 1 powers", srs->n - 1, n); return MZK_E_LENGTH; }
  const HostField* fr = host_field(MZK_FIELD_FR);
  hipStream_t s = ctx().stream;
  WsGuard wsg(s);
  char* d;
  MZK_TRY(ws.get(WS_MISC_E, (2 * n - 1) * 32, (void**)&d));
  {   // the rounds' sums land in WS_NTT_IO_B; the lease ends with the rounds, gm_open_host below takes the slot for its results
    WsFrame rounds("mzk_sumcheck_prove_srs (rounds)");
    char* d_g;
    MZK_TRY(rounds.get(WS_NTT_IO_B, 64, (void**)&d_g));
    MZK_HIP(hipMemcpyAsync(d, coef, n * 32, hipMemcpyHostToDevice, s));
    // round 0: g_0 = A_0 + B_0 X from f_0 (m = el - 1)
    MZK_TRY(gm_sums(d, n, nullptr, nullptr, el - 1, 1, 1, d_g, s));
    for (int j = 0; j < el; j++) {
      MZK_TRY(d2h_sync(gs + 8 * j, d_g, 64, s));
      uint64_t r[4] = {0, 0, 0, 0};
      if (cb(user, j, gs + 8 * j, r) != 0) { set_error("sumcheck_prove: the challenge callback failed in round %d", j); return MZK_E_CALLBACK; }
      if (!h_is_canonical(fr, r)) { set_error("sumcheck_prove: r_%d not canonical", j); return MZK_E_RANGE; }
      memcpy(rs + 4 * j, r, 32);
      // f_{j+1} = fold(f_j, r_j), and in the same pass g_{j+1}'s sums (m = el - 2 - j; none after the last round)
      const size_t len = n >> j;
      MZK_TRY(gm_sums(d + gm_level_off(n, j) * 32, len / 2, r, d + gm_level_off(n, j + 1) * 32, el - 2 - j, 1, 1, d_g, s));
    }
  }
  uint64_t b[4] = {0, 0, 0, 0};
  if (cb(user, el, nullptr, b) != 0) { (void)hipStreamSynchronize(s); set_error("sumcheck_prove: the challenge callback failed for beta"); return MZK_E_CALLBACK; }
  if (!h_is_canonical(fr, b)) { (void)hipStreamSynchronize(s); set_error("sumcheck_prove: beta not canonical"); return MZK_E_RANGE; }
  memcpy(beta, b, 32);
  char* d_c;
  MZK_TRY(ws.get(WS_NTT_IO_A, (size_t)(el + 1) * 64, (void**)&d_c));
  int rc = gemini_commit_impl(srs, d, n, d_c, s);
  if (rc == MZK_OK) rc = d2h_sync(commits_xy, d_c, (size_t)(el + 1) * 64, s);
  if (rc != MZK_OK) { (void)hipStreamSynchronize(s); return rc; }
  return gm_open_host(srs, d, n, el, b, ys, ws_xy, deg_xy, s);
}

}  // extern "C"
