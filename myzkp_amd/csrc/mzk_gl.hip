// mzk_gl.hip -- transforms, coset LDE and the FRI fold over the Goldilocks field M64 and its cubic extension M64X3 (mzk_gl.h).
//
// The transform is over the BASE field for both ids: every element of 2-power order in F_{p^3}* lies in F_p (p^2 + p + 1 is odd), so
// the roots are base values and an id-4 transform is three base transforms over the coefficients c0, c1, c2 of the array-of-structures
// input (NC = 3: workgroup b works on coefficient b % 3 of tile b / 3, so the three workgroups that share every cache line run
// side by side).
//
// Shape (the pass structure of mzk_ntt.hip's k_ntt_strided / k_ntt_last, natural order in and out):
//   n <= 2^12             one pass: rows of n elements, 4096 / n rows per tile
//   larger                ceil(log2 n / 8) passes of 2^5 .. 2^8-point levels; pass t < last works in place on the 2^lgn strided
//                         columns of a block, 2^lgc = 4096 / 2^lgn adjacent columns per tile (>= 128-byte runs), and multiplies by the
//                         inter-pass twiddle; the last pass transforms contiguous rows and scatters them transposed, 2^lgr >= 16
//                         adjacent rows per tile (>= 128-byte runs again)
// A tile is 4096 base elements = 32 KiB of LDS (+ padding + 16 KiB of in-tile twiddles: three workgroups per CU).  Inside a tile the
// radix-2 DIT stages run four at a time on a lane's registers: 16 elements per lane, three LDS round trips for a 2^12-point level.
//
// Twiddles: an element is 8 bytes, so an n-entry inter-pass table would cost as much traffic as the data.  Instead w^E comes from
// three small tables of the plan, w^E = lo[E & 4095] * mid[(E >> 12) & 4095] * hi[E >> 24] (66 KiB, cache resident; the third factor
// only above 2^24 points): one or two products more per element and pass, against six in the butterflies.  The coset LDE's
// offset^i pre-scale uses tables of the same form and is fused into the first pass's loads (zero padding included).
#include "mzk_common.h"
#include "mzk_gl.h"
#include "mzk_ntt_plan.h"

namespace mzk {

typedef uint64_t u64;

constexpr int GL_TL = NTT_GEOS[NTT_GEO_GL].tl, GL_TILE = 1 << GL_TL, GL_NT = NTT_GEOS[NTT_GEO_GL].nt, GL_EPL = GL_TILE / GL_NT;      // 16 elements per lane
constexpr int GL_TW = GL_TILE / 2;                 // in-tile twiddles w_4096^j
constexpr int GL_POW_LO = 4096, GL_POW_MID = 4096, GL_POW_HI = 256, GL_POW = GL_POW_LO + GL_POW_MID + GL_POW_HI;
// tile position -> LDS slot: one slot of padding per 16 and per 256 elements, so that neither the bit-reversed scatter of the loads
// (strides of 256 elements and more) nor the stride-16 groups of the first register round fall onto one bank
__device__ __forceinline__ int gl_phys(int p) { return p + (p >> 4) + (p >> 8); }
constexpr int GL_LDS_DATA = GL_TILE + (GL_TILE >> 4) + (GL_TILE >> 8);

// g^E from the three tables of g (E < 2^32)
__device__ __forceinline__ u64 gl_pow_lookup(const u64* __restrict__ tab, u64 E, int big) {
  u64 r = gl::mul(tab[E & 4095], tab[GL_POW_LO + ((E >> 12) & 4095)]);
  if (big) r = gl::mul(r, tab[GL_POW_LO + GL_POW_MID + (E >> 24)]);
  return r;
}

// R radix-2 DIT stages (b + 1 .. b + R of a 2^lgn-point level) on registers.  The tile is [2^lgn rows][2^lgc columns], position
// (row << lgc) | col; a group is the 2^R rows that differ in row bits [b, b + R), at fixed column and other row bits.
template <int R>
__device__ __forceinline__ void gl_round(u64* lds, const u64* tw, int lgn, int lgc, int b, int groups) {
  constexpr int GS = 1 << R;
  const int lowbits = lgc + b;
#pragma unroll
  for (int q = 0; q < (GL_EPL >> R); q++) {
    const int gid = (int)threadIdx.x + q * GL_NT;
    if (gid >= groups) break;
    const int lowpos = gid & ((1 << lowbits) - 1);
    const int p0 = lowpos | ((gid >> lowbits) << (lowbits + R));
    const int rlow = lowpos >> lgc;                        // row bits below b
    u64 x[GS];
#pragma unroll
    for (int g = 0; g < GS; g++) x[g] = lds[gl_phys(p0 | (g << lowbits))];
#pragma unroll
    for (int i = 0; i < R; i++) {
      const int sh = lgn - (b + i + 1);                    // w_{2^s}^jj = w_{2^lgn}^(jj << (lgn - s)), s = b + i + 1
#pragma unroll
      for (int a = 0; a < GS; a++) {
        if (a & (1 << i)) continue;
        const int jj = rlow | ((a & ((1 << i) - 1)) << b);
        const u64 y = gl::mul(x[a | (1 << i)], tw[jj << sh]);
        x[a | (1 << i)] = gl::sub(x[a], y);
        x[a] = gl::add(x[a], y);
      }
    }
#pragma unroll
    for (int g = 0; g < GS; g++) lds[gl_phys(p0 | (g << lowbits))] = x[g];
  }
}
// all stages of a level whose bit-reversed input is in LDS; the result is in natural row order
__device__ __forceinline__ void gl_tile_stages(u64* lds, const u64* tw, int lgn, int lgc, int tile_elems) {
  for (int b = 0; b < lgn;) {
    const int R = lgn - b >= 4 ? 4 : lgn - b;
    __syncthreads();
    const int groups = tile_elems >> R;
    if (R == 4) gl_round<4>(lds, tw, lgn, lgc, b, groups);
    else if (R == 3) gl_round<3>(lds, tw, lgn, lgc, b, groups);
    else if (R == 2) gl_round<2>(lds, tw, lgn, lgc, b, groups);
    else gl_round<1>(lds, tw, lgn, lgc, b, groups);
    b += R;
  }
  __syncthreads();
}
// in-tile twiddles of a 2^lgn-point level out of the plan's w_{2^tl}^j table
__device__ __forceinline__ void gl_stage_twiddles(u64* tw, const u64* __restrict__ t12, int lgn, int tl) {
  const int cnt = lgn ? 1 << (lgn - 1) : 0;
  for (int j = threadIdx.x; j < cnt; j += GL_NT) tw[j] = t12[(size_t)j << (tl - lgn)];
}

// coset LDE: element idx of transform o is coef[o * n_coef + idx] * offset^idx below n_coef and zero beyond (ntt.rs:254-269)
struct GlPre { const u64* coef; size_t n_coef; const u64* otab; int obig; };

// Pass t < last: in place on the strided columns of block o (2^(lgn + lgM) elements), then the inter-pass twiddle
// w^(escale * column * k), escale = n / block size.  lgn + lgc = 12.
template <int NC, bool PRE>
__global__ __launch_bounds__(GL_NT) void k_gl_ntt_strided(const u64* __restrict__ in, u64* __restrict__ out, const u64* __restrict__ tab, int lgn, int lgM,
                                                          int lgc, int tl, int big, u64 escale, GlPre pre) {
  __shared__ u64 lds[GL_LDS_DATA + GL_TW];
  u64* tw = lds + GL_LDS_DATA;
  const int tid = threadIdx.x;
  const size_t tile = (size_t)blockIdx.x / NC;
  const int comp = (int)((size_t)blockIdx.x - tile * NC);
  const int lg_tiles = lgM - lgc;
  const size_t o = tile >> lg_tiles, ct = tile & (((size_t)1 << lg_tiles) - 1);
  const size_t base = (o << (lgn + lgM)) + (ct << lgc);
  const int cmask = (1 << lgc) - 1;
  gl_stage_twiddles(tw, tab, lgn, tl);
  u64 v[GL_EPL];
#pragma unroll
  for (int u = 0; u < GL_EPL; u++) {
    const int e = tid + u * GL_NT;
    const size_t j1 = (size_t)(e >> lgc);
    const int c = e & cmask;
    if constexpr (PRE) {
      const size_t idx = (j1 << lgM) + (ct << lgc) + c;       // the first pass spans a whole transform: o is the batch index
      v[u] = 0;
      if (idx < pre.n_coef) v[u] = gl::mul(pre.coef[(o * pre.n_coef + idx) * NC + comp], gl_pow_lookup(pre.otab, idx, pre.obig));
    } else {
      v[u] = in[(base + (j1 << lgM) + c) * NC + comp];
    }
  }
#pragma unroll
  for (int u = 0; u < GL_EPL; u++) {
    const int e = tid + u * GL_NT;
    const int k = (int)(__brev((unsigned)(e >> lgc)) >> (32 - lgn));
    lds[gl_phys((k << lgc) | (e & cmask))] = v[u];
  }
  gl_tile_stages(lds, tw, lgn, lgc, GL_TILE);
#pragma unroll
  for (int u = 0; u < GL_EPL; u++) {
    const int e = tid + u * GL_NT;
    const size_t k = (size_t)(e >> lgc);
    const int c = e & cmask;
    const u64 E = escale * (((ct << lgc) + c) * k);          // < n <= 2^32
    out[(base + (k << lgM) + c) * NC + comp] = gl::mul(lds[gl_phys(e)], gl_pow_lookup(tab + GL_TW, E, big));
  }
}

// Last pass: contiguous rows of 2^lgn, 2^lgr rows per tile, transposed scatter; optional final scale (n^-1 of the inverse).  The
// grid may cover a batch (row r belongs to transform r >> lg_rows).  Logical row r is the digit reversal of its memory row
// (row_base, as in k_ntt_last).
template <int NC, bool PRE>
__global__ __launch_bounds__(GL_NT) void k_gl_ntt_last(const u64* __restrict__ in, u64* __restrict__ out, const u64* __restrict__ tab, NttLevels li, int lgn,
                                                       int lgr, int lg_rows, u64 scale, int has_scale, size_t total_rows, int tl, GlPre pre) {
  __shared__ u64 lds[GL_LDS_DATA + GL_TW];
  u64* tw = lds + GL_LDS_DATA;
  const int tid = threadIdx.x;
  const size_t tile = (size_t)blockIdx.x / NC;
  const int comp = (int)((size_t)blockIdx.x - tile * NC);
  const size_t p0 = tile << lgr;
  const int rmask = (1 << lgr) - 1, nmask = (1 << lgn) - 1;
  const int tile_elems = 1 << (lgn + lgr);
  const size_t rowmask = ((size_t)1 << lg_rows) - 1;
  const int logn = lg_rows + lgn;
  gl_stage_twiddles(tw, tab, lgn, tl);
  auto row_base = [&](size_t r) -> size_t {
    size_t rem = r & rowmask, row = 0;
    for (int i = 0; i < li.nlev - 1; i++) {
      row = (row << li.lg[i]) | (rem & (((size_t)1 << li.lg[i]) - 1));
      rem >>= li.lg[i];
    }
    return ((r >> lg_rows) << logn) + (row << lgn);
  };
  u64 v[GL_EPL];
#pragma unroll
  for (int u = 0; u < GL_EPL; u++) {
    const int e = tid + u * GL_NT;
    const int rr = e >> lgn, j = e & nmask;
    const size_t r = p0 + rr;
    v[u] = 0;
    if (e < tile_elems && r < total_rows) {
      if constexpr (PRE) {        // single-pass LDE: row r is transform r
        if ((size_t)j < pre.n_coef) v[u] = gl::mul(pre.coef[(r * pre.n_coef + j) * NC + comp], gl_pow_lookup(pre.otab, (u64)j, pre.obig));
      } else {
        v[u] = in[(row_base(r) + j) * NC + comp];
      }
    }
  }
#pragma unroll
  for (int u = 0; u < GL_EPL; u++) {
    const int e = tid + u * GL_NT;
    if (e >= tile_elems) break;
    const int rr = e >> lgn, j = e & nmask;
    const int k = lgn ? (int)(__brev((unsigned)j) >> (32 - lgn)) : 0;
    lds[gl_phys((k << lgr) | rr)] = v[u];
  }
  gl_tile_stages(lds, tw, lgn, lgr, tile_elems);
#pragma unroll
  for (int u = 0; u < GL_EPL; u++) {
    const int e = tid + u * GL_NT;
    if (e >= tile_elems) break;
    // one pass (lg_rows = 0): a row's outputs are contiguous, lanes run along the row; otherwise output k of the tile's adjacent
    // rows is one run of 2^lgr elements, lanes run across the rows
    const int rr = lg_rows ? (e & rmask) : (e >> lgn), k = lg_rows ? (e >> lgr) : (e & nmask);
    const size_t r = p0 + rr;
    if (r >= total_rows) continue;
    u64 x = lds[gl_phys((k << lgr) | rr)];
    if (has_scale) x = gl::mul(x, scale);
    out[(((r >> lg_rows) << logn) + (r & rowmask) + ((size_t)k << lg_rows)) * NC + comp] = x;
  }
}

// FRI split-and-fold (zkstark/fri.rs:182-193): out[i] = 2^-1 (a + b) + (2^-1 alpha) q_i (a - b), a = cw[i], b = cw[h + i],
// q_i = (offset omega^i)^-1 = oinv winv^i -- a base value; alpha is any element of the field.  A workgroup folds GL_FOLD_BLOCK
// consecutive outputs, lane t those at t, t + 256, ...: one power of winv per lane, then steps of winv^256.
constexpr int GL_FOLD_PER_LANE = 4, GL_FOLD_BLOCK = GL_FOLD_PER_LANE * GL_NT;
template <int NC>
__global__ __launch_bounds__(GL_NT) void k_gl_fri_fold(const u64* __restrict__ cw, size_t h, gl::El<NC> alpha_half, u64 half, u64 oinv, u64 winv, u64 winv_step,
                                                       u64* __restrict__ out) {
  size_t i = (size_t)blockIdx.x * GL_FOLD_BLOCK + threadIdx.x;
  if (i >= h) return;
  u64 q = gl::mul(oinv, gl::pow(winv, (u64)i));
  for (int t = 0; t < GL_FOLD_PER_LANE && i < h; t++, i += GL_NT) {
    gl::El<NC> a, b;
#pragma unroll
    for (int c = 0; c < NC; c++) { a.c[c] = cw[i * NC + c]; b.c[c] = cw[(h + i) * NC + c]; }
    const gl::El<NC> o = gl::el_add<NC>(gl::el_scale<NC>(gl::el_add<NC>(a, b), half), gl::el_mul(gl::el_scale<NC>(alpha_half, q), gl::el_sub<NC>(a, b)));
#pragma unroll
    for (int c = 0; c < NC; c++) out[i * NC + c] = o.c[c];
    q = gl::mul(q, winv_step);
  }
}
// The same fold with alpha in device memory (mzk_fri_prove_gl: the round's transcript kernel wrote it there, NC canonical words);
// 2^-1 alpha is formed here as gl_fri_fold_dev forms it on the host, everything else is k_gl_fri_fold.
template <int NC>
__global__ __launch_bounds__(GL_NT) void k_gl_fri_fold_dev_alpha(const u64* __restrict__ cw, size_t h, const u64* __restrict__ alpha, u64 half, u64 oinv, u64 winv,
                                                                 u64 winv_step, u64* __restrict__ out) {
  size_t i = (size_t)blockIdx.x * GL_FOLD_BLOCK + threadIdx.x;
  if (i >= h) return;
  gl::El<NC> alpha_half;
#pragma unroll
  for (int c = 0; c < NC; c++) alpha_half.c[c] = gl::mul(alpha[c], half);
  u64 q = gl::mul(oinv, gl::pow(winv, (u64)i));
  for (int t = 0; t < GL_FOLD_PER_LANE && i < h; t++, i += GL_NT) {
    gl::El<NC> a, b;
#pragma unroll
    for (int c = 0; c < NC; c++) { a.c[c] = cw[i * NC + c]; b.c[c] = cw[(h + i) * NC + c]; }
    const gl::El<NC> o = gl::el_add<NC>(gl::el_scale<NC>(gl::el_add<NC>(a, b), half), gl::el_mul(gl::el_scale<NC>(alpha_half, q), gl::el_sub<NC>(a, b)));
#pragma unroll
    for (int c = 0; c < NC; c++) out[i * NC + c] = o.c[c];
    q = gl::mul(q, winv_step);
  }
}

// ---- plans ------------------------------------------------------------------------------------------------------------------
// Per (context, log2 n, direction, root): ONE device table [w_{2^tl}^j, j < 2048 | lo | mid | hi] of the effective
// root (root^-1 for the inverse).  Offset tables of the LDE: [lo | mid | hi] of the offset, kept per (context, offset).
struct GlPlan { unsigned logn; bool inverse; u64 root; int tl; DevMem d_tab; u64 scale; int has_scale; uint64_t stamp; };
struct GlOffTab { u64 offset; DevMem d_tab; uint64_t stamp; };
static std::vector<std::unique_ptr<GlPlan>> g_gl_plans[MZK_MAX_CTX];
static std::vector<std::unique_ptr<GlOffTab>> g_gl_offs[MZK_MAX_CTX];
constexpr size_t GL_MAX_PLANS = 48, GL_MAX_OFFS = 8;

void gl_release_plans() {
  g_gl_plans[ctx().index].clear();
  g_gl_offs[ctx().index].clear();
}

static void gl_fill_pow(u64 g, u64* t) {        // [lo | mid | hi] of g
  u64 x = 1;
  for (int i = 0; i < GL_POW_LO; i++) { t[i] = x; x = gl::mul(x, g); }
  const u64 g12 = x;                            // g^4096
  x = 1;
  for (int i = 0; i < GL_POW_MID; i++) { t[GL_POW_LO + i] = x; x = gl::mul(x, g12); }
  const u64 g24 = x;                            // g^(2^24)
  x = 1;
  for (int i = 0; i < GL_POW_HI; i++) { t[GL_POW_LO + GL_POW_MID + i] = x; x = gl::mul(x, g24); }
}
static int gl_upload(const std::vector<u64>& host, DevMem* d_tab, hipStream_t s) {
  MZK_TRY(d_tab->alloc(host.size() * 8, "goldilocks twiddle tables"));
  // (pageable source: the copy is staged before the call returns, as everywhere in this library)
  MZK_HIP(hipMemcpyAsync(d_tab->get(), host.data(), host.size() * 8, hipMemcpyHostToDevice, s));
  return MZK_OK;
}
static int gl_get_plan(unsigned logn, bool inverse, u64 root, hipStream_t s, GlPlan** out) {
  auto& plans = g_gl_plans[ctx().index];
  for (auto& p : plans)
    if (p->logn == logn && p->inverse == inverse && p->root == root) { p->stamp = lru_stamp(); *out = p.get(); return MZK_OK; }
  // reference assertions, ntt.rs:15-22
  const u64 n = (u64)1 << logn;
  if (gl::pow(root, n) != 1) { set_error("primitive root must be nth root of unity, where n is len(values)"); return MZK_E_ROOT_ORDER; }
  if (gl::pow(root, n / 2) == 1) { set_error("primitive root is not primitive nth root of unity, where n is len(values)"); return MZK_E_ROOT_PRIM; }
  MZK_TRY(lru_evict(plans, GL_MAX_PLANS, s));
  std::unique_ptr<GlPlan> pl(new GlPlan());
  pl->logn = logn; pl->inverse = inverse; pl->root = root;
  pl->tl = logn < (unsigned)GL_TL ? (int)logn : GL_TL;
  pl->stamp = lru_stamp();
  const u64 w = inverse ? gl::pow(root, n - 1) : root;          // root^-1 = root^(n-1)                      (ntt.rs:59)
  pl->has_scale = inverse ? 1 : 0;
  pl->scale = inverse ? gl::inv(n % gl::P) : 1;                 // F::from_value(n).inverse()                (ntt.rs:58)
  std::vector<u64> host(GL_TW + GL_POW, 0);
  const u64 wt = gl::pow(w, n >> pl->tl);                       // of order 2^tl
  u64 x = 1;
  for (int j = 0; j < (1 << pl->tl) / 2; j++) { host[j] = x; x = gl::mul(x, wt); }
  gl_fill_pow(w, host.data() + GL_TW);
  MZK_TRY(gl_upload(host, &pl->d_tab, s));
  *out = pl.get();
  plans.push_back(std::move(pl));
  return MZK_OK;
}
static int gl_get_offtab(u64 offset, hipStream_t s, const u64** out) {
  auto& offs = g_gl_offs[ctx().index];
  for (auto& p : offs)
    if (p->offset == offset) { p->stamp = lru_stamp(); *out = p->d_tab.as<u64>(); return MZK_OK; }
  MZK_TRY(lru_evict(offs, GL_MAX_OFFS, s));
  std::vector<u64> host(GL_POW);
  gl_fill_pow(offset, host.data());
  std::unique_ptr<GlOffTab> t(new GlOffTab{offset, DevMem(), lru_stamp()});
  MZK_TRY(gl_upload(host, &t->d_tab, s));
  *out = t->d_tab.as<u64>();
  offs.push_back(std::move(t));
  return MZK_OK;
}

// Walks the steps of ntt_plan (mzk_ntt_plan.h) over the tables of `pl`.
template <int NC>
static int gl_run_plan(const GlPlan* pl, const u64* d_in, u64* d_out, size_t batch, const GlPre* pre, hipStream_t s) {
  WsFrame ws("gl_run_plan");
  const unsigned logn = pl->logn;
  const NttSchedule sc = ntt_plan(NC == 3 ? MZK_FIELD_M64X3 : MZK_FIELD_M64, logn, batch, NttKnobs());
  if (sc.err != MZK_OK) { set_error("%s", sc.msg); return sc.err; }
  const int big = logn > 24 ? 1 : 0;
  const GlPre none{nullptr, 0, nullptr, 0};
  ProfScope whole(s, MZK_PH_NTT_TOTAL);
  const u64* src = d_in;
  u64* tmp = nullptr;
  if (sc.tmp_bytes) MZK_TRY(ws.get(WS_NTT_TMP, sc.tmp_bytes, (void**)&tmp));
  for (int t = 0; t < sc.nsteps; t++) {
    const NttStep& st = sc.steps[t];
    const bool with_pre = t == 0 && pre;
    if (st.kind == NTT_STEP_STRIDED) {
      const u64 escale = (u64)1 << (logn - (unsigned)(st.lgn + st.lgM));
      hipLaunchKernelGGL((with_pre ? k_gl_ntt_strided<NC, true> : k_gl_ntt_strided<NC, false>), dim3(st.grid), dim3(st.block), 0, s, src, tmp, pl->d_tab.as<u64>(),
                         st.lgn, st.lgM, st.lgc, pl->tl, big, escale, with_pre ? *pre : none);
      src = tmp;
    } else {
      hipLaunchKernelGGL((with_pre ? k_gl_ntt_last<NC, true> : k_gl_ntt_last<NC, false>), dim3(st.grid), dim3(st.block), 0, s, src, d_out, pl->d_tab.as<u64>(), sc.li,
                         st.lgn, st.lgr, st.lg_rows, pl->scale, pl->has_scale, st.total_rows, pl->tl, with_pre ? *pre : none);
    }
  }
  MZK_HIP(hipGetLastError());
  return MZK_OK;
}

int gl_param_check(int fid, const uint64_t* x, const char* who, const char* what, bool base_only) {
  const int nc = field_gl_comps(fid);
  for (int i = 0; i < nc; i++)
    if (!gl::is_canonical(x[i])) { set_error("%s: %s not canonical", who, what); return MZK_E_RANGE; }
  if (base_only)
    for (int i = 1; i < nc; i++)
      if (x[i]) { set_error("%s: %s must lie in the base field (c1 = c2 = 0)", who, what); return MZK_E_ARG; }
  return MZK_OK;
}

// `batch` transforms of n points each, back to back, in place allowed; the argument checks of ntt_dev_impl / ntt_batch_dev_impl
int gl_ntt_dev_impl(int fid, const uint64_t* root_host, const void* d_in, void* d_out, size_t n, size_t batch, int inverse, hipStream_t s) {
  if (n == 0 || batch == 0) return MZK_OK;
  if (!is_pow2(n)) { set_error("cannot compute ntt of non-power-of-two sequence"); return MZK_E_NOT_POW2; }
  if (!d_in || !d_out || (!root_host && n > 1)) { set_error("ntt: null pointer"); return MZK_E_ARG; }
  const size_t esz = field_bytes(fid);
  if (n > 1) MZK_TRY(gl_param_check(fid, root_host, "ntt", "root", false));
  if (ilog2(n) > gl::TWO_ADICITY || batch > ((size_t)1 << 40) / n) { set_error(batch == 1 ? "ntt: n too large" : "ntt: batch too large"); return MZK_E_ARG; }
  if (n == 1) {      // ntt.rs:12-14 / :54-56: returned unchanged
    if (d_in != d_out) MZK_HIP(hipMemcpyAsync(d_out, d_in, batch * esz, hipMemcpyDeviceToDevice, s));
    return MZK_OK;
  }
  for (int i = 1; i < field_gl_comps(fid); i++)      // an element outside the base field has no 2-power order
    if (root_host[i]) { set_error("primitive root must be nth root of unity, where n is len(values)"); return MZK_E_ROOT_ORDER; }
  GlPlan* pl = nullptr;
  MZK_TRY(gl_get_plan(ilog2(n), inverse != 0, root_host[0], s, &pl));
  return with_gl(fid, [&](auto tag) { return gl_run_plan<decltype(tag)::NC>(pl, (const u64*)d_in, (u64*)d_out, batch, nullptr, s); });
}

// ntt::fast_coset_evaluate (ntt.rs:254-269) for `batch` coefficient vectors of n_coef each; the argument checks of coset_lde_dev_impl
int gl_coset_lde_dev_impl(int fid, const void* d_coef, size_t n_coef, const uint64_t* offset_host, const uint64_t* generator_host, void* d_out,
                          size_t order, hipStream_t s, size_t batch) {
  if (batch == 0) return MZK_OK;
  if (n_coef > order) { set_error("attempt to subtract with overflow (order - polynomial.coef.len())"); return MZK_E_LENGTH; }
  if (order == 0) return MZK_OK;
  if (!is_pow2(order)) { set_error("cannot compute ntt of non-power-of-two sequence"); return MZK_E_NOT_POW2; }
  if (!d_out || (!d_coef && n_coef) || !offset_host || !generator_host) { set_error("coset_lde: null pointer"); return MZK_E_ARG; }
  MZK_TRY(gl_param_check(fid, offset_host, "coset_lde", "parameter", true));
  MZK_TRY(gl_param_check(fid, generator_host, "coset_lde", "parameter", true));
  const unsigned logn = ilog2(order);
  if (logn > gl::TWO_ADICITY || batch > ((size_t)1 << 40) / order) { set_error("coset_lde: order * batch too large"); return MZK_E_ARG; }
  const u64* otab = nullptr;
  MZK_TRY(gl_get_offtab(offset_host[0], s, &otab));
  if (order == 1) {      // one point: the constant coefficient (or zero), no root involved
    const GlPre pre{(const u64*)d_coef, n_coef, otab, 0};
    const NttLevels li{1, {0, 0, 0, 0}};
    const int nc = field_gl_comps(fid);
    const size_t blocks = batch * nc;
    if (blocks > 0x7fffffffu) { set_error("coset_lde: order * batch too large"); return MZK_E_ARG; }
    // the last-pass kernel with lgn = 0 copies (and pads); any cached table pointer serves as the unused twiddle source
    MZK_TRY(with_gl(fid, [&](auto tag) {
      hipLaunchKernelGGL((k_gl_ntt_last<decltype(tag)::NC, true>), dim3((unsigned)blocks), dim3(GL_NT), 0, s, (const u64*)d_coef, (u64*)d_out, otab, li, 0, 0, 0, (u64)1, 0,
                         batch, 0, pre);
      return MZK_OK;
    }));
    MZK_HIP(hipGetLastError());
    return MZK_OK;
  }
  GlPlan* pl = nullptr;
  MZK_TRY(gl_get_plan(logn, false, generator_host[0], s, &pl));
  const GlPre pre{(const u64*)d_coef, n_coef, otab, logn > 24 ? 1 : 0};
  return with_gl(fid, [&](auto tag) { return gl_run_plan<decltype(tag)::NC>(pl, (const u64*)d_coef, (u64*)d_out, batch, &pre, s); });
}

int gl_fri_fold_dev(int fid, const void* d_cw, size_t n, const uint64_t* alpha, uint64_t half, uint64_t oinv, uint64_t winv, void* d_out, hipStream_t s) {
  const size_t h = n / 2;
  if (h == 0) return MZK_OK;
  const size_t blocks = (h + GL_FOLD_BLOCK - 1) / GL_FOLD_BLOCK;
  if (blocks > 0x7fffffffu) { set_error("fri_fold: codeword too long"); return MZK_E_ARG; }
  const u64 step = gl::pow(winv, GL_NT);
  MZK_TRY(with_gl(fid, [&](auto tag) {
    constexpr int NC = decltype(tag)::NC;
    gl::El<NC> ah;
    for (int c = 0; c < NC; c++) ah.c[c] = gl::mul(alpha[c], half);
    hipLaunchKernelGGL((k_gl_fri_fold<NC>), dim3((unsigned)blocks), dim3(GL_NT), 0, s, (const u64*)d_cw, h, ah, half, oinv, winv, step, (u64*)d_out);
    return MZK_OK;
  }));
  MZK_HIP(hipGetLastError());
  return MZK_OK;
}

int gl_fri_fold_dev_alpha(int fid, const void* d_cw, size_t n, const uint64_t* d_alpha, uint64_t half, uint64_t oinv, uint64_t winv, void* d_out, hipStream_t s) {
  const size_t h = n / 2;
  if (h == 0) return MZK_OK;
  const size_t blocks = (h + GL_FOLD_BLOCK - 1) / GL_FOLD_BLOCK;
  if (blocks > 0x7fffffffu) { set_error("fri_fold: codeword too long"); return MZK_E_ARG; }
  const u64 step = gl::pow(winv, GL_NT);
  MZK_TRY(with_gl(fid, [&](auto tag) {
    hipLaunchKernelGGL((k_gl_fri_fold_dev_alpha<decltype(tag)::NC>), dim3((unsigned)blocks), dim3(GL_NT), 0, s, (const u64*)d_cw, h, d_alpha, half, oinv, winv, step,
                       (u64*)d_out);
    return MZK_OK;
  }));
  MZK_HIP(hipGetLastError());
  return MZK_OK;
}

}  // namespace mzk
