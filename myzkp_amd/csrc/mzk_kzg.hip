// mzk_kzg.hip -- the non-MSM parts of KZG setup / open on gfx950.
//
// setup_kzg (myzkp/src/modules/algebra/kzg.rs:27-40, G1 part): powers[i] = alpha^i * g1.  The reference
// runs max_d + 1 independent double-and-add scalar multiplications; here a fixed-base table
// T[w][d] = d * 2^(8 w) * g1 (w < 32, d < 256) turns each into 32 mixed additions.
//
// open_kzg (kzg.rs:61-72): y = f(u) (Polynomial::eval, polynomial.rs:120-128) and the quotient
// (f - y) / (X - u) (div_rem_ref, polynomial.rs:371-405).  Dividing by a monic linear factor is
// synthetic division: b_{n-1} = c_{n-1}, b_i = c_i + u b_{i+1}; then y = b_0 and q_j = b_{j+1}.  The
// suffix recurrence is solved by recursive chunking (chunk value at u, then the same recurrence on
// the chunk values with base u^K), so it is parallel at every level.  The witness MSM then runs in
// mzk_msm.hip on q.
#include "mzk_common.h"
#include "mzk_srs.h"
#include "mzk_elem.h"
#include "mzk_ec.h"

namespace mzk {
// fixed-base table cache of kzg_setup_g1_dev, one entry per context (the tables live in that context's workspace, the
// event on its device); kzg_release_cache() drops the current context's entry -- mzk_shutdown calls it, so a re-init that
// puts another device at the same index starts clean.
static struct { uint64_t g[8]; uint64_t gen; bool have8, have16; hipEvent_t ready; } g_fb_cache[MZK_MAX_CTX] = {};
void kzg_release_cache() {
  auto& c = g_fb_cache[ctx().index];
  if (c.ready) (void)hipEventDestroy(c.ready);
  memset(&c, 0, sizeof c);
}

// ---- fixed-base table ---------------------------------------------------------------------------------
// bases[w] = 2^(8 w) * g1, affine Montgomery (16 words); infinity base -> zeros
__global__ void k_fb_bases(Words16 g1_plain, u32* __restrict__ bases) {
  const int w = blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= 32) return;
  u32 o[16];
  for (int i = 0; i < 16; i++) o[i] = 0;
  if (!affine_words_is_inf(g1_plain.w)) {
    Xyzz p = xyzz_from_affine(affine_load_plain(g1_plain.w));
    for (int d = 0; d < 8 * w; d++) p = xyzz_dbl(p);
    Affine a;
    if (xyzz_to_affine(p, &a)) affine_store_mont(a, o);
  }
  store_words8(bases + 16 * w, o);
  store_words8(bases + 16 * w + 8, o + 8);
}
// table[w][d] = d * bases[w], d = 0..255 (d = 0 and infinity -> zeros), affine Montgomery
__global__ void k_fb_table(const u32* __restrict__ bases, u32* __restrict__ table) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= 32 * 256) return;
  const int w = t >> 8, d = t & 255;
  u32 bw[16], o[16];
  load_words8(bases + 16 * w, bw);
  load_words8(bases + 16 * w + 8, bw + 8);
  for (int i = 0; i < 16; i++) o[i] = 0;
  if (d != 0 && !affine_words_is_inf(bw)) {
    Affine b = affine_load_mont(bw);
    Xyzz acc = xyzz_inf();
    for (int bit = 7; bit >= 0; bit--) {
      acc = xyzz_dbl(acc);
      if ((d >> bit) & 1) acc = xyzz_madd(acc, b);
    }
    Affine a;
    if (xyzz_to_affine(acc, &a)) affine_store_mont(a, o);
  }
  store_words8(table + 16 * t, o);
  store_words8(table + 16 * t + 8, o + 8);
}
// table16[w][d] = d * 2^(16 w) * g1 for d < 65536 from the 8-bit table: T8[2w][d & 255] + T8[2w+1][d >> 8], written
// as XYZZ records (converted to affine in one batched pass afterwards).  Halves the additions per SRS power.
__global__ __launch_bounds__(128) void k_fb_table16(const u32* __restrict__ table8, u32* __restrict__ out_xyzz) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (size_t)16 << 16) return;
  const int w = (int)(t >> 16);
  const u32 d = (u32)t & 65535u, lo = d & 255u, hi = d >> 8;
  u32 a[16], b[16];
  load_words8(table8 + 16 * ((size_t)(2 * w) * 256 + lo), a);
  load_words8(table8 + 16 * ((size_t)(2 * w) * 256 + lo) + 8, a + 8);
  load_words8(table8 + 16 * ((size_t)(2 * w + 1) * 256 + hi), b);
  load_words8(table8 + 16 * ((size_t)(2 * w + 1) * 256 + hi) + 8, b + 8);
  Xyzz acc = xyzz_inf();
  if (!affine_words_is_inf(a)) acc = xyzz_from_affine(affine_load_mont(a));
  if (!affine_words_is_inf(b)) acc = xyzz_madd(acc, affine_load_mont(b));
  u32 o[32];
  xyzz_store(acc, o);
#pragma unroll
  for (int q = 0; q < 4; q++) store_words8(out_xyzz + 32 * t + 8 * q, o + 8 * q);
}
// atab[l][j] = alpha^(j * 2^(11 l)), l < 3, j < 2048, canonical Montgomery: alpha^e for e < 2^33 is then two
// products instead of a ~96-product square-and-multiply per SRS power.
constexpr int ATAB_BITS = 11;
__global__ void k_alpha_table(Words8 alpha_plain, u32* __restrict__ atab) {
  typedef FrParams R;
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= 3 << ATAB_BITS) return;
  const int l = t >> ATAB_BITS, j = t & ((1 << ATAB_BITS) - 1);
  Fe<R> a = fe_to_mont<R>(fe_unpack<R>(alpha_plain.w));
  Fe<R> v = fe_reduce<R>(fe_pow_u64<R>(a, (u64)j << (ATAB_BITS * l)));
  u32 o[8];
  fe_pack<R>(v, o);
  store_words8(atab + 8 * t, o);
}
// acc[i] = alpha^(first+i) * g1 as XYZZ (32 words); the affine conversion is batched afterwards.
template <int WB>   // window bits of the fixed-base table: 8 (32 windows, 512 KiB) or 16 (16 windows, 64 MiB)
__global__ __launch_bounds__(128) void k_fb_powers(Words8 alpha_plain, const u32* __restrict__ atab, const u32* __restrict__ table,
                                                   size_t first, size_t count, u32* __restrict__ out_xyzz) {
  typedef FrParams R;
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  const u64 e = (u64)(first + i);
  Fe<R> km;
  if (e >> (3 * ATAB_BITS)) {
    km = fe_pow_u64<R>(fe_to_mont<R>(fe_unpack<R>(alpha_plain.w)), e);
  } else {
    const u32 m = (1u << ATAB_BITS) - 1;
    u32 w0[8], w1[8], w2[8];
    load_words8(atab + 8 * (size_t)(e & m), w0);
    load_words8(atab + 8 * (size_t)((1u << ATAB_BITS) + ((e >> ATAB_BITS) & m)), w1);
    load_words8(atab + 8 * (size_t)((2u << ATAB_BITS) + ((e >> (2 * ATAB_BITS)) & m)), w2);
    km = fe_mul<R>(fe_mul<R>(fe_unpack<R>(w0), fe_unpack<R>(w1)), fe_unpack<R>(w2));
  }
  Fe<R> k = fe_from_mont<R>(km);   // canonical alpha^(first+i)   (kzg.rs:33-36)
  u32 kw[8];
  fe_pack<R>(k, kw);
  Xyzz acc = xyzz_inf();
#pragma unroll 1
  for (int w = 0; w < 256 / WB; w++) {
    const u32 d = (WB == 8) ? ((kw[w >> 2] >> (8 * (w & 3))) & 255u) : ((kw[w >> 1] >> (16 * (w & 1))) & 65535u);
    if (d == 0) continue;
    u32 tw[16];
    const size_t idx = ((size_t)w << WB) + d;
    load_words8(table + 16 * idx, tw);
    load_words8(table + 16 * idx + 8, tw + 8);
    if (affine_words_is_inf(tw)) continue;
    acc = xyzz_madd_with<FeAsm>(acc, affine_load_mont(tw));
  }
  u32 o[32];
  xyzz_store(acc, o);
#pragma unroll
  for (int q = 0; q < 4; q++) store_words8(out_xyzz + 32 * i + 8 * q, o + 8 * q);
}

// XYZZ -> affine for a whole array with Montgomery's batch-inversion trick: one lane owns BATCH consecutive
// points, multiplies their denominators ZZ*ZZZ into running prefix products (parked in `scratch`, 9 words
// each), inverts the total ONCE (Fermat: all lanes in lockstep) and unwinds.  ~33 products per point instead
// of ~390.  Infinity (all-zero record) contributes the factor 1 and comes out as the all-zero encoding.
constexpr int BATCH_INV = 16;
__global__ __launch_bounds__(128) void k_xyzz_batch_to_affine(const u32* __restrict__ xyzz, size_t count, u32* __restrict__ scratch,
                                                              u32* __restrict__ out, int out_mont) {
  typedef FqParams P;
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t i0 = t * BATCH_INV;
  if (i0 >= count) return;
  const int len = (int)((count - i0 < (size_t)BATCH_INV) ? (count - i0) : (size_t)BATCH_INV);
  Fq run = fe_one<P>();
  for (int j = 0; j < len; j++) {
    u32 w[16];
    load_words8(xyzz + 32 * (i0 + j) + 16, w);       // ZZ
    load_words8(xyzz + 32 * (i0 + j) + 24, w + 8);   // ZZZ
    const bool inf = affine_words_is_inf(w);
    Fq d = FeAsm<P>::mul(fe_unpack<P>(w), fe_unpack<P>(w + 8));
    if (inf) d = fe_one<P>();
    // prefix BEFORE including element j
#pragma unroll
    for (int k = 0; k < P::L; k++) scratch[(i0 + j) * P::L + k] = run.l[k];
    run = FeAsm<P>::mul(run, d);
  }
  Fq inv = fe_inv<P>(run);
  for (int j = len - 1; j >= 0; j--) {
    u32 w[32];
#pragma unroll
    for (int q = 0; q < 4; q++) load_words8(xyzz + 32 * (i0 + j) + 8 * q, w + 8 * q);
    const bool inf = affine_words_is_inf(w + 16);
    const Fq X = fe_unpack<P>(w), Y = fe_unpack<P>(w + 8), ZZ = fe_unpack<P>(w + 16), ZZZ = fe_unpack<P>(w + 24);
    Fq pre;
#pragma unroll
    for (int k = 0; k < P::L; k++) pre.l[k] = scratch[(i0 + j) * P::L + k];
    const Fq dinv = FeAsm<P>::mul(inv, pre);                       // 1 / (ZZ ZZZ) of element j
    Fq d = FeAsm<P>::mul(ZZ, ZZZ);
    if (inf) d = fe_one<P>();
    inv = FeAsm<P>::mul(inv, d);                                   // drop element j from the running inverse
    u32 o[16];
    if (inf) {
#pragma unroll
      for (int k = 0; k < 16; k++) o[k] = 0;
    } else {
      Affine a;
      a.x = fe_reduce<P>(FeAsm<P>::mul(X, FeAsm<P>::mul(dinv, ZZZ)));   // X / ZZ
      a.y = fe_reduce<P>(FeAsm<P>::mul(Y, FeAsm<P>::mul(dinv, ZZ)));    // Y / ZZZ
      if (out_mont) affine_store_mont(a, o); else affine_store_plain(a, o);
    }
    store_words8(out + 16 * (i0 + j), o);
    store_words8(out + 16 * (i0 + j) + 8, o + 8);
  }
}
int xyzz_batch_to_affine(const void* d_xyzz, size_t count, void* d_out, bool out_mont, hipStream_t s) {
  WsFrame ws("xyzz_batch_to_affine");
  if (count == 0) return MZK_OK;
  u32* scratch;
  MZK_TRY(ws.get(WS_BATCHINV, count * FqParams::L * sizeof(u32), (void**)&scratch));
  const size_t threads = (count + BATCH_INV - 1) / BATCH_INV;
  hipLaunchKernelGGL(k_xyzz_batch_to_affine, dim3((unsigned)((threads + 127) / 128)), dim3(128), 0, s, (const u32*)d_xyzz, count, scratch,
                     (u32*)d_out, out_mont ? 1 : 0);
  MZK_HIP(hipGetLastError());
  return MZK_OK;
}

int kzg_setup_g1_dev(const uint64_t* alpha_host, const uint64_t* g1_host, size_t first, size_t count, void* d_powers_xy, hipStream_t s) {
  WsFrame ws("kzg_setup_g1_dev");
  if (!alpha_host || !g1_host || (!d_powers_xy && count)) { set_error("kzg_setup: null pointer"); return MZK_E_ARG; }
  if (count == 0) return MZK_OK;
  if (!h_is_canonical(host_field(MZK_FIELD_FR), alpha_host) || !h_is_canonical(host_field(MZK_FIELD_FQ), g1_host) ||
      !h_is_canonical(host_field(MZK_FIELD_FQ), g1_host + 4)) { set_error("kzg_setup: operand not canonical"); return MZK_E_RANGE; }
  Words8 aw;
  Words16 gw;
  h_words(alpha_host, 4, aw.w);
  h_words(g1_host, 4, gw.w);          // x
  h_words(g1_host + 4, 4, gw.w + 8);  // y
  u32 *bases, *table, *acc, *atab;
  MZK_TRY(ws.get(WS_MISC_C, (size_t)(3 << ATAB_BITS) * 32, (void**)&atab));
  MZK_TRY(ws_cache_get(WS_FB_TABLE8, 32 * 64 + 32 * 256 * 64, (void**)&bases));
  table = bases + 32 * 16;
  const bool wide = count >= ((size_t)1 << 16);      // the 64 MiB table pays for itself from ~2^16 powers on
  const size_t t16 = (size_t)16 << 16;
  MZK_TRY(ws.get(WS_XYZZ_TMP, (wide && t16 > count ? t16 : count) * 128, (void**)&acc));
  u32* table16 = nullptr;
  if (wide) MZK_TRY(ws_cache_get(WS_FB_TABLE16, t16 * 64, (void**)&table16));
  // The fixed-base tables depend only on g1 (in practice always BN128::generator_g1()) and their construction is a
  // latency chain (248 serial doublings for the window bases + two inversions: ~1.4 ms, more than a whole 2^16-power
  // setup), so they are kept across calls, keyed by g1 and by the workspace generation.
  auto& cache = g_fb_cache[ctx().index];
  if (cache.gen != ws_generation() || memcmp(cache.g, g1_host, sizeof cache.g) != 0) {
    cache.gen = ws_generation(); cache.have8 = cache.have16 = false;
    memcpy(cache.g, g1_host, sizeof cache.g);
  }
  if (!cache.ready) MZK_HIP(hipEventCreateWithFlags(&cache.ready, hipEventDisableTiming));
  bool built = false;
  if (!cache.have8) {
    hipLaunchKernelGGL(k_fb_bases, dim3(1), dim3(32), 0, s, gw, bases);
    hipLaunchKernelGGL(k_fb_table, dim3(32), dim3(256), 0, s, (const u32*)bases, table);
    cache.have8 = true; built = true;
  }
  if (wide && !cache.have16) {
    hipLaunchKernelGGL(k_fb_table16, dim3((unsigned)(t16 / 128)), dim3(128), 0, s, (const u32*)table, acc);
    MZK_TRY(xyzz_batch_to_affine(acc, t16, table16, true, s));
    cache.have16 = true; built = true;
  }
  if (built) MZK_HIP(hipEventRecord(cache.ready, s));
  else MZK_HIP(hipStreamWaitEvent(s, cache.ready, 0));     // tables may have been built on another stream
  hipLaunchKernelGGL(k_alpha_table, dim3((3 << ATAB_BITS) / 256), dim3(256), 0, s, aw, atab);
  if (wide) {
    hipLaunchKernelGGL((k_fb_powers<16>), dim3((unsigned)((count + 127) / 128)), dim3(128), 0, s, aw, (const u32*)atab, (const u32*)table16,
                       first, count, acc);
  } else {
    hipLaunchKernelGGL((k_fb_powers<8>), dim3((unsigned)((count + 127) / 128)), dim3(128), 0, s, aw, (const u32*)atab, (const u32*)table,
                       first, count, acc);
  }
  MZK_HIP(hipGetLastError());
  return xyzz_batch_to_affine(acc, count, d_powers_xy, false, s);
}

// ---- synthetic division by (X - u): the one engine behind every opening --------------------------------------------------
// b_len = end (0 without one), b_t = c_t + u b_{t+1}; y = b_0, q = b_1 .. b_{len-1}, or b_1 .. b_len with an end.
// A round whose longest job has at most SD_BLOCK_MAX coefficients is one launch of k_sd_block, one workgroup per job.  Otherwise
// every job is cut into chunks of SD_K: k_sd_eval gives each chunk's value at u (the end folded into the last chunk), the same
// division one level up on those values at u^SD_K yields b at every chunk start, and k_sd_fill rebuilds each chunk from b at the
// start of the next.  b_0 is the same value at every level, so y comes from the top level; a job without q needs no fill.
constexpr int SD_K_LOG = 5;                       // chunk of 32: the per-lane recurrence is a serial chain, short chunks win
constexpr size_t SD_K = (size_t)1 << SD_K_LOG;
// one workgroup per job up to 2^13: every doubling doubles each lane's serial chain (a single opening of 2^12: 0.042 ms, 2^13: 0.064),
// while 2^14 through one chunk level takes 0.074
constexpr size_t SD_BLOCK_MAX = (size_t)1 << 13;
constexpr int SD_THREADS = 256;
// SD_K_LOG and SD_BLOCK_MAX were measured for Fr; not measured for M128.
struct SdRec {          // one job of one level, as the kernels read it; u / end hold P::NW words (8 for Fr, 4 for M128)
  const u32* src;       // len coefficients
  u32* q;               // b_1 .., or null
  u32* y;               // b_0, or null
  u64 len;
  u64 chunk0;           // first chunk of this job in its level's chunk arrays
  u32 u[8];             // canonical
  u32 end[8];           // b_len, canonical
  u32 has_end;          // q also gets b_len
};
// b_lo from b_hi = acc over the coefficients [lo, hi); u in Montgomery form (fe_mul(x, u R) = x u)
template <class P> __device__ __forceinline__ Fe<P> sd_horner(const u32* __restrict__ c, u64 lo, u64 hi, const Fe<P>& u, Fe<P> acc) {
  for (u64 t = hi; t-- > lo;) acc = fe_add<P>(fe_mul<P>(acc, u), fe_gload<P>(c, t));
  return fe_reduce<P>(acc);
}
// b_hi-1 .. b_lo from b_hi = acc into q (b_t at q[t - 1]; b_0 is y's)
template <class P> __device__ __forceinline__ void sd_fill(const SdRec& J, u64 lo, u64 hi, const Fe<P>& u, Fe<P> acc) {
  if (hi == J.len && J.has_end) fe_gstore<P>(J.q, hi - 1, acc);
  for (u64 t = hi; t-- > lo;) {
    acc = fe_reduce<P>(fe_add<P>(fe_mul<P>(acc, u), fe_gload<P>(J.src, t)));
    if (t > 0) fe_gstore<P>(J.q, t - 1, acc);
  }
}
// a job's values are wave-uniform: held in VGPRs, the powers of u of the scan below do not overflow the scalar registers
template <class P> __device__ __forceinline__ Fe<P> sd_vgpr(Fe<P> x) {
#pragma unroll
  for (int i = 0; i < P::L; i++) asm volatile("" : "+v"(x.l[i]));
  return x;
}
// one workgroup per job: lane L owns the K = ceil(len / 256) coefficients [L K, (L + 1) K); the lanes' chunk values are scanned
// with u^K, u^2K, ... through LDS, so S[L] = b_{L K}; then every lane fills its chunk from S[L + 1]
template <class P>
__global__ __launch_bounds__(SD_THREADS) void k_sd_block(const SdRec* __restrict__ jobs) {
  typedef Fe<P> E;
  __shared__ u32 S[SD_THREADS][P::L];
  const SdRec& J = jobs[blockIdx.x];
  const int L = threadIdx.x;
  const u64 n = J.len;
  const E u = sd_vgpr<P>(fe_to_mont<P>(fe_unpack<P>(J.u))), end = sd_vgpr<P>(fe_unpack<P>(J.end));
  const u64 K = (n + SD_THREADS - 1) / SD_THREADS;
  const u64 lo = (u64)L * K;
  const u64 hi = (lo + K < n) ? lo + K : n;
  E mine = fe_zero<P>();
  if (lo < n) mine = sd_horner<P>(J.src, lo, hi, u, hi == n ? end : fe_zero<P>());
  E pw = fe_one<P>(), base = u;                             // u^K in Montgomery form
  for (u64 k = K; k; k >>= 1) {
    if (k & 1) pw = fe_mul<P>(pw, base);
    base = fe_sqr<P>(base);
  }
#pragma unroll
  for (int i = 0; i < P::L; i++) S[L][i] = mine.l[i];
  for (int d = 1; d < SD_THREADS; d <<= 1) {
    __syncthreads();
    E other = fe_zero<P>();
    if (L + d < SD_THREADS) {
#pragma unroll
      for (int i = 0; i < P::L; i++) other.l[i] = S[L + d][i];
    }
    __syncthreads();
    mine = fe_reduce<P>(fe_add<P>(mine, fe_mul<P>(other, pw)));
#pragma unroll
    for (int i = 0; i < P::L; i++) S[L][i] = mine.l[i];
    pw = fe_sqr<P>(pw);
  }
  if (L == 0 && J.y) fe_gstore<P>(J.y, 0, mine);
  __syncthreads();
  if (!J.q || lo >= n) return;
  E acc = end;                                              // b_hi
  if (hi < n) {
#pragma unroll
    for (int i = 0; i < P::L; i++) acc.l[i] = S[L + 1][i];
  }
  sd_fill<P>(J, lo, hi, u, acc);
}
__device__ __forceinline__ int sd_job_of(const SdRec* __restrict__ jobs, int njobs, u64 g) {
  int lo = 0, hi = njobs - 1;     // last job with chunk0 <= g
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (jobs[mid].chunk0 <= g) lo = mid; else hi = mid - 1;
  }
  return lo;
}
// h[g] = the value of chunk g at u, from b = end behind the job's last chunk
template <class P>
__global__ __launch_bounds__(64) void k_sd_eval(const SdRec* __restrict__ jobs, int njobs, u64 nchunks, u32* __restrict__ h) {
  const u64 g = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= nchunks) return;
  const SdRec& J = jobs[sd_job_of(jobs, njobs, g)];
  const u64 lo = (g - J.chunk0) << SD_K_LOG;
  const u64 hi = (lo + SD_K < J.len) ? lo + SD_K : J.len;
  const Fe<P> u = fe_to_mont<P>(fe_unpack<P>(J.u));
  fe_gstore<P>(h, g, sd_horner<P>(J.src, lo, hi, u, hi == J.len ? fe_unpack<P>(J.end) : fe_zero<P>()));
}
// chunk g from b at the start of the next chunk, carry[g] (the level above wrote it as its quotient), or from the end
template <class P>
__global__ __launch_bounds__(64) void k_sd_fill(const SdRec* __restrict__ jobs, int njobs, u64 nchunks, const u32* __restrict__ carry) {
  const u64 g = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= nchunks) return;
  const SdRec& J = jobs[sd_job_of(jobs, njobs, g)];
  if (!J.q) return;
  const u64 lo = (g - J.chunk0) << SD_K_LOG;
  const u64 hi = (lo + SD_K < J.len) ? lo + SD_K : J.len;
  const Fe<P> u = fe_to_mont<P>(fe_unpack<P>(J.u));
  sd_fill<P>(J, lo, hi, u, hi == J.len ? fe_unpack<P>(J.end) : fe_gload<P>(carry, g));
}

template <class P>
static int synth_div_impl(int fid, const SdJob* jobs, const size_t* rounds, int nrounds, hipStream_t s) {
  WsFrame ws("synth_div_impl");
  const HostField* hf = host_field(fid);
  const int nl = hf->nl;
  const size_t ub = 8 * (size_t)nl;                        // bytes of one host element
  enum { BLOCK, EVAL, FILL };
  struct Step { int kind; size_t first, count; u64 nchunks; size_t arr; };   // arr: the level's chunk values / carries in WS_MISC_D
  std::vector<SdRec> tab;
  std::vector<Step> steps;
  // The table of every round and level is built here and uploaded once: a round's kernels then never wait for a host copy, and no
  // upload can overwrite a table that earlier kernels still read.  walk(nullptr) only measures WS_MISC_D (its records are dropped).
  auto walk = [&](u32* D) -> size_t {
    tab.clear();
    steps.clear();
    size_t need = 0, j0 = 0;
    for (int r = 0; r < nrounds; j0 += rounds[r], r++) {
      size_t first = tab.size();
      std::vector<uint64_t> us;                             // plain u of the current level's records
      bool fill = false;
      for (size_t i = j0; i < j0 + rounds[r]; i++) {
        const SdJob& J = jobs[i];
        if (J.len == 0) continue;
        SdRec x = {};
        x.src = (const u32*)J.src; x.q = (u32*)J.q; x.y = (u32*)J.y; x.len = J.len;
        h_words(J.u, nl, x.u);
        if (J.end) { h_words(J.end, nl, x.end); x.has_end = 1; }
        tab.push_back(x);
        us.insert(us.end(), J.u, J.u + nl);
        fill |= J.q != nullptr;                            // every level above has q where level 0 has
      }
      std::vector<Step> fills;
      size_t off = 0;                                       // a round's levels reuse WS_MISC_D from 0: the rounds run in order
      while (tab.size() > first) {
        const size_t count = tab.size() - first;
        u64 longest = 0, nch = 0;
        for (size_t k = first; k < tab.size(); k++) {
          longest = tab[k].len > longest ? tab[k].len : longest;
          tab[k].chunk0 = nch;
          nch += (tab[k].len + SD_K - 1) >> SD_K_LOG;
        }
        if (longest <= SD_BLOCK_MAX) { steps.push_back({BLOCK, first, count, 0, 0}); break; }
        steps.push_back({EVAL, first, count, nch, off});
        if (fill) fills.push_back({FILL, first, count, nch, off + nch});
        // one level up: each job's chunk values at u^SD_K; its quotient (b at chunks 1, 2, ..) is this level's carries
        std::vector<uint64_t> uk((size_t)nl * count);
        for (size_t k = 0; k < count; k++) {
          const SdRec b = tab[first + k];
          SdRec x = {};
          x.src = D ? D + P::NW * (off + b.chunk0) : nullptr;
          x.q = (D && b.q) ? D + P::NW * (off + nch + b.chunk0) : nullptr;
          x.y = b.y;
          x.len = (b.len + SD_K - 1) >> SD_K_LOG;
          if (D) {                                          // host powers are the call's set-up latency: once per run of equal points
            if (k > 0 && !memcmp(&us[nl * k], &us[nl * (k - 1)], ub)) memcpy(&uk[nl * k], &uk[nl * (k - 1)], ub);
            else h_powmod_u64(hf, &uk[nl * k], &us[nl * k], SD_K);
            h_words(&uk[nl * k], nl, x.u);
          }
          tab.push_back(x);
        }
        us.swap(uk);
        off += 2 * nch;
        first += count;
      }
      need = off > need ? off : need;
      steps.insert(steps.end(), fills.rbegin(), fills.rend());   // fills from the top level down
    }
    return need;
  };
  u32* D = nullptr;
  const size_t need = walk(nullptr);
  if (need) {
    MZK_TRY(ws.get(WS_MISC_D, need * field_bytes(fid), (void**)&D));
    walk(D);
  }
  if (tab.empty()) return MZK_OK;
  SdRec* d_tab;
  MZK_TRY(ws.get(WS_MISC_C, tab.size() * sizeof(SdRec), (void**)&d_tab));
  MZK_HIP(hipMemcpyAsync(d_tab, tab.data(), tab.size() * sizeof(SdRec), hipMemcpyHostToDevice, s));
  for (const Step& st : steps) {
    const SdRec* jt = d_tab + st.first;
    const unsigned grid = (unsigned)((st.nchunks + 63) / 64);
    if (st.kind == BLOCK) hipLaunchKernelGGL((k_sd_block<P>), dim3((unsigned)st.count), dim3(SD_THREADS), 0, s, jt);
    else if (st.kind == EVAL) hipLaunchKernelGGL((k_sd_eval<P>), dim3(grid), dim3(64), 0, s, jt, (int)st.count, st.nchunks, D + P::NW * st.arr);
    else hipLaunchKernelGGL((k_sd_fill<P>), dim3(grid), dim3(64), 0, s, jt, (int)st.count, st.nchunks, (const u32*)D + P::NW * st.arr);
  }
  MZK_HIP(hipGetLastError());
  return MZK_OK;
}
int synth_div_field_dev(int fid, const SdJob* jobs, const size_t* rounds, int nrounds, hipStream_t s) {
  return with_field(fid, [&](auto tag) { return synth_div_impl<typename decltype(tag)::P>(fid, jobs, rounds, nrounds, s); });
}
int synth_div_dev(const SdJob* jobs, const size_t* rounds, int nrounds, hipStream_t s) { return synth_div_field_dev(MZK_FIELD_FR, jobs, rounds, nrounds, s); }

// ---- division by a product of linear factors, many rows at once (the boundary quotients of FastStark::prove, fast_stark.rs:217-224) ----
// floor(f / prod_j (X - r_j)) is one synthetic division per root with each remainder b_0 dropped (what kzg_batch_open_dev does for one
// polynomial), and it equals (f - I) / Z of polynomial.rs:371-405 for ANY I of lower degree than Z: the interpolant never comes here.
// Round r divides every row that has more than r roots; a row's rounds ping-pong between WS_MISC_A and WS_MISC_B and its last round
// writes the out row.  The division runs over the lens[i] coefficients as given: leading zeros only give leading zeros in the quotient
// (division with remainder is unique), so the reference's trim is one pass at the end (rows_trimmed_len_dev), which also clears the rows' tails.
int poly_div_roots_check(int fid, const void* polys, size_t stride, const size_t* lens, size_t count, const uint64_t* roots, const size_t* root_offsets,
                         const void* out, const size_t* out_lens) {
  MZK_TRY(field_check(fid, "poly_div_roots"));
  if (count == 0) return MZK_OK;
  if (!lens || !root_offsets || !out_lens || (stride && (!polys || !out))) { set_error("poly_div_roots: null pointer"); return MZK_E_ARG; }
  const HostField* hf = host_field(fid);
  for (size_t i = 0; i < count; i++) {
    if (root_offsets[i + 1] < root_offsets[i]) {
      set_error("poly_div_roots: root_offsets[%zu] = %zu is below root_offsets[%zu] = %zu", i + 1, root_offsets[i + 1], i, root_offsets[i]);
      return MZK_E_LENGTH;
    }
    if (lens[i] > stride) { set_error("poly_div_roots: row %zu has %zu coefficients, stride is %zu", i, lens[i], stride); return MZK_E_LENGTH; }
  }
  if (root_offsets[count] > root_offsets[0] && !roots) { set_error("poly_div_roots: null pointer"); return MZK_E_ARG; }
  for (size_t j = root_offsets[0]; j < root_offsets[count]; j++)
    if (!h_is_canonical(hf, roots + j * hf->nl)) { set_error("poly_div_roots: roots[%zu] not canonical", j); return MZK_E_RANGE; }
  const size_t bpr = (stride + 255) / 256;
  if (stride > ((size_t)1 << 32) || count > ((size_t)1 << 40) / (stride ? stride : 1) || (bpr && count > (((size_t)1 << 31) - 1) / bpr)) {
    set_error("poly_div_roots: %zu rows of %zu elements are too many", count, stride);
    return MZK_E_LENGTH;
  }
  return MZK_OK;
}
// validated arguments (poly_div_roots_check); d_out must not overlap d_polys.  Workspace: WS_MISC_A, B (the rounds in between), C, D (synth_div),
// E (lengths).  Returns when d_out and out_lens are complete.
int poly_div_roots_dev_impl(int fid, const void* d_polys, size_t stride, const size_t* lens, size_t count, const uint64_t* roots, const size_t* root_offsets,
                            void* d_out, size_t* out_lens, hipStream_t s) {
  WsFrame ws("poly_div_roots_dev_impl");
  if (count == 0) return MZK_OK;
  const size_t esz = field_bytes(fid);
  const int nl = host_field(fid)->nl;
  size_t maxk = 0;
  std::vector<unsigned long long> meta(count, 0);          // quotient lengths before the trim
  for (size_t i = 0; i < count; i++) {
    const size_t k = root_offsets[i + 1] - root_offsets[i];
    meta[i] = lens[i] > k ? lens[i] - k : (k ? 0 : lens[i]);       // self.degree() < other.degree(): the zero polynomial (polynomial.rs:372)
    if (meta[i] && k > maxk) maxk = k;
    out_lens[i] = 0;
  }
  if (stride == 0) return MZK_OK;
  char *bA = nullptr, *bB = nullptr;
  if (maxk >= 2) MZK_TRY(ws.get(WS_MISC_A, count * stride * esz, (void**)&bA));
  if (maxk >= 3) MZK_TRY(ws.get(WS_MISC_B, count * stride * esz, (void**)&bB));
  std::vector<SdJob> jobs;
  std::vector<size_t> rounds(maxk, 0);
  for (size_t r = 0; r < maxk; r++)
    for (size_t i = 0; i < count; i++) {
      const size_t k = root_offsets[i + 1] - root_offsets[i];
      if (k <= r || !meta[i]) continue;
      const char* src = r == 0 ? (const char*)d_polys + i * stride * esz : ((r & 1) ? bA : bB) + i * stride * esz;
      char* dst = r == k - 1 ? (char*)d_out + i * stride * esz : ((r & 1) ? bB : bA) + i * stride * esz;
      jobs.push_back({src, lens[i] - r, roots + (root_offsets[i] + r) * nl, nullptr, nullptr, dst});
      rounds[r]++;
    }
  auto fail = [&](int rc) { (void)hipStreamSynchronize(s); return rc; };
  for (size_t i = 0; i < count; i++)                        // no roots: the row itself
    if (root_offsets[i + 1] == root_offsets[i] && lens[i] &&
        hipMemcpyAsync((char*)d_out + i * stride * esz, (const char*)d_polys + i * stride * esz, lens[i] * esz, hipMemcpyDeviceToDevice, s) != hipSuccess)
      return fail(MZK_E_HIP);
  int rc = synth_div_field_dev(fid, jobs.data(), rounds.data(), (int)maxk, s);
  if (rc != MZK_OK) return fail(rc);
  std::vector<size_t> qlens(count);
  for (size_t i = 0; i < count; i++) qlens[i] = (size_t)meta[i];
  rc = rows_trimmed_len_dev(fid, d_out, stride, qlens.data(), count, stride, nullptr, 0, ws, WS_MISC_E, out_lens, s);
  if (rc != MZK_OK) return fail(rc);
  return MZK_OK;
}
// batch_open_kzg (kzg.rs:74-88).  y_i = f(u_i) is b_0 of the division of f by (X - u_i).  The quotient of f by prod (X - u_i) --
// which equals (f - I)/Z because I = f mod Z -- is k successive divisions (each drops the remainder b_0): one round of k
// evaluations, then one round per quotient.  d_ys: k * 8 words, d_w_xy: 16 words.
int kzg_batch_open_dev(const void* d_coef, size_t n, const uint64_t* us_host, size_t k, MsmPoints pts, void* d_ys, void* d_w_xy, hipStream_t s) {
  WsFrame ws("kzg_batch_open_dev");
  if (!d_w_xy || (!d_coef && n) || ((!us_host || !d_ys) && k)) { set_error("batch_open: null pointer"); return MZK_E_ARG; }
  const HostField* fr = host_field(MZK_FIELD_FR);
  for (size_t i = 0; i < k; i++) if (!h_is_canonical(fr, us_host + 4 * i)) { set_error("batch_open: u not canonical"); return MZK_E_RANGE; }
  if (n == 0) {  // zero polynomial: every y = 0, quotient empty
    if (k) MZK_HIP(hipMemsetAsync(d_ys, 0, k * 32, s));
    MZK_HIP(hipMemsetAsync(d_w_xy, 0, 64, s));
    return MZK_OK;
  }
  u32 *bA, *bB;
  MZK_TRY(ws.get(WS_MISC_A, n * 32, (void**)&bA));
  MZK_TRY(ws.get(WS_MISC_B, n * 32, (void**)&bB));
  std::vector<SdJob> jobs;
  std::vector<size_t> rounds;
  for (size_t i = 0; i < k; i++) jobs.push_back({d_coef, n, us_host + 4 * i, nullptr, (char*)d_ys + 32 * i, nullptr});
  rounds.push_back(k);
  const void* cur = d_coef;
  size_t len = n;
  for (size_t i = 0; i < k && len > 0; i++, len--) {
    u32* dst = (i & 1) ? bB : bA;
    jobs.push_back({cur, len, us_host + 4 * i, nullptr, nullptr, dst});
    rounds.push_back(1);
    cur = dst;
  }
  MZK_TRY(synth_div_dev(jobs.data(), rounds.data(), (int)rounds.size(), s));
  return msm_dev_impl(cur, pts, len, d_w_xy, false, s);
}

// open_kzg (kzg.rs:61-72) as one division: y = f(u) into d_y (8 words); the quotient q = b_1 .. b_{n-1} into d_q when given; the
// witness w = MSM(q, points) into d_w_xy (16 words) when given, q then in workspace unless d_q holds it.
int kzg_open_dev(const void* d_coef, size_t n, const uint64_t* u_host, MsmPoints pts, void* d_y, void* d_w_xy, void* d_q, hipStream_t s) {
  WsFrame ws("kzg_open_dev");
  if (!u_host || !d_y || (!d_coef && n) || (d_w_xy && !pts.d && n > 1)) { set_error("kzg_open: null pointer"); return MZK_E_ARG; }
  if (!h_is_canonical(host_field(MZK_FIELD_FR), u_host)) { set_error("kzg_open: u not canonical"); return MZK_E_RANGE; }
  if (n == 0) {  // empty polynomial: y = 0, quotient empty -> infinity
    MZK_HIP(hipMemsetAsync(d_y, 0, 32, s));
    if (d_w_xy) MZK_HIP(hipMemsetAsync(d_w_xy, 0, 64, s));
    return MZK_OK;
  }
  if (d_w_xy && !d_q) MZK_TRY(ws.get(WS_MISC_A, n * 32, &d_q));
  const SdJob job = {d_coef, n, u_host, nullptr, d_y, d_q};
  const size_t one = 1;
  MZK_TRY(synth_div_dev(&job, &one, 1, s));
  if (!d_w_xy) return MZK_OK;
  return msm_dev_impl(d_q, pts, n - 1, d_w_xy, false, s);   // w = MSM(q, powers)  (kzg.rs:70)
}

// ---- open_kzg of MANY short polynomials, polynomial j at its own point u_j (kzg.rs:61-72 once per polynomial, as das/avail.rs:132
// does per cell): one round of divisions, y_j = b_0, q_j = b_1 .. b_{n-1} (row j of q, n elements apart); the witness MSMs then run
// as one grid-batched pass (msm_many_srs).  Field arithmetic is exact, so the outputs equal the single openings bit for bit.
constexpr size_t OPEN_MANY_MAX_N = (size_t)1 << 14;      // the witness pass's range; the division takes any n
bool kzg_open_many_supported(const mzk_srs* srs, size_t n) { return n <= OPEN_MANY_MAX_N && srs_many_capable(srs); }
// d_ys: count * 8 words, d_ws_xy: count * 16 words.
int kzg_open_many_dev(const mzk_srs* srs, const void* d_coefs, size_t n, size_t count, const uint64_t* us_host, void* d_ys, void* d_ws_xy, hipStream_t s) {
  WsFrame ws("kzg_open_many_dev");
  if (count == 0) return MZK_OK;
  if (!srs || !us_host || !d_ys || !d_ws_xy || (!d_coefs && n)) { set_error("kzg_open_many: null pointer"); return MZK_E_ARG; }
  const HostField* fr = host_field(MZK_FIELD_FR);
  for (size_t i = 0; i < count; i++) if (!h_is_canonical(fr, us_host + 4 * i)) { set_error("kzg_open: u not canonical"); return MZK_E_RANGE; }
  if (n == 0) {  // empty polynomials: y = 0, quotient empty -> infinity
    MZK_HIP(hipMemsetAsync(d_ys, 0, count * 32, s));
    MZK_HIP(hipMemsetAsync(d_ws_xy, 0, count * 64, s));
    return MZK_OK;
  }
  const size_t per_pass = (((size_t)1 << 22) + n - 1) / n;
  char* d_q;
  MZK_TRY(ws.get(WS_MISC_A, (count < per_pass ? count : per_pass) * n * 32, (void**)&d_q));
  std::vector<SdJob> jobs;
  for (size_t first = 0; first < count; first += per_pass) {
    const size_t cnt = (count - first < per_pass) ? count - first : per_pass;
    jobs.clear();
    for (size_t j = first; j < first + cnt; j++)
      jobs.push_back({(const char*)d_coefs + j * n * 32, n, us_host + 4 * j, nullptr, (char*)d_ys + j * 32, d_q + (j - first) * n * 32});
    MZK_TRY(synth_div_dev(jobs.data(), &cnt, 1, s));
    // w_j = MSM(q_j, powers), q_j of n - 1 coefficients     (kzg.rs:70)
    MZK_TRY(msm_many_srs(srs, d_q, n - 1, n, cnt, (u32*)d_ws_xy + first * 16, s));
  }
  return MZK_OK;
}

}  // namespace mzk

using namespace mzk;

extern "C" {

int mzk_poly_div_roots_dev(int field_id, const void* d_polys, size_t stride, const size_t* lens, size_t count, const uint64_t* roots,
                           const size_t* root_offsets, void* d_out, size_t* out_lens, void* stream) {
  MZK_ENTER();
  MZK_TRY(poly_div_roots_check(field_id, d_polys, stride, lens, count, roots, root_offsets, d_out, out_lens));
  WsGuard wsg((hipStream_t)stream);
  return poly_div_roots_dev_impl(field_id, d_polys, stride, lens, count, roots, root_offsets, d_out, out_lens, (hipStream_t)stream);
}

int mzk_poly_div_roots(int field_id, const uint64_t* polys, size_t stride, const size_t* lens, size_t count, const uint64_t* roots,
                       const size_t* root_offsets, uint64_t* out, size_t* out_lens) {
  MZK_ENTER();
  WsFrame ws("mzk_poly_div_roots");
  MZK_TRY(poly_div_roots_check(field_id, polys, stride, lens, count, roots, root_offsets, out, out_lens));
  if (count == 0) return MZK_OK;
  const HostField* hf = host_field(field_id);
  for (size_t i = 0; i < count; i++)
    for (size_t j = 0; j < lens[i]; j++)
      if (!h_is_canonical(hf, polys + (i * stride + j) * hf->nl)) { set_error("poly_div_roots: row %zu, coefficient %zu not canonical", i, j); return MZK_E_RANGE; }
  const size_t bytes = count * stride * field_bytes(field_id);
  hipStream_t s = ctx().stream;
  WsGuard wsg(s);
  char* d;
  MZK_TRY(ws.get(WS_MISC_F, 2 * bytes + 16, (void**)&d));
  if (bytes) MZK_HIP(hipMemcpyAsync(d, polys, bytes, hipMemcpyHostToDevice, s));
  const int rc = poly_div_roots_dev_impl(field_id, d, stride, lens, count, roots, root_offsets, d + bytes, out_lens, s);
  if (rc != MZK_OK) { (void)hipStreamSynchronize(s); return rc; }
  if (bytes == 0) return MZK_OK;
  return d2h_sync(out, d + bytes, bytes, s);
}

}  // extern "C"
