// mzk_rs.hip -- Reed-Solomon over GF(2^8), batched: algebra/reedsolomon.rs (ReedSolomon, ReedSolomon2D with g = x = 0x02) on the device.
// Every chunk, row and column of das/avail.rs, das/eigenda.rs and das/celestia.rs is an independent codeword, so the batch is the grid.
//
// Inputs and outputs are VIEWS (RsView: base pointer, byte stride between the symbols of a codeword, byte stride between codewords):
// the column pass of the 2D code and a transposed output are the same kernels, and nothing is ever transposed by a launch of its own.
// What is launched and with which tables is decided by rs_plan / rs_tables (mzk_rs_plan.h); the arithmetic is mzk_gf256.h.
//
//   encode, d <= 32   k_rs_encode_lane<PW>: one codeword per lane, the parity an LFSR of PW = 1, 2, 4 or 8 packed registers
//   encode, d >  32   k_rs_encode_wave: one codeword per wave, lane j owns parity bytes 4j .. 4j + 3
//   columns           k_rs_columns: the codewords once more as BN254 Fr elements, symbol-major (the layout mzk_kzg_commit_srs_many_dev takes)
//   syndromes         k_rs_syndromes: a group of W lanes per codeword, a Horner chain per syndrome
//   decode            k_rs_decode: the same group; Berlekamp-Massey, Chien search and Forney with sigma, B, S and Omega in LDS
#include <memory>
#include <vector>
#include "mzk_common.h"
#include "mzk_rs_plan.h"

using namespace mzk;
using gf256::gf_inv;
using gf256::gf_mul;

namespace mzk {

struct RsView { uint8_t* p; ptrdiff_t sym, cw; };
struct RsGenArgs { uint32_t f[8][8]; };      // gen_shifted[b][w], w < PW: wave-uniform kernel arguments

// ---- encode (reedsolomon.rs:54-78) --------------------------------------------------------------------------------------------------
// The codeword is (m(x) x^d mod g) in positions 0 .. d-1 and the message in d .. n-1.  The remainder is an LFSR over the message bytes
// from the top: R <- R x + m x^D mod G with G = g x^pad monic of degree D = 4 PW, so feedback = m ^ top byte of R, R <- (R << 8 bits)
// ^ feedback * (G - x^D), and the parity is bytes pad .. D-1 of R.  Everything that indexes p[] is unrolled: no scratch.
template <int PW>
__device__ __forceinline__ void rs_lfsr_step(uint32_t (&p)[PW], uint32_t mb, const RsGenArgs& G) {
  const uint32_t fb = mb ^ (p[PW - 1] >> 24);
#pragma unroll
  for (int w = PW - 1; w > 0; w--) p[w] = (p[w] << 8) | (p[w - 1] >> 24);
  p[0] <<= 8;
#pragma unroll
  for (int b = 0; b < 8; b++) {
    const uint32_t mask = 0u - ((fb >> b) & 1u);
#pragma unroll
    for (int w = 0; w < PW; w++) p[w] ^= mask & G.f[b][w];
  }
}

// WORDS: symbol strides 1, every pointer and codeword stride a multiple of 4, k a multiple of 4 and pad = 0 (d = 4 PW): the message is
// read and the codeword written in 32-bit words.
template <int PW, bool WORDS>
__global__ __launch_bounds__(256) void k_rs_encode_lane(const uint8_t* msg,ptrdiff_t msym, ptrdiff_t mcw, uint8_t* out, ptrdiff_t osym,
                                                        ptrdiff_t ocw, int k, int pad, size_t batch, unsigned iters, RsGenArgs G) {
  for (unsigned it = 0; it < iters; it++) {
    const size_t cw = ((size_t)it * gridDim.x + blockIdx.x) * 256 + threadIdx.x;
    if (cw >= batch) continue;
    uint32_t p[PW];
#pragma unroll
    for (int w = 0; w < PW; w++) p[w] = 0;
    if constexpr (WORDS) {
      const uint32_t* m = (const uint32_t*)(msg + (ptrdiff_t)cw * mcw);
      uint32_t* o = (uint32_t*)(out + (ptrdiff_t)cw * ocw);
      for (int i = k / 4 - 1; i >= 0; i--) {
        const uint32_t mw = m[i];
        o[PW + i] = mw;
        rs_lfsr_step<PW>(p, mw >> 24, G);
        rs_lfsr_step<PW>(p, (mw >> 16) & 0xFF, G);
        rs_lfsr_step<PW>(p, (mw >> 8) & 0xFF, G);
        rs_lfsr_step<PW>(p, mw & 0xFF, G);
      }
#pragma unroll
      for (int w = 0; w < PW; w++) o[w] = p[w];
    } else {
      const uint8_t* m = msg + (ptrdiff_t)cw * mcw;
      uint8_t* o = out + (ptrdiff_t)cw * ocw;
      const int d = 4 * PW - pad;
      for (int i = k - 1; i >= 0; i--) {
        const uint32_t mb = m[i * msym];
        o[(d + i) * osym] = (uint8_t)mb;
        rs_lfsr_step<PW>(p, mb, G);
      }
#pragma unroll
      for (int j = 0; j < 4 * PW; j++)
        if (j >= pad) o[(j - pad) * osym] = (uint8_t)(p[j / 4] >> (8 * (j % 4)));
    }
  }
}

// d = 0: the codeword is the message
__global__ __launch_bounds__(256) void k_rs_copy(const uint8_t* msg,ptrdiff_t msym, ptrdiff_t mcw, uint8_t* out, ptrdiff_t osym, ptrdiff_t ocw,
                                                 int k, size_t batch, unsigned iters) {
  for (unsigned it = 0; it < iters; it++) {
    const size_t cw = ((size_t)it * gridDim.x + blockIdx.x) * 256 + threadIdx.x;
    if (cw >= batch) continue;
    for (int i = 0; i < k; i++) out[(ptrdiff_t)cw * ocw + i * osym] = msg[(ptrdiff_t)cw * mcw + i * msym];
  }
}

// One codeword per wave, D = 256: lane j holds bytes 4j .. 4j + 3 of R and its word of the eight shifted forms of G.  The message
// comes in 64 bytes at a time, one per lane, and is handed round with a wave-uniform readlane; the byte that moves from lane j - 1 to
// lane j goes through ds_bpermute (__shfl_up).  Four waves of a workgroup work on four codewords and never meet: no barrier.
__global__ __launch_bounds__(256) void k_rs_encode_wave(const uint8_t* msg,ptrdiff_t msym, ptrdiff_t mcw, uint8_t* out, ptrdiff_t osym,
                                                        ptrdiff_t ocw, const uint32_t* __restrict__ gsh, int k, int pad, size_t batch, unsigned iters) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t g[8];
#pragma unroll
  for (int b = 0; b < 8; b++) g[b] = gsh[b * 64 + lane];
  const int d = 256 - pad;
  for (unsigned it = 0; it < iters; it++) {
    const size_t cw = ((size_t)it * gridDim.x + blockIdx.x) * 4 + wave;
    if (cw >= batch) continue;                                    // wave-uniform
    const uint8_t* m = msg + (ptrdiff_t)cw * mcw;
    uint8_t* o = out + (ptrdiff_t)cw * ocw;
    uint32_t p = 0;
    for (int base = k; base > 0; base -= 64) {
      const int idx = base - 1 - lane;                            // lane 0 holds the top byte of the chunk
      uint32_t chunk = 0;
      if (idx >= 0) {
        chunk = m[idx * msym];
        o[(d + idx) * osym] = (uint8_t)chunk;
      }
      const int cnt = base < 64 ? base : 64;
      for (int j = 0; j < cnt; j++) {
        const uint32_t mb = (uint32_t)__builtin_amdgcn_readlane((int)chunk, j);
        const uint32_t fb = mb ^ ((uint32_t)__builtin_amdgcn_readlane((int)p, 63) >> 24);
        const uint32_t below = (uint32_t)__shfl_up((int)p, 1, 64);
        p = (p << 8) | (lane ? below >> 24 : 0u);
#pragma unroll
        for (int b = 0; b < 8; b++) p ^= (0u - ((fb >> b) & 1u)) & g[b];
      }
    }
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const int q = 4 * lane + j - pad;
      if (q >= 0) o[q * osym] = (uint8_t)(p >> (8 * j));
    }
  }
}

// Symbol i of codeword b as the Fr element of that value at cols[i * batch + b]: a lane stores 32 contiguous bytes, a wave 2 KiB.
__global__ __launch_bounds__(256) void k_rs_columns(const uint8_t* __restrict__ code, ptrdiff_t sym, ptrdiff_t cwst, uint4* __restrict__ cols, size_t batch,
                                                    unsigned iters) {
  const size_t i = blockIdx.y;
  for (unsigned it = 0; it < iters; it++) {
    const size_t cw = ((size_t)it * gridDim.x + blockIdx.x) * 256 + threadIdx.x;
    if (cw >= batch) continue;
    const uint32_t v = code[(ptrdiff_t)cw * cwst + (ptrdiff_t)i * sym];
    uint4* dst = cols + 2 * (i * batch + cw);
    dst[0] = make_uint4(v, 0, 0, 0);
    dst[1] = make_uint4(0, 0, 0, 0);
  }
}

// ---- syndromes and decode (reedsolomon.rs:80-253) ------------------------------------------------------------------------------------
// A group of W lanes (a power of two, 8 .. 64, inside one wave) per codeword.  Lane l owns syndromes / coefficients l, l + W, ... and
// positions l, l + W, ...
__device__ __forceinline__ uint32_t rs_group_xor(uint32_t v, int W) {
  for (int o = W >> 1; o; o >>= 1) v ^= (uint32_t)__shfl_xor((int)v, o, W);
  return v;
}
__device__ __forceinline__ uint32_t rs_group_or(uint32_t v, int W) {
  for (int o = W >> 1; o; o >>= 1) v |= (uint32_t)__shfl_xor((int)v, o, W);
  return v;
}
__device__ __forceinline__ int rs_group_max(int v, int W) {
  for (int o = W >> 1; o; o >>= 1) { const int u = __shfl_xor(v, o, W); v = u > v ? u : v; }
  return v;
}
__device__ __forceinline__ int rs_group_sum(int v, int W) {
  for (int o = W >> 1; o; o >>= 1) v += __shfl_xor(v, o, W);
  return v;
}

// A Horner chain multiplies by the same element at every step -- the point 2^j of a syndrome, the point 2^-i of a Chien position -- so
// its eight forms a x^b are made once (rs_forms) and a step is a bit extract, an and and a xor per bit of the running value (rs_mulc)
// where the general product also walks a through its eight multiples.
struct RsForms { uint32_t f[8]; };
__device__ __forceinline__ RsForms rs_forms(uint32_t a) {
  RsForms F;
#pragma unroll
  for (int b = 0; b < 8; b++) { F.f[b] = a; a = gf256::xtime(a); }
  return F;
}
__device__ __forceinline__ uint32_t rs_mulc(const RsForms& F, uint32_t s) {
  uint32_t r = 0;
#pragma unroll
  for (int b = 0; b < 8; b++) r ^= (0u - ((s >> b) & 1u)) & F.f[b];
  return r;
}

// S_j = sum_i r_i 2^(i j), j < d (compute_syndromes, :90-102), by Horner from the top position; out: d bytes per codeword
__global__ __launch_bounds__(256) void k_rs_syndromes(const uint8_t* __restrict__ in, ptrdiff_t isym, ptrdiff_t icw, uint8_t* __restrict__ out,
                                                      const uint8_t* __restrict__ pts, int n, int d, int lgW, size_t batch, unsigned iters) {
  const int W = 1 << lgW, l = threadIdx.x & (W - 1), grp = threadIdx.x >> lgW, groups = 256 >> lgW;
  for (unsigned it = 0; it < iters; it++) {
    const size_t cw = ((size_t)it * gridDim.x + blockIdx.x) * groups + grp;
    if (cw >= batch) continue;
    const uint8_t* r = in + (ptrdiff_t)cw * icw;
    for (int j = l; j < d; j += W) {
      const RsForms a = rs_forms(pts[j]);
      uint32_t s = 0;
      for (int i = n - 1; i >= 0; i--) s = rs_mulc(a, s) ^ r[i * isym];
      out[cw * (size_t)d + j] = (uint8_t)s;
    }
  }
}

// correct_errors (:206-253) and decode (:80-86).  status: 0 clean, else the number of corrected symbols, 255 = the reference's None
// (corrected / messages then hold the received word unchanged).  Groups of one workgroup take different paths -- clean, e errors,
// failure -- and every loop that holds a barrier runs to a bound that is uniform over the workgroup (d, the round count): what a group
// does not need it skips by predication, and no barrier stands inside a divergent branch.  The whole error path is skipped when no
// group of the workgroup has a non-zero syndrome (__syncthreads_or: the common case of reconstruct).
__global__ __launch_bounds__(256) void k_rs_decode(const uint8_t* __restrict__ in, ptrdiff_t isym, ptrdiff_t icw, uint8_t* corr, ptrdiff_t csym, ptrdiff_t ccw,
                                                   uint8_t* msgs, ptrdiff_t msym, ptrdiff_t mcw, uint8_t* __restrict__ status,
                                                   const uint8_t* __restrict__ pts, const uint8_t* __restrict__ inv_pts, int n, int d, int lgW, int npad,
                                                   int dpad, size_t batch, unsigned iters) {
  extern __shared__ __align__(16) uint8_t rs_lds[];      // every array of a group starts on a word: npad and dpad are multiples of 4
  const int W = 1 << lgW, l = threadIdx.x & (W - 1), grp = threadIdx.x >> lgW, groups = 256 >> lgW;
  uint8_t* word = rs_lds + (size_t)grp * (2 * npad + 5 * dpad);      // the received word
  uint8_t* mag = word + npad;                                         // error magnitudes by position
  uint8_t* S = mag + npad;                                            // syndromes
  uint8_t* sig = S + dpad;                                            // sigma
  uint8_t* bb = sig + dpad;                                           // B
  uint8_t* tmp = bb + dpad;                                           // sigma before the update of this round
  uint8_t* om = tmp + dpad;                                           // Omega
  const int t2 = 2 * (d / 2);
  for (unsigned it = 0; it < iters; it++) {
    const size_t cw = ((size_t)it * gridDim.x + blockIdx.x) * groups + grp;
    const bool active = cw < batch;
    for (int i = l; i < npad; i += W) {                               // zeros behind position n-1: the syndromes read whole words
      word[i] = active && i < n ? in[(ptrdiff_t)cw * icw + i * isym] : 0;
      mag[i] = 0;
    }
    for (int i = l; i < dpad; i += W) {
      S[i] = 0; tmp[i] = 0; om[i] = 0;
      sig[i] = bb[i] = (i == 0);
    }
    __syncthreads();
    uint32_t any = 0;
    for (int j = l; j < d; j += W) {
      const RsForms a = rs_forms(pts[j]);
      uint32_t s = 0;
      for (int i = npad / 4 - 1; i >= 0; i--) {                       // four positions per LDS read, the top one first
        const uint32_t w4 = ((const uint32_t*)word)[i];
        s = rs_mulc(a, s) ^ (w4 >> 24);
        s = rs_mulc(a, s) ^ ((w4 >> 16) & 0xFF);
        s = rs_mulc(a, s) ^ ((w4 >> 8) & 0xFF);
        s = rs_mulc(a, s) ^ (w4 & 0xFF);
      }
      S[j] = (uint8_t)s;
      any |= s;
    }
    any = rs_group_or(any, W);
    int roots = 0, deg = 0;
    uint32_t bad = 0;
    if (__syncthreads_or((int)any)) {                                 // uniform over the workgroup; also publishes S
      // berlekamp_massey (:106-153): el, m, b are the same in every lane of the group; b is kept as its inverse, which changes only
      // where b does
      int el = 0, m = 1;
      uint32_t b_inv = 1;
      for (int r = 0; r < d; r++) {
        uint32_t acc = 0;
        for (int i = l; i <= el; i += W) acc ^= gf_mul(sig[i], S[r - i]);       // sig[0] = 1: the term S[r]; el <= r
        const uint32_t disc = rs_group_xor(acc, W);
        const bool upd = disc != 0;
        const uint32_t factor = gf_mul(disc, b_inv);                            // d / b (:131); zero when there is nothing to update
        for (int i = l; i <= d; i += W) {
          const uint32_t old = sig[i];
          tmp[i] = (uint8_t)old;
          if (upd && i >= m) sig[i] = (uint8_t)(old ^ gf_mul(factor, bb[i - m]));
        }
        __syncthreads();                                              // every read of B is done
        if (upd && 2 * el <= r) {
          for (int i = l; i <= d; i += W) bb[i] = tmp[i];
          el = r + 1 - el; b_inv = gf_inv(disc); m = 1;
        } else m++;
        __syncthreads();
      }
      for (int i = l; i <= d; i += W) if (sig[i]) deg = i;
      deg = rs_group_max(deg, W);
      // compute_error_evaluator (:169-182): Omega = sigma * S truncated to 2t terms
      for (int j = l; j < t2; j += W) {
        uint32_t acc = 0;
        const int top = j < deg ? j : deg;
        for (int i = 0; i <= top; i++) acc ^= gf_mul(sig[i], S[j - i]);
        om[j] = (uint8_t)acc;
      }
      __syncthreads();
      // find_error_locations (:189-200) and Forney (:237-250) at x = (2^pos)^-1; sigma' keeps the odd-index terms (from_value(i) = i mod 2)
      if (any) {
        for (int pos = l; pos < n; pos += W) {
          const RsForms x = rs_forms(inv_pts[pos]);
          uint32_t v = 0, dv = 0;
          for (int i = deg; i >= 0; i--) v = rs_mulc(x, v) ^ sig[i];
          if (v) continue;
          roots++;
          for (int i = deg; i >= 1; i--) dv = rs_mulc(x, dv) ^ ((i & 1) ? sig[i] : 0);
          if (!dv) { bad = 1; continue; }
          uint32_t ov = 0;
          for (int i = t2 - 1; i >= 0; i--) ov = rs_mulc(x, ov) ^ om[i];
          mag[pos] = (uint8_t)gf_mul(gf_mul(pts[pos], ov), gf_inv(dv));
        }
      }
      roots = rs_group_sum(roots, W);
      bad = rs_group_or(bad, W);
    }
    const bool fail = any && (roots != deg || bad);
    if (active) {
      for (int i = l; i < n; i += W) {                                // mag[i] was written by this lane
        const uint8_t v = word[i] ^ (fail ? 0 : mag[i]);
        if (corr) corr[(ptrdiff_t)cw * ccw + i * csym] = v;
        if (msgs && i >= d) msgs[(ptrdiff_t)cw * mcw + (i - d) * msym] = v;
      }
      if (l == 0) status[cw] = (uint8_t)(!any ? 0 : (fail ? 255 : roots));
    }
    __syncthreads();                                                  // the next round stages into the same LDS
  }
}

// ---- ReedSolomon2D (reedsolomon.rs:256-350) -------------------------------------------------------------------------------------------
// organize_data_matrix (:326-337) straight into the code: data[i * size + j] at code[d_col + i][d_row + j], zero behind message_len
__global__ __launch_bounds__(256) void k_rs2d_place(const uint8_t* __restrict__ data, size_t message_len, uint8_t* __restrict__ code, int size, int row_n,
                                                    int d_col, int d_row) {
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (size_t)size * size) return;
  const int i = (int)(idx / size), j = (int)(idx % size);
  code[(size_t)(d_col + i) * row_n + d_row + j] = idx < message_len ? data[idx] : 0;
}
// :315-323: the first message_len bytes of the size x size matrix; ok = no status of either pass is 255
__global__ __launch_bounds__(256) void k_rs2d_finish(const uint8_t* __restrict__ rows, size_t message_len, uint8_t* __restrict__ data,
                                                     const uint8_t* __restrict__ col_status, int ncol, const uint8_t* __restrict__ row_status, int nrow, int* ok) {
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx < message_len) data[idx] = rows[idx];
  if (idx == 0) {
    int good = 1;
    for (int i = 0; i < ncol; i++) good &= col_status[i] != 255;
    for (int i = 0; i < nrow; i++) good &= row_status[i] != 255;
    *ok = good;
  }
}

// ---- plans: the tables of (n, k) in device memory, per context -----------------------------------------------------------------------
struct RsEntry { int n, k; RsTables host; DevMem d_tab; uint64_t stamp; };      // d_tab: gen_shifted | pts | inv_pts
static std::vector<std::unique_ptr<RsEntry>> g_rs_plans[MZK_MAX_CTX];
constexpr size_t RS_MAX_PLANS = 16;
constexpr size_t RS_TAB_BYTES = sizeof(uint32_t) * 8 * 64 + 256 + 256;

void rs_release_plans() { g_rs_plans[ctx().index].clear(); }

static int rs_get_entry(const RsPlan& P, hipStream_t s, RsEntry** out) {
  auto& plans = g_rs_plans[ctx().index];
  for (auto& e : plans)
    if (e->n == P.n && e->k == P.k) { e->stamp = lru_stamp(); *out = e.get(); return MZK_OK; }
  MZK_TRY(lru_evict(plans, RS_MAX_PLANS, s));
  std::unique_ptr<RsEntry> e(new RsEntry());
  e->n = P.n; e->k = P.k; e->stamp = lru_stamp();
  rs_tables((size_t)P.n, (size_t)P.k, P.enc_pad, &e->host);
  MZK_TRY(e->d_tab.alloc(RS_TAB_BYTES, "reed-solomon tables"));
  // (the source lives as long as the entry; a pageable copy is staged before the call returns, as everywhere in this library)
  MZK_HIP(hipMemcpyAsync(e->d_tab.get(), e->host.gen_shifted, sizeof e->host.gen_shifted, hipMemcpyHostToDevice, s));
  MZK_HIP(hipMemcpyAsync(e->d_tab.as<uint8_t>() + sizeof e->host.gen_shifted, e->host.pts, 512, hipMemcpyHostToDevice, s));
  static_assert(offsetof(RsTables, inv_pts) == offsetof(RsTables, pts) + 256, "pts and inv_pts are uploaded as one piece");
  *out = e.get();
  plans.push_back(std::move(e));
  return MZK_OK;
}
static const uint32_t* rs_dev_gen(const RsEntry* e) { return e->d_tab.as<uint32_t>(); }
static const uint8_t* rs_dev_pts(const RsEntry* e) { return e->d_tab.as<uint8_t>() + sizeof(uint32_t) * 8 * 64; }
static const uint8_t* rs_dev_inv(const RsEntry* e) { return rs_dev_pts(e) + 256; }

static int rs_plan_checked(size_t n, size_t k, size_t batch, RsPlan* P) {
  *P = rs_plan(n, k, batch);
  if (P->err != MZK_OK) { set_error("%s", P->msg); return P->err; }
  return MZK_OK;
}

template <int PW>
static void rs_launch_lane(const RsPlan& P, const RsEntry* e, RsView m, RsView o, size_t batch, hipStream_t s) {
  RsGenArgs G;
  for (int b = 0; b < 8; b++) for (int w = 0; w < 8; w++) G.f[b][w] = e->host.gen_shifted[b][w];
  const bool words = P.enc_pad == 0 && P.k % 4 == 0 && m.sym == 1 && o.sym == 1 && m.cw % 4 == 0 && o.cw % 4 == 0 && (uintptr_t)m.p % 4 == 0 && (uintptr_t)o.p % 4 == 0;
  if (words) hipLaunchKernelGGL((k_rs_encode_lane<PW, true>), dim3(P.enc.grid), dim3(P.enc.block), 0, s, m.p, m.sym, m.cw, o.p, o.sym, o.cw, P.k, P.enc_pad, batch, P.enc.iters, G);
  else hipLaunchKernelGGL((k_rs_encode_lane<PW, false>), dim3(P.enc.grid), dim3(P.enc.block), 0, s, m.p, m.sym, m.cw, o.p, o.sym, o.cw, P.k, P.enc_pad, batch, P.enc.iters, G);
}

// messages -> codewords (and, when d_columns_fr is not null, the codewords once more as Fr columns)
static int rs_encode_views(size_t n, size_t k, RsView m, size_t batch, RsView o, void* d_columns_fr, hipStream_t s) {
  RsPlan P;
  MZK_TRY(rs_plan_checked(n, k, batch, &P));
  if (!m.p || !o.p) { set_error("rs_encode: null pointer"); return MZK_E_ARG; }
  RsEntry* e;
  MZK_TRY(rs_get_entry(P, s, &e));
  if (P.form == RS_FORM_COPY) hipLaunchKernelGGL(k_rs_copy, dim3(P.enc.grid), dim3(P.enc.block), 0, s, m.p, m.sym, m.cw, o.p, o.sym, o.cw, P.k, batch, P.enc.iters);
  else if (P.form == RS_FORM_WAVE)
    hipLaunchKernelGGL(k_rs_encode_wave, dim3(P.enc.grid), dim3(P.enc.block), 0, s, m.p, m.sym, m.cw, o.p, o.sym, o.cw, rs_dev_gen(e), P.k, P.enc_pad, batch, P.enc.iters);
  else if (P.enc_pw == 1) rs_launch_lane<1>(P, e, m, o, batch, s);
  else if (P.enc_pw == 2) rs_launch_lane<2>(P, e, m, o, batch, s);
  else if (P.enc_pw == 4) rs_launch_lane<4>(P, e, m, o, batch, s);
  else rs_launch_lane<8>(P, e, m, o, batch, s);
  MZK_HIP(hipGetLastError());
  if (d_columns_fr) {
    const RsLaunch L = rs_launch(batch, RS_BLOCK, 0);
    hipLaunchKernelGGL(k_rs_columns, dim3(L.grid, n), dim3(L.block), 0, s, o.p, o.sym, o.cw, (uint4*)d_columns_fr, batch, L.iters);
    MZK_HIP(hipGetLastError());
  }
  return MZK_OK;
}

static int rs_syndromes_views(size_t n, size_t k, RsView in, size_t batch, uint8_t* d_syndromes, hipStream_t s) {
  RsPlan P;
  MZK_TRY(rs_plan_checked(n, k, batch, &P));
  if (!in.p || (!d_syndromes && P.d)) { set_error("rs_syndromes: null pointer"); return MZK_E_ARG; }
  if (P.d == 0) return MZK_OK;
  RsEntry* e;
  MZK_TRY(rs_get_entry(P, s, &e));
  hipLaunchKernelGGL(k_rs_syndromes, dim3(P.syn.grid), dim3(P.syn.block), 0, s, in.p, in.sym, in.cw, d_syndromes, rs_dev_pts(e), P.n, P.d, (int)ilog2((size_t)P.dec_w), batch, P.syn.iters);
  MZK_HIP(hipGetLastError());
  return MZK_OK;
}

static int rs_decode_views(size_t n, size_t k, RsView in, size_t batch, RsView corr, RsView msgs, uint8_t* d_status, hipStream_t s) {
  RsPlan P;
  MZK_TRY(rs_plan_checked(n, k, batch, &P));
  if (!in.p || !d_status) { set_error("rs_decode: null pointer"); return MZK_E_ARG; }
  RsEntry* e;
  MZK_TRY(rs_get_entry(P, s, &e));
  hipLaunchKernelGGL(k_rs_decode, dim3(P.dec.grid), dim3(P.dec.block), P.dec.lds, s, in.p, in.sym, in.cw, corr.p, corr.sym, corr.cw, msgs.p, msgs.sym, msgs.cw, d_status,
                     rs_dev_pts(e), rs_dev_inv(e), P.n, P.d, (int)ilog2((size_t)P.dec_w), P.dec_npad, P.dec_dpad, batch, P.dec.iters);
  MZK_HIP(hipGetLastError());
  return MZK_OK;
}

static size_t rs2d_size(size_t message_len) {      // ceil(sqrt(message_len)) in integers (reedsolomon.rs:264)
  size_t s = 0;
  while (s * s < message_len) s++;
  return s;
}
static int rs2d_check(size_t col_n, size_t row_n, size_t message_len, size_t* size) {
  if (message_len > RS_MAX_N * RS_MAX_N) { set_error("rs2d: message_len = %zu is beyond 255 x 255", message_len); return MZK_E_ARG; }
  *size = rs2d_size(message_len);
  RsPlan P;
  MZK_TRY(rs_plan_checked(row_n, *size, *size ? *size : 1, &P));
  return rs_plan_checked(col_n, *size, row_n, &P);
}

static int rs2d_encode_impl(size_t col_n, size_t row_n, const void* d_data, size_t message_len, void* d_code, hipStream_t s) {
  size_t size;
  MZK_TRY(rs2d_check(col_n, row_n, message_len, &size));
  if (!d_data || !d_code) { set_error("rs2d_encode: null pointer"); return MZK_E_ARG; }
  uint8_t* code = (uint8_t*)d_code;
  const size_t d_col = col_n - size, d_row = row_n - size;
  hipLaunchKernelGGL(k_rs2d_place, dim3((size * size + 255) / 256), dim3(256), 0, s, (const uint8_t*)d_data, message_len, code, (int)size, (int)row_n, (int)d_col,
                     (int)d_row);
  MZK_HIP(hipGetLastError());
  // rows d_col .. col_n-1 in place (:279-282), then every column in place (:286-291): a column is a view of symbol stride row_n
  uint8_t* first = code + d_col * row_n;
  MZK_TRY(rs_encode_views(row_n, size, RsView{first + d_row, 1, (ptrdiff_t)row_n}, size, RsView{first, 1, (ptrdiff_t)row_n}, nullptr, s));
  return rs_encode_views(col_n, size, RsView{first, (ptrdiff_t)row_n, 1}, row_n, RsView{code, (ptrdiff_t)row_n, 1}, nullptr, s);
}

static int rs2d_decode_impl(size_t col_n, size_t row_n, const void* d_code, size_t message_len, void* d_data, int* d_ok, uint8_t* d_col_status,
                            uint8_t* d_row_status, hipStream_t s) {
  size_t size;
  MZK_TRY(rs2d_check(col_n, row_n, message_len, &size));
  if (!d_code || !d_data || !d_ok) { set_error("rs2d_decode: null pointer"); return MZK_E_ARG; }
  WsFrame ws("rs2d_decode");
  uint8_t* scratch;      // size x row_n column messages | size x size row messages | row_n + size statuses
  MZK_TRY(ws.get(WS_MISC_A, size * row_n + size * size + row_n + size, (void**)&scratch));
  uint8_t* cols = scratch;
  uint8_t* rows = cols + size * row_n;
  if (!d_col_status) d_col_status = rows + size * size;
  if (!d_row_status) d_row_status = rows + size * size + row_n;
  // every column (:299-305): message symbol i of column c at cols[i][c]; then every one of the `size` rows (:308-313)
  MZK_TRY(rs_decode_views(col_n, size, RsView{(uint8_t*)d_code, (ptrdiff_t)row_n, 1}, row_n, RsView{nullptr, 0, 0}, RsView{cols, (ptrdiff_t)row_n, 1}, d_col_status, s));
  MZK_TRY(rs_decode_views(row_n, size, RsView{cols, 1, (ptrdiff_t)row_n}, size, RsView{nullptr, 0, 0}, RsView{rows, 1, (ptrdiff_t)size}, d_row_status, s));
  hipLaunchKernelGGL(k_rs2d_finish, dim3((message_len + 255) / 256), dim3(256), 0, s, rows, message_len, (uint8_t*)d_data, d_col_status, (int)row_n, d_row_status,
                     (int)size, d_ok);
  MZK_HIP(hipGetLastError());
  return MZK_OK;
}

static int rs_stage_in(WsFrame& ws, WsSlot slot, const void* host, size_t bytes, void** dev, hipStream_t s) {
  MZK_TRY(ws.get(slot, bytes ? bytes : 16, dev));
  if (bytes) MZK_HIP(hipMemcpyAsync(*dev, host, bytes, hipMemcpyHostToDevice, s));
  return MZK_OK;
}

}  // namespace mzk

// ---- C ABI (include/mzk.h, "Reed-Solomon over GF(2^8)") ------------------------------------------------------------------------------
extern "C" {

int mzk_rs_generator_poly(size_t n, size_t k, uint8_t* g) {
  const RsPlan P = rs_plan(n, k, 1);
  if (P.err != MZK_OK) { set_error("%s", P.msg); return P.err; }
  if (!g) { set_error("rs_generator_poly: null pointer"); return MZK_E_ARG; }
  RsTables T;
  rs_tables(n, k, P.enc_pad, &T);
  memcpy(g, T.gen, (size_t)P.d + 1);
  return MZK_OK;
}

int mzk_rs_encode_view_dev(size_t n, size_t k, const void* d_messages, size_t msg_symbol_stride, size_t msg_stride, size_t batch, void* d_codewords,
                           size_t cw_symbol_stride, size_t cw_stride, void* d_columns_fr, void* stream) {
  MZK_ENTER();
  WsGuard wsg((hipStream_t)stream);
  return rs_encode_views(n, k, RsView{(uint8_t*)d_messages, (ptrdiff_t)msg_symbol_stride, (ptrdiff_t)msg_stride}, batch,
                         RsView{(uint8_t*)d_codewords, (ptrdiff_t)cw_symbol_stride, (ptrdiff_t)cw_stride}, d_columns_fr, (hipStream_t)stream);
}
int mzk_rs_encode_dev(size_t n, size_t k, const void* d_messages, size_t batch, void* d_codewords, void* d_columns_fr, void* stream) {
  return mzk_rs_encode_view_dev(n, k, d_messages, 1, k, batch, d_codewords, 1, n, d_columns_fr, stream);
}
int mzk_rs_encode(size_t n, size_t k, const uint8_t* messages, size_t batch, uint8_t* codewords) {
  MZK_ENTER();
  WsFrame ws("mzk_rs_encode");
  RsPlan P;
  MZK_TRY(rs_plan_checked(n, k, batch, &P));
  if (!messages || !codewords) { set_error("rs_encode: null pointer"); return MZK_E_ARG; }
  hipStream_t s = ctx().stream;
  WsGuard wsg(s);
  void *d_m, *d_c;
  MZK_TRY(rs_stage_in(ws, WS_MISC_B, messages, k * batch, &d_m, s));
  MZK_TRY(ws.get(WS_MISC_C, n * batch, &d_c));
  MZK_TRY(rs_encode_views(n, k, RsView{(uint8_t*)d_m, 1, (ptrdiff_t)k}, batch, RsView{(uint8_t*)d_c, 1, (ptrdiff_t)n}, nullptr, s));
  return d2h_sync(codewords, d_c, n * batch, s);
}

int mzk_rs_syndromes_dev(size_t n, size_t k, const void* d_words, size_t batch, void* d_syndromes, void* stream) {
  MZK_ENTER();
  WsGuard wsg((hipStream_t)stream);
  return rs_syndromes_views(n, k, RsView{(uint8_t*)d_words, 1, (ptrdiff_t)n}, batch, (uint8_t*)d_syndromes, (hipStream_t)stream);
}
int mzk_rs_syndromes(size_t n, size_t k, const uint8_t* words, size_t batch, uint8_t* syndromes) {
  MZK_ENTER();
  WsFrame ws("mzk_rs_syndromes");
  RsPlan P;
  MZK_TRY(rs_plan_checked(n, k, batch, &P));
  if (!words || (!syndromes && P.d)) { set_error("rs_syndromes: null pointer"); return MZK_E_ARG; }
  if (P.d == 0) return MZK_OK;
  hipStream_t s = ctx().stream;
  WsGuard wsg(s);
  void *d_w, *d_s;
  MZK_TRY(rs_stage_in(ws, WS_MISC_B, words, n * batch, &d_w, s));
  MZK_TRY(ws.get(WS_MISC_C, (size_t)P.d * batch, &d_s));
  MZK_TRY(rs_syndromes_views(n, k, RsView{(uint8_t*)d_w, 1, (ptrdiff_t)n}, batch, (uint8_t*)d_s, s));
  return d2h_sync(syndromes, d_s, (size_t)P.d * batch, s);
}

int mzk_rs_decode_dev(size_t n, size_t k, const void* d_received, size_t batch, void* d_corrected, void* d_messages, void* d_status, void* stream) {
  MZK_ENTER();
  WsGuard wsg((hipStream_t)stream);
  return rs_decode_views(n, k, RsView{(uint8_t*)d_received, 1, (ptrdiff_t)n}, batch, RsView{(uint8_t*)d_corrected, 1, (ptrdiff_t)n},
                         RsView{(uint8_t*)d_messages, 1, (ptrdiff_t)k}, (uint8_t*)d_status, (hipStream_t)stream);
}
int mzk_rs_decode(size_t n, size_t k, const uint8_t* received, size_t batch, uint8_t* corrected, uint8_t* messages, uint8_t* status) {
  MZK_ENTER();
  WsFrame ws("mzk_rs_decode");
  RsPlan P;
  MZK_TRY(rs_plan_checked(n, k, batch, &P));
  if (!received || !status) { set_error("rs_decode: null pointer"); return MZK_E_ARG; }
  hipStream_t s = ctx().stream;
  WsGuard wsg(s);
  void* d_r;
  uint8_t* d_o;      // corrected | messages | status
  MZK_TRY(rs_stage_in(ws, WS_MISC_B, received, n * batch, &d_r, s));
  MZK_TRY(ws.get(WS_MISC_C, (n + k + 1) * batch, (void**)&d_o));
  uint8_t *d_c = corrected ? d_o : nullptr, *d_m = messages ? d_o + n * batch : nullptr, *d_st = d_o + (n + k) * batch;
  MZK_TRY(rs_decode_views(n, k, RsView{(uint8_t*)d_r, 1, (ptrdiff_t)n}, batch, RsView{d_c, 1, (ptrdiff_t)n}, RsView{d_m, 1, (ptrdiff_t)k}, d_st, s));
  if (corrected) MZK_HIP(hipMemcpyAsync(corrected, d_c, n * batch, hipMemcpyDeviceToHost, s));
  if (messages) MZK_HIP(hipMemcpyAsync(messages, d_m, k * batch, hipMemcpyDeviceToHost, s));
  return d2h_sync(status, d_st, batch, s);
}

int mzk_rs2d_encode_dev(size_t col_n, size_t row_n, const void* d_data, size_t message_len, void* d_code, void* stream) {
  MZK_ENTER();
  WsGuard wsg((hipStream_t)stream);
  return rs2d_encode_impl(col_n, row_n, d_data, message_len, d_code, (hipStream_t)stream);
}
int mzk_rs2d_encode(size_t col_n, size_t row_n, const uint8_t* data, size_t message_len, uint8_t* code) {
  MZK_ENTER();
  WsFrame ws("mzk_rs2d_encode");
  size_t size;
  MZK_TRY(rs2d_check(col_n, row_n, message_len, &size));
  if (!data || !code) { set_error("rs2d_encode: null pointer"); return MZK_E_ARG; }
  hipStream_t s = ctx().stream;
  WsGuard wsg(s);
  void *d_d, *d_c;
  MZK_TRY(rs_stage_in(ws, WS_MISC_B, data, message_len, &d_d, s));
  MZK_TRY(ws.get(WS_MISC_C, col_n * row_n, &d_c));
  MZK_HIP(hipMemsetAsync(d_c, 0, col_n * row_n, s));
  MZK_TRY(rs2d_encode_impl(col_n, row_n, d_d, message_len, d_c, s));
  return d2h_sync(code, d_c, col_n * row_n, s);
}

int mzk_rs2d_decode_dev(size_t col_n, size_t row_n, const void* d_code, size_t message_len, void* d_data, int* d_ok, void* d_col_status, void* d_row_status,
                        void* stream) {
  MZK_ENTER();
  WsGuard wsg((hipStream_t)stream);
  return rs2d_decode_impl(col_n, row_n, d_code, message_len, d_data, d_ok, (uint8_t*)d_col_status, (uint8_t*)d_row_status, (hipStream_t)stream);
}
int mzk_rs2d_decode(size_t col_n, size_t row_n, const uint8_t* code, size_t message_len, uint8_t* data, int* ok, uint8_t* col_status, uint8_t* row_status) {
  MZK_ENTER();
  WsFrame ws("mzk_rs2d_decode");
  size_t size;
  MZK_TRY(rs2d_check(col_n, row_n, message_len, &size));
  if (!code || !data || !ok) { set_error("rs2d_decode: null pointer"); return MZK_E_ARG; }
  hipStream_t s = ctx().stream;
  WsGuard wsg(s);
  void* d_c;
  uint8_t* d_o;      // ok (4 bytes) | data | column statuses | row statuses
  MZK_TRY(rs_stage_in(ws, WS_MISC_B, code, col_n * row_n, &d_c, s));
  MZK_TRY(ws.get(WS_MISC_C, 4 + message_len + row_n + size, (void**)&d_o));
  uint8_t *d_d = d_o + 4, *d_cs = d_d + message_len, *d_rs = d_cs + row_n;
  MZK_TRY(rs2d_decode_impl(col_n, row_n, d_c, message_len, d_d, (int*)d_o, d_cs, d_rs, s));
  std::vector<uint8_t> back(4 + message_len + row_n + size);
  MZK_TRY(d2h_sync(back.data(), d_o, back.size(), s));
  memcpy(ok, back.data(), 4);
  memcpy(data, back.data() + 4, message_len);
  if (col_status) memcpy(col_status, back.data() + 4 + message_len, row_n);
  if (row_status) memcpy(row_status, back.data() + 4 + message_len + row_n, size);
  return MZK_OK;
}

}  // extern "C"
