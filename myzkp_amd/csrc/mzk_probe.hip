// mzk_probe.hip -- the device side of the arithmetic probe (mzk_probe.h): mzk_selftest_field_probe / mzk_selftest_g1_probe /
// mzk_selftest_g2_probe.
// One kernel per (field, op, form): a probe kernel holds one device function and its loads and stores, so what it compiles to is
// that function under no other register pressure, and a failure names the operation and the form.  Operands come from the host as
// raw limbs and go back as raw limbs; tests/test_gpu_arith_probe.py judges them against the integer model of tests/arith_model.py.
#include "mzk_common.h"
#include "mzk_probe.h"
#include "mzk_coop.h"
#include "mzk_row.h"
#include "mzk_affine_wave.h"

namespace mzk {

// the forms a field op exists in: portable everywhere; asm for the products that mzk_field_asm.h generates; the wave-cooperative
// inversion for Fq (mzk_inv_wave.h)
template <class P> constexpr bool probe_field_form_ok(int op, int form) {
  if (!probe_field_has<P>(op)) return false;
  if (form == PR_FORM_CPP) return true;
  if (form == PR_FORM_ASM) return op == PR_MUL || op == PR_SQR || op == PR_MUL_ADD2 || op == PR_SHOUP_MUL || op == PR_SMUL;
  if (form == PR_FORM_WAVE) return op == PR_INV && P::L == 9 && P::P[0] == FqParams::P[0];
  return false;
}

// one thread per case.  The precomputed-quotient product takes w, wq from the FIRST lane of the wave through readfirstlane, as
// the transform holds them (scalar registers: the asm form's "s" operands): the 64 cases of a wave share one constant pair.
template <class P, int OP, int FORM>
__global__ __launch_bounds__(256) void k_probe_field(size_t n, const u32* __restrict__ in, u32* __restrict__ out) {
  constexpr int L = P::L, AR = probe_field_arity(OP);
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  u32 x[AR * L], r[L];
#pragma unroll
  for (int k = 0; k < AR * L; k++) x[k] = in[i * (AR * L) + k];
  if constexpr (OP == PR_SHOUP_MUL) {
#pragma unroll
    for (int k = L; k < 3 * L; k++) x[k] = (u32)__builtin_amdgcn_readfirstlane((int)x[k]);
  }
  if constexpr (FORM == PR_FORM_CPP) {
    probe_field_cpp<P, OP>(x, r);
  } else {
    const Fe<P> a = probe_ld<P>(x);
    if constexpr (OP == PR_MUL) probe_st<P>(FeAsm<P>::mul(a, probe_ld<P>(x + L)), r);
    else if constexpr (OP == PR_SQR) probe_st<P>(FeAsm<P>::sqr(a), r);
    else if constexpr (OP == PR_MUL_ADD2) probe_st<P>(FeAsm<P>::mul_add2(a, probe_ld<P>(x + L), probe_ld<P>(x + 2 * L), probe_ld<P>(x + 3 * L)), r);
    else if constexpr (OP == PR_SHOUP_MUL) probe_st<P>(FeAsm<P>::shoup_mul(a, x + L, x + 2 * L), r);
    else if constexpr (OP == PR_SMUL) probe_st<P>(FeAsm<P>::smul(a, probe_ld<P>(x + L)), r);
  }
#pragma unroll
  for (int k = 0; k < L; k++) out[i * L + k] = r[k];
}
// invw::inv: one value per wave, every lane active (a ragged tail repeats the last case), lane 0 stores
template <class P>
__global__ __launch_bounds__(256) void k_probe_inv_wave(size_t n, const u32* __restrict__ in, u32* __restrict__ out) {
  constexpr int L = P::L;
  size_t i = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const bool tail = i >= n;
  if (tail) i = n - 1;
  u32 x[L];
#pragma unroll
  for (int k = 0; k < L; k++) x[k] = in[i * L + k];
  const Fe<P> r = invw::inv<P>(probe_ld<P>(x));
  if (!tail && (threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < L; k++) out[i * L + k] = r.l[k];
  }
}

template <class P, int FORM, int OP = 0>
static int probe_field_launch(int op, size_t n, const u32* in, u32* out, hipStream_t s) {
  if constexpr (OP == PR_FIELD_OPS) {
    return MZK_E_ARG;
  } else {
    if (op != OP) return probe_field_launch<P, FORM, OP + 1>(op, n, in, out, s);
    if constexpr (!probe_field_form_ok<P>(OP, FORM)) {
      return MZK_E_ARG;
    } else if constexpr (FORM == PR_FORM_WAVE) {
      hipLaunchKernelGGL(k_probe_inv_wave<P>, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, s, n, in, out);
      return MZK_OK;
    } else {
      hipLaunchKernelGGL((k_probe_field<P, OP, FORM>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, n, in, out);
      return MZK_OK;
    }
  }
}
template <class P> static int probe_field_forms(int op, int form, size_t n, const u32* in, u32* out, hipStream_t s) {
  if (form == PR_FORM_CPP) return probe_field_launch<P, PR_FORM_CPP>(op, n, in, out, s);
  if (form == PR_FORM_ASM) return probe_field_launch<P, PR_FORM_ASM>(op, n, in, out, s);
  if (form == PR_FORM_WAVE) return probe_field_launch<P, PR_FORM_WAVE>(op, n, in, out, s);
  return MZK_E_ARG;
}

int selftest_field_probe_arity(int fid, int op, int form, int* limbs) {
  int arity = 0;      // stays 0 for an unknown id: both callers report that in their own words
  (void)with_field3(fid, [&](auto tag) -> int {
    typedef typename decltype(tag)::P P;
    *limbs = P::L;
    if (probe_field_form_ok<P>(op, form)) arity = probe_field_arity(op);
    return MZK_OK;
  });
  return arity;
}
int selftest_field_probe_impl(int fid, int op, int form, size_t n, const uint32_t* in_host, uint32_t* out_host, hipStream_t s) {
  WsFrame ws("selftest_field_probe_impl");
  int L = 0;
  const int ar = selftest_field_probe_arity(fid, op, form, &L);
  if (ar == 0) { set_error("field_probe: no field %d / op %d / form %d", fid, op, form); return MZK_E_ARG; }
  if (n == 0) return MZK_OK;
  const size_t in_bytes = n * (size_t)ar * L * 4, out_bytes = n * (size_t)L * 4;
  void *din, *dout;
  MZK_TRY(ws.get(WS_MISC_A, in_bytes, &din));
  MZK_TRY(ws.get(WS_MISC_B, out_bytes, &dout));
  MZK_HIP(hipMemcpyAsync(din, in_host, in_bytes, hipMemcpyHostToDevice, s));
  MZK_HIP(hipMemsetAsync(dout, 0, out_bytes, s));
  MZK_TRY(with_field3(fid, [&](auto tag) { return probe_field_forms<typename decltype(tag)::P>(op, form, n, (const u32*)din, (u32*)dout, s); }));
  MZK_HIP(hipGetLastError());
  MZK_HIP(hipMemcpyAsync(out_host, dout, out_bytes, hipMemcpyDeviceToHost, s));
  MZK_HIP(hipStreamSynchronize(s));
  return MZK_OK;
}

// ---- group law ---------------------------------------------------------------------------------------------------------------
// single-lane forms (FeCpp / FeAsm products): one thread per case
template <int OP, template <class> class A>
__global__ __launch_bounds__(256) void k_probe_g1_lane(size_t n, const u32* __restrict__ a, const u32* __restrict__ b, const uint8_t* __restrict__ neg,
                                                        u32* __restrict__ out) {
  constexpr int AW = OP == PR_G1_DBL_AFFINE ? PR_AFF : PR_SLOT;
  constexpr int BW = OP == PR_G1_ADD ? PR_SLOT : (OP == PR_G1_MADD || OP == PR_G1_MADD_SIGNED) ? PR_AFF : 0;
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  u32 x[AW], y[BW ? BW : 1], r[PR_SLOT];
#pragma unroll
  for (int k = 0; k < AW; k++) x[k] = a[i * AW + k];
#pragma unroll
  for (int k = 0; k < BW; k++) y[k] = b[i * BW + k];
  bool ng = false;
  if constexpr (OP == PR_G1_MADD_SIGNED) ng = neg[i] != 0;
  probe_g1_lane<OP, A>(x, y, ng, r);
#pragma unroll
  for (int k = 0; k < PR_SLOT; k++) out[i * PR_SLOT + k] = r[k];
}
// quad forms (mzk_coop.h): one case per DPP quad, operands replicated in its four lanes.  Every lane of the wave stays active and
// control flow is wave-uniform (a DPP read of a disabled lane returns 0; xyzz_add_quad ballots): a ragged tail repeats the last case.
template <int OP>
__global__ __launch_bounds__(256) void k_probe_g1_quad(size_t n, const u32* __restrict__ a, const u32* __restrict__ b, u32* __restrict__ out) {
  size_t i = (size_t)blockIdx.x * 64 + (threadIdx.x >> 2);
  const int lane = (int)(threadIdx.x & 3);
  const bool tail = i >= n;
  if (tail) i = n - 1;
  u32 x[PR_SLOT], y[PR_SLOT], r[PR_SLOT];
#pragma unroll
  for (int k = 0; k < PR_SLOT; k++) { x[k] = a[i * PR_SLOT + k]; y[k] = (OP == PR_G1_ADD) ? b[i * PR_SLOT + k] : 0u; }
  Xyzz o;
  if constexpr (OP == PR_G1_ADD) o = xyzz_add_quad(probe_ld_slot(x), probe_ld_slot(y), lane);
  else o = xyzz_dbl_quad(probe_ld_slot(x), lane);
  probe_st_slot(o, r);
  // every lane of the quad holds the result: lane k writes limbs k, k + 4, ... so that a lane that disagrees shows in the slot
  if (!tail) {
#pragma unroll
    for (int k = 0; k < PR_SLOT; k++) if ((k & 3) == lane) out[i * PR_SLOT + k] = r[k];
  }
}
// row forms (mzk_row.h) and the wave conversion (mzk_affine_wave.h): one case per wave, through the packed 4 x 8-word records
// their loads and stores define (as k_rowtest_run): the raw slot is re-cut into 32-bit words (fe_pack: bit re-slicing of
// normalised limbs below 2^256, no reduction) in LDS, the result record is re-cut back into limbs.
template <int OP>
__global__ __launch_bounds__(256) void k_probe_g1_wave(size_t n, const u32* __restrict__ a, const u32* __restrict__ b, u32* __restrict__ out) {
  __shared__ u32 sh[4][3][32];
  const int wv = (int)(threadIdx.x >> 6), lane = (int)(threadIdx.x & 63);
  size_t i = (size_t)blockIdx.x * 4 + wv;
  const bool tail = i >= n;
  if (tail) i = n - 1;
  if (lane < 8) {
    const int src = lane >> 2, c = lane & 3;         // lanes 0..3: coordinates of a, 4..7: of b
    const u32* g = (src ? b : a) + i * PR_SLOT + 9 * c;
    u32 w[8];
    if (src == 0 || OP == PR_G1_ADD) {
      fe_pack<FqParams>(probe_ld<FqParams>(g), w);
      for (int k = 0; k < 8; k++) sh[wv][src][8 * c + k] = w[k];
    }
  }
  if (lane < 32) sh[wv][2][lane] = 0;
  __syncthreads();
  if constexpr (OP == PR_G1_TO_AFFINE) {
    wave_store_affine(sh[wv][0], sh[wv][2]);
    __syncthreads();
    if (!tail && lane < PR_SLOT) out[i * PR_SLOT + lane] = lane < 16 ? sh[wv][2][lane] : 0u;
  } else {
    const rowop::Lane ln = rowop::lane_init();
    const rowop::Pt x = rowop::load(sh[wv][0], ln);
    rowop::Pt r;
    if constexpr (OP == PR_G1_ADD) r = rowop::add(x, rowop::load(sh[wv][1], ln), ln);
    else r = rowop::dbl(x, ln);
    rowop::store(sh[wv][2], r, ln);
    __syncthreads();
    if (!tail && lane < 4) {
      const Fq c = fe_unpack<FqParams>(&sh[wv][2][8 * lane]);
      for (int k = 0; k < 9; k++) out[i * PR_SLOT + 9 * lane + k] = c.l[k];
    }
  }
}

static bool probe_g1_form_ok(int op, int form) {
  if (op < 0 || op >= PR_G1_OPS) return false;
  if (op == PR_G1_DBL_AFFINE) return form == PR_FORM_CPP;
  if (op == PR_G1_TO_AFFINE) return form == PR_FORM_CPP || form == PR_FORM_WAVE;
  if (form == PR_FORM_CPP || form == PR_FORM_ASM) return true;
  return (op == PR_G1_ADD || op == PR_G1_DBL) && (form == PR_FORM_QUAD || form == PR_FORM_ROW);
}
int selftest_g1_probe_check(int op, int form, int* a_words, int* b_words) {
  if (!probe_g1_form_ok(op, form)) return MZK_E_ARG;
  *a_words = op == PR_G1_DBL_AFFINE ? PR_AFF : PR_SLOT;
  *b_words = op == PR_G1_ADD ? PR_SLOT : (op == PR_G1_MADD || op == PR_G1_MADD_SIGNED) ? PR_AFF : 0;
  return MZK_OK;
}
template <int OP> static void probe_g1_lane_launch(int form, size_t n, const u32* a, const u32* b, const uint8_t* neg, u32* out, hipStream_t s) {
  const dim3 grid((unsigned)((n + 255) / 256)), block(256);
  if (form == PR_FORM_ASM) hipLaunchKernelGGL((k_probe_g1_lane<OP, FeAsm>), grid, block, 0, s, n, a, b, neg, out);
  else hipLaunchKernelGGL((k_probe_g1_lane<OP, FeCpp>), grid, block, 0, s, n, a, b, neg, out);
}
int selftest_g1_probe_impl(int op, int form, size_t n, const uint32_t* a_host, const uint32_t* b_host, const uint8_t* neg_host, uint32_t* out_host,
                           hipStream_t s) {
  WsFrame ws("selftest_g1_probe_impl");
  int aw = 0, bw = 0;
  if (selftest_g1_probe_check(op, form, &aw, &bw) != MZK_OK) { set_error("g1_probe: no op %d / form %d", op, form); return MZK_E_ARG; }
  if (n == 0) return MZK_OK;
  void *da, *db, *dn, *dout;
  const size_t out_bytes = n * (size_t)PR_SLOT * 4;
  MZK_TRY(ws.get(WS_MISC_A, n * (size_t)aw * 4, &da));
  MZK_TRY(ws.get(WS_MISC_B, n * (size_t)(bw ? bw : 1) * 4, &db));
  MZK_TRY(ws.get(WS_MISC_C, n, &dn));
  MZK_TRY(ws.get(WS_MISC_D, out_bytes, &dout));
  MZK_HIP(hipMemcpyAsync(da, a_host, n * (size_t)aw * 4, hipMemcpyHostToDevice, s));
  if (bw) MZK_HIP(hipMemcpyAsync(db, b_host, n * (size_t)bw * 4, hipMemcpyHostToDevice, s));
  if (op == PR_G1_MADD_SIGNED) MZK_HIP(hipMemcpyAsync(dn, neg_host, n, hipMemcpyHostToDevice, s));
  MZK_HIP(hipMemsetAsync(dout, 0, out_bytes, s));
  const u32 *A = (const u32*)da, *B = (const u32*)db;
  u32* O = (u32*)dout;
  if (form == PR_FORM_QUAD) {
    const dim3 grid((unsigned)((n + 63) / 64)), block(256);
    if (op == PR_G1_ADD) hipLaunchKernelGGL(k_probe_g1_quad<PR_G1_ADD>, grid, block, 0, s, n, A, B, O);
    else hipLaunchKernelGGL(k_probe_g1_quad<PR_G1_DBL>, grid, block, 0, s, n, A, B, O);
  } else if (form == PR_FORM_ROW || form == PR_FORM_WAVE) {
    const dim3 grid((unsigned)((n + 3) / 4)), block(256);
    if (op == PR_G1_ADD) hipLaunchKernelGGL(k_probe_g1_wave<PR_G1_ADD>, grid, block, 0, s, n, A, B, O);
    else if (op == PR_G1_DBL) hipLaunchKernelGGL(k_probe_g1_wave<PR_G1_DBL>, grid, block, 0, s, n, A, B, O);
    else hipLaunchKernelGGL(k_probe_g1_wave<PR_G1_TO_AFFINE>, grid, block, 0, s, n, A, B, O);
  } else {
    const uint8_t* N = (const uint8_t*)dn;
    switch (op) {
      case PR_G1_MADD_SIGNED: probe_g1_lane_launch<PR_G1_MADD_SIGNED>(form, n, A, B, N, O, s); break;
      case PR_G1_MADD: probe_g1_lane_launch<PR_G1_MADD>(form, n, A, B, N, O, s); break;
      case PR_G1_ADD: probe_g1_lane_launch<PR_G1_ADD>(form, n, A, B, N, O, s); break;
      case PR_G1_DBL: probe_g1_lane_launch<PR_G1_DBL>(form, n, A, B, N, O, s); break;
      case PR_G1_DBL_AFFINE: probe_g1_lane_launch<PR_G1_DBL_AFFINE>(PR_FORM_CPP, n, A, B, N, O, s); break;
      default: probe_g1_lane_launch<PR_G1_TO_AFFINE>(PR_FORM_CPP, n, A, B, N, O, s); break;
    }
  }
  MZK_HIP(hipGetLastError());
  MZK_HIP(hipMemcpyAsync(out_host, dout, out_bytes, hipMemcpyDeviceToHost, s));
  MZK_HIP(hipStreamSynchronize(s));
  return MZK_OK;
}

// ---- G2 (mzk_g2.h) -------------------------------------------------------------------------------------------------------------
// one thread per case, 64 per workgroup like the G2 kernels of mzk_g2.hip (the group law over Fq2 wants the whole register file)
template <int OP>
__global__ __launch_bounds__(64) void k_probe_g2_lane(size_t n, const u32* __restrict__ a, const u32* __restrict__ b, const u32* __restrict__ k,
                                                       u32* __restrict__ out) {
  constexpr int AW = probe_g2_a_words(OP), BW = probe_g2_b_words(OP), KW = probe_g2_k_words(OP), OW = probe_g2_out_words(OP);
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  u32 x[AW], y[BW ? BW : 1], kk[KW ? KW : 1], r[OW];
  for (int j = 0; j < AW; j++) x[j] = a[i * AW + j];
  for (int j = 0; j < BW; j++) y[j] = b[i * BW + j];
  for (int j = 0; j < KW; j++) kk[j] = k[i * KW + j];
  probe_g2_lane<OP>(x, y, kk, r);
  for (int j = 0; j < OW; j++) out[i * OW + j] = r[j];
}
template <int OP = 0> static void probe_g2_launch(int op, size_t n, const u32* a, const u32* b, const u32* k, u32* out, hipStream_t s) {
  if constexpr (OP < PR_G2_OPS) {
    if (op != OP) return probe_g2_launch<OP + 1>(op, n, a, b, k, out, s);
    hipLaunchKernelGGL(k_probe_g2_lane<OP>, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, s, n, a, b, k, out);
  }
}
static int selftest_g2_probe_impl(int op, size_t n, const uint32_t* a_host, const uint32_t* b_host, const uint32_t* k_host, uint32_t* out_host, hipStream_t s) {
  WsFrame ws("selftest_g2_probe_impl");
  const size_t aw = probe_g2_a_words(op), bw = probe_g2_b_words(op), kw = probe_g2_k_words(op), ow = probe_g2_out_words(op);
  void *da, *db, *dk, *dout;
  MZK_TRY(ws.get(WS_MISC_A, n * aw * 4, &da));
  MZK_TRY(ws.get(WS_MISC_B, n * (bw ? bw : 1) * 4, &db));
  MZK_TRY(ws.get(WS_MISC_C, n * (kw ? kw : 1) * 4, &dk));
  MZK_TRY(ws.get(WS_MISC_D, n * ow * 4, &dout));
  MZK_HIP(hipMemcpyAsync(da, a_host, n * aw * 4, hipMemcpyHostToDevice, s));
  if (bw) MZK_HIP(hipMemcpyAsync(db, b_host, n * bw * 4, hipMemcpyHostToDevice, s));
  if (kw) MZK_HIP(hipMemcpyAsync(dk, k_host, n * kw * 4, hipMemcpyHostToDevice, s));
  MZK_HIP(hipMemsetAsync(dout, 0, n * ow * 4, s));
  probe_g2_launch(op, n, (const u32*)da, (const u32*)db, (const u32*)dk, (u32*)dout, s);
  MZK_HIP(hipGetLastError());
  MZK_HIP(hipMemcpyAsync(out_host, dout, n * ow * 4, hipMemcpyDeviceToHost, s));
  MZK_HIP(hipStreamSynchronize(s));
  return MZK_OK;
}

}  // namespace mzk

using namespace mzk;
extern "C" int mzk_selftest_g2_probe(int op, size_t n, const uint32_t* a, const uint32_t* b, const uint32_t* k, uint32_t* out) {
  MZK_ENTER();
  if (op < 0 || op >= PR_G2_OPS) { set_error("g2_probe: no op %d", op); return MZK_E_ARG; }
  if (!a || !out || (probe_g2_b_words(op) && !b) || (probe_g2_k_words(op) && !k) || n > ((size_t)1 << 20)) {
    set_error("g2_probe: null pointer or more than 2^20 cases");
    return MZK_E_ARG;
  }
  if (n == 0) return MZK_OK;
  WsGuard wsg(ctx().stream);
  return selftest_g2_probe_impl(op, n, a, b, k, out, ctx().stream);
}
