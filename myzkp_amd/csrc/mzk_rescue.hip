// mzk_rescue.hip -- Rescue-Prime on the device (zkstark/rescueprime.rs): batched hashes, hash chains and their traces, ONE chain per
// lane.  A hash is n_rounds x 2 x m power chains of up to 256 bits (the reference's parameters: 27 x 2 x 2 chains of 163 + 2 products),
// every one of them the same straight-line program in every lane: the work is data-parallel field products and nothing else.  The
// per-lane code is mzk_rescue.h, the programs and the grid are decided in mzk_rescue_plan.h; this file is the kernel around them and the
// entry points.
//
// Launch shape: workgroups of one wave, lane = chain; a capped grid walks the batch in rounds.  Lanes past the end compute the last
// chain again and store nothing, so that control stays wave-uniform.  The trace of a chain is stored as it is made, one element
// (16 or 32 bytes) per lane and store, strided by the caller's trace_stride: ~0.9 KB per hash next to ~4 10^5 instructions.
#include <memory>
#include <vector>
#include "mzk_common.h"
#include "mzk_elem.h"
#include "mzk_rescue.h"

namespace mzk {

template <class P, int M> struct RsDevOut {
  u32* traces;
  u32* outs;
  size_t slot0, stride;            // first slot of the lane's chain (b * links); elements between two slots
  bool live;
  __device__ __forceinline__ void row(size_t l, u32 r, u32 i, const Fe<P>& v) const {
    if (live) fe_gstore<P>(traces, (slot0 + l) * stride + (size_t)r * M + i, v);
  }
  __device__ __forceinline__ void output(size_t l, const Fe<P>& v) const {
    if (live && outs != nullptr) fe_gstore<P>(outs, slot0 + l, v);
  }
};

template <class P, int M, bool TRACE>
__global__ __launch_bounds__(RESCUE_BLOCK) void k_rescue(RescueConsts c, const u32* __restrict__ in, size_t batch, size_t links, u32* __restrict__ traces, size_t stride,
                                                          u32* __restrict__ outs, unsigned iters) {
  const size_t wgs = (batch + RESCUE_BLOCK - 1) / RESCUE_BLOCK;
#pragma unroll 1
  for (unsigned it = 0; it < iters; it++) {
    const size_t wg = (size_t)it * gridDim.x + blockIdx.x;
    if (wg >= wgs) break;                                    // wave-uniform
    const size_t b = wg * RESCUE_BLOCK + threadIdx.x;
    const size_t bb = b < batch ? b : batch - 1;
    RsDevOut<P, M> out{traces, outs, bb * links, stride, b < batch};
    rs_chain<P, M, TRACE>(c, fe_gload<P>(in, bb), links, out);
  }
}

}  // namespace mzk

using namespace mzk;

struct mzk_rescue {
  RescuePlan plan;                 // at batch 0: the programs and the layout of the constants
  DevMem mem;                      // the constants
  // Owner: the context (and its device) whose memory holds the constants, as for a mzk_das_grid
  int ctx_index = 0;
  int device = -1;
};

namespace mzk {

struct RescueScope {
  CtxScope sc;
  int rc;
  explicit RescueScope(const mzk_rescue* h) : sc(h->ctx_index), rc(MZK_OK) {
    if (!sc.ok || ctx().device != h->device) {
      set_error("rescue handle was made on context %d (device %d); that context %s", h->ctx_index, h->device, sc.ok ? "drives another device now" : "no longer exists");
      rc = MZK_E_ARG;
    }
  }
};

static int rescue_plan_checked(int fid, size_t m, size_t n_rounds, uint64_t alpha, const uint64_t* alphainv, size_t batch, RescuePlan* P) {
  if (!alphainv) { set_error("rescue: null pointer (alphainv)"); return MZK_E_ARG; }
  *P = rescue_plan(fid, m, n_rounds, alpha, alphainv, batch);
  if (P->err != MZK_OK) { set_error("%s", P->msg); return P->err; }
  return MZK_OK;
}

// canonical host element -> Montgomery-form limbs
template <class P> static void rescue_mont_limbs(const HostField* hf, const uint64_t* v, u32* out) {
  u32 w[8];
  h_mont_words(hf, v, w);
  const Fe<P> f = fe_unpack<P>(w);
  for (int i = 0; i < P::L; i++) out[i] = f.l[i];
}

// sizes of a call, all products checked: slots = batch * links, trace elements = slots * stride
static int rescue_sizes(const mzk_rescue* h, const char* who, size_t batch, size_t links, bool trace, size_t stride, size_t* slots, size_t* trace_elems) {
  const size_t esz = field_bytes(h->plan.fid);
  *trace_elems = 0;
  if (batch > RESCUE_MAX_BATCH) { set_error("%s: batch = %zu is beyond 2^40", who, batch); return MZK_E_LENGTH; }
  if (__builtin_mul_overflow(batch, links, slots) || *slots > ((size_t)1 << 56) / esz) { set_error("%s: batch * links = %zu * %zu overflows", who, batch, links); return MZK_E_LENGTH; }
  if (trace) {
    if (stride < h->plan.min_stride) { set_error("%s: trace_stride = %zu is below (n_rounds + 1) * m = %zu", who, stride, h->plan.min_stride); return MZK_E_LENGTH; }
    if (__builtin_mul_overflow(*slots, stride, trace_elems) || *trace_elems > ((size_t)1 << 56) / esz) {
      set_error("%s: batch * links * trace_stride = %zu * %zu overflows", who, *slots, stride);
      return MZK_E_LENGTH;
    }
  }
  return MZK_OK;
}

template <class P, int M> static void rescue_launch_m(const RescueConsts& c, const RescueGrid& L, const void* d_in, size_t batch, size_t links, void* d_traces, size_t stride,
                                                      void* d_outs, hipStream_t s) {
  if (d_traces)
    hipLaunchKernelGGL((k_rescue<P, M, true>), dim3((unsigned)L.grid), dim3(RESCUE_BLOCK), 0, s, c, (const u32*)d_in, batch, links, (u32*)d_traces, stride, (u32*)d_outs, L.iters);
  else
    hipLaunchKernelGGL((k_rescue<P, M, false>), dim3((unsigned)L.grid), dim3(RESCUE_BLOCK), 0, s, c, (const u32*)d_in, batch, links, (u32*)nullptr, (size_t)0, (u32*)d_outs, L.iters);
}

// validated arguments, batch and links not zero; d_traces null: hashes only
static int rescue_run(const mzk_rescue* h, const void* d_in, size_t batch, size_t links, void* d_traces, size_t stride, void* d_outs, hipStream_t s) {
  const RescuePlan& P0 = h->plan;
  const RescueGrid L = rescue_grid(batch);      // the grid alone depends on the batch
  RescueConsts c;
  c.words = h->mem.as<u32>();
  c.prog[0] = (u32)P0.prog_off[0]; c.prog[1] = (u32)P0.prog_off[1];
  c.steps[0] = (u32)P0.alpha.steps; c.steps[1] = (u32)P0.alphainv.steps;
  c.mds = (u32)P0.mds_off; c.rc = (u32)P0.rc_off; c.n_rounds = (u32)P0.n_rounds;
  MZK_TRY(with_field(P0.fid, [&](auto tag) {
    typedef typename decltype(tag)::P P;
    switch (P0.m) {
      case 1: rescue_launch_m<P, 1>(c, L, d_in, batch, links, d_traces, stride, d_outs, s); break;
      case 2: rescue_launch_m<P, 2>(c, L, d_in, batch, links, d_traces, stride, d_outs, s); break;
      case 3: rescue_launch_m<P, 3>(c, L, d_in, batch, links, d_traces, stride, d_outs, s); break;
      default: rescue_launch_m<P, 4>(c, L, d_in, batch, links, d_traces, stride, d_outs, s); break;
    }
    return MZK_OK;
  }));
  MZK_HIP(hipGetLastError());
  return MZK_OK;
}

static int rescue_host_inputs(const mzk_rescue* h, const char* who, const uint64_t* inputs, size_t batch) {
  const HostField* hf = host_field(h->plan.fid);
  for (size_t i = 0; i < batch; i++)
    if (!h_is_canonical(hf, inputs + i * hf->nl)) { set_error("%s: inputs[%zu] not canonical", who, i); return MZK_E_RANGE; }
  return MZK_OK;
}

}  // namespace mzk

// ---- C ABI (include/mzk.h, "Rescue-Prime") -------------------------------------------------------------------------------------------------
extern "C" {

int mzk_rescue_plan_get(int field_id, size_t m, size_t n_rounds, uint64_t alpha, const uint64_t alphainv[4], size_t batch, uint64_t* plan) {
  RescuePlan P;
  MZK_TRY(rescue_plan_checked(field_id, m, n_rounds, alpha, alphainv, batch, &P));
  if (!plan) { set_error("rescue_plan: null pointer"); return MZK_E_ARG; }
  rescue_plan_export(P, plan);
  return MZK_OK;
}

int mzk_rescue_new(int field_id, size_t m, size_t n_rounds, uint64_t alpha, const uint64_t alphainv[4], const uint64_t* mds, const uint64_t* round_constants,
                   mzk_rescue** out) {
  if (!out) { set_error("rescue_new: null output handle"); return MZK_E_ARG; }
  *out = nullptr;
  RescuePlan P;
  MZK_TRY(rescue_plan_checked(field_id, m, n_rounds, alpha, alphainv, 0, &P));
  if (!mds || !round_constants) { set_error("rescue_new: null pointer"); return MZK_E_ARG; }
  const HostField* hf = host_field(field_id);
  for (size_t i = 0; i < m * m; i++)
    if (!h_is_canonical(hf, mds + i * hf->nl)) { set_error("rescue_new: mds[%zu] not canonical", i); return MZK_E_RANGE; }
  for (size_t i = 0; i < 2 * n_rounds * m; i++)
    if (!h_is_canonical(hf, round_constants + i * hf->nl)) { set_error("rescue_new: round_constants[%zu] not canonical", i); return MZK_E_RANGE; }
  MZK_ENTER();
  std::vector<u32> words(P.const_words, 0);
  for (int k = 0; k < P.alpha.steps; k++) words[P.prog_off[0] + (size_t)k] = P.alpha.prog[k];
  for (int k = 0; k < P.alphainv.steps; k++) words[P.prog_off[1] + (size_t)k] = P.alphainv.prog[k];
  with_field(field_id, [&](auto tag) {
    typedef typename decltype(tag)::P PP;
    for (size_t i = 0; i < m * m; i++) rescue_mont_limbs<PP>(hf, mds + i * hf->nl, words.data() + P.mds_off + i * (size_t)PP::L);
    for (size_t i = 0; i < 2 * n_rounds * m; i++) rescue_mont_limbs<PP>(hf, round_constants + i * hf->nl, words.data() + P.rc_off + i * (size_t)PP::L);
    return MZK_OK;
  });
  std::unique_ptr<mzk_rescue> h(new mzk_rescue());
  h->plan = P;
  h->ctx_index = ctx().index;
  h->device = ctx().device;
  MZK_TRY(h->mem.alloc(P.const_bytes, "rescue constants"));
  hipStream_t s = ctx().stream;
  MZK_HIP(hipMemcpyAsync(h->mem.get(), words.data(), P.const_bytes, hipMemcpyHostToDevice, s));
  MZK_HIP(hipStreamSynchronize(s));                          // `words` is memory of this call; the constants are complete on return
  *out = h.release();
  return MZK_OK;
}

void mzk_rescue_free(mzk_rescue* h) { delete h; }

int mzk_rescue_hash_dev(mzk_rescue* h, const void* d_inputs, size_t batch, size_t links, void* d_outputs, void* stream) {
  if (!h) { set_error("rescue_hash: null handle"); return MZK_E_ARG; }
  if (batch == 0 || links == 0) return MZK_OK;
  if (!d_inputs || !d_outputs) { set_error("rescue_hash: null pointer"); return MZK_E_ARG; }
  if (((uintptr_t)d_inputs | (uintptr_t)d_outputs) & 15) { set_error("rescue_hash: d_inputs and d_outputs must be 16-byte aligned"); return MZK_E_ARG; }
  size_t slots, te;
  MZK_TRY(rescue_sizes(h, "rescue_hash", batch, links, false, 0, &slots, &te));
  MZK_ENTER();
  RescueScope rs(h);
  MZK_TRY(rs.rc);
  return rescue_run(h, d_inputs, batch, links, nullptr, 0, d_outputs, (hipStream_t)stream);
}

int mzk_rescue_trace_dev(mzk_rescue* h, const void* d_inputs, size_t batch, size_t links, void* d_traces, size_t trace_stride, void* d_outputs, void* stream) {
  if (!h) { set_error("rescue_trace: null handle"); return MZK_E_ARG; }
  if (batch == 0 || links == 0) return MZK_OK;
  if (!d_inputs || !d_traces) { set_error("rescue_trace: null pointer"); return MZK_E_ARG; }
  if (((uintptr_t)d_inputs | (uintptr_t)d_traces | (uintptr_t)d_outputs) & 15) { set_error("rescue_trace: d_inputs, d_traces and d_outputs must be 16-byte aligned"); return MZK_E_ARG; }
  size_t slots, te;
  MZK_TRY(rescue_sizes(h, "rescue_trace", batch, links, true, trace_stride, &slots, &te));
  MZK_ENTER();
  RescueScope rs(h);
  MZK_TRY(rs.rc);
  return rescue_run(h, d_inputs, batch, links, d_traces, trace_stride, d_outputs, (hipStream_t)stream);
}

int mzk_rescue_hash(mzk_rescue* h, const uint64_t* inputs, size_t batch, size_t links, uint64_t* outputs) {
  if (!h) { set_error("rescue_hash: null handle"); return MZK_E_ARG; }
  if (batch == 0 || links == 0) return MZK_OK;
  if (!inputs || !outputs) { set_error("rescue_hash: null pointer"); return MZK_E_ARG; }
  size_t slots, te;
  MZK_TRY(rescue_sizes(h, "rescue_hash", batch, links, false, 0, &slots, &te));
  MZK_TRY(rescue_host_inputs(h, "rescue_hash", inputs, batch));
  MZK_ENTER();
  WsFrame ws("mzk_rescue_hash");
  RescueScope rs(h);
  MZK_TRY(rs.rc);
  hipStream_t s = ctx().stream;
  WsGuard wsg(s);
  const size_t esz = field_bytes(h->plan.fid);
  void *d_in, *d_out;
  MZK_TRY(ws.get(WS_MISC_A, batch * esz, &d_in));
  MZK_TRY(ws.get(WS_MISC_B, slots * esz, &d_out));
  MZK_HIP(hipMemcpyAsync(d_in, inputs, batch * esz, hipMemcpyHostToDevice, s));
  const int rc = rescue_run(h, d_in, batch, links, nullptr, 0, d_out, s);
  if (rc != MZK_OK) { (void)hipStreamSynchronize(s); return rc; }
  return d2h_sync(outputs, d_out, slots * esz, s);
}

int mzk_rescue_trace(mzk_rescue* h, const uint64_t* inputs, size_t batch, size_t links, uint64_t* traces, size_t trace_stride, uint64_t* outputs) {
  if (!h) { set_error("rescue_trace: null handle"); return MZK_E_ARG; }
  if (batch == 0 || links == 0) return MZK_OK;
  if (!inputs || !traces) { set_error("rescue_trace: null pointer"); return MZK_E_ARG; }
  size_t slots, te;
  MZK_TRY(rescue_sizes(h, "rescue_trace", batch, links, true, trace_stride, &slots, &te));
  MZK_TRY(rescue_host_inputs(h, "rescue_trace", inputs, batch));
  MZK_ENTER();
  WsFrame ws("mzk_rescue_trace");
  RescueScope rs(h);
  MZK_TRY(rs.rc);
  hipStream_t s = ctx().stream;
  WsGuard wsg(s);
  const size_t esz = field_bytes(h->plan.fid), dense = h->plan.min_stride;
  void *d_in, *d_out, *d_tr;
  MZK_TRY(ws.get(WS_MISC_A, batch * esz, &d_in));
  MZK_TRY(ws.get(WS_MISC_B, slots * esz, &d_out));
  MZK_TRY(ws.get(WS_MISC_C, slots * dense * esz, &d_tr));       // dense on the device; the caller's stride is applied on the way back
  MZK_HIP(hipMemcpyAsync(d_in, inputs, batch * esz, hipMemcpyHostToDevice, s));
  const int rc = rescue_run(h, d_in, batch, links, d_tr, dense, d_out, s);
  if (rc != MZK_OK) { (void)hipStreamSynchronize(s); return rc; }
  // only the rows travel: what the caller keeps behind them in a slot stays as it is
  if (hipMemcpy2DAsync(traces, trace_stride * esz, d_tr, dense * esz, dense * esz, slots, hipMemcpyDeviceToHost, s) != hipSuccess) {
    (void)hipGetLastError();
    (void)hipStreamSynchronize(s);
    set_error("rescue_trace: copying the traces back failed");
    return MZK_E_HIP;
  }
  if (outputs) return d2h_sync(outputs, d_out, slots * esz, s);
  MZK_HIP(hipStreamSynchronize(s));
  return MZK_OK;
}

}  // extern "C"
