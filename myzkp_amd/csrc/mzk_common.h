// mzk_common.h -- process context, error reporting, workspace and host-side parameter math shared by
// the library's translation units.  One process drives one GPU (one rank per GPU under torch.distributed).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include <stdio.h>
#include <string.h>
#include <functional>
#include <string>
#include <vector>
#include "../../include/mzk.h"
#include "mzk_field.h"
#include "mzk_hostfield.h"
#include "mzk_msm_plan.h"
#include "mzk_srs_plan.h"
#include "mzk_ws.h"

namespace mzk {

// ---- tuning switches --------------------------------------------------------------------------------
// The SHIPPED library reads no environment variable: a caller's environment must not be able to change the code path.  The switches of
// tools/timing exist only in the tuning build (python -m myzkp_amd.build --tuning -> myzkp_amd/libmzk_hip_tuning.so, compiled with
// -DMZK_TUNING, loaded through MZK_HIP_LIB); there tune_int reads MZK_<NAME>, here it is the constant default.
#ifdef MZK_TUNING
#include <stdlib.h>
static inline int tune_int(const char* name, int dflt) { const char* v = getenv(name); return v ? atoi(v) : dflt; } static inline const char* tune_str(const char* name) { return getenv(name); }
#else
static inline constexpr int tune_int(const char*, int dflt) { return dflt; }
static inline constexpr const char* tune_str(const char*) { return nullptr; }
#endif

// ---- error plumbing ------------------------------------------------------------------------------
void set_error(const char* fmt, ...);
int hip_fail(hipError_t e, const char* what, const char* file, int line);
#define MZK_HIP(x)                                                        \
  do {                                                                    \
    hipError_t _e = (x);                                                  \
    if (_e != hipSuccess) return mzk::hip_fail(_e, #x, __FILE__, __LINE__); \
  } while (0)
#define MZK_TRY(x)        \
  do {                    \
    int _rc = (x);        \
    if (_rc != MZK_OK) return _rc; \
  } while (0)

// ---- contexts -----------------------------------------------------------------------------------------
// A context = (device ordinal, library-owned stream, grow-only workspace, cached tables).  mzk_init creates one;
// mzk_init_devices creates one per listed ordinal (duplicates allowed: several contexts may share one GPU, which is
// how the multi-GPU path is exercised on a one-GPU box).  Every entry point works on the CURRENT context
// (mzk_ctx_select; context 0 after init); the *_multi entry points walk all of them.
enum AttrFlag { ATTR_FINE_SCATTER4 = 0, ATTR_FINE_SCATTER8, ATTR_DIGITS_LDS, ATTR_SMALL_MSM, ATTR_NTT_LARGE_FR, ATTR_NTT_LARGE_M128, ATTR_NTT_LARGE_M128_2WG, ATTR_MANY_SORT1, ATTR_TAIL_ROW, ATTR_COARSE_STAGED4, ATTR_COARSE_STAGED8, ATTR_FINE_SORT, ATTR_COUNT };
struct Context {
  bool ready = false;
  int index = 0;                 // position in the context table (keys the per-context caches of the other translation units)
  int device = -1;
  int num_cu = 256;
  hipStream_t stream = nullptr;  // library-owned stream for the host-buffer entry points
  WsTable ws;                    // scratch slots, cache slots and their generation (mzk_ws.h)
  // Stream-order guard of the shared workspace: ws_last = stream of the last entry point; an entry point on another
  // stream records ws_event on ws_last and waits for it before touching the slots (WsGuard).
  hipEvent_t ws_event = nullptr;
  hipEvent_t fork_event = nullptr, join_event = nullptr;     // mzk_kzg_commit_srs_batch_dev: caller stream -> lanes -> caller stream
  int lanes_in_flight = 1;       // > 1 while run_in_flight (mzk_api.hip) enqueues a job here that runs beside the other lanes' jobs
  hipStream_t ws_last = nullptr;
  bool ws_used = false;
  bool attr_done[ATTR_COUNT] = {};   // hipFuncSetAttribute(MaxDynamicSharedMemorySize) applied on this context's device
  // mzk_ntt_multi's all-to-all: destination context pulls its chunk of every source on a stream of its own per source
  // (created on first use), so all inbound xGMI links of the GPU carry data at once; xready orders them behind the
  // context's stream, xdone[k] joins them back.
  hipStream_t xstream[MZK_MAX_CTX] = {};
  hipEvent_t xdone[MZK_MAX_CTX] = {};
  hipEvent_t xready = nullptr;
  void* bounce = nullptr;        // SMALL_D2H_MAX bytes of pinned host memory: the landing zone of d2h_sync's small results
};
// Result of a call -> host memory, and wait: the stream is idle on return.  A commitment, a Merkle root, a handful of lengths are 32-128
// bytes, and hipMemcpyAsync into PAGEABLE memory costs ~12 us more than the same copy into pinned memory before the synchronize returns
// (tools/microbench/root_mailbox.hip: 73.8 against 63.6 us around a 50-us kernel; a host-mapped mailbox the host polls saves 4 more and was
// not worth its moving parts) -- per FRI round, per small commitment.  Up to SMALL_D2H_MAX bytes land in the context's pinned buffer and
// are copied on from there; larger results go straight to the caller's buffer as before (56 GB/s either way).
constexpr size_t SMALL_D2H_MAX = 4096;
int d2h_sync(void* host, const void* dev, size_t bytes, hipStream_t s);
// peer access between the devices of two contexts: 1 = enabled (or same device), 0 = the runtime refused (copies then stage
// through the host inside hipMemcpyPeerAsync; still correct)
int ctx_peer_enabled(int a, int b);
// One host thread at a time (include/mzk.h): every entry point that touches contexts, workspaces or caches starts with
// MZK_ENTER().  A second THREAD arriving while a call is in progress gets MZK_E_BUSY before any state is read; nested calls on
// the owning thread (entry points calling entry points, callbacks calling back in) pass.
struct EntryGuard {
  bool ok;
  bool nested;      // this thread was already inside a call (an entry point calling an entry point, a callback calling back in)
  EntryGuard();
  ~EntryGuard();
};
#define MZK_ENTER()                        \
  mzk::EntryGuard _mzk_entry;              \
  if (!_mzk_entry.ok) return MZK_E_BUSY;   \
  MZK_TRY(mzk::ensure_init())
Context& ctx();
int ctx_count();
int ctx_select(int index);       // hipSetDevice + make it current
int ensure_init();
// Makes context `index` current for a scope and restores the previous context AND the caller's HIP device on exit
// (torch keeps its own idea of the current device).
struct CtxScope {
  int prev_ctx, prev_dev; bool ok;
  explicit CtxScope(int index);
  ~CtxScope();
};

// Device scratch of the current context: WsFrame leases, ws_cache_get, ws_trim_idle, dev_alloc -- all in mzk_ws.h.
// Put one at the top of every entry point that enqueues work using workspace slots on stream s.
struct WsGuard {
  hipStream_t s;
  explicit WsGuard(hipStream_t s_);
  ~WsGuard();
};

// ---- per-phase timing (no-ops unless mzk_prof_enable(1)) ---------------------------------------------
void prof_begin(hipStream_t s, int phase);
void prof_end(hipStream_t s, int phase);
struct ProfScope {
  hipStream_t s; int ph;
  ProfScope(hipStream_t s_, int ph_) : s(s_), ph(ph_) { prof_begin(s, ph); }
  ~ProfScope() { prof_end(s, ph); }
};

// ---- host parameter math: mzk_hostfield.h.  The reference's two assertions on a root and its order as an entry point's refusal:
static inline int root_check(const HostField* f, const uint64_t* root, size_t root_order) {
  const char* msg;
  const int rc = h_root_check(f, root, root_order, &msg);
  if (rc != MZK_OK) set_error("%s", msg);
  return rc;
}

static inline bool is_pow2(size_t n) { return n && !(n & (n - 1)); }
static inline unsigned ilog2(size_t n) { unsigned l = 0; while (((size_t)1 << l) < n) l++; return l; }   // ceil(log2 n); 0 for n <= 1

// field_is_gl, field_gl_comps, field_words, field_limbs64, field_bytes: the element shapes per field id, in mzk_hostfield.h
static inline unsigned field_max_log(int fid) { return fid == MZK_FIELD_FR ? 28 : 32; }   // mzk.h "Size limits"

// ---- field id -> template instantiation ---------------------------------------------------------------
// The ONE place that knows which field id selects which parameter set.  field_check / field_check_ntt are the argument checks of
// the Fr / M128 entry points (fq_too: Fq passes as well): MZK_OK, or MZK_E_ARG with "<who>: bad field id <id>" /
// "<who>: field id <id> has no NTT on this path".
int field_check(int fid, const char* who, bool fq_too = false);
int field_check_ntt(int fid, const char* who);
// with_field(fid, f) returns f(FieldTag<FrParams or M128Params>()); f is a generic lambda that names the parameter set as
// `typename decltype(tag)::P` (word-count templates take P::NW) and returns int.  An id that is neither is an error here, never Fr's
// kernels -- callers have validated theirs, so that is a bug's landing place, not a path.
template <class P_> struct FieldTag { typedef P_ P; };
template <class F> static inline int with_field(int fid, F&& f) {
  if (fid == MZK_FIELD_M128) return f(FieldTag<M128Params>());
  if (fid == MZK_FIELD_FR) return f(FieldTag<FrParams>());
  return field_check(fid, "with_field");
}
// The Goldilocks ids select no parameter set but a coefficient count: with_gl(fid, f) returns f(GlTag<1>()) for MZK_FIELD_M64 and
// f(GlTag<3>()) for MZK_FIELD_M64X3 (kernels take decltype(tag)::NC).  field_check_gl is the argument check of the entry points
// that serve the Goldilocks ids next to Fr / M128 (transforms, coset LDE, fold, the unsigned Merkle and FRI commit calls); every
// other call keeps field_check and so keeps refusing them in its present words.
template <int NC_> struct GlTag { static constexpr int NC = NC_; };
template <class F> static inline int with_gl(int fid, F&& f) {
  if (fid == MZK_FIELD_M64) return f(GlTag<1>());
  if (fid == MZK_FIELD_M64X3) return f(GlTag<3>());
  return field_check(fid, "with_gl");
}
static inline int field_check_gl(int fid, const char* who) { return field_is_gl(fid) ? MZK_OK : field_check(fid, who); }
// ... and Fq as well (synthetic data, self-tests, probes)
template <class F> static inline int with_field3(int fid, F&& f) {
  if (fid == MZK_FIELD_FR) return f(FieldTag<FrParams>());
  if (fid == MZK_FIELD_FQ) return f(FieldTag<FqParams>());
  if (fid == MZK_FIELD_M128) return f(FieldTag<M128Params>());
  return field_check(fid, "with_field", true);
}
// One launch of kernel<P> (or kernel<P::NW>) for the field: the arguments after the kernel are hipLaunchKernelGGL's.
#define MZK_FIELD_LAUNCH(fid, kernel, ...) \
  mzk::with_field(fid, [&](auto tag_) { typedef typename decltype(tag_)::P P; hipLaunchKernelGGL((kernel), __VA_ARGS__); return MZK_OK; })

// ---- entry points implemented per translation unit ------------------------------------------------
int ntt_dev_impl(int fid, const uint64_t* root_host, const void* d_in, void* d_out, size_t n, int inverse,
                 const uint64_t* extra_scale_host, hipStream_t s);
int ntt_batch_dev_impl(int fid, const uint64_t* root_host, const void* d_in, void* d_out, size_t n, size_t batch, int inverse, hipStream_t s);
int coset_lde_dev_impl(int fid, const void* d_coef, size_t n_coef, const uint64_t* offset_host,
                       const uint64_t* generator_host, void* d_out, size_t order, hipStream_t s, size_t batch = 1);
int ntt_columns_dev_impl(int fid, const uint64_t* root_host, const void* d_in, void* d_out, size_t n_points, size_t cols, int inverse, hipStream_t s);
int transpose_elems_dev_impl(int fid, const void* d_in, void* d_out, size_t rows, size_t cols, hipStream_t s);
int poly_scale_dev_impl(int fid, const void* d_in, size_t n, const uint64_t* ratio_host, const uint64_t* lead_host, void* d_out, hipStream_t s);
int coset_divide_dev_impl(int fid, const void* d_lhs, size_t tl, const void* d_rhs, size_t tr, const uint64_t* offset_host,
                          const uint64_t* root_host, size_t order, void* d_out, hipStream_t s);
// Trimmed length (1 + index of the last non-zero coefficient among the lens[i] given) of `count` rows `stride` elements apart, plus --
// when d_extra is not null -- of one more vector of extra_len elements elsewhere (out_lens[count]), into host memory, in ONE launch and
// one wait.  clear_to != 0: elements [lens[i], clear_to) of every row are zeroed in the same pass (d_rows is written only then).
// Workspace: `slot` alone, leased from the caller's frame (the caller reads nothing of it, but it is the caller that names it).
int rows_trimmed_len_dev(int fid, void* d_rows, size_t stride, const size_t* lens, size_t count, size_t clear_to, const void* d_extra, size_t extra_len,
                         WsFrame& ws, WsSlot slot, size_t* out_lens, hipStream_t s);
// coset_divide_dev_impl for several numerators of ONE squared-down order over one denominator: rows[k] = (row index in d_lhs / d_out,
// trimmed length); quotient row = tl - tr + 1 coefficients, zeros behind them up to out_stride.  Workspace: WS_MISC_A, B, F and the
// transform slots.
struct CdRow { size_t row, tl; };
int coset_divide_rows_dev_impl(int fid, const void* d_lhs, size_t lhs_stride, const CdRow* rows, size_t nrows, const void* d_rhs, size_t tr,
                               const uint64_t* offset_host, const uint64_t* root_host, size_t order, void* d_out, size_t out_stride, hipStream_t s);
int pointwise_div_dev(int fid, const void* d_a, const void* d_b, void* d_out, size_t n, hipStream_t s);
int pointwise_div_shared_dev(int fid, const void* d_a, size_t a_stride, const void* d_b, void* d_out, size_t out_stride, size_t n, size_t regs, hipStream_t s);
int pointwise_mul_shared_dev(int fid, const void* d_a, size_t a_stride, const void* d_b, void* d_out, size_t out_stride, size_t n, size_t regs, hipStream_t s);
int pointwise_mul_dev(int fid, const void* d_a, const void* d_b, void* d_out, size_t n, hipStream_t s);
void ntt_release_plans();
// ---- Goldilocks family (mzk_gl.hip); same contracts as the calls above, parameters as canonical u64 (id 4: three of them, c0 c1 c2)
// gl_param_check: every word of x[0 .. comps) canonical (MZK_E_RANGE otherwise); base_only: an id-4 parameter must have c1 = c2 = 0
// (MZK_E_ARG: omega, generator and offset lie in the base field, mzk.h)
int gl_param_check(int fid, const uint64_t* x, const char* who, const char* what, bool base_only);
int gl_ntt_dev_impl(int fid, const uint64_t* root_host, const void* d_in, void* d_out, size_t n, size_t batch, int inverse, hipStream_t s);
int gl_coset_lde_dev_impl(int fid, const void* d_coef, size_t n_coef, const uint64_t* offset_host, const uint64_t* generator_host, void* d_out,
                          size_t order, hipStream_t s, size_t batch);
int gl_fri_fold_dev(int fid, const void* d_cw, size_t n, const uint64_t* alpha, uint64_t half, uint64_t oinv, uint64_t winv, void* d_out, hipStream_t s);
int gl_fri_fold_dev_alpha(int fid, const void* d_cw, size_t n, const uint64_t* d_alpha, uint64_t half, uint64_t oinv, uint64_t winv, void* d_out,
                          hipStream_t s);       // alpha: NC canonical words in device memory
void gl_release_plans();
void rs_release_plans();        // mzk_rs.hip: Reed-Solomon tables of the current context
void kzg_release_cache();       // mzk_kzg.hip: fixed-base tables of the current context
void poly_release_plans();      // mzk_poly.hip: cached interpolation plans of the current context
int fri_fold_dev_impl(int fid, const void* d_cw, size_t n, const uint64_t* alpha, const uint64_t* offset, const uint64_t* omega,
                      void* d_out, hipStream_t s);
struct FriFoldConsts { uint64_t half[4], oinv[4], winv[4], rmod[4]; };
int fri_fold_consts(int fid, const uint64_t* offset, const uint64_t* omega, FriFoldConsts* fc);
void fri_fold_consts_square(int fid, FriFoldConsts* fc);
int fri_fold_dev_consts(int fid, const void* d_cw, size_t n, const uint64_t* alpha, const FriFoldConsts& fc, void* d_out, hipStream_t s);
int fri_fold_dev_alpha(int fid, const void* d_cw, size_t n, const uint64_t* d_alpha, const FriFoldConsts& fc, void* d_out, hipStream_t s);
int kzg_batch_open_dev(const void* d_coef, size_t n, const uint64_t* us_host, size_t k, MsmPoints pts, void* d_ys, void* d_w_xy, hipStream_t s);

// point_kind, window tables: mzk_msm_plan.h; MsmPoints, the one argument for a point set, and the width by SRS size: mzk_srs_plan.h.
// One MSM computed in CHUNKS of consecutive pairs (msm_chunked_impl): every chunk is sorted and accumulated on its own -- as soon as
// ITS scalars (and points) are on the device -- into its own bucket array, the chunks' bucket arrays are summed and reduced once.
// msm_dev_impl in chunk mode (cc != null) takes the chunk's scalars, the WHOLE point array, and stops after the segment combine.
// the MSM's scratch, one pointer per slot that msm_plan sizes (null where the plan asks for nothing)
struct MsmWs { uint32_t *points, *counts, *offsets, *cursor, *entries, *scan, *buckets, *slots, *wghist, *out; };
struct MsmChunkCtx {
  const MsmWs* ws;       // the slots, taken ONCE by msm_chunked_impl for all chunks: K regions in the per-chunk ones, chunk k works in the k-th
  int k, K;              // this chunk, number of chunks
  size_t i0;             // index of the chunk's first pair in the whole problem
  size_t n_total;        // pairs of the whole problem: decides the window width / bucket layout of every chunk
  size_t n_alloc;        // the largest chunk: size of the per-chunk buffers (the same in every call, so that no workspace slot is regrown)
};
struct MsmChunk { const void* d_scalars; size_t i0, n; hipEvent_t ready; };    // ready (or null): recorded when the chunk's inputs are on the device
int msm_chunked_impl(const MsmChunk* chunks, int K, MsmPoints pts, size_t n_total, void* d_out, bool out_partial_xyzz, hipStream_t s,
                     const std::function<int(int)>* before_chunk = nullptr);
bool msm_chunkable(size_t n_total, MsmPoints pts);      // mzk_msm_plan.h, with the library's MsmKnobs
int msm_dev_impl(const void* d_scalars, MsmPoints pts, size_t n, void* d_out, bool out_partial_xyzz, hipStream_t s,
                 const std::function<int()>* points_ready = nullptr, const MsmChunkCtx* cc = nullptr);

// Grid-batched form for many short polynomials against one set of narrow window tables (mzk_msm.hip, mzk_kzg.hip)
bool msm_many_supported(int window_bits);
int msm_generic_window_bits(size_t n);        // window width of the generic (GLV) layout for n pairs
int msm_many_dev_impl(const void* d_scalars, size_t n, size_t stride_elems, size_t count, const void* d_tables, int c, size_t table_stride, void* d_out,
                      hipStream_t s);
constexpr size_t MSM_DIRECT_MAX_N = (size_t)1 << 14;
int msm_build_direct(const void* d_points_mont, size_t n, int c, void* d_direct, hipStream_t s);
int msm_direct_many_dev_impl(const void* d_scalars, size_t n, size_t stride_elems, size_t count, const void* d_direct, int c, size_t table_stride, void* d_out,
                             hipStream_t s);

int xyzz_batch_to_affine(const void* d_xyzz, size_t count, void* d_out, bool out_mont, hipStream_t s);
int msm_build_tables(const void* d_points_mont, size_t n, void* d_tables, int window_bits, hipStream_t s);
int msm_fold_partials_impl(const void* d_partials, int count, void* d_out_xy, hipStream_t s);
int msm_prepare_points(const void* d_points_plain, size_t n, void* d_points_mont, void* d_phi, hipStream_t s);
int msm_phi_points(const void* d_points_mont, size_t n, void* d_phi, hipStream_t s);
int synth_field_impl(int fid, uint64_t seed, size_t n, void* d_out, hipStream_t s);
int synth_g1_impl(uint64_t seed, size_t n, void* d_out, hipStream_t s);
int selftest_inv_wave_impl(uint64_t seed, size_t n, uint64_t* mismatches_host, hipStream_t s);
int selftest_row_ec_impl(uint64_t seed, size_t n, int dbl_reps, uint64_t* mismatches_host, hipStream_t s);
int selftest_field_asm_impl(int fid, uint64_t seed, size_t n, uint64_t* mismatches_host, hipStream_t s);
int selftest_copy_impl(const void* d_src, void* d_dst, size_t bytes, hipStream_t s);
// the arithmetic probe (mzk_probe.hip): _arity / _check validate without launching (0 / MZK_E_ARG: no such field, op or form)
int selftest_field_probe_arity(int fid, int op, int form, int* limbs);
int selftest_field_probe_impl(int fid, int op, int form, size_t n, const uint32_t* in_host, uint32_t* out_host, hipStream_t s);
int selftest_g1_probe_check(int op, int form, int* a_words, int* b_words);
int selftest_g1_probe_impl(int op, int form, size_t n, const uint32_t* a_host, const uint32_t* b_host, const uint8_t* neg_host, uint32_t* out_host,
                           hipStream_t s);
int kzg_setup_g1_dev(const uint64_t* alpha_host, const uint64_t* g1_host, size_t first, size_t count, void* d_powers_xy, hipStream_t s);
int kzg_open_dev(const void* d_coef, size_t n, const uint64_t* u_host, MsmPoints pts, void* d_y, void* d_w_xy, void* d_q, hipStream_t s);
// Synthetic division by (X - u) (mzk_kzg.hip): b_len = *end (0 when end is null),
// b_t = src[t] + u b_{t+1}; y = b_0, q = b_1 .. b_{len-1}, or b_1 .. b_len with an end.  u and end are canonical host values;
// y and q are device outputs or null; a job of length 0 writes nothing.
struct SdJob { const void* src; size_t len; const uint64_t* u; const uint64_t* end; void* y; void* q; };
// rounds[r] consecutive jobs form round r; the jobs of a round are independent, a later round may read what an earlier one wrote.
// Workspace: WS_MISC_C (the job table) and WS_MISC_D (chunk values and carries).
int synth_div_dev(const SdJob* jobs, const size_t* rounds, int nrounds, hipStream_t s);
// The same engine over Fr or M128 (u and end then hold 2 limbs).
int synth_div_field_dev(int fid, const SdJob* jobs, const size_t* rounds, int nrounds, hipStream_t s);
// Row i of d_polys (lens[i] coefficients, rows `stride` elements apart) divided by prod_j (X - roots[j]), j in [root_offsets[i],
// root_offsets[i+1]): quotient rows into d_out (same stride, zero behind the quotient), trimmed lengths into out_lens (mzk.h:
// mzk_poly_div_roots).  _check validates, _dev_impl enqueues and returns when d_out is complete.  Workspace: WS_MISC_A .. E.
int poly_div_roots_check(int fid, const void* polys, size_t stride, const size_t* lens, size_t count, const uint64_t* roots, const size_t* root_offsets,
                         const void* out, const size_t* out_lens);
int poly_div_roots_dev_impl(int fid, const void* d_polys, size_t stride, const size_t* lens, size_t count, const uint64_t* roots, const size_t* root_offsets,
                            void* d_out, size_t* out_lens, hipStream_t s);

}  // namespace mzk

// ---- against an SRS handle (struct mzk_srs: mzk_srs.h) ------------------------------------------------------------------------------
namespace mzk {
// `count` commitments of n coefficients each (polynomial j at d_scalars + j * stride_elems * 32 bytes) against one handle, as ONE
// pass: over the direct tables when the handle has them, over its narrow window tables otherwise (srs_many_capable).
// shift != 0: against the points [shift, shift + n) of the handle (every layout keeps point i of a table at row offset i, so the
// tables are entered `shift` rows further on with the row stride unchanged); shift + n <= srs->n.  mzk_srs.hip.
int msm_many_srs(const mzk_srs* srs, const void* d_scalars, size_t n, size_t stride_elems, size_t count, void* d_out, hipStream_t s,
                 size_t shift = 0);
// The one body of mzk_srs_upload, mzk_srs_from_device_ex and mzk_srs_load's rebuild: a handle of the layout that fits (srs_new), filled
// from n affine canonical points in host memory (host_xy, staged through WS_MISC_A) or on the device (d_xy); the stream is idle on return.
int srs_from_points(const uint64_t* host_xy, const void* d_xy, size_t n, int with_tables, mzk_srs** out, hipStream_t s);
bool kzg_open_many_supported(const mzk_srs* srs, size_t n);
int kzg_open_many_dev(const mzk_srs* srs, const void* d_coefs, size_t n, size_t count, const uint64_t* us_host, void* d_ys, void* d_ws_xy, hipStream_t s);
}  // namespace mzk
