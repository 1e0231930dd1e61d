// mzk_api.hip -- process context and the host-buffer entry points of
// include/mzk.h (H2D copy -> device implementation -> D2H copy, as the reference's only device
// boundary does: examples/sumcheck/src/prover.rs:149-170).
#include <stdarg.h>
#include <stdlib.h>
#include <atomic>
#include "mzk_common.h"
#include "mzk_divide_plan.h"
#include "mzk_gl.h"
#include "mzk_mul_plan.h"
#include "mzk_srs.h"

namespace mzk {

static thread_local char g_err[512] = "";
void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof g_err, fmt, ap);
  va_end(ap);
}
void clear_error() { g_err[0] = 0; }
int hip_fail(hipError_t e, const char* what, const char* file, int line) {
  set_error("HIP error %d (%s) in %s at %s:%d", (int)e, hipGetErrorString(e), what, file, line);
  return MZK_E_HIP;
}

// the thread that is inside the library (0 = nobody); depth counts its nested entries
static std::atomic<uint64_t> g_owner{0};
static thread_local int t_depth = 0;
static thread_local char t_marker;            // its address is this thread's id
EntryGuard::EntryGuard() : ok(true), nested(false) {
  if (t_depth > 0) { t_depth++; nested = true; return; }
  uint64_t expected = 0;
  if (!g_owner.compare_exchange_strong(expected, (uint64_t)(uintptr_t)&t_marker, std::memory_order_acquire)) {
    ok = false;
    set_error("another host thread is inside the library: calls must come from one thread at a time (MZK_E_BUSY)");
    return;
  }
  t_depth = 1;
  g_ws_epoch++;
}
EntryGuard::~EntryGuard() {
  if (!ok) return;
  if (--t_depth == 0) g_owner.store(0, std::memory_order_release);
}

static Context g_ctxs[MZK_MAX_CTX];
static int g_nctx = 0, g_cur = 0;
static int g_last_ordinal = 0;                   // what ensure_init() re-initialises on after a shutdown
static signed char g_peer[MZK_MAX_CTX][MZK_MAX_CTX];
int ctx_peer_enabled(int a, int b) { return (a >= 0 && b >= 0 && a < g_nctx && b < g_nctx) ? g_peer[a][b] : 0; }
Context& ctx() { return g_ctxs[g_cur]; }
int ctx_count() { return g_nctx; }
// What mzk_init's unguarded fast path may look at, and nothing else: the ordinal context 0 drives WHILE it is ready and current, -1
// otherwise.  Every writer of g_cur / of context 0 (ctx_select, CtxScope, mzk_init_devices, mzk_shutdown) publishes it with release
// order, the fast path reads it with acquire order -- it never touches g_nctx, g_ctxs or g_cur, which those writers change under the
// entry guard the fast path does not take.
static std::atomic<int> g_ctx0_current_on{-1};
static void publish_ctx0() {
  g_ctx0_current_on.store((g_nctx > 0 && g_cur == 0 && g_ctxs[0].ready) ? g_ctxs[0].device : -1, std::memory_order_release);
}
int ctx_select(int index) {
  if (index < 0 || index >= g_nctx || !g_ctxs[index].ready) { set_error("context %d does not exist (%d initialised)", index, g_nctx); return MZK_E_ARG; }
  MZK_HIP(hipSetDevice(g_ctxs[index].device));
  g_cur = index;
  publish_ctx0();
  return MZK_OK;
}
CtxScope::CtxScope(int index) : prev_ctx(g_cur), prev_dev(-1), ok(false) {
  if (hipGetDevice(&prev_dev) != hipSuccess) prev_dev = -1;
  ok = ctx_select(index) == MZK_OK;
}
CtxScope::~CtxScope() {
  g_cur = prev_ctx;
  publish_ctx0();
  if (prev_dev >= 0) (void)hipSetDevice(prev_dev);
}

// The workspace's bookkeeping is mzk_ws.h; here it meets the device.  A refused hipMalloc is MZK_E_NOMEM (dev_alloc trims the idle
// slots and tries once more before it says so), not MZK_E_HIP.
int ws_hook_alloc(void** out, size_t bytes, const char* what) {
  const hipError_t e = hipMalloc(out, bytes);
  if (e == hipSuccess) return MZK_OK;
  (void)hipGetLastError();
  *out = nullptr;
  if (e == hipErrorOutOfMemory || e == hipErrorMemoryAllocation) return MZK_E_NOMEM;
  return hip_fail(e, what, __FILE__, __LINE__);
}
int ws_hook_free(void* p) { MZK_HIP(hipFree(p)); return MZK_OK; }
int ws_hook_sync() { MZK_HIP(hipDeviceSynchronize()); return MZK_OK; }
int ws_hook_wait(void* stream) { MZK_HIP(hipStreamSynchronize((hipStream_t)stream)); return MZK_OK; }
WsTable* ws_table_of(int ctx_index) { return &g_ctxs[ctx_index].ws; }
int ws_current_ctx() { return g_cur; }
int d2h_sync(void* host, const void* dev, size_t bytes, hipStream_t s) {
  if (bytes == 0 || bytes > SMALL_D2H_MAX) {
    if (bytes) MZK_HIP(hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, s));
    MZK_HIP(hipStreamSynchronize(s));
    return MZK_OK;
  }
  Context& c = ctx();
  if (!c.bounce) MZK_HIP(hipHostMalloc(&c.bounce, SMALL_D2H_MAX, hipHostMallocPortable));
  MZK_HIP(hipMemcpyAsync(c.bounce, dev, bytes, hipMemcpyDeviceToHost, s));
  MZK_HIP(hipStreamSynchronize(s));
  memcpy(host, c.bounce, bytes);
  return MZK_OK;
}
// The workspace slots are shared by every entry point of a context.  *_dev calls only enqueue work, so a call on
// stream B could overwrite slots that kernels of an earlier call on stream A are still reading: the guard orders B
// behind the last user's completion event (no host synchronisation), and records its own at scope exit.
// The event is recorded LAZILY, on the previous user's stream, at the moment a different stream shows up: that still
// covers everything enqueued there, and steady single-stream use (every benchmark loop) pays no marker per call.
WsGuard::WsGuard(hipStream_t s_) : s(s_) {
  Context& c = ctx();
  if (!c.ready) return;
  if (c.ws_used && c.ws_last != s) {
    if (!c.ws_event && hipEventCreateWithFlags(&c.ws_event, hipEventDisableTiming) != hipSuccess) c.ws_event = nullptr;
    // (the previous stream may be gone by now -- a destroyed caller stream: fall back to a device-wide wait)
    if (c.ws_event && hipEventRecord(c.ws_event, c.ws_last) == hipSuccess) (void)hipStreamWaitEvent(s, c.ws_event, 0);
    else { (void)hipGetLastError(); (void)hipDeviceSynchronize(); }
  }
}
WsGuard::~WsGuard() {
  Context& c = ctx();
  if (!c.ready) return;
  c.ws_last = s;
  c.ws_used = true;
}

// ---- profiling --------------------------------------------------------------------------------------
static bool g_prof_on = false;
static uint32_t g_prof_mask = 0xffffffffu;     // phases that get event pairs while profiling is on
struct ProfPair { hipEvent_t a, b; int phase; };
static std::vector<ProfPair> g_prof_pending;
static std::vector<hipEvent_t> g_prof_pool;
static hipEvent_t g_prof_open[MZK_PH_COUNT];
static double g_prof_ms[MZK_PH_COUNT];
static uint64_t g_prof_cnt[MZK_PH_COUNT];
static hipEvent_t prof_event() {
  if (!g_prof_pool.empty()) { hipEvent_t e = g_prof_pool.back(); g_prof_pool.pop_back(); return e; }
  hipEvent_t e = nullptr;
  (void)hipEventCreate(&e);
  return e;
}
// Phases are keyed by number only, so only context 0 is instrumented: the lanes of mzk_*_batch_dev enqueue the same phase
// on several contexts interleaved, and begin/end pairs of different lanes would cross.
void prof_begin(hipStream_t s, int phase) {
  if (!g_prof_on || !((g_prof_mask >> phase) & 1u) || ctx().index != 0) return;
  hipEvent_t e = prof_event();
  (void)hipEventRecord(e, s);
  g_prof_open[phase] = e;
}
void prof_end(hipStream_t s, int phase) {
  if (!g_prof_on || !g_prof_open[phase] || ctx().index != 0) return;
  hipEvent_t e = prof_event();
  (void)hipEventRecord(e, s);
  g_prof_pending.push_back({g_prof_open[phase], e, phase});
  g_prof_open[phase] = nullptr;
}
static void prof_drain() {
  (void)hipDeviceSynchronize();
  for (auto& pr : g_prof_pending) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, pr.a, pr.b) == hipSuccess) { g_prof_ms[pr.phase] += ms; g_prof_cnt[pr.phase]++; }
    g_prof_pool.push_back(pr.a);
    g_prof_pool.push_back(pr.b);
  }
  g_prof_pending.clear();
}

// Every entry point starts here.  torch (or the caller) may have switched the thread's current HIP device since the last
// call: re-assert the context's device so that allocations and launches land on the GPU the context drives.
int ensure_init() {
  if (g_nctx > 0 && ctx().ready) {
    int cur = -1;
    if (hipGetDevice(&cur) != hipSuccess || cur != ctx().device) MZK_HIP(hipSetDevice(ctx().device));
    return MZK_OK;
  }
  return mzk_init(g_last_ordinal);
}

static_assert(HOST_LIMBS29_FR == FrParams::L && HOST_LIMBS29_FQ == FqParams::L && HOST_LIMBS29_M128 == M128Params::L,
              "mzk_hostfield.h states the device's limb counts");
int field_check(int fid, const char* who, bool fq_too) {
  if (fid == MZK_FIELD_FR || fid == MZK_FIELD_M128 || (fq_too && fid == MZK_FIELD_FQ)) return MZK_OK;
  set_error("%s: bad field id %d", who, fid);
  return MZK_E_ARG;
}
int field_check_ntt(int fid, const char* who) {
  if (fid == MZK_FIELD_FR || fid == MZK_FIELD_M128) return MZK_OK;
  set_error("%s: field id %d has no NTT on this path", who, fid);
  return MZK_E_ARG;
}

}  // namespace mzk

using namespace mzk;

extern "C" {

int mzk_abi_version(void) { return 2; }
const char* mzk_last_error(void) { return g_err; }

static int check_device(int device_ordinal, int* num_cu) {
  int count = 0;
  hipError_t e = hipGetDeviceCount(&count);
  if (e != hipSuccess || count <= 0) {
    set_error("no HIP device visible (hipGetDeviceCount: %s); this library has no CPU fallback",
              e == hipSuccess ? "0 devices" : hipGetErrorString(e));
    return MZK_E_NOGPU;
  }
  if (device_ordinal < 0 || device_ordinal >= count) { set_error("mzk_init: device %d out of range (%d visible)", device_ordinal, count); return MZK_E_ARG; }
  hipDeviceProp_t prop;
  MZK_HIP(hipGetDeviceProperties(&prop, device_ordinal));
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
    set_error("device %d is %s; this library is built for gfx950 (MI355X) only", device_ordinal, prop.gcnArchName);
    return MZK_E_NOGPU;
  }
  *num_cu = prop.multiProcessorCount;
  return MZK_OK;
}

int mzk_init_devices(const int* device_ordinals, int n_devices) {
  mzk::EntryGuard entry;
  if (!entry.ok) return MZK_E_BUSY;
  if (!device_ordinals || n_devices < 1 || n_devices > MZK_MAX_CTX) { set_error("mzk_init_devices: need 1..%d device ordinals", MZK_MAX_CTX); return MZK_E_ARG; }
  bool same = g_nctx == n_devices;
  for (int i = 0; same && i < n_devices; i++) same = g_ctxs[i].ready && g_ctxs[i].device == device_ordinals[i];
  if (same) return ctx_select(0);
  int ncu[MZK_MAX_CTX];
  for (int i = 0; i < n_devices; i++) MZK_TRY(check_device(device_ordinals[i], &ncu[i]));
  if (g_nctx) mzk_shutdown();
  for (int i = 0; i < n_devices; i++) {
    Context& c = g_ctxs[i];
    c = Context();
    c.index = i;
    c.device = device_ordinals[i];
    c.num_cu = ncu[i];
    ws_new_generation(c.ws);
    MZK_HIP(hipSetDevice(c.device));
    // Contexts that share a GPU are there to keep several calls in flight: give each its own stream PRIORITY level, which
    // also puts them on different hardware queues (streams of one priority may share a queue and then serialise).
    int dup = 0;
    for (int j = 0; j < i; j++) dup += g_ctxs[j].device == c.device;
    int prio_least = 0, prio_greatest = 0;
    (void)hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest);
    int prio = prio_least - dup;                        // numerically lower = higher priority
    if (prio < prio_greatest) prio = prio_greatest;
    if (dup == 0) MZK_HIP(hipStreamCreateWithFlags(&c.stream, hipStreamNonBlocking));
    else MZK_HIP(hipStreamCreateWithPriority(&c.stream, hipStreamNonBlocking, prio));
    c.ready = true;
    g_nctx = i + 1;
  }
  g_last_ordinal = device_ordinals[0];
  // Peer access between every pair of distinct devices (mzk_ntt_multi's exchanges are device-to-device copies: without it
  // the runtime may stage them through host memory).  "Already enabled" is fine -- torch or an earlier init did it.
  for (int a = 0; a < n_devices; a++)
    for (int b = 0; b < n_devices; b++) {
      g_peer[a][b] = 1;
      const int da = g_ctxs[a].device, db = g_ctxs[b].device;
      if (da == db) continue;
      int can = 0;
      if (hipDeviceCanAccessPeer(&can, da, db) != hipSuccess) { (void)hipGetLastError(); can = 0; }
      if (can) {
        MZK_HIP(hipSetDevice(da));
        hipError_t e = hipDeviceEnablePeerAccess(db, 0);
        if (e == hipErrorPeerAccessAlreadyEnabled) (void)hipGetLastError();
        else if (e != hipSuccess) { (void)hipGetLastError(); can = 0; }
      }
      g_peer[a][b] = (signed char)can;
    }
  return ctx_select(0);
}
// Idempotent: when context 0 already drives this ordinal nothing is torn down (further contexts made by mzk_init_devices,
// their streams, workspaces and the handles that live on them all stay valid).
// It takes the entry guard like every other entry point: wrappers call it once per thread, and a second thread arriving while
// a call is in progress must get MZK_E_BUSY instead of flipping the current context (ctx_select below) under that call's
// CtxScope switches.  Called from inside a call on the owning thread (a callback), the fast path leaves the current context
// and the device alone -- the enclosing call owns them.
int mzk_init(int device_ordinal) {
  // Idempotent fast path WITHOUT the entry guard: a second host thread's first call during a long call of another
  // thread used to get MZK_E_BUSY here, where mzk_init had been a harmless no-op.  It reads ONE atomic (g_ctx0_current_on: context 0
  // ready on this ordinal and current), nothing is written, and the caller's HIP device is set for ITS thread only.  While another
  // thread's *_multi call has switched contexts, or a shutdown / re-initialisation is under way, the flag is -1 and the guarded
  // path below answers (MZK_E_BUSY in those windows, as for every other entry point).
  if (g_ctx0_current_on.load(std::memory_order_acquire) == device_ordinal) {
    int dev = -1;
    if (hipGetDevice(&dev) == hipSuccess && (dev == device_ordinal || hipSetDevice(device_ordinal) == hipSuccess)) return MZK_OK;
    (void)hipGetLastError();
  }
  mzk::EntryGuard entry;
  if (!entry.ok) return MZK_E_BUSY;
  if (g_nctx > 0 && g_ctxs[0].ready && g_ctxs[0].device == device_ordinal) return entry.nested ? MZK_OK : ctx_select(0);
  return mzk_init_devices(&device_ordinal, 1);
}
int mzk_ctx_count(void) { return g_nctx; }
int mzk_ctx_select(int index) {
  mzk::EntryGuard entry;
  if (!entry.ok) return MZK_E_BUSY;
  return ctx_select(index);
}
int mzk_ctx_peer_enabled(int a, int b) { return ctx_peer_enabled(a, b); }
int mzk_ctx_device(int index) { return (index >= 0 && index < g_nctx) ? g_ctxs[index].device : -1; }
void* mzk_ctx_stream(int index) { return (index >= 0 && index < g_nctx) ? (void*)g_ctxs[index].stream : nullptr; }

void mzk_shutdown(void) {
  mzk::EntryGuard entry;
  if (!entry.ok) return;          // another thread is inside a call: tearing its contexts down under it is not an option
  if (g_nctx) {        // the profiler's events belong to context 0's device
    CtxScope sc(0);
    prof_drain();
    for (hipEvent_t e : g_prof_pool) (void)hipEventDestroy(e);
    g_prof_pool.clear();
    for (auto& e : g_prof_open) { if (e) (void)hipEventDestroy(e); e = nullptr; }
  }
  g_ctx0_current_on.store(-1, std::memory_order_release);     // mzk_init's fast path must not answer for a context that is going away
  for (int i = 0; i < g_nctx; i++) {
    Context& c = g_ctxs[i];
    if (!c.ready) continue;
    g_cur = i;
    (void)hipSetDevice(c.device);
    (void)hipDeviceSynchronize();
    ntt_release_plans();
    rs_release_plans();
    kzg_release_cache();
    poly_release_plans();          // their blocks park in the pool, which goes next
    ws_release_all();
    if (c.ws_event) (void)hipEventDestroy(c.ws_event);
    if (c.fork_event) (void)hipEventDestroy(c.fork_event);
    if (c.join_event) (void)hipEventDestroy(c.join_event);
    if (c.xready) (void)hipEventDestroy(c.xready);
    for (int k = 0; k < MZK_MAX_CTX; k++) {
      if (c.xdone[k]) (void)hipEventDestroy(c.xdone[k]);
      if (c.xstream[k]) (void)hipStreamDestroy(c.xstream[k]);
    }
    if (c.stream) (void)hipStreamDestroy(c.stream);
    if (c.bounce) (void)hipHostFree(c.bounce);
    c = Context();
  }
  g_nctx = 0;
  g_cur = 0;
}

int mzk_prof_enable(int on) { g_prof_on = on != 0; return MZK_OK; }
int mzk_prof_select(uint32_t phase_mask) { g_prof_mask = phase_mask; return MZK_OK; }
int mzk_prof_reset(void) {
  prof_drain();
  for (int i = 0; i < MZK_PH_COUNT; i++) { g_prof_ms[i] = 0; g_prof_cnt[i] = 0; }
  return MZK_OK;
}
int mzk_prof_read(int phase, double* total_ms, uint64_t* launches) {
  if (phase < 0 || phase >= MZK_PH_COUNT || !total_ms || !launches) { set_error("prof_read: bad argument"); return MZK_E_ARG; }
  prof_drain();
  *total_ms = g_prof_ms[phase];
  *launches = g_prof_cnt[phase];
  return MZK_OK;
}
const char* mzk_prof_name(int phase) {
  static const char* names[MZK_PH_COUNT] = {"msm_prepare_points", "msm_digit_sort", "msm_bucket_accumulate", "msm_bucket_reduce",
                                            "msm_window_combine", "ntt_pass0", "ntt_pass1", "ntt_pass2", "ntt_pass3", "ntt_coset_prescale", "merkle_sha3_levels",
                                            "msm_segment_combine", "ntt_whole_transform", "scp_round0", "scp_rounds", "scp_round_ends", "scp_tail", "hypercube_tables"};
  return (phase >= 0 && phase < MZK_PH_COUNT) ? names[phase] : "?";
}

// Host parameter arithmetic (mzk_hostfield.h) as the library carries it, checked without a GPU (tests/test_abi_load.py): op 0 = a * b,
// 1 = a^-1 (0 -> 0), 2 = a^b[0], 3 = a * b by the bit-serial reference implementation, 4 = h_mont_words(a): a R mod p as the eight
// 32-bit words of a kernel argument, in four uint64 whatever the field (M128: the upper two are zero).  b is not read by 1 and 4.
int mzk_host_field_op(int field_id, int op, const uint64_t* a, const uint64_t* b, uint64_t* out) {
  const HostField* f = host_field(field_id);
  if (!f || !a || !out || (!b && op != 1 && op != 4)) { set_error("host_field_op: bad argument"); return MZK_E_ARG; }
  if (!h_is_canonical(f, a) || ((op == 0 || op == 3) && !h_is_canonical(f, b))) { set_error("host_field_op: operand not canonical"); return MZK_E_RANGE; }
  switch (op) {
    case 0: h_mulmod(f, out, a, b); return MZK_OK;
    case 1: h_invmod(f, out, a); return MZK_OK;
    case 2: h_powmod_u64(f, out, a, b[0]); return MZK_OK;
    case 3: h_mulmod_slow(f, out, a, b); return MZK_OK;
    case 4: {
      u32 w[8];
      h_mont_words(f, a, w);
      for (int i = 0; i < 4; i++) out[i] = (uint64_t)w[2 * i] | ((uint64_t)w[2 * i + 1] << 32);
      return MZK_OK;
    }
    default: set_error("host_field_op: bad op %d", op); return MZK_E_ARG;
  }
}

int mzk_root_of_unity(int field_id, unsigned log2_n, uint64_t* out) {
  if (!out) { set_error("root_of_unity: null pointer"); return MZK_E_ARG; }
  const HostField* f = host_field(field_id);
  if (field_id == MZK_FIELD_M128) {
    // get_nth_root_of_m128, zkstark/fri.rs:423-447
    if (log2_n > 119) { set_error("Field does not have nth root of unity where n > 2^119 or not power of two."); return MZK_E_ARG; }
    uint64_t r[4] = {0xb5038f9c18f6f7d1ULL, 0x4040fbed12ee470fULL, 0, 0};  // 85408008396924667383611388730472331217
    for (unsigned o = 119; o > log2_n; o--) h_mulmod(f, r, r, r);
    out[0] = r[0]; out[1] = r[1];
    return MZK_OK;
  }
  if (field_id == MZK_FIELD_FR) {
    // omega_2^28 = 5^((r-1)/2^28); the reference ships no Fr root helper
    if (log2_n > 28) { set_error("Fr has 2-adicity 28"); return MZK_E_ARG; }
    uint64_t r[4] = {0x9bd61b6e725b19f0ULL, 0x402d111e41112ed4ULL, 0x00e0a7eb8ef62abcULL, 0x2a3c09f0a58a7e85ULL};
    for (unsigned o = 28; o > log2_n; o--) h_mulmod(f, r, r, r);
    for (int i = 0; i < 4; i++) out[i] = r[i];
    return MZK_OK;
  }
  if (field_is_gl(field_id)) {
    // get_nth_root_of_m64, zkstark/fri.rs:449-473; for the extension the same value, embedded (c1 = c2 = 0)
    if (log2_n > gl::TWO_ADICITY) { set_error("Field does not have nth root of unity where n > 2^32 or not power of two."); return MZK_E_ARG; }
    uint64_t r = gl::ROOT_2_32;
    for (unsigned o = gl::TWO_ADICITY; o > log2_n; o--) r = gl::sqr(r);
    out[0] = r;
    for (int i = 1; i < field_gl_comps(field_id); i++) out[i] = 0;
    return MZK_OK;
  }
  return field_check(field_id, "root_of_unity");
}

// ---- host-buffer NTT family ---------------------------------------------------------------------------
// host buffer -> workspace slot, leased from the caller's frame (the caller uses the pointer).  A plain hipMemcpyAsync from pageable memory: on this runtime (ROCm 7.2) it already moves 56 GB/s
// in either direction, the same as a DMA from pinned memory (tools/timing/pcie_probe.py, profiles/r03h_pcie_probe.txt); a pinned
// staging ring with copy threads was built in round 3 and measured SLOWER (generic MSM 4.5 vs 3.7 ms, NTT 4.8 vs 3.6 ms), so
// what the host-buffer entry points can gain is overlap, not a faster copy (see mzk_msm_g1_bn254).
static int stage_in(WsFrame& ws, WsSlot slot, const void* host, size_t bytes, void** dev, hipStream_t s) {
  MZK_TRY(ws.get(slot, bytes ? bytes : 16, dev));
  if (bytes) MZK_HIP(hipMemcpyAsync(*dev, host, bytes, hipMemcpyHostToDevice, s));
  return MZK_OK;
}
// device result -> host buffer; returns with the host buffer complete
static int stage_out(void* host, const void* dev, size_t bytes, hipStream_t s) { return d2h_sync(host, dev, bytes, s); }
// a second stream of the current context for transfers that should run beside its kernels, with the two events that fork it
// from / join it to the context's stream (created on first use; shared with mzk_ntt_multi's exchange, which never overlaps a call)
static int side_stream(hipStream_t* side, hipEvent_t* fork, hipEvent_t* join) {
  Context& c = ctx();
  if (!c.xstream[1]) MZK_HIP(hipStreamCreateWithFlags(&c.xstream[1], hipStreamNonBlocking));
  if (!c.xready) MZK_HIP(hipEventCreateWithFlags(&c.xready, hipEventDisableTiming));
  if (!c.xdone[1]) MZK_HIP(hipEventCreateWithFlags(&c.xdone[1], hipEventDisableTiming));
  *side = c.xstream[1]; *fork = c.xready; *join = c.xdone[1];
  return MZK_OK;
}

// Host buffers in PIECES (the callers own host Vecs: kzg.rs:57-72): piece k + 1 crosses PCIe on the side stream -- a pageable
// hipMemcpyAsync keeps the host in the call until the piece is staged -- while the GPU sorts and accumulates piece k
// (msm_chunked_impl).  Split points in 1/256ths of n: MZK_HOST_CHUNKS_COMMIT / _MSM in the tuning build, e.g. "64,256" = 25 % + 75 %.
// The first piece is small (nothing runs under its transfer), the later ones must keep the accumulate's lanes busy; every piece is
// rounded to whole sort workgroups (4096 pairs).
static int host_chunk_plan(size_t n, const char* env_name, const int* dflt, int dflt_count, mzk::MsmChunk* ch) {
  int cuts[8], K = 0;
  if (const char* v = mzk::tune_str(env_name)) {           // (tuning build only: null in the shipped library)
    for (const char* p = v; *p && K < 8;) { cuts[K++] = atoi(p); while (*p && *p != ',') p++; if (*p == ',') p++; }
  }
  if (K == 0) for (; K < dflt_count; K++) cuts[K] = dflt[K];
  size_t prev = 0;
  int out = 0;
  for (int k = 0; k < K; k++) {
    size_t end = (k + 1 == K) ? n : ((n * (size_t)cuts[k] / 256) & ~(size_t)4095);
    if (end > n) end = n;
    if (end <= prev) continue;
    ch[out++] = mzk::MsmChunk{nullptr, prev, end - prev, nullptr};
    prev = end;
  }
  if (prev < n) { if (out) ch[out - 1].n += n - prev; else ch[out++] = mzk::MsmChunk{nullptr, 0, n, nullptr}; }
  return out;
}
static bool host_chunks_enabled() {
  static const int v = mzk::tune_int("MZK_HOST_CHUNKS", 1);        // tuning build: 0 = one piece, the form of rounds 2-5
  return v != 0;
}
// scalars (32 bytes per pair) and, for the generic MSM, points (64 bytes per pair) of every piece: host -> their workspace slots on
// the side stream; `ev[k]` fires when piece k has landed
struct HostChunkUpload {
  const uint64_t *scalars, *points;
  void *d_s, *d_p;
  mzk::MsmChunk* ch;
  hipEvent_t* ev;
  hipStream_t side;
  int operator()(int k) const {
    const size_t i0 = ch[k].i0, m = ch[k].n;
    MZK_HIP(hipMemcpyAsync((uint8_t*)d_s + i0 * 32, scalars + i0 * 4, m * 32, hipMemcpyHostToDevice, side));
    if (points) MZK_HIP(hipMemcpyAsync((uint8_t*)d_p + i0 * 64, points + i0 * 8, m * 64, hipMemcpyHostToDevice, side));
    MZK_HIP(hipEventRecord(ev[k], side));
    return MZK_OK;
  }
};
struct EventSet {          // a few events for the length of one call
  hipEvent_t ev[8] = {};
  int make(int count) { for (int k = 0; k < count; k++) MZK_HIP(hipEventCreateWithFlags(&ev[k], hipEventDisableTiming)); return MZK_OK; }
  ~EventSet() { for (auto e : ev) if (e) (void)hipEventDestroy(e); }
};
static int msm_host_chunked(const uint64_t* scalars, const uint64_t* points, void* d_s, void* d_p, mzk::MsmPoints pts, size_t n, void* d_o, hipStream_t s,
                            mzk::MsmChunk* ch, int K) {
  hipStream_t side;
  hipEvent_t fork, join;
  MZK_TRY(side_stream(&side, &fork, &join));
  MZK_HIP(hipEventRecord(fork, s));              // the side stream starts behind everything enqueued so far (the slots' previous readers)
  MZK_HIP(hipStreamWaitEvent(side, fork, 0));
  EventSet es;
  MZK_TRY(es.make(K));
  for (int k = 0; k < K; k++) { ch[k].d_scalars = (const uint8_t*)d_s + ch[k].i0 * 32; ch[k].ready = es.ev[k]; }
  const HostChunkUpload up{scalars, points, d_s, d_p, ch, es.ev, side};
  const std::function<int(int)> before = [&](int k) -> int { return up(k); };
  const int rc = msm_chunked_impl(ch, K, pts, n, d_o, false, s, &before);
  if (rc != MZK_OK) (void)hipStreamSynchronize(side);      // no piece may still be reading the caller's host buffers on return
  return rc;
}

int mzk_ntt(int field_id, const uint64_t* root, const uint64_t* in, uint64_t* out, size_t n, int inverse) {
  MZK_ENTER();
  WsFrame ws("mzk_ntt");
  MZK_TRY(field_check_gl(field_id, "ntt"));
  if (n == 0) return MZK_OK;
  if (!in || !out) { set_error("ntt: null pointer"); return MZK_E_ARG; }
  hipStream_t s = ctx().stream;
  WsGuard wsg(s);
  const size_t bytes = n * field_bytes(field_id);
  void *d_in, *d_out;
  MZK_TRY(stage_in(ws, WS_NTT_IO_A, in, bytes, &d_in, s));
  MZK_TRY(ws.get(WS_NTT_IO_B, bytes, &d_out));
  MZK_TRY(ntt_dev_impl(field_id, root, d_in, d_out, n, inverse, nullptr, s));
  MZK_TRY(stage_out(out, d_out, bytes, s));
  return MZK_OK;
}

int mzk_ntt_dev(int field_id, const uint64_t* root_host, const void* d_in, void* d_out, size_t n, int inverse, void* stream) {
  MZK_ENTER();
  WsGuard wsg((hipStream_t)stream);
  return ntt_dev_impl(field_id, root_host, d_in, d_out, n, inverse, nullptr, (hipStream_t)stream);
}

int mzk_coset_lde_batch_dev(int field_id, const void* d_coefs, size_t n_coef, const uint64_t* offset_host, const uint64_t* generator_host,
                            void* d_out, size_t order, size_t batch, void* stream) {
  MZK_ENTER();
  WsGuard wsg((hipStream_t)stream);
  return coset_lde_dev_impl(field_id, d_coefs, n_coef, offset_host, generator_host, d_out, order, (hipStream_t)stream, batch);
}
int mzk_coset_lde_batch(int field_id, const uint64_t* coefs, size_t n_coef, const uint64_t* offset, const uint64_t* generator,
                        uint64_t* out, size_t order, size_t batch) {
  MZK_ENTER();
  WsFrame ws("mzk_coset_lde_batch");
  MZK_TRY(field_check_gl(field_id, "coset_lde"));
  if (n_coef > order) { set_error("attempt to subtract with overflow (order - polynomial.coef.len())"); return MZK_E_LENGTH; }
  if (order == 0 || batch == 0) return MZK_OK;
  if (!out || (!coefs && n_coef)) { set_error("coset_lde: null pointer"); return MZK_E_ARG; }
  hipStream_t s = ctx().stream;
  WsGuard wsg(s);
  const size_t esz = field_bytes(field_id);
  void *d_coef, *d_out;
  MZK_TRY(stage_in(ws, WS_MISC_A, coefs, batch * n_coef * esz, &d_coef, s));
  MZK_TRY(ws.get(WS_NTT_IO_B, batch * order * esz, &d_out));
  MZK_TRY(coset_lde_dev_impl(field_id, d_coef, n_coef, offset, generator, d_out, order, s, batch));
  MZK_TRY(stage_out(out, d_out, batch * order * esz, s));
  return MZK_OK;
}
int mzk_ntt_batch_dev(int field_id, const uint64_t* root_host, const void* d_in, void* d_out, size_t n, size_t batch, int inverse, void* stream) {
  MZK_ENTER();
  WsGuard wsg((hipStream_t)stream);
  return ntt_batch_dev_impl(field_id, root_host, d_in, d_out, n, batch, inverse, (hipStream_t)stream);
}
int mzk_ntt_batch(int field_id, const uint64_t* root, const uint64_t* in, uint64_t* out, size_t n, size_t batch, int inverse) {
  MZK_ENTER();
  WsFrame ws("mzk_ntt_batch");
  MZK_TRY(field_check_gl(field_id, "ntt"));
  if (n == 0 || batch == 0) return MZK_OK;
  if (!in || !out) { set_error("ntt: null pointer"); return MZK_E_ARG; }
  hipStream_t s = ctx().stream;
  WsGuard wsg(s);
  const size_t bytes = batch * n * field_bytes(field_id);
  void* d;
  MZK_TRY(stage_in(ws, WS_NTT_IO_A, in, bytes, &d, s));
  MZK_TRY(ntt_batch_dev_impl(field_id, root, d, d, n, batch, inverse, s));
  MZK_TRY(stage_out(out, d, bytes, s));
  return MZK_OK;
}

int mzk_coset_lde(int field_id, const uint64_t* coef, size_t n_coef, const uint64_t* offset, const uint64_t* generator,
                  uint64_t* out, size_t order) {
  MZK_ENTER();
  WsFrame ws("mzk_coset_lde");
  MZK_TRY(field_check_gl(field_id, "coset_lde"));
  if (n_coef > order) { set_error("attempt to subtract with overflow (order - polynomial.coef.len())"); return MZK_E_LENGTH; }
  if (order == 0) return MZK_OK;
  if (!out || (!coef && n_coef)) { set_error("coset_lde: null pointer"); return MZK_E_ARG; }
  hipStream_t s = ctx().stream;
  WsGuard wsg(s);
  const size_t esz = field_bytes(field_id);
  void *d_coef, *d_out;
  MZK_TRY(stage_in(ws, WS_MISC_A, coef, n_coef * esz, &d_coef, s));
  MZK_TRY(ws.get(WS_NTT_IO_B, order * esz, &d_out));
  MZK_TRY(coset_lde_dev_impl(field_id, d_coef, n_coef, offset, generator, d_out, order, s));
  MZK_TRY(stage_out(out, d_out, order * esz, s));
  return MZK_OK;
}

int mzk_coset_lde_dev(int field_id, const void* d_coef, size_t n_coef, const uint64_t* offset_host,
                      const uint64_t* generator_host, void* d_out, size_t order, void* stream) {
  MZK_ENTER();
  WsGuard wsg((hipStream_t)stream);
  return coset_lde_dev_impl(field_id, d_coef, n_coef, offset_host, generator_host, d_out, order, (hipStream_t)stream);
}

int mzk_ntt_columns_dev(int field_id, const uint64_t* root, const void* d_in, void* d_out, size_t n_points, size_t cols, int inverse, void* stream) {
  MZK_ENTER();
  return ntt_columns_dev_impl(field_id, root, d_in, d_out, n_points, cols, inverse, (hipStream_t)stream);
}
int mzk_poly_scale(int field_id, const uint64_t* coef, size_t n, const uint64_t* ratio, const uint64_t* lead, uint64_t* out) {
  MZK_ENTER();
  WsFrame ws("mzk_poly_scale");
  if (n == 0) return MZK_OK;
  if (!coef || !out) { set_error("poly_scale: null pointer"); return MZK_E_ARG; }
  MZK_TRY(field_check(field_id, "poly_scale"));
  hipStream_t s = ctx().stream;
  WsGuard wsg(s);
  const size_t esz = field_bytes(field_id);
  void* d;
  MZK_TRY(stage_in(ws, WS_MISC_A, coef, n * esz, &d, s));
  MZK_TRY(poly_scale_dev_impl(field_id, d, n, ratio, lead, d, s));
  MZK_TRY(stage_out(out, d, n * esz, s));
  return MZK_OK;
}
int mzk_poly_scale_dev(int field_id, const void* d_coef, size_t n, const uint64_t* ratio_host, const uint64_t* lead_host, void* d_out, void* stream) {
  MZK_ENTER();
  return poly_scale_dev_impl(field_id, d_coef, n, ratio_host, lead_host, d_out, (hipStream_t)stream);
}

static size_t trimmed_len(const uint64_t* c, size_t n, int nl) {
  while (n > 0) {
    uint64_t acc = 0;
    for (int i = 0; i < nl; i++) acc |= c[(n - 1) * nl + i];
    if (acc) break;
    n--;
  }
  return n;
}

// The product a plan admits (mzk_mul_plan.h): the leading copy_a / copy_b elements of the host polynomials zero-padded to `order` on the
// device, both forward-transformed, Hadamard, inverse; then the first `keep` elements, trimmed or not, to the caller.  The three
// buffers are leases of the caller's frame, `order` elements each: the plan keeps every copy within them.
static int conv_on_device(WsFrame& ws, int fid, const MulPlan& P, const uint64_t* a, const uint64_t* b, const uint64_t* root, uint64_t* out,
                          size_t* out_len, hipStream_t s) {
  const size_t esz = field_bytes(fid), order = P.order;
  if (P.copy_a > order || P.copy_b > order || P.keep > order) { set_error("polynomial product: plan outside its buffers"); return MZK_E_ARG; }
  void *da, *db, *dc;
  MZK_TRY(ws.get(WS_MISC_A, order * esz, &da));
  MZK_TRY(ws.get(WS_MISC_B, order * esz, &db));
  MZK_TRY(ws.get(WS_MISC_C, order * esz, &dc));
  MZK_HIP(hipMemsetAsync(da, 0, order * esz, s));
  MZK_HIP(hipMemsetAsync(db, 0, order * esz, s));
  MZK_HIP(hipMemcpyAsync(da, a, P.copy_a * esz, hipMemcpyHostToDevice, s));
  MZK_HIP(hipMemcpyAsync(db, b, P.copy_b * esz, hipMemcpyHostToDevice, s));
  MZK_TRY(ntt_dev_impl(fid, root, da, da, order, 0, nullptr, s));      // order 1: the identity, the root is not looked at
  MZK_TRY(ntt_dev_impl(fid, root, db, db, order, 0, nullptr, s));
  MZK_TRY(pointwise_mul_dev(fid, da, db, dc, order, s));
  MZK_TRY(ntt_dev_impl(fid, root, dc, dc, order, 1, nullptr, s));
  const int nl = field_limbs64(fid);
  std::vector<uint64_t> res(order * nl);
  MZK_TRY(d2h_sync(res.data(), dc, order * esz, s));
  const size_t lo = P.trim ? trimmed_len(res.data(), P.keep, nl) : P.keep;
  memcpy(out, res.data(), lo * esz);
  *out_len = lo;
  return MZK_OK;
}

int mzk_fft_multiply(int field_id, const uint64_t* a, size_t la, const uint64_t* b, size_t lb, const uint64_t* omega,
                     uint64_t* out, size_t* out_len) {
  MZK_ENTER();
  WsFrame ws("mzk_fft_multiply");
  MZK_TRY(field_check(field_id, "fft_multiply"));
  if (!out_len || (!a && la) || (!b && lb)) { set_error("fft_multiply: null pointer"); return MZK_E_ARG; }
  const MulPlan P = fft_mul_plan(la, lb);
  if (P.err) { set_error(P.msg); return P.err; }
  if (P.empty) { *out_len = 0; return MZK_OK; }
  if (!out) { set_error("fft_multiply: null pointer"); return MZK_E_ARG; }
  // 1 x 1: the reference's fft() of length 1 is the identity (polynomial.rs:280-282) and omega is not used
  if (P.order > 1 && !omega) { set_error("fft_multiply: null omega"); return MZK_E_ARG; }
  hipStream_t s = ctx().stream;
  WsGuard wsg(s);
  return conv_on_device(ws, field_id, P, a, b, omega, out, out_len, s);
}

int mzk_fast_multiply(int field_id, const uint64_t* a, size_t la, const uint64_t* b, size_t lb, const uint64_t* root,
                      size_t root_order, uint64_t* out, size_t* out_len) {
  MZK_ENTER();
  WsFrame ws("mzk_fast_multiply");
  MZK_TRY(field_check(field_id, "fast_multiply"));
  if (!out_len || !root || (!a && la) || (!b && lb)) { set_error("fast_multiply: null pointer"); return MZK_E_ARG; }
  const HostField* hf = host_field(field_id);
  const int nl = hf->nl;
  if (!h_is_canonical(hf, root)) { set_error("fast_multiply: root not canonical"); return MZK_E_RANGE; }
  MZK_TRY(root_check(hf, root, root_order));  // ntt.rs:75-76
  const MulPlan P = fast_mul_plan(la, lb, trimmed_len(a, la, nl), trimmed_len(b, lb, nl), root_order);
  if (P.err) { set_error(P.msg); return P.err; }
  if (P.empty) { *out_len = 0; return MZK_OK; }  // ntt.rs:78-80
  if (!out) { set_error("fast_multiply: null pointer"); return MZK_E_ARG; }
  uint64_t r[4] = {0, 0, 0, 0};
  memcpy(r, root, 8 * nl);
  if (P.small) MZK_TRY(mzk_root_of_unity(field_id, MUL_SMALL_LOG, r));       // ntt.rs:86-88 `return lhs * rhs`: not the caller's root
  for (int i = 0; i < P.squarings; i++) h_mulmod(hf, r, r, r);               // ntt.rs:90-93
  hipStream_t s = ctx().stream;
  WsGuard wsg(s);
  return conv_on_device(ws, field_id, P, a, b, r, out, out_len, s);
}

// lhs / rhs of at most 8 coefficients (trimmed lengths tl <= 8, 0 < tr <= tl): the trimmed quotient into out, its length returned
static size_t small_poly_div(const HostField* hf, const uint64_t* lhs, size_t tl, const uint64_t* rhs, size_t tr, uint64_t* out) {
  const int nl = hf->nl;
  const size_t ql = tl - tr + 1;
  // ntt.rs:295-297 `return lhs / rhs`: true long division (polynomial.rs:371-405) of at most 8 coefficients --
  // parameter-sized work, done with the host parameter arithmetic
  uint64_t rem[8][4], quo[8][4], linv[4], lead[4], prod[4];
  memset(rem, 0, sizeof rem); memset(quo, 0, sizeof quo);
  for (size_t i = 0; i < tl; i++) memcpy(rem[i], lhs + i * nl, 8 * nl);
  h_invmod(hf, linv, rhs + (tr - 1) * nl);
  size_t rl = tl;
  while (rl >= tr) {
    h_mulmod(hf, lead, rem[rl - 1], linv);
    const size_t dd = rl - tr;
    memcpy(quo[dd], lead, 8 * nl);
    for (size_t i = 0; i < tr; i++) {
      h_mulmod(hf, prod, lead, rhs + i * nl);
      h_submod(hf, rem[dd + i], rem[dd + i], prod);
    }
    while (rl > 0 && h_is_zero(hf, rem[rl - 1])) rl--;
  }
  size_t qt = ql;
  while (qt > 0 && h_is_zero(hf, quo[qt - 1])) qt--;
  for (size_t i = 0; i < qt; i++) memcpy(out + i * nl, quo[i], 8 * nl);
  return qt;
}
// ntt::fast_coset_divide (ntt.rs:271-330): the quotient step of FastStark::prove (fast_stark.rs:265).
int mzk_fast_coset_divide(int field_id, const uint64_t* lhs, size_t ll, const uint64_t* rhs, size_t lr, const uint64_t* offset,
                          const uint64_t* root, size_t root_order, uint64_t* out, size_t* out_len) {
  MZK_ENTER();
  WsFrame ws("mzk_fast_coset_divide");
  MZK_TRY(field_check(field_id, "fast_coset_divide"));
  if (!out || !out_len || !root || !offset || (!lhs && ll) || (!rhs && lr)) { set_error("fast_coset_divide: null pointer"); return MZK_E_ARG; }
  const HostField* hf = host_field(field_id);
  const int nl = hf->nl;
  if (!h_is_canonical(hf, root) || !h_is_canonical(hf, offset)) { set_error("fast_coset_divide: parameter not canonical"); return MZK_E_RANGE; }
  MZK_TRY(root_check(hf, root, root_order));       // ntt.rs:281-282
  for (size_t i = 0; i < ll; i++) if (!h_is_canonical(hf, lhs + i * nl)) { set_error("fast_coset_divide: lhs[%zu] not canonical", i); return MZK_E_RANGE; }
  for (size_t i = 0; i < lr; i++) if (!h_is_canonical(hf, rhs + i * nl)) { set_error("fast_coset_divide: rhs[%zu] not canonical", i); return MZK_E_RANGE; }
  const size_t tl = trimmed_len(lhs, ll, nl), tr = trimmed_len(rhs, lr, nl);
  const DividePlan D = coset_divide_plan(tl, tr, root_order);
  if (D.err) { set_error("%s", D.msg); return D.err; }
  if (D.small) {
    *out_len = small_poly_div(hf, lhs, tl, rhs, tr, out);
    return MZK_OK;
  }
  uint64_t r[4] = {0, 0, 0, 0};
  memcpy(r, root, 8 * nl);
  for (int i = 0; i < D.squarings; i++) h_mulmod(hf, r, r, r);        // ntt.rs:298-302
  hipStream_t s = ctx().stream;
  WsGuard wsg(s);
  const size_t esz = field_bytes(field_id);
  void *d_l, *d_r, *d_o;
  MZK_TRY(stage_in(ws, WS_MISC_C, lhs, tl * esz, &d_l, s));
  MZK_TRY(stage_in(ws, WS_MISC_D, rhs, tr * esz, &d_r, s));
  MZK_TRY(ws.get(WS_NTT_IO_B, D.ql * esz, &d_o));
  MZK_TRY(coset_divide_dev_impl(field_id, d_l, tl, d_r, tr, offset, r, D.order, d_o, s));
  MZK_TRY(stage_out(out, d_o, D.ql * esz, s));
  *out_len = D.ql;
  return MZK_OK;
}

// fast_coset_divide of `count` numerators in HBM over ONE denominator (the transition quotients of fast_stark.rs:261-273), each row
// bit-identical to mzk_fast_coset_divide.  The trimmed lengths -- which decide the error checks, the degree < 8 branch and the
// squared-down order of ntt.rs:298-302 -- are found on the device first (one wait); rows of one order then share one batched forward
// transform, one denominator transform, one division launch, one batched inverse transform and one scale-back launch.
int mzk_fast_coset_divide_batch_dev(int field_id, const void* d_lhs, size_t lhs_stride, const size_t* lhs_lens, size_t count, const void* d_rhs,
                                    size_t rhs_len, const uint64_t* offset, const uint64_t* root, size_t root_order, void* d_out, size_t out_stride,
                                    size_t* out_lens, void* stream) {
  MZK_ENTER();
  MZK_TRY(field_check(field_id, "fast_coset_divide"));
  if (!root || !offset || (!d_rhs && rhs_len) || (count && (!lhs_lens || !out_lens || (!d_lhs && lhs_stride) || (!d_out && out_stride)))) {
    set_error("fast_coset_divide: null pointer");
    return MZK_E_ARG;
  }
  const HostField* hf = host_field(field_id);
  const int nl = hf->nl;
  if (!h_is_canonical(hf, root) || !h_is_canonical(hf, offset)) { set_error("fast_coset_divide: parameter not canonical"); return MZK_E_RANGE; }
  MZK_TRY(root_check(hf, root, root_order));       // ntt.rs:281-282
  for (size_t i = 0; i < count; i++)
    if (lhs_lens[i] > lhs_stride) { set_error("fast_coset_divide: row %zu has %zu coefficients, lhs_stride is %zu", i, lhs_lens[i], lhs_stride); return MZK_E_LENGTH; }
  if (count > ((size_t)1 << 20) || (lhs_stride && count > ((size_t)1 << 40) / lhs_stride) || (out_stride && count > ((size_t)1 << 40) / out_stride)) {
    set_error("fast_coset_divide: %zu rows are too many", count);
    return MZK_E_LENGTH;
  }
  if (count == 0) return MZK_OK;
  hipStream_t s = (hipStream_t)stream;
  WsGuard wsg(s);
  const size_t esz = field_bytes(field_id);
  if (rhs_len == 0) { set_error("assertion failed: !rhs.is_zero()"); return MZK_E_ARG; }                    // ntt.rs:284: no launch for an empty denominator
  std::vector<size_t> tl(count + 1);
  {   // the lengths are on the host when this returns: the lease ends here, coset_divide_rows_dev_impl takes WS_MISC_F itself
    WsFrame ws("mzk_fast_coset_divide_batch_dev (lengths)");
    MZK_TRY(rows_trimmed_len_dev(field_id, const_cast<void*>(d_lhs), lhs_stride, lhs_lens, count, 0, d_rhs, rhs_len, ws, WS_MISC_F, tl.data(), s));
  }
  const size_t tr = tl[count];
  struct Group { size_t order; uint64_t root[4]; std::vector<CdRow> rows; };
  std::vector<Group> groups;
  std::vector<size_t> small;
  for (size_t i = 0; i < count; i++) {
    // a row's refusals in order: the assertion on the degrees, this call's own check of the quotient against out_stride, then the
    // inner transform's assertions (a zero denominator, ntt.rs:283, has no quotient length and refuses row 0 in the last line)
    const DividePlan D = coset_divide_plan(tl[i], tr, root_order);
    if (D.err == MZK_E_LENGTH) { set_error("%s (row %zu)", D.msg, i); return D.err; }
    if (D.ql > out_stride) { set_error("fast_coset_divide: row %zu has a quotient of %zu coefficients, out_stride is %zu", i, D.ql, out_stride); return MZK_E_LENGTH; }
    if (D.err) { set_error("%s", D.msg); return D.err; }
    if (D.small) { small.push_back(i); continue; }
    size_t g = 0;
    while (g < groups.size() && groups[g].order != D.order) g++;
    if (g == groups.size()) {
      groups.push_back(Group());
      groups[g].order = D.order;
      memset(groups[g].root, 0, sizeof groups[g].root);
      memcpy(groups[g].root, root, 8 * nl);
      for (int k = 0; k < D.squarings; k++) h_mulmod(hf, groups[g].root, groups[g].root, groups[g].root);      // ntt.rs:298-302
    }
    groups[g].rows.push_back({i, tl[i]});
    out_lens[i] = D.ql;
  }
  auto fail = [&](int rc) { (void)hipStreamSynchronize(s); return rc; };
  if (!small.empty()) {      // ntt.rs:295-297 `return lhs / rhs`: at most 8 coefficients of a row visit the host; one wait in, one out for all
    const size_t ns = small.size();
    std::vector<uint64_t> hl(ns * 32, 0), hq(ns * 32, 0);
    uint64_t hr[8][4];
    for (size_t j = 0; j < ns; j++)
      if (hipMemcpyAsync(&hl[j * 32], (const char*)d_lhs + small[j] * lhs_stride * esz, tl[small[j]] * esz, hipMemcpyDeviceToHost, s) != hipSuccess) return fail(MZK_E_HIP);
    int rc = d2h_sync(hr, d_rhs, tr * esz, s);                // the stream is idle afterwards: the rows above have arrived too
    if (rc != MZK_OK) return fail(rc);
    for (size_t j = 0; j < ns; j++) {
      const size_t i = small[j];
      // the copies pack elements of nl limbs back to back: view the arrays that way
      const size_t qt = small_poly_div(hf, &hl[j * 32], tl[i], (const uint64_t*)hr, tr, &hq[j * 32]);
      char* row = (char*)d_out + i * out_stride * esz;
      if (hipMemsetAsync(row, 0, out_stride * esz, s) != hipSuccess) return fail(MZK_E_HIP);
      if (qt && hipMemcpyAsync(row, &hq[j * 32], qt * esz, hipMemcpyHostToDevice, s) != hipSuccess) return fail(MZK_E_HIP);
      out_lens[i] = qt;
    }
    if (hipStreamSynchronize(s) != hipSuccess) return fail(MZK_E_HIP);          // hq leaves scope
  }
  for (const Group& g : groups) {
    const int rc = coset_divide_rows_dev_impl(field_id, d_lhs, lhs_stride, g.rows.data(), g.rows.size(), d_rhs, tr, offset, g.root, g.order, d_out, out_stride, s);
    if (rc != MZK_OK) return fail(rc);
  }
  MZK_HIP(hipStreamSynchronize(s));
  return MZK_OK;
}

// ---- MSM / KZG ---------------------------------------------------------------------------------------------
// (the SRS handle, its constructors and its tables: mzk_srs.h, mzk_srs.hip)
int mzk_msm_g1_bn254(const uint64_t* scalars, const uint64_t* points_xy, size_t n, uint64_t out_xy[8]) {
  MZK_ENTER();
  WsFrame ws("mzk_msm_g1_bn254");
  if (!out_xy || ((!scalars || !points_xy) && n)) { set_error("msm: null pointer"); return MZK_E_ARG; }
  hipStream_t s = ctx().stream;
  WsGuard wsg(s);
  void *d_s, *d_p, *d_o;
  // The points (64 n bytes) travel on a side stream while the context's stream already sorts the scalars' digits: the side
  // stream starts behind everything enqueued so far (the previous call may still read the points' slot), the kernels that read
  // the points wait for it (msm_dev_impl calls points_ready after the sort is enqueued).
  hipStream_t side;
  hipEvent_t fork, join;
  MZK_TRY(side_stream(&side, &fork, &join));
  MZK_TRY(ws.get(WS_MISC_A, n ? n * 64 : 16, &d_p));
  MZK_TRY(ws.get(WS_MISC_B, 256, &d_o));
  if (msm_chunkable(n, MsmPoints::plain(d_p)) && host_chunks_enabled()) {
    // four equal pieces of scalars + points: the transfers (96 bytes per pair: 1.7 ms at 2^20) run under the pieces' kernels but for
    // the first piece's (profiles/round6_host_buffer_chunks.txt)
    static const int quarters[4] = {64, 128, 192, 256};
    MsmChunk ch[8];
    MZK_TRY(ws.get(WS_MSM_SCALARS, n * 32, &d_s));
    const int K = host_chunk_plan(n, "MZK_HOST_CHUNKS_MSM", quarters, 4, ch);
    MZK_TRY(msm_host_chunked(scalars, points_xy, d_s, d_p, MsmPoints::plain(d_p), n, d_o, s, ch, K));
    MZK_TRY(d2h_sync(out_xy, d_o, 64, s));
    return MZK_OK;
  }
  MZK_HIP(hipEventRecord(fork, s));
  MZK_HIP(hipStreamWaitEvent(side, fork, 0));
  MZK_TRY(stage_in(ws, WS_MSM_SCALARS, scalars, n * 32, &d_s, s));
  const std::function<int()> points_ready = [&]() -> int {
    if (n) MZK_HIP(hipMemcpyAsync(d_p, points_xy, n * 64, hipMemcpyHostToDevice, side));
    MZK_HIP(hipEventRecord(join, side));
    MZK_HIP(hipStreamWaitEvent(s, join, 0));
    return MZK_OK;
  };
  MZK_TRY(msm_dev_impl(d_s, MsmPoints::plain(d_p), n, d_o, false, s, &points_ready));
  MZK_TRY(d2h_sync(out_xy, d_o, 64, s));
  return MZK_OK;
}
int mzk_msm_g1_bn254_dev(const void* d_scalars, const void* d_points_xy, size_t n, void* d_out_xy, void* stream) {
  MZK_ENTER();
  WsGuard wsg((hipStream_t)stream);
  return msm_dev_impl(d_scalars, MsmPoints::plain(d_points_xy), n, d_out_xy, false, (hipStream_t)stream);
}
int mzk_msm_g1_bn254_partial_dev(const void* d_scalars, const void* d_points_xy, size_t n, void* d_partial16, void* stream) {
  MZK_ENTER();
  WsGuard wsg((hipStream_t)stream);
  return msm_dev_impl(d_scalars, MsmPoints::plain(d_points_xy), n, d_partial16, true, (hipStream_t)stream);
}
int mzk_g1_fold_partials_dev(const void* d_partials16, int count, void* d_out_xy, void* stream) {
  MZK_ENTER();
  WsGuard wsg((hipStream_t)stream);
  return msm_fold_partials_impl(d_partials16, count, d_out_xy, (hipStream_t)stream);
}

int mzk_set_workspace_budget(size_t bytes) {
  MZK_ENTER();
  g_ws_budget = bytes;
  if (bytes) {
    for (int i = 0; i < ctx_count(); i++) {
      CtxScope sc(i);
      if (sc.ok && ws_bytes_held() > bytes) (void)ws_trim_idle();
    }
  }
  return MZK_OK;
}
int mzk_trim_workspace(size_t* bytes_released) {
  MZK_ENTER();
  size_t total = 0;
  for (int i = 0; i < ctx_count(); i++) {
    CtxScope sc(i);
    if (!sc.ok) continue;
    total += ws_trim_idle();
    (void)hipDeviceSynchronize();
    ntt_release_plans();           // tables of the cached transform plans: rebuilt on the next call that needs them
  }
  if (bytes_released) *bytes_released = total;
  return MZK_OK;
}
int mzk_workspace_bytes(size_t* bytes) {
  MZK_ENTER();
  if (!bytes) { set_error("workspace_bytes: null pointer"); return MZK_E_ARG; }
  size_t total = 0;
  for (int i = 0; i < ctx_count(); i++) {
    CtxScope sc(i);
    if (sc.ok) total += ws_bytes_held();
  }
  *bytes = total;
  return MZK_OK;
}
int mzk_kzg_commit_srs(const mzk_srs* srs, const uint64_t* coef, size_t n, uint64_t out_xy[8]) {
  MZK_ENTER();
  WsFrame ws("mzk_kzg_commit_srs");
  if (!srs || !out_xy || (!coef && n)) { set_error("commit_srs: null pointer"); return MZK_E_ARG; }
  MZK_TRY(srs_check_ctx(srs));
  if (n > srs->n) { set_error("index out of bounds: the len is %zu but the index is %zu", srs->n, srs->n); return MZK_E_LENGTH; }  // powers[i], polynomial.rs:162
  hipStream_t s = ctx().stream;
  WsGuard wsg(s);
  void *d_s, *d_o;
  MZK_TRY(ws.get(WS_MISC_B, 256, &d_o));
  if (msm_chunkable(n, srs->points()) && host_chunks_enabled()) {
    // a quarter of the coefficients first, the rest under its kernels (two pieces: every piece costs a segment combine of its own)
    static const int quarter_then_rest[2] = {64, 256};
    MsmChunk ch[8];
    MZK_TRY(ws.get(WS_MSM_SCALARS, n * 32, &d_s));
    const int K = host_chunk_plan(n, "MZK_HOST_CHUNKS_COMMIT", quarter_then_rest, 2, ch);
    MZK_TRY(msm_host_chunked(coef, nullptr, d_s, nullptr, srs->points(), n, d_o, s, ch, K));
    MZK_TRY(d2h_sync(out_xy, d_o, 64, s));
    return MZK_OK;
  }
  MZK_TRY(stage_in(ws, WS_MSM_SCALARS, coef, n * 32, &d_s, s));
  MZK_TRY(msm_dev_impl(d_s, srs->points(), n, d_o, false, s));
  MZK_TRY(d2h_sync(out_xy, d_o, 64, s));
  return MZK_OK;
}

int mzk_kzg_commit_srs_dev(const mzk_srs* srs, const void* d_coef, size_t n, void* d_out, int out_partial, void* stream) {
  MZK_ENTER();
  WsGuard wsg((hipStream_t)stream);
  if (!srs || !d_out || (!d_coef && n)) { set_error("commit_srs_dev: null pointer"); return MZK_E_ARG; }
  MZK_TRY(srs_check_ctx(srs));
  if (n > srs->n) { set_error("index out of bounds: the len is %zu but the index is %zu", srs->n, srs->n); return MZK_E_LENGTH; }
  return msm_dev_impl(d_coef, srs->points(), n, d_out, out_partial != 0, (hipStream_t)stream);
}

}  // extern "C" (the lane scheduler is a template)

// `count` independent jobs (commitments, openings) against one SRS, one job in flight per context of this GPU.  Context k of
// the same device runs jobs k, k + K, ... on its own stream and workspace (the bucket reduction / inversion tail and the
// memory-bound sort of one MSM run under the accumulation of the others); the caller's stream forks into them and joins
// them.  job(i, stream) enqueues job i under the current context.
template <class JOB>
static int run_in_flight(size_t count, int max_in_flight, hipStream_t caller, JOB job) {
  const int home = ctx().index, dev = ctx().device;
  int lanes[MZK_MAX_CTX], K = 0;
  lanes[K++] = home;
  // default four: more in flight measured slower at 2^20; an explicit request may go up to eight
  const int cap = max_in_flight < 1 ? 4 : (max_in_flight > 8 ? 8 : max_in_flight);
  for (int i = 0; i < g_nctx && K < cap; i++)
    if (i != home && g_ctxs[i].ready && g_ctxs[i].device == dev) lanes[K++] = i;
  if ((size_t)K > count) K = (int)count;
  if (K == 1) {                                         // no second context on this GPU: plain sequence on the caller's stream
    WsGuard wsg(caller);
    for (size_t i = 0; i < count; i++) MZK_TRY(job(i, caller));
    return MZK_OK;
  }
  // Lane 0 is the current context ON THE CALLER'S STREAM (no further stream: one of the same priority as the caller's
  // may share its hardware queue, and the join below would then hold that lane back until all others are done --
  // measured: 1.87 instead of 1.51 ms per commit with two lanes); lanes 1.. are the other contexts on their own streams.
  // fork: those streams wait for what the caller's stream has enqueued so far (the inputs)
  Context& h = g_ctxs[home];
  if (!h.fork_event) MZK_HIP(hipEventCreateWithFlags(&h.fork_event, hipEventDisableTiming));
  MZK_HIP(hipEventRecord(h.fork_event, caller));
  int rc = MZK_OK;
  for (int k = 1; k < K && rc == MZK_OK; k++)
    if (hipStreamWaitEvent(g_ctxs[lanes[k]].stream, h.fork_event, 0) != hipSuccess) rc = hip_fail(hipGetLastError(), "hipStreamWaitEvent", __FILE__, __LINE__);
  // job i goes to lane i mod K, enqueued in that order: the lanes start one enqueue time apart and stay staggered,
  // which is what puts one MSM's tail under another's accumulation (lane by lane they would start a whole lane's work
  // apart and run their accumulations side by side)
  for (size_t i = 0; i < count && rc == MZK_OK; i++) {
    const int k = (int)(i % (size_t)K);
    CtxScope scope(lanes[k]);
    if (!scope.ok) { rc = MZK_E_ARG; break; }
    hipStream_t ls = k == 0 ? caller : ctx().stream;
    WsGuard wsg(ls);
    ctx().lanes_in_flight = K;       // the job's launches are chosen for a chip that other jobs occupy (launch_halving_steps)
    rc = job(i, ls);
    ctx().lanes_in_flight = 1;
  }
  // join: the caller's stream continues after every lane's last job (also after a failure: nothing may be left running
  // behind the caller's back)
  for (int k = 1; k < K; k++) {
    Context& c = g_ctxs[lanes[k]];
    if (!c.join_event && hipEventCreateWithFlags(&c.join_event, hipEventDisableTiming) != hipSuccess) { (void)hipGetLastError(); (void)hipStreamSynchronize(c.stream); continue; }
    if (hipEventRecord(c.join_event, c.stream) != hipSuccess || hipStreamWaitEvent(caller, c.join_event, 0) != hipSuccess) {
      (void)hipGetLastError();
      (void)hipStreamSynchronize(c.stream);
    }
  }
  return rc;
}

extern "C" {

// Short polynomials against narrow window tables: the whole batch as ONE bucket problem (msm_many_dev_impl) instead of one
// commit per lane -- every kernel of it runs over (polynomial x bucket), one tail workgroup per polynomial.

int mzk_msm_generic_window_bits(size_t n) { return mzk::msm_generic_window_bits(n); }
// The _many forms take the grid pass whenever the handle can (any count >= 1); the _batch forms from MANY_MIN_COUNT polynomials
// on (two or three are served as well by the lanes: the pass has ~10 launches and an 80-us tail of its own).
constexpr size_t MANY_MIN_COUNT = 4;
static int commit_batch_route(const mzk_srs* srs, const void* d_coefs, size_t n, size_t count, void* d_out_xy, int max_in_flight, size_t many_from, hipStream_t stream) {
  if (!srs || ((!d_coefs || !d_out_xy) && count)) { set_error("commit_srs_batch_dev: null pointer"); return MZK_E_ARG; }
  MZK_TRY(srs_check_ctx(srs));
  if (n > srs->n) { set_error("index out of bounds: the len is %zu but the index is %zu", srs->n, srs->n); return MZK_E_LENGTH; }
  if (count == 0) return MZK_OK;
  if (count >= many_from && srs_many_capable(srs)) {
    WsGuard wsg(stream);
    return msm_many_srs(srs, d_coefs, n, n, count, d_out_xy, stream);
  }
  const char* coefs = (const char*)d_coefs;
  char* outs = (char*)d_out_xy;
  return run_in_flight(count, max_in_flight, stream, [&](size_t i, hipStream_t ls) {
    return msm_dev_impl(coefs + i * n * 32, srs->points(), n, outs + i * 64, false, ls);
  });
}
// open_kzg (kzg.rs:61-72) of `count` polynomials, polynomial i at the point us[i]: y_i = f_i(u_i) and the witness
// commitment w_i, the quotient and its MSM of each opening on one lane
static int open_batch_route(const mzk_srs* srs, const void* d_coefs, size_t n, size_t count, const uint64_t* us_host, void* d_ys, void* d_ws_xy, int max_in_flight,
                            size_t many_from, hipStream_t stream) {
  if (!srs || ((!d_coefs || !us_host || !d_ys || !d_ws_xy) && count)) { set_error("open_srs_batch_dev: null pointer"); return MZK_E_ARG; }
  MZK_TRY(srs_check_ctx(srs));
  if (n > 1 && n - 1 > srs->n) { set_error("index out of bounds: the len is %zu but the index is %zu", srs->n, srs->n); return MZK_E_LENGTH; }
  if (count == 0) return MZK_OK;
  if (count >= many_from && kzg_open_many_supported(srs, n)) {
    WsGuard wsg(stream);
    return kzg_open_many_dev(srs, d_coefs, n, count, us_host, d_ys, d_ws_xy, stream);
  }
  const char* coefs = (const char*)d_coefs;
  char *ys = (char*)d_ys, *ws = (char*)d_ws_xy;
  return run_in_flight(count, max_in_flight, stream, [&](size_t i, hipStream_t ls) {
    return kzg_open_dev(coefs + i * n * 32, n, us_host + 4 * i, srs->points(), ys + i * 32, ws + i * 64, nullptr, ls);
  });
}
int mzk_kzg_commit_srs_many_dev(const mzk_srs* srs, const void* d_coefs, size_t n, size_t count, void* d_out_xy, void* stream) {
  MZK_ENTER();
  return commit_batch_route(srs, d_coefs, n, count, d_out_xy, 0, 1, (hipStream_t)stream);
}
int mzk_kzg_open_srs_many_dev(const mzk_srs* srs, const void* d_coefs, size_t n, size_t count, const uint64_t* us_host, void* d_ys, void* d_ws_xy,
                              void* stream) {
  MZK_ENTER();
  return open_batch_route(srs, d_coefs, n, count, us_host, d_ys, d_ws_xy, 0, 1, (hipStream_t)stream);
}
int mzk_kzg_commit_srs_batch_dev(const mzk_srs* srs, const void* d_coefs, size_t n, size_t count, void* d_out_xy, int max_in_flight,
                                 void* stream) {
  MZK_ENTER();
  return commit_batch_route(srs, d_coefs, n, count, d_out_xy, max_in_flight, MANY_MIN_COUNT, (hipStream_t)stream);
}
int mzk_kzg_open_srs_batch_dev(const mzk_srs* srs, const void* d_coefs, size_t n, size_t count, const uint64_t* us_host, void* d_ys, void* d_ws_xy,
                               int max_in_flight, void* stream) {
  MZK_ENTER();
  return open_batch_route(srs, d_coefs, n, count, us_host, d_ys, d_ws_xy, max_in_flight, MANY_MIN_COUNT, (hipStream_t)stream);
}
// open_kzg of `count` polynomials with everything in host memory: ys = count * 4 limbs, ws_xy = count * 8 limbs
int mzk_kzg_open_srs_batch(const mzk_srs* srs, const uint64_t* coefs, size_t n, size_t count, const uint64_t* us, uint64_t* ys, uint64_t* ws_xy) {
  MZK_ENTER();
  WsFrame ws("mzk_kzg_open_srs_batch");
  if (!srs || ((!coefs || !us || !ys || !ws_xy) && count)) { set_error("open_srs_batch: null pointer"); return MZK_E_ARG; }
  if (count == 0) return MZK_OK;
  hipStream_t s = ctx().stream;
  void *d_c, *d_o;
  {
    WsGuard wsg(s);
    MZK_TRY(stage_in(ws, WS_MISC_E, coefs, count * n * 32, &d_c, s));
    MZK_TRY(ws.get(WS_MISC_F, count * 96, &d_o));
  }
  char* d_y = (char*)d_o;
  char* d_w = d_y + count * 32;
  MZK_TRY(open_batch_route(srs, d_c, n, count, us, d_y, d_w, 0, MANY_MIN_COUNT, s));
  MZK_HIP(hipMemcpyAsync(ys, d_y, count * 32, hipMemcpyDeviceToHost, s));
  MZK_TRY(d2h_sync(ws_xy, d_w, count * 64, s));
  return MZK_OK;
}
int mzk_kzg_commit_srs_batch(const mzk_srs* srs, const uint64_t* coefs, size_t n, size_t count, uint64_t* out_xy) {
  MZK_ENTER();
  WsFrame ws("mzk_kzg_commit_srs_batch");
  if (!srs || ((!coefs || !out_xy) && count)) { set_error("commit_srs_batch: null pointer"); return MZK_E_ARG; }
  if (count == 0) return MZK_OK;
  hipStream_t s = ctx().stream;
  void *d_c, *d_o;
  {
    WsGuard wsg(s);
    MZK_TRY(stage_in(ws, WS_MISC_E, coefs, count * n * 32, &d_c, s));
    MZK_TRY(ws.get(WS_MISC_F, count * 64, &d_o));
  }
  MZK_TRY(mzk_kzg_commit_srs_batch_dev(srs, d_c, n, count, d_o, 0, s));
  MZK_TRY(d2h_sync(out_xy, d_o, count * 64, s));
  return MZK_OK;
}

int mzk_kzg_open_srs_dev(const mzk_srs* srs, const void* d_coef, size_t n, const uint64_t u_host[4], void* d_y, void* d_w_xy, void* stream) {
  MZK_ENTER();
  WsGuard wsg((hipStream_t)stream);
  if (!srs) { set_error("open_srs_dev: null srs"); return MZK_E_ARG; }
  MZK_TRY(srs_check_ctx(srs));
  if (n > 1 && n - 1 > srs->n) { set_error("index out of bounds: the len is %zu but the index is %zu", srs->n, srs->n); return MZK_E_LENGTH; }
  if (!d_w_xy) { set_error("kzg_open: null pointer"); return MZK_E_ARG; }
  return kzg_open_dev(d_coef, n, u_host, srs->points(), d_y, d_w_xy, nullptr, (hipStream_t)stream);
}
int mzk_kzg_setup_g1_dev(const uint64_t alpha_host[4], const uint64_t g1_xy_host[8], size_t max_d, void* d_powers_xy, void* stream) {
  MZK_ENTER();
  WsGuard wsg((hipStream_t)stream);
  return kzg_setup_g1_dev(alpha_host, g1_xy_host, 0, max_d + 1, d_powers_xy, (hipStream_t)stream);
}
int mzk_kzg_setup_g1_range_dev(const uint64_t alpha_host[4], const uint64_t g1_xy_host[8], size_t first, size_t count, void* d_powers_xy,
                               void* stream) {
  MZK_ENTER();
  WsGuard wsg((hipStream_t)stream);
  return kzg_setup_g1_dev(alpha_host, g1_xy_host, first, count, d_powers_xy, (hipStream_t)stream);
}
int mzk_kzg_open_quotient_dev(const void* d_coef, size_t n, const uint64_t u_host[4], void* d_y, void* d_q, void* stream) {
  MZK_ENTER();
  WsGuard wsg((hipStream_t)stream);
  if (!d_q && n > 1) { set_error("open_quotient: null pointer"); return MZK_E_ARG; }
  return kzg_open_dev(d_coef, n, u_host, MsmPoints::plain(nullptr), d_y, nullptr, d_q, (hipStream_t)stream);
}
int mzk_kzg_open_slice_value_dev(const void* d_coef_slice, size_t len, const uint64_t u_host[4], void* d_value, void* stream) {
  MZK_ENTER();
  WsGuard wsg((hipStream_t)stream);
  if (!d_value || !u_host || (!d_coef_slice && len)) { set_error("open_slice_value: null pointer"); return MZK_E_ARG; }
  // the slice's own recurrence with nothing behind it: b_lo = the slice as a polynomial, evaluated at u (kzg_open_dev's y)
  return kzg_open_dev(d_coef_slice, len, u_host, MsmPoints::plain(nullptr), d_value, nullptr, nullptr, (hipStream_t)stream);
}
int mzk_kzg_open_slice_quotient_dev(const void* d_coef_slice, size_t len, const uint64_t u_host[4], const uint64_t carry_in[4], void* d_q_slice,
                                    void* stream) {
  MZK_ENTER();
  hipStream_t s = (hipStream_t)stream;
  WsGuard wsg(s);
  if (!u_host || !carry_in || ((!d_coef_slice || !d_q_slice) && len)) { set_error("open_slice_quotient: null pointer"); return MZK_E_ARG; }
  if (!h_is_canonical(host_field(MZK_FIELD_FR), carry_in)) { set_error("open_slice_quotient: carry not canonical"); return MZK_E_RANGE; }
  if (len == 0) return MZK_OK;
  if (!h_is_canonical(host_field(MZK_FIELD_FR), u_host)) { set_error("kzg_open: u not canonical"); return MZK_E_RANGE; }
  // b over the slice from b_len = carry: one division whose end is the carry (read into the job table here); its quotient
  // b_1 .. b_len is the slice of q
  const SdJob job = {d_coef_slice, len, u_host, carry_in, nullptr, d_q_slice};
  const size_t one = 1;
  return synth_div_dev(&job, &one, 1, s);
}
int mzk_fri_fold_dev(int field_id, const void* d_codeword, size_t n, const uint64_t* alpha_host, const uint64_t* offset_host,
                     const uint64_t* omega_host, void* d_out, void* stream) {
  MZK_ENTER();
  WsGuard wsg((hipStream_t)stream);
  return fri_fold_dev_impl(field_id, d_codeword, n, alpha_host, offset_host, omega_host, d_out, (hipStream_t)stream);
}
int mzk_fri_fold(int field_id, const uint64_t* codeword, size_t n, const uint64_t* alpha, const uint64_t* offset,
                 const uint64_t* omega, uint64_t* out) {
  MZK_ENTER();
  WsFrame ws("mzk_fri_fold");
  MZK_TRY(field_check_gl(field_id, "fri_fold"));
  if (n / 2 == 0) return MZK_OK;
  if (!codeword || !out) { set_error("fri_fold: null pointer"); return MZK_E_ARG; }
  hipStream_t s = ctx().stream;
  WsGuard wsg(s);
  const size_t esz = field_bytes(field_id);
  void *d_in, *d_out;
  MZK_TRY(stage_in(ws, WS_NTT_IO_A, codeword, n * esz, &d_in, s));
  MZK_TRY(ws.get(WS_NTT_IO_B, (n / 2) * esz, &d_out));
  MZK_TRY(fri_fold_dev_impl(field_id, d_in, n, alpha, offset, omega, d_out, s));
  MZK_TRY(stage_out(out, d_out, (n / 2) * esz, s));
  return MZK_OK;
}

int mzk_kzg_batch_open(const uint64_t* coef, size_t n, const uint64_t* us, size_t k, const uint64_t* powers_xy, uint64_t* ys,
                       uint64_t w_xy[8]) {
  MZK_ENTER();
  WsFrame ws("mzk_kzg_batch_open");
  if (!w_xy || (!coef && n) || ((!us || !ys) && k) || (!powers_xy && n > k)) { set_error("batch_open: null pointer"); return MZK_E_ARG; }
  hipStream_t s = ctx().stream;
  WsGuard wsg(s);
  const size_t nq = n > k ? n - k : 0;
  void *d_c, *d_p, *d_o;
  MZK_TRY(stage_in(ws, WS_MSM_SCALARS, coef, n * 32, &d_c, s));
  MZK_TRY(stage_in(ws, WS_NTT_IO_A, powers_xy, nq * 64, &d_p, s));
  MZK_TRY(ws.get(WS_NTT_IO_B, 64 + k * 32 + 64, &d_o));
  MZK_TRY(kzg_batch_open_dev(d_c, n, us, k, MsmPoints::plain(d_p), (char*)d_o + 64, d_o, s));
  std::vector<uint64_t> tmp(8 + 4 * k + 8);
  MZK_TRY(d2h_sync(tmp.data(), d_o, 64 + k * 32, s));
  memcpy(w_xy, tmp.data(), 64);
  if (k) memcpy(ys, tmp.data() + 8, k * 32);
  return MZK_OK;
}

int mzk_kzg_prove_degree_bound(const uint64_t* coef, size_t n, const uint64_t* powers_xy, size_t n_powers, size_t d, uint64_t out_xy[8]) {
  MZK_ENTER();
  if (!out_xy || (!coef && n) || (!powers_xy && n_powers)) { set_error("degree_bound: null pointer"); return MZK_E_ARG; }
  if (n_powers == 0 || d > n_powers - 1) { set_error("attempt to subtract with overflow (max_d - d)"); return MZK_E_LENGTH; }
  const size_t shift = n_powers - 1 - d;
  const size_t tl = trimmed_len(coef, n, 4);   // f * q is trimmed (polynomial.rs:313-315)
  if (tl == 0) { memset(out_xy, 0, 64); return MZK_OK; }
  if (shift + tl > n_powers) { set_error("index out of bounds: the len is %zu but the index is %zu", n_powers, n_powers); return MZK_E_LENGTH; }
  // MSM(f * X^shift, powers) = MSM(f, powers[shift..])
  return mzk_msm_g1_bn254(coef, powers_xy + 8 * shift, tl, out_xy);
}

int mzk_kzg_setup_g1(const uint64_t alpha[4], const uint64_t g1_xy[8], size_t max_d, uint64_t* powers_xy) {
  MZK_ENTER();
  WsFrame ws("mzk_kzg_setup_g1");
  if (!alpha || !g1_xy || !powers_xy) { set_error("kzg_setup: null pointer"); return MZK_E_ARG; }
  hipStream_t s = ctx().stream;
  WsGuard wsg(s);
  const size_t count = max_d + 1;  // `for _ in 0..1 + max_d`, kzg.rs:32
  void* d_p;
  MZK_TRY(ws.get(WS_MSM_POINTS, count * 64, &d_p));
  MZK_TRY(kzg_setup_g1_dev(alpha, g1_xy, 0, count, d_p, s));
  MZK_TRY(stage_out(powers_xy, d_p, count * 64, s));
  return MZK_OK;
}

int mzk_kzg_open(const uint64_t* coef, size_t n, const uint64_t u[4], const uint64_t* powers_xy, uint64_t y[4], uint64_t w_xy[8]) {
  MZK_ENTER();
  WsFrame ws("mzk_kzg_open");
  if (!u || !y || !w_xy || (!coef && n) || (!powers_xy && n > 1)) { set_error("kzg_open: null pointer"); return MZK_E_ARG; }
  hipStream_t s = ctx().stream;
  WsGuard wsg(s);
  void *d_c, *d_p, *d_o;
  MZK_TRY(stage_in(ws, WS_MSM_SCALARS, coef, n * 32, &d_c, s));
  MZK_TRY(stage_in(ws, WS_NTT_IO_A, powers_xy, (n > 1 ? n - 1 : 0) * 64, &d_p, s));
  MZK_TRY(ws.get(WS_NTT_IO_B, 256, &d_o));
  MZK_TRY(kzg_open_dev(d_c, n, u, MsmPoints::plain(d_p), d_o, (char*)d_o + 64, nullptr, s));
  uint64_t tmp[16];
  MZK_TRY(d2h_sync(tmp, d_o, 128, s));
  memcpy(y, tmp, 32);
  memcpy(w_xy, tmp + 8, 64);
  return MZK_OK;
}

int mzk_synth_field_dev(int field_id, uint64_t seed, size_t n, void* d_out, void* stream) {
  MZK_ENTER();
  WsGuard wsg((hipStream_t)stream);
  if (!d_out && n) { set_error("synth: null pointer"); return MZK_E_ARG; }
  return synth_field_impl(field_id, seed, n, d_out, (hipStream_t)stream);
}
int mzk_selftest_copy_dev(const void* d_src, void* d_dst, size_t bytes, void* stream) {
  MZK_ENTER();
  if ((bytes && (!d_src || !d_dst)) || (bytes & 15) || ((uintptr_t)d_src & 15) || ((uintptr_t)d_dst & 15)) { set_error("selftest_copy: pointers and size must be 16-byte multiples"); return MZK_E_ARG; }
  return selftest_copy_impl(d_src, d_dst, bytes, (hipStream_t)stream);
}
int mzk_selftest_field_asm(int field_id, uint64_t seed, size_t n, uint64_t* mismatches) {
  MZK_ENTER();
  if (!mismatches) { set_error("selftest: null pointer"); return MZK_E_ARG; }
  WsGuard wsg(ctx().stream);
  return selftest_field_asm_impl(field_id, seed, n, mismatches, ctx().stream);
}
int mzk_selftest_row_ec(uint64_t seed, size_t n, int dbl_reps, uint64_t* mismatches) {
  MZK_ENTER();
  if (!mismatches || dbl_reps < 0 || n > ((size_t)1 << 22)) { set_error("selftest_row_ec: bad argument"); return MZK_E_ARG; }
  WsGuard wsg(ctx().stream);
  return selftest_row_ec_impl(seed, n, dbl_reps, mismatches, ctx().stream);
}
int mzk_selftest_inv_wave(uint64_t seed, size_t n, uint64_t* mismatches) {
  MZK_ENTER();
  if (!mismatches || n > ((size_t)1 << 22)) { set_error("selftest_inv_wave: bad argument"); return MZK_E_ARG; }
  WsGuard wsg(ctx().stream);
  return selftest_inv_wave_impl(seed, n, mismatches, ctx().stream);
}
int mzk_selftest_field_probe(int field_id, int op, int form, size_t n, const uint32_t* in, uint32_t* out) {
  MZK_ENTER();
  int limbs = 0;
  if (selftest_field_probe_arity(field_id, op, form, &limbs) == 0) { set_error("field_probe: no field %d / op %d / form %d", field_id, op, form); return MZK_E_ARG; }
  if (!in || !out || n > ((size_t)1 << 20)) { set_error("field_probe: null pointer or more than 2^20 cases"); return MZK_E_ARG; }
  WsGuard wsg(ctx().stream);
  return selftest_field_probe_impl(field_id, op, form, n, in, out, ctx().stream);
}
int mzk_selftest_g1_probe(int op, int form, size_t n, const uint32_t* a, const uint32_t* b, const uint8_t* neg, uint32_t* out) {
  MZK_ENTER();
  int aw = 0, bw = 0;
  if (selftest_g1_probe_check(op, form, &aw, &bw) != MZK_OK) { set_error("g1_probe: no op %d / form %d", op, form); return MZK_E_ARG; }
  if (!a || !out || (bw && !b) || (op == MZK_PROBE_G1_MADD_SIGNED && !neg) || n > ((size_t)1 << 20)) {
    set_error("g1_probe: null pointer or more than 2^20 cases");
    return MZK_E_ARG;
  }
  WsGuard wsg(ctx().stream);
  return selftest_g1_probe_impl(op, form, n, a, b, neg, out, ctx().stream);
}
int mzk_synth_g1_points_dev(uint64_t seed, size_t n, void* d_out_xy, void* stream) {
  MZK_ENTER();
  WsGuard wsg((hipStream_t)stream);
  if (!d_out_xy && n) { set_error("synth: null pointer"); return MZK_E_ARG; }
  return synth_g1_impl(seed, n, d_out_xy, (hipStream_t)stream);
}

}  // extern "C"
