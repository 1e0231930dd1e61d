// mzk_ws.h -- the workspace's bookkeeping: which scratch slot holds how many bytes, who holds it, which outermost call last asked for
// it, the budget, the trim and the growth.  Host only and free of HIP, so tests/hostcheck/ws_shim.cpp runs every rule below on a CPU
// with malloc behind it; the library binds the four device hooks in mzk_api.hip.
//
// Scratch slots are LEASED.  A function that takes scratch puts a WsFrame on its stack and asks it for slots; the frame holds them
// until it goes out of scope.  A slot that is held is refused to everybody (MZK_E_ARG, naming both parties, nothing enqueued, freed or
// grown) -- the frame that holds it included: a callee that would have been handed its caller's live buffer, or would have freed it by
// asking for more bytes, now fails where it asks.  Releasing waits for nothing: reuse is safe for the reasons it always was (stream
// order on one stream, WsGuard across streams).
// Cache slots hold device tables that SURVIVE calls (fixed-base tables of g, offset powers); they are not leased, and every cache
// keyed by ws_generation() dies when one of them is freed.
//
// Everything else the library keeps on the device comes through dev_alloc and leaves through ws_hook_free as well: WsBlock, the
// polynomial routines' temporaries out of a per-context pool of size classes, and DevMem, the owner of one plain allocation (plan
// tables, handle buffers).  The plan caches share one stamp counter and one eviction, lru_evict.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <memory>
#include <utility>
#include <vector>
#include "../../include/mzk.h"

namespace mzk {

constexpr int MZK_MAX_CTX = 16;

#define MZK_WS_SLOTS(X)                                                                                                              \
  X(WS_NTT_TMP) X(WS_NTT_IO_A) X(WS_NTT_IO_B) X(WS_MSM_POINTS) X(WS_MSM_SCALARS) X(WS_MSM_COUNTS) X(WS_MSM_OFFSETS) X(WS_MSM_CURSOR) \
  X(WS_MSM_ENTRIES) X(WS_MSM_BUCKETS) X(WS_MSM_SCAN) X(WS_MSM_OUT) X(WS_MSM_SLOTS) X(WS_MSM_WGHIST) X(WS_BATCHINV) X(WS_XYZZ_TMP)    \
  X(WS_MERKLE_NODES) X(WS_MISC_A) X(WS_MISC_B) X(WS_MISC_C) X(WS_MISC_D) X(WS_MISC_E) X(WS_MISC_F)
#define MZK_WS_CACHE_SLOTS(X) X(WS_FB_TABLE16) X(WS_FB_TABLE8) X(WS_NTT_PRE) X(WS_NTT_PRE_M128)
#define MZK_WS_ENUM(name) name,
#define MZK_WS_NAME(name) #name,
enum WsSlot { MZK_WS_SLOTS(MZK_WS_ENUM) WS_COUNT };
enum WsCacheSlot { MZK_WS_CACHE_SLOTS(MZK_WS_ENUM) WS_CACHE_COUNT };
inline const char* ws_slot_name(WsSlot slot) {
  static const char* const names[WS_COUNT] = {MZK_WS_SLOTS(MZK_WS_NAME)};
  return names[slot];
}
#undef MZK_WS_ENUM
#undef MZK_WS_NAME
static_assert(WS_COUNT <= 32, "WsFrame keeps one bit per slot");

// epoch: the outermost API call that last asked for the slot; holder: the frame that has it (null = free; never set on a cache slot)
struct WsBuf { void* p = nullptr; size_t cap = 0; uint64_t epoch = 0; const char* holder = nullptr; };
// The blocks that WsBlock hands out: what is parked waits for the next request of its size, what is lent is inside a live WsBlock.
struct WsPool {
  struct Block { void* p; size_t cap; };
  std::vector<Block> parked;
  size_t parked_bytes = 0, lent_bytes = 0;
};
// One per context, owned by it.  gen bumps whenever a cache slot has been freed (the cached device tables die with it).
struct WsTable { WsBuf slot[WS_COUNT]; WsBuf cache[WS_CACHE_COUNT]; uint64_t gen = 1; WsPool pool; };

// ---- what the embedding program supplies ----------------------------------------------------------------------------------
// The four device hooks.  ws_hook_alloc: MZK_OK; MZK_E_NOMEM (no message yet) when the device has no room; any other code with its
// message set.  `what` names the request in messages.  ws_hook_sync waits for the device, ws_hook_wait for one stream.
int ws_hook_alloc(void** out, size_t bytes, const char* what);
int ws_hook_free(void* p);
int ws_hook_sync();
int ws_hook_wait(void* stream);
WsTable* ws_table_of(int ctx_index);
int ws_current_ctx();
void set_error(const char* fmt, ...);
// mzk_poly.hip: deletes the cached interpolation plans of the current context that the running call does not use, behind a wait for
// the device if there is one to delete (enqueued work of an earlier call may still read it).  Their blocks park in the pool.
void poly_drop_idle_plans();

inline uint64_t g_ws_epoch = 1;                // one per outermost API call: which slots the running call has asked for
inline uint64_t g_ws_gen_counter = 1;
inline size_t g_ws_budget = 0;                 // mzk_set_workspace_budget: bytes of workspace a context may keep (0 = no limit)
inline size_t g_ws_pool_cap = (size_t)2 << 30; // bytes a context's pool may keep parked: a block released beyond that is freed
inline WsTable& ws_table() { return *ws_table_of(ws_current_ctx()); }
inline uint64_t ws_generation() { return ws_table().gen; }
inline void ws_new_generation(WsTable& t) { t.gen = ++g_ws_gen_counter; }

// Workspace memory gives itself back.  A slot remembers the outermost call that last asked for it; when an allocation would exceed
// the caller's budget (mzk_set_workspace_budget) or the device refuses it, every slot that the RUNNING call has not asked for and
// that no frame holds is freed and the allocation tried again; what is still refused is MZK_E_NOMEM.
inline size_t ws_bytes_held() {
  const WsTable& w = ws_table();
  size_t t = w.pool.parked_bytes + w.pool.lent_bytes;      // lent: the running call's temporaries and the cached interpolation plans
  for (const auto& b : w.slot) t += b.cap;
  for (const auto& b : w.cache) t += b.cap;
  return t;
}
inline bool ws_idle(const WsBuf& b) { return b.p && b.epoch != g_ws_epoch && !b.holder; }
// Frees the idle slots of the current context (all of them between calls) and the blocks parked in its pool, those of the idle
// interpolation plans included; waits for the device first (earlier *_dev calls may still be reading them).  A lent block stays.
// Returns the bytes given back.
inline size_t ws_trim_idle() {
  WsTable& w = ws_table();
  poly_drop_idle_plans();
  size_t idle = w.pool.parked_bytes;
  for (const auto& b : w.slot) if (ws_idle(b)) idle += b.cap;
  for (const auto& b : w.cache) if (ws_idle(b)) idle += b.cap;
  if (!idle) return 0;
  (void)ws_hook_sync();
  for (const auto& b : w.pool.parked) (void)ws_hook_free(b.p);
  w.pool.parked.clear();
  w.pool.parked_bytes = 0;
  const auto drop = [](WsBuf& b) { (void)ws_hook_free(b.p); b.p = nullptr; b.cap = 0; };
  for (auto& b : w.slot) if (ws_idle(b)) drop(b);
  // device tables cached inside slots are gone with THEIR slots only: a trim in the middle of a call that uses them leaves the caches
  // valid (a budgeted loop that alternates call kinds rebuilt them on every call otherwise)
  bool cache_slot_freed = false;
  for (auto& b : w.cache) if (ws_idle(b)) { drop(b); cache_slot_freed = true; }
  if (cache_slot_freed) ws_new_generation(w);
  return idle;
}
// Allocation that tries again after ws_trim_idle() when the device is out of memory; MZK_E_NOMEM if it still is.
inline int dev_alloc(void** out, size_t bytes, const char* what) {
  *out = nullptr;
  int rc = ws_hook_alloc(out, bytes, what);
  if (rc == MZK_E_NOMEM && ws_trim_idle()) rc = ws_hook_alloc(out, bytes, what);
  if (rc == MZK_OK) return MZK_OK;
  *out = nullptr;
  if (rc == MZK_E_NOMEM) set_error("%s: the device has no %zu bytes left (idle workspace already released)", what, bytes);
  return rc;
}
// Grow-only: a request within the slot's capacity is the same pointer again, so steady-state calls never allocate; a larger one waits
// for the device, frees and allocates anew (4096 bytes at least).
inline int ws_take(WsBuf& b, size_t bytes, void** out) {
  b.epoch = g_ws_epoch;
  if (bytes > b.cap) {
    if (b.p) {
      int rc = ws_hook_sync();
      if (rc == MZK_OK) rc = ws_hook_free(b.p);
      if (rc != MZK_OK) return rc;
      b.p = nullptr; b.cap = 0;
    }
    const size_t cap = bytes < 4096 ? 4096 : bytes;
    if (g_ws_budget && ws_bytes_held() + cap > g_ws_budget) (void)ws_trim_idle();
    const int rc = dev_alloc(&b.p, cap, "workspace");
    if (rc != MZK_OK) return rc;
    b.cap = cap;
  }
  *out = b.p;
  return MZK_OK;
}
inline int ws_cache_get(WsCacheSlot slot, size_t bytes, void** out) { return ws_take(ws_table().cache[slot], bytes, out); }
// Shutdown, with no frame and no WsBlock alive: everything of the current context goes.
inline void ws_release_all() {
  WsTable& w = ws_table();
  ws_new_generation(w);
  for (const auto& b : w.pool.parked) (void)ws_hook_free(b.p);
  w.pool.parked.clear();
  w.pool.parked_bytes = 0;
  const auto drop = [](WsBuf& b) { if (b.p) (void)ws_hook_free(b.p); b = WsBuf(); };
  for (auto& b : w.slot) drop(b);
  for (auto& b : w.cache) drop(b);
}

// The leases of one function.  A frame may take slots on several contexts (the *_multi loops): holders live in the context's own
// table, so the same slot on two contexts does not collide.  One bit per (context, slot): no heap, and no count to overflow.
class WsFrame {
 public:
  explicit WsFrame(const char* who) : who_(who) {}
  ~WsFrame() {
    for (int c = 0; c < MZK_MAX_CTX; c++) {
      if (!taken_[c]) continue;
      WsTable* w = ws_table_of(c);
      for (int k = 0; k < WS_COUNT; k++) if (taken_[c] >> k & 1) w->slot[k].holder = nullptr;
    }
  }
  WsFrame(const WsFrame&) = delete;
  WsFrame& operator=(const WsFrame&) = delete;
  int get(WsSlot slot, size_t bytes, void** out) {
    const int c = ws_current_ctx();
    WsBuf& b = ws_table_of(c)->slot[slot];
    if (b.holder) {
      set_error("workspace: %s asked for by %s while %s holds it", ws_slot_name(slot), who_, b.holder);
      return MZK_E_ARG;
    }
    const int rc = ws_take(b, bytes, out);
    if (rc != MZK_OK) return rc;
    b.holder = who_;
    taken_[c] |= 1u << slot;
    return MZK_OK;
  }

 private:
  const char* who_;
  uint32_t taken_[MZK_MAX_CTX] = {};
};

// A temporary of the polynomial routines.  A call makes a dozen whose sizes repeat from call to call; allocating and freeing cost more
// than the kernels of a small tree (and freeing synchronises the device), so a released block waits in the pool of the context it was
// taken on -- whichever is current when it is released -- and is handed out again (everything runs on the context's own stream, so
// reuse is stream-ordered).  Sizes are N * element size, powers of two anyway: the classes are the powers of two from 4096 up.
class WsBlock {
 public:
  void* p = nullptr;
  size_t cap = 0;
  WsBlock() = default;
  WsBlock(WsBlock&& o) noexcept : p(o.p), cap(o.cap), ctx_(o.ctx_) { o.p = nullptr; o.cap = 0; }
  WsBlock& operator=(WsBlock&& o) noexcept {
    if (this != &o) { release(); p = o.p; cap = o.cap; ctx_ = o.ctx_; o.p = nullptr; o.cap = 0; }
    return *this;
  }
  ~WsBlock() { release(); }
  // the most recently parked block of the request's class, else dev_alloc (which gives the idle workspace back before it reports
  // MZK_E_NOMEM, as mzk.h promises)
  int alloc(size_t bytes) {
    release();
    size_t want = 4096;
    while (want < bytes) want <<= 1;
    ctx_ = ws_current_ctx();
    WsPool& pool = ws_table_of(ctx_)->pool;
    for (size_t i = pool.parked.size(); i-- > 0;) {
      if (pool.parked[i].cap != want) continue;
      p = pool.parked[i].p;
      pool.parked_bytes -= want;
      pool.parked.erase(pool.parked.begin() + (long)i);
      break;
    }
    if (!p) {
      const int rc = dev_alloc(&p, want, "polynomial scratch");
      if (rc != MZK_OK) return rc;
    }
    cap = want;
    pool.lent_bytes += want;
    return MZK_OK;
  }
  void release() {
    if (!p) return;
    WsPool& pool = ws_table_of(ctx_)->pool;
    pool.lent_bytes -= cap;
    if (pool.parked_bytes + cap > g_ws_pool_cap) (void)ws_hook_free(p);
    else { pool.parked.push_back({p, cap}); pool.parked_bytes += cap; }
    p = nullptr; cap = 0;
  }
  uint32_t* w() const { return (uint32_t*)p; }

 private:
  int ctx_ = 0;
};

// One device allocation of exactly the bytes asked for, freed with its owner: the tables of a cached plan, the buffers of a handle.
// Not workspace: mzk_workspace_bytes does not count it and no trim takes it.
class DevMem {
 public:
  DevMem() = default;
  DevMem(DevMem&& o) noexcept : p_(o.p_) { o.p_ = nullptr; }
  DevMem& operator=(DevMem&& o) noexcept {
    if (this != &o) { reset(); p_ = o.p_; o.p_ = nullptr; }
    return *this;
  }
  ~DevMem() { reset(); }
  int alloc(size_t bytes, const char* what) { reset(); return dev_alloc(&p_, bytes, what); }
  void reset() { if (p_) (void)ws_hook_free(p_); p_ = nullptr; }
  void* get() const { return p_; }
  template <class T> T* as() const { return (T*)p_; }
  explicit operator bool() const { return p_ != nullptr; }

 private:
  void* p_ = nullptr;
};

// The caches of device tables (transform plans, offset tables, interpolation plans) keep entries with a `stamp`, set from this one
// counter on every use, and evict through this one routine: with `cap` entries or more, the one used longest ago goes, behind a wait
// for `stream`, whose enqueued work may still read its tables.  If the wait fails nothing is removed.
inline uint64_t g_lru_stamp = 0;
inline uint64_t lru_stamp() { return ++g_lru_stamp; }
template <class T> int lru_evict(std::vector<std::unique_ptr<T>>& entries, size_t cap, void* stream) {
  if (entries.empty() || entries.size() < cap) return MZK_OK;
  size_t victim = 0;
  for (size_t i = 1; i < entries.size(); i++) if (entries[i]->stamp < entries[victim]->stamp) victim = i;
  const int rc = ws_hook_wait(stream);
  if (rc != MZK_OK) return rc;
  entries.erase(entries.begin() + (long)victim);
  return MZK_OK;
}

}  // namespace mzk
