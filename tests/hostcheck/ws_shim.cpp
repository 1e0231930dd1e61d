// The workspace's bookkeeping (myzkp_amd/csrc/mzk_ws.h: leases, refusal, growth, trim, budget, cache generation, the pool of WsBlock,
// DevMem and lru_evict) run on the host for tests/test_hostcheck_ws.py.  Stand-alone: the four device hooks are malloc, free and two
// counters, two contexts' tables live here, and the cached interpolation plans are a vector of blocks.
// Prints one "ok <letter> ..." line per rule (a .. o as the test lists them) and "ok all"; the first rule that does not hold prints
// "FAIL <file>:<line> <condition>" and exits 1.  Built with -fsanitize=address,undefined: a block freed under a live lease, or one
// left behind at exit, is the sanitizer's finding.
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <map>
#include <memory>
#include <vector>
#include "../../myzkp_amd/csrc/mzk_ws.h"

using namespace mzk;

static WsTable g_tab[2];
static int g_cur = 0;
static char g_msg[512];
static std::map<void*, size_t> g_live;  // block -> bytes
static size_t g_allocs = 0, g_frees = 0, g_freed_bytes = 0, g_syncs = 0, g_waits = 0;
static int g_refuse = 0;                // this many allocations from now on are refused
static bool g_wait_fails = false;
static std::vector<WsBlock> g_idle_plans;        // stands for the cached interpolation plans that the running call does not use

namespace mzk {
int ws_hook_alloc(void** out, size_t bytes, const char*) {
  if (g_refuse > 0) { g_refuse--; *out = nullptr; return MZK_E_NOMEM; }
  *out = malloc(bytes);
  g_live[*out] = bytes;
  g_allocs++;
  return MZK_OK;
}
int ws_hook_free(void* p) {
  if (!g_live.count(p)) { printf("FAIL free of a block that is not live\n"); exit(1); }
  g_freed_bytes += g_live[p];
  g_live.erase(p);
  free(p);
  g_frees++;
  return MZK_OK;
}
int ws_hook_sync() { g_syncs++; return MZK_OK; }
int ws_hook_wait(void*) { g_waits++; return g_wait_fails ? MZK_E_HIP : MZK_OK; }
void poly_drop_idle_plans() { g_idle_plans.clear(); }
WsTable* ws_table_of(int ctx_index) { return &g_tab[ctx_index]; }
int ws_current_ctx() { return g_cur; }
void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_msg, sizeof g_msg, fmt, ap);
  va_end(ap);
}
}  // namespace mzk

#define CHECK(c) do { if (!(c)) { printf("FAIL %s:%d %s   [%s]\n", __FILE__, __LINE__, #c, g_msg); exit(1); } } while (0)

static bool live(void* p) { return g_live.count(p) != 0; }
static int holders() {
  int h = 0;
  for (auto& t : g_tab) for (auto& b : t.slot) h += b.holder != nullptr;
  for (auto& t : g_tab) for (auto& b : t.cache) h += b.holder != nullptr;
  return h;
}
static void new_call() { g_ws_epoch++; }          // what the entry guard of an outermost API call does
static bool parked(int c, void* p) {
  for (const auto& b : g_tab[c].pool.parked) if (b.p == p) return true;
  return false;
}
struct Entry { uint64_t stamp; DevMem mem; };     // what a plan cache keeps

static int inner_asks(WsSlot slot, size_t bytes, void** out) {
  WsFrame ws("inner");
  return ws.get(slot, bytes, out);
}
static int fails_after_taking(void** out) {
  WsFrame ws("early_return");
  int rc = ws.get(WS_MISC_C, 100, out);
  if (rc != MZK_OK) return rc;
  void* q;
  rc = ws.get(WS_MISC_C, 100, &q);          // refused: the early return
  if (rc != MZK_OK) return rc;
  return MZK_OK;
}

int main() {
  void *p = nullptr, *q = nullptr, *r = nullptr;
  // ---- a: a held slot is refused, to the frame that holds it and to a nested one; nothing is freed, grown or waited for
  {
    WsFrame ws("outer");
    CHECK(ws.get(WS_NTT_IO_A, 1000, &p) == MZK_OK && p && live(p));
    CHECK(g_tab[0].slot[WS_NTT_IO_A].cap == 4096);                 // the 4096-byte minimum
    CHECK(g_tab[0].slot[WS_NTT_IO_A].epoch == g_ws_epoch);
    memset(p, 1, 1000);
    const size_t a0 = g_allocs, f0 = g_frees, s0 = g_syncs;
    q = (void*)16;
    CHECK(ws.get(WS_NTT_IO_A, 1 << 20, &q) == MZK_E_ARG);          // the same frame, more bytes
    CHECK(!strcmp(g_msg, "workspace: WS_NTT_IO_A asked for by outer while outer holds it"));
    CHECK(q == (void*)16);
    CHECK(inner_asks(WS_NTT_IO_A, 1 << 20, &q) == MZK_E_ARG);      // a nested frame
    CHECK(!strcmp(g_msg, "workspace: WS_NTT_IO_A asked for by inner while outer holds it"));
    CHECK(inner_asks(WS_NTT_IO_A, 8, &q) == MZK_E_ARG);            // ... also for fewer bytes
    CHECK(g_allocs == a0 && g_frees == f0 && g_syncs == s0 && live(p) && g_tab[0].slot[WS_NTT_IO_A].p == p && g_tab[0].slot[WS_NTT_IO_A].cap == 4096);
    memset(p, 2, 1000);                                            // still the caller's block
    // ---- b: once the inner frame has ended the slot can be taken again
    CHECK(inner_asks(WS_NTT_IO_B, 5000, &q) == MZK_OK && live(q));
    CHECK(holders() == 1);
    CHECK(inner_asks(WS_NTT_IO_B, 5000, &r) == MZK_OK && r == q);  // not larger: the same pointer, no traffic
    CHECK(inner_asks(WS_NTT_IO_B, 100, &r) == MZK_OK && r == q);
    CHECK(g_allocs == a0 + 1 && g_frees == f0 && g_syncs == s0);
    CHECK(inner_asks(WS_NTT_IO_B, 5001, &r) == MZK_OK && live(r) && !live(q));      // larger: one wait, one free, a new block
    CHECK(g_allocs == a0 + 2 && g_frees == f0 + 1 && g_syncs == s0 + 1);
    CHECK(g_tab[0].slot[WS_NTT_IO_B].cap == 5001);
    printf("ok a\nok b\n");
  }
  CHECK(holders() == 0);

  // ---- g: a frame that took nothing, and one destroyed after an early error return, leave no holder behind
  { WsFrame nothing("nothing"); }
  CHECK(holders() == 0);
  CHECK(fails_after_taking(&q) == MZK_E_ARG && holders() == 0);
  CHECK(!strcmp(g_msg, "workspace: WS_MISC_C asked for by early_return while early_return holds it"));
  CHECK(inner_asks(WS_MISC_C, 100, &r) == MZK_OK && r == q);
  printf("ok g\n");

  // ---- c: a refused allocation trims the slots of EARLIER calls that nobody holds, and only those; then it is tried again
  void *held_p, *cur_p, *idle_a = p, *idle_c = q;               // WS_NTT_IO_A, WS_MISC_C (and WS_NTT_IO_B) were last asked for by call 1
  {
    WsFrame held("held_across_calls");                           // (no library frame outlives its call; the rule must not depend on that)
    CHECK(held.get(WS_MISC_D, 3000, &held_p) == MZK_OK);
    new_call();
    WsFrame ws("call2");
    CHECK(ws.get(WS_MISC_E, 3000, &cur_p) == MZK_OK);
    { void* t; CHECK(inner_asks(WS_MISC_F, 3000, &t) == MZK_OK); }      // this call's, free again: the epoch protects it, not a holder
    void* cur_f = g_tab[0].slot[WS_MISC_F].p;
    const uint64_t gen0 = ws_generation();
    const size_t f0 = g_frees, s0 = g_syncs;
    g_refuse = 1;
    CHECK(ws.get(WS_MSM_OUT, 9000, &r) == MZK_OK && live(r));    // refused once, trimmed, then granted
    CHECK(g_refuse == 0);
    CHECK(!live(idle_a) && !live(idle_c) && !g_tab[0].slot[WS_NTT_IO_A].p && !g_tab[0].slot[WS_NTT_IO_B].p && !g_tab[0].slot[WS_MISC_C].p);
    CHECK(g_tab[0].slot[WS_NTT_IO_A].cap == 0);
    CHECK(g_frees == f0 + 3 && g_syncs == s0 + 1);               // one wait in front of the trim's frees
    CHECK(live(held_p) && g_tab[0].slot[WS_MISC_D].p == held_p);   // held, from an earlier call: stays
    CHECK(live(cur_p) && live(cur_f));                             // this call's: stay
    memset(held_p, 3, 3000); memset(cur_p, 3, 3000);
    CHECK(ws_generation() == gen0);                                // e: scratch slots alone do not end the caches
    // refused again after the trim: MZK_E_NOMEM, and the slot stays free
    new_call();
    g_refuse = 2;
    CHECK(inner_asks(WS_MSM_SCAN, 100, &q) == MZK_E_NOMEM && g_refuse == 0);
    CHECK(strstr(g_msg, "workspace: the device has no 4096 bytes left") == g_msg);
    CHECK(!g_tab[0].slot[WS_MSM_SCAN].p && !g_tab[0].slot[WS_MSM_SCAN].holder && holders() == 3);
    CHECK(live(held_p) && live(cur_p) && live(r));                 // held by `held` and `ws`: no trim touches them
    CHECK(!live(cur_f));                                           // (WS_MISC_F belonged to the call before this one by now)
    // nothing idle: no second attempt at all
    g_refuse = 1;
    CHECK(inner_asks(WS_MSM_SCAN, 100, &q) == MZK_E_NOMEM && g_refuse == 0);
    CHECK(inner_asks(WS_MSM_SCAN, 100, &q) == MZK_OK);
    printf("ok c\n");
  }
  CHECK(holders() == 0);

  // ---- d: the budget.  Idle slots go when a new one would exceed it; what is held stays at or below it when they suffice
  new_call();
  (void)ws_trim_idle();
  CHECK(ws_bytes_held() == 0 && g_live.empty());
  CHECK(inner_asks(WS_MISC_A, 40000, &p) == MZK_OK && inner_asks(WS_MISC_B, 40000, &p) == MZK_OK);
  { WsBlock b; CHECK(b.alloc(5000) == MZK_OK); }                    // the pool counts: 8192 bytes parked ...
  new_call();
  g_ws_budget = 120000;
  {
    WsBlock lent;
    CHECK(lent.alloc(100) == MZK_OK);                              // ... and 4096 lent to the running call
    WsFrame ws("budgeted");
    CHECK(ws.get(WS_MISC_C, 20000, &p) == MZK_OK);
    CHECK(ws_bytes_held() == 112288);                              // an earlier call's 80000 + the pool's 12288 + 20000 ...
    CHECK(ws.get(WS_MISC_D, 20000, &q) == MZK_OK);                // ... now past the budget: the idle 80000 and the parked 8192 go
    CHECK(ws_bytes_held() == 44096 && ws_bytes_held() <= g_ws_budget);
    CHECK(live(p) && live(q) && live(lent.p) && g_live.size() == 3);
    CHECK(ws.get(WS_MISC_E, 80000, &r) == MZK_OK);                // nothing idle is left: the budget trims what it can, it does not refuse
    CHECK(ws_bytes_held() == 124096 && live(p) && live(q) && live(lent.p));
  }
  g_ws_budget = 0;
  printf("ok d\n");

  // ---- e: freeing a cache slot ends the caches (the generation moves); cache slots take no lease
  {
    new_call();
    CHECK(ws_cache_get(WS_FB_TABLE8, 7000, &p) == MZK_OK && ws_cache_get(WS_FB_TABLE8, 7000, &q) == MZK_OK && p == q);
    CHECK(holders() == 0 && g_tab[0].cache[WS_FB_TABLE8].cap == 7000);
    const uint64_t gen0 = ws_generation();
    CHECK(ws_trim_idle() == 120000 + 4096 && ws_generation() == gen0 && live(p));     // this call asked for the table: only call d's scratch and its parked block go
    CHECK(inner_asks(WS_MISC_A, 100, &r) == MZK_OK);
    new_call();
    CHECK(ws_cache_get(WS_NTT_PRE, 100, &r) == MZK_OK);
    CHECK(ws_trim_idle() == 7000 + 4096 && !live(p) && live(r));
    CHECK(ws_generation() != gen0);
    const uint64_t gen1 = ws_generation();
    CHECK(ws_trim_idle() == 0 && ws_generation() == gen1);
    printf("ok e\n");
  }

  // ---- f: the same slot on two contexts does not collide, in one frame
  {
    new_call();
    WsFrame ws("both_contexts");
    g_cur = 0;
    CHECK(ws.get(WS_MISC_D, 100, &p) == MZK_OK);
    g_cur = 1;
    CHECK(ws.get(WS_MISC_D, 100, &q) == MZK_OK && q != p && live(p) && live(q));
    CHECK(ws.get(WS_MISC_D, 100, &r) == MZK_E_ARG);
    g_cur = 0;
    CHECK(ws.get(WS_MISC_D, 100, &r) == MZK_E_ARG);
    CHECK(holders() == 2 && g_tab[1].slot[WS_MISC_D].holder && g_tab[0].slot[WS_MISC_D].holder);
    g_cur = 1;                                                     // the frame ends with another context current than it began with
  }
  CHECK(holders() == 0);
  g_cur = 0;
  printf("ok f\n");

  // every scratch slot has its name in the table
  for (int k = 0; k < WS_COUNT; k++) CHECK(!strncmp(ws_slot_name((WsSlot)k), "WS_", 3));
  CHECK(!strcmp(ws_slot_name(WS_NTT_TMP), "WS_NTT_TMP") && !strcmp(ws_slot_name(WS_MISC_F), "WS_MISC_F"));

  // ---- i: the pool's size classes.  A request is rounded up to a power of two, 4096 at least; a released block waits for the next
  // request of its class, the one parked last first, and costs no hook call; another class allocates
  new_call();
  g_cur = 1;
  (void)ws_trim_idle();
  g_cur = 0;
  (void)ws_trim_idle();
  CHECK(ws_bytes_held() == 0 && g_live.empty());
  {
    WsPool& pool = g_tab[0].pool;
    const size_t a0 = g_allocs, f0 = g_frees;
    void *first, *second;
    {
      WsBlock a, tiny, b;
      CHECK(a.alloc(5000) == MZK_OK && a.cap == 8192 && live(a.p) && g_live[a.p] == 8192);
      CHECK(tiny.alloc(1) == MZK_OK && tiny.cap == 4096);
      CHECK(b.alloc(8192) == MZK_OK && b.cap == 8192 && b.p != a.p);          // a power of two is its own class
      CHECK(g_allocs == a0 + 3 && pool.lent_bytes == 20480 && pool.parked_bytes == 0);
      memset(a.p, 4, 8192);
      first = a.p; second = b.p;
    }                                                                          // parked in the order b, tiny, a
    CHECK(g_frees == f0 && pool.parked.size() == 3 && pool.parked_bytes == 20480 && pool.lent_bytes == 0);
    WsBlock x, y, z;
    CHECK(x.alloc(8000) == MZK_OK && x.p == first && x.cap == 8192);
    CHECK(y.alloc(4097) == MZK_OK && y.p == second);
    CHECK(g_allocs == a0 + 3 && g_frees == f0 && pool.parked_bytes == 4096 && pool.lent_bytes == 16384);
    CHECK(z.alloc(8193) == MZK_OK && z.cap == 16384 && g_allocs == a0 + 4);     // no parked block of that class
    WsBlock moved(std::move(x));                                               // one owner at a time
    CHECK(!x.p && moved.p == first && pool.lent_bytes == 32768);
    y = std::move(moved);                                                      // y's own block goes back first
    CHECK(y.p == first && !moved.p && parked(0, second) && pool.lent_bytes == 24576 && pool.parked_bytes == 12288);
    CHECK(y.alloc(100) == MZK_OK && y.cap == 4096 && parked(0, first));        // so does the block of one that allocates again
    CHECK(g_allocs == a0 + 4 && g_frees == f0);
  }
  printf("ok i\n");

  // ---- j: the pool keeps no more than its cap: a release that would pass it frees the block
  {
    WsPool& pool = g_tab[0].pool;
    CHECK(pool.lent_bytes == 0 && pool.parked_bytes == 36864);
    const size_t cap0 = g_ws_pool_cap, f0 = g_frees;
    CHECK(cap0 == (size_t)2 << 30);
    WsBlock a, b;
    CHECK(a.alloc(3000) == MZK_OK && b.alloc(20000) == MZK_OK);                // a parked 4096, a new 32768
    g_ws_pool_cap = 36864;
    void* bp = b.p;
    a.release();                                                               // 32768 + 4096: exactly the cap, parked
    CHECK(g_frees == f0 && pool.parked_bytes == 36864);
    b.release();
    CHECK(g_frees == f0 + 1 && !live(bp) && !b.p && pool.parked_bytes == 36864 && pool.lent_bytes == 0);
    g_ws_pool_cap = cap0;
  }
  printf("ok j\n");

  // ---- k: a refused allocation gives the parked blocks and the idle slots back and is tried again; refused twice, it is MZK_E_NOMEM
  {
    WsPool& pool = g_tab[0].pool;
    CHECK(inner_asks(WS_MISC_A, 6000, &p) == MZK_OK);
    new_call();
    const size_t f0 = g_frees, nparked = pool.parked.size();
    WsBlock held, big;
    CHECK(held.alloc(4096) == MZK_OK && g_frees == f0);
    g_refuse = 1;
    CHECK(big.alloc(100000) == MZK_OK && big.cap == 131072 && g_refuse == 0);
    CHECK(g_frees == f0 + nparked - 1 + 1 && pool.parked.empty() && pool.parked_bytes == 0 && !live(p) && live(held.p));
    CHECK(pool.lent_bytes == 4096 + 131072);
    big.release();
    CHECK(inner_asks(WS_MISC_A, 6000, &p) == MZK_OK);
    new_call();
    g_refuse = 2;
    WsBlock none;
    CHECK(none.alloc(300000) == MZK_E_NOMEM && g_refuse == 0 && !none.p && !none.cap);
    CHECK(!strcmp(g_msg, "polynomial scratch: the device has no 524288 bytes left (idle workspace already released)"));
    CHECK(pool.parked.empty() && !live(p) && live(held.p) && pool.lent_bytes == 4096);
  }
  printf("ok k\n");

  // ---- l: what is held counts parked and lent bytes; a trim drops the idle plans, frees what is parked, says exactly what it freed
  // and leaves a lent block alone
  new_call();
  (void)ws_trim_idle();
  CHECK(ws_bytes_held() == 0 && g_live.empty());
  {
    WsPool& pool = g_tab[0].pool;
    WsBlock lent;
    CHECK(lent.alloc(10000) == MZK_OK);
    { WsBlock t; CHECK(t.alloc(4096) == MZK_OK); }
    g_idle_plans.resize(2);
    CHECK(g_idle_plans[0].alloc(30000) == MZK_OK && g_idle_plans[1].alloc(100) == MZK_OK);      // the second is the parked 4096
    CHECK(inner_asks(WS_MISC_B, 5000, &p) == MZK_OK);
    { WsBlock t; CHECK(t.alloc(70000) == MZK_OK); }
    CHECK(pool.lent_bytes == 16384 + 32768 + 4096 && pool.parked_bytes == 131072);
    CHECK(ws_bytes_held() == 5000 + 16384 + 32768 + 4096 + 131072);
    new_call();
    const size_t freed0 = g_freed_bytes, s0 = g_syncs;
    const size_t gave = ws_trim_idle();
    CHECK(gave == 5000 + 32768 + 4096 + 131072 && g_freed_bytes - freed0 == gave && g_syncs == s0 + 1);
    CHECK(g_idle_plans.empty() && pool.parked.empty() && live(lent.p) && g_live.size() == 1);
    CHECK(ws_bytes_held() == 16384 && pool.lent_bytes == 16384);
    memset(lent.p, 5, 10000);
    CHECK(ws_trim_idle() == 0 && g_syncs == s0 + 1);                           // nothing idle: no wait either
  }
  printf("ok l\n");

  // ---- m: a block goes back to the context it was taken on, whichever is current when it is released
  {
    void* bp;
    {
      WsBlock b;
      g_cur = 0;
      CHECK(b.alloc(9000) == MZK_OK && g_tab[0].pool.lent_bytes == 16384 && g_tab[1].pool.lent_bytes == 0);
      bp = b.p;
      g_cur = 1;
    }
    CHECK(parked(0, bp) && g_tab[0].pool.lent_bytes == 0 && g_tab[1].pool.parked.empty() && g_tab[1].pool.parked_bytes == 0);
    WsBlock other;
    CHECK(other.alloc(9000) == MZK_OK && other.p != bp && parked(0, bp));      // context 1 has a pool of its own
    g_cur = 0;
    CHECK(ws_bytes_held() == 16384);                                           // parked here,
    g_cur = 1;
    CHECK(ws_bytes_held() == 16384);                                           // lent there
  }
  g_cur = 0;
  printf("ok m\n");

  // ---- n: lru_evict.  Below the cap nothing goes and nothing is waited for; at the cap the entry with the oldest stamp goes, behind
  // one wait, and its memory is freed exactly once; a wait that fails removes nothing
  {
    std::vector<std::unique_ptr<Entry>> cache;
    const auto add = [&]() {
      std::unique_ptr<Entry> e(new Entry{lru_stamp(), DevMem()});
      CHECK(e->mem.alloc(1000, "table") == MZK_OK && g_live[e->mem.get()] == 1000);
      cache.push_back(std::move(e));
      return cache.back()->mem.get();
    };
    const size_t f0 = g_frees, w0 = g_waits;
    void* t0 = add();
    void* t1 = add();
    CHECK(lru_evict(cache, 3, nullptr) == MZK_OK && cache.size() == 2 && g_frees == f0 && g_waits == w0);
    void* t2 = add();
    cache[0]->stamp = lru_stamp();                                             // used again: the second entry is the oldest now
    g_wait_fails = true;
    CHECK(lru_evict(cache, 3, nullptr) == MZK_E_HIP && cache.size() == 3 && g_frees == f0 && g_waits == w0 + 1);
    g_wait_fails = false;
    CHECK(lru_evict(cache, 3, nullptr) == MZK_OK && cache.size() == 2 && g_frees == f0 + 1 && g_waits == w0 + 2);
    CHECK(live(t0) && !live(t1) && live(t2) && cache[0]->mem.get() == t0 && cache[1]->mem.get() == t2);
    CHECK(lru_evict(cache, 3, nullptr) == MZK_OK && cache.size() == 2 && g_frees == f0 + 1 && g_waits == w0 + 2);
    DevMem taken(std::move(cache[1]->mem));                                    // one owner at a time here as well
    CHECK(taken.get() == t2 && !cache[1]->mem);
    cache.clear();
    CHECK(g_frees == f0 + 2 && !live(t0) && live(t2));
    g_refuse = 1;                                                              // DevMem allocates through dev_alloc: trim, then once more
    CHECK(taken.alloc(2000, "table") == MZK_OK && !live(t2) && g_live[taken.get()] == 2000 && g_refuse == 0);
    CHECK(g_tab[0].pool.parked.empty());
    g_refuse = 1;
    CHECK(taken.alloc(3000, "table") == MZK_E_NOMEM && !taken && !strncmp(g_msg, "table: the device has no 3000 bytes left", 40));
    CHECK(ws_bytes_held() == 0);                                               // what DevMem owns is no workspace
  }
  printf("ok n\n");

  // ---- h, o: shutdown gives everything back, on both contexts, the parked blocks too (the leak check at exit is the sanitizer's)
  for (g_cur = 0; g_cur < 2; g_cur++) {
    { WsBlock a, b; CHECK(a.alloc(5000) == MZK_OK && b.alloc(50000) == MZK_OK); }
    CHECK(inner_asks(WS_MISC_A, 100, &p) == MZK_OK && ws_cache_get(WS_FB_TABLE16, 100, &q) == MZK_OK);
  }
  CHECK(g_tab[0].pool.parked.size() == 2 && g_tab[1].pool.parked.size() == 3 && g_live.size() == 9);     // context 1 still had rule m's block
  for (g_cur = 0; g_cur < 2; g_cur++) {
    const uint64_t gen0 = ws_generation();
    ws_release_all();
    CHECK(ws_generation() != gen0 && ws_bytes_held() == 0 && g_tab[g_cur].pool.parked.empty());
  }
  CHECK(g_live.empty() && g_allocs == g_frees);
  printf("ok h\nok o\nok all\n");
  return 0;
}
