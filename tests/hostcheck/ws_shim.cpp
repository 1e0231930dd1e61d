// The workspace's bookkeeping (myzkp_amd/csrc/mzk_ws.h: leases, refusal, growth, trim, budget, cache generation) run on the host for
// tests/test_hostcheck_ws.py.  Stand-alone: the three device hooks are malloc, free and a counter, two contexts' tables live here.
// Prints one "ok <letter> ..." line per rule (a .. h as the test lists them) and "ok all"; the first rule that does not hold prints
// "FAIL <file>:<line> <condition>" and exits 1.  Built with -fsanitize=address,undefined: a block freed under a live lease, or one
// left behind at exit, is the sanitizer's finding.
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <set>
#include "../../myzkp_amd/csrc/mzk_ws.h"

using namespace mzk;

static WsTable g_tab[2];
static int g_cur = 0;
static char g_msg[512];
static std::set<void*> g_live;
static size_t g_allocs = 0, g_frees = 0, g_syncs = 0;
static int g_refuse = 0;                // this many allocations from now on are refused
static size_t g_pool_held = 0;          // what the polynomial pool reports

namespace mzk {
int ws_hook_alloc(void** out, size_t bytes, const char*) {
  if (g_refuse > 0) { g_refuse--; *out = nullptr; return MZK_E_NOMEM; }
  *out = malloc(bytes);
  g_live.insert(*out);
  g_allocs++;
  return MZK_OK;
}
int ws_hook_free(void* p) {
  if (!g_live.erase(p)) { printf("FAIL free of a block that is not live\n"); exit(1); }
  free(p);
  g_frees++;
  return MZK_OK;
}
int ws_hook_sync() { g_syncs++; return MZK_OK; }
WsTable* ws_table_of(int ctx_index) { return &g_tab[ctx_index]; }
int ws_current_ctx() { return g_cur; }
void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_msg, sizeof g_msg, fmt, ap);
  va_end(ap);
}
size_t poly_bytes_held() { return g_pool_held; }
size_t poly_trim_idle() { return 0; }
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
  new_call();
  g_ws_budget = 120000;
  g_pool_held = 10000;                                             // the polynomial pool counts
  {
    WsFrame ws("budgeted");
    CHECK(ws.get(WS_MISC_C, 20000, &p) == MZK_OK);
    CHECK(ws_bytes_held() == 110000);                              // an earlier call's 80000 + the pool + 20000 ...
    CHECK(ws.get(WS_MISC_D, 20000, &q) == MZK_OK);                // ... now past the budget: the idle 80000 go
    CHECK(ws_bytes_held() == 50000 && ws_bytes_held() <= g_ws_budget);
    CHECK(live(p) && live(q) && g_live.size() == 2);
    CHECK(ws.get(WS_MISC_E, 80000, &r) == MZK_OK);                // nothing idle is left: the budget trims what it can, it does not refuse
    CHECK(ws_bytes_held() == 130000 && live(p) && live(q));
  }
  g_ws_budget = 0;
  g_pool_held = 0;
  printf("ok d\n");

  // ---- e: freeing a cache slot ends the caches (the generation moves); cache slots take no lease
  {
    new_call();
    CHECK(ws_cache_get(WS_FB_TABLE8, 7000, &p) == MZK_OK && ws_cache_get(WS_FB_TABLE8, 7000, &q) == MZK_OK && p == q);
    CHECK(holders() == 0 && g_tab[0].cache[WS_FB_TABLE8].cap == 7000);
    const uint64_t gen0 = ws_generation();
    CHECK(ws_trim_idle() == 120000 && ws_generation() == gen0 && live(p));     // this call asked for the table: only call d's scratch goes
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

  // ---- h: shutdown gives everything back (the leak check at exit is the sanitizer's)
  for (g_cur = 0; g_cur < 2; g_cur++) {
    const uint64_t gen0 = ws_generation();
    ws_release_all();
    CHECK(ws_generation() != gen0 && ws_bytes_held() == 0);
  }
  CHECK(g_live.empty() && g_allocs == g_frees);
  printf("ok h\nok all\n");
  return 0;
}
