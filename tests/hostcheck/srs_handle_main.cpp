// The SRS handle (myzkp_amd/csrc/mzk_srs.h: srs_new over the layout ladder, the owner, the direct and wide table sets) run on the host
// for tests/test_hostcheck_srs_handle.py.  Stand-alone, as ws_shim.cpp is: the device hooks are malloc, free and counters, with a
// refusal counter, and the idle workspace is a list of cached plans of which every trim drops one -- so that each refused rung finds
// something to release and is tried a second time, as a device with other work on it would have it.
// Prints one "ok <letter>" line per rule and "ok all"; the first rule that does not hold prints "FAIL <file>:<line> <condition>" and
// exits 1.  Built plain and with -fsanitize=address,undefined: a table set freed twice, or left behind at exit, is the sanitizer's.
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <map>
#include <vector>
#include "../../myzkp_amd/csrc/mzk_srs.h"

using namespace mzk;

static WsTable g_tab[2];
static int g_cur = 0;
static char g_msg[512];
static std::map<void*, size_t> g_live;  // block -> bytes
static size_t g_live_bytes = 0, g_allocs = 0, g_refused = 0, g_syncs = 0;
static int g_refuse = 0;                // this many allocations from now on are refused
static std::vector<WsBlock> g_idle_plans;

namespace mzk {
int ws_hook_alloc(void** out, size_t bytes, const char*) {
  if (g_refuse > 0) { g_refuse--; g_refused++; *out = nullptr; return MZK_E_NOMEM; }
  *out = malloc(bytes);
  g_live[*out] = bytes;
  g_live_bytes += bytes;
  g_allocs++;
  return MZK_OK;
}
int ws_hook_free(void* p) {
  if (!g_live.count(p)) { printf("FAIL free of a block that is not live\n"); exit(1); }
  g_live_bytes -= g_live[p];
  g_live.erase(p);
  free(p);
  return MZK_OK;
}
int ws_hook_sync() { g_syncs++; return MZK_OK; }
int ws_hook_wait(void*) { return MZK_OK; }
void poly_drop_idle_plans() { if (!g_idle_plans.empty()) g_idle_plans.pop_back(); }      // its block parks in the pool, the trim frees it
WsTable* ws_table_of(int ctx_index) { return &g_tab[ctx_index]; }
int ws_current_ctx() { return g_cur; }
void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_msg, sizeof g_msg, fmt, ap);
  va_end(ap);
}
void clear_error() { g_msg[0] = 0; }
}  // namespace mzk

#define CHECK(c) do { if (!(c)) { printf("FAIL %s:%d %s   [%s]\n", __FILE__, __LINE__, #c, g_msg); exit(1); } } while (0)

// `plans` idle plans of 4096 bytes each, then srs_new with the next `refuse` allocations refused
static int make(size_t n, int with_tables, int refuse, size_t plans, SrsOwner* h) {
  g_idle_plans.resize(plans);
  for (auto& b : g_idle_plans) CHECK(b.alloc(4096) == MZK_OK);
  g_ws_epoch++;                          // a new outermost call: nothing of the workspace is this call's
  g_msg[0] = 0;
  g_refuse = refuse;
  g_refused = 0;
  const int rc = srs_new(n, with_tables, h);
  g_refuse = 0;
  g_idle_plans.clear();
  (void)ws_trim_idle();
  return rc;
}

int main() {
  const size_t n = ((size_t)1 << 15) + 5;
  // ---- a: srs_new lands on each rung in turn as 0, 2, 4, 6 allocations are refused: every rung is tried, the idle workspace is
  // released, the rung is tried again, and only then does the layout degrade
  const struct { int refuse; bool tables; int sets; size_t rows; } want[4] = {{0, true, 1, 16}, {2, true, 2, 8}, {4, true, 4, 4}, {6, false, 1, 2}};
  for (const auto& w : want) {
    SrsOwner h;
    const size_t s0 = g_syncs;
    CHECK(make(n, 1, w.refuse, 4, &h) == MZK_OK && h);
    CHECK(g_refused == (size_t)w.refuse && g_syncs == s0 + (size_t)w.refuse / 2 + 1);      // one trim per refused rung (and make's own)
    CHECK(h->n == n && h->ctx_index == 0 && h->has_tables == w.tables && h->sets == w.sets && h->own.bits == 16);
    CHECK(h->table_rows() == w.rows && h->own.bytes == w.rows * n * 64 && h->table_bytes() == h->own.bytes);
    CHECK(h->own.mem && g_live.size() == 1 && g_live[h->own.mem.get()] == h->own.bytes && g_live_bytes == h->own.bytes);
    CHECK(h->kind() == (w.tables ? (MSM_PTS_TABLES | (16 << 8) | (w.sets << 16)) : (int)MSM_PTS_MONT));
    const MsmPoints p = h->points(3);
    CHECK(p.d == h->own.mem.as<char>() + 192 && p.kind == h->kind() && p.stride == n);
    memset(h->own.mem.get(), 1, h->own.bytes);
    h.reset();
    CHECK(g_live.empty() && g_live_bytes == 0);
  }
  // with nothing idle a refused rung is not tried twice: two refusals pass two rungs
  {
    SrsOwner h;
    CHECK(make(n, 1, 2, 0, &h) == MZK_OK && h->sets == 4 && g_refused == 2);
    h.reset();
    CHECK(g_live_bytes == 0);
  }
  // a rung over the table budget is not even asked for
  {
    SrsOwner h;
    g_table_budget = 8 * n * 64;
    const size_t a0 = g_allocs;
    CHECK(make(n, 1, 0, 0, &h) == MZK_OK && h->sets == 2 && g_allocs == a0 + 1);
    g_table_budget = 0;
    h.reset();
    CHECK(g_live_bytes == 0);
  }
  printf("ok a\n");

  // ---- b: the last rung refused too: MZK_E_NOMEM in the words of the prepared points, no handle, nothing left behind
  {
    SrsOwner h;
    CHECK(make(n, 1, 8, 4, &h) == MZK_E_NOMEM && !h && g_refused == 8);
    char text[256];
    snprintf(text, sizeof text, "SRS handle: the device has no %zu bytes left for the prepared points alone (idle workspace already released)", n * 128);
    CHECK(!strcmp(g_msg, text));
    CHECK(g_live.empty() && g_live_bytes == 0);
    CHECK(make(n, 0, 2, 4, &h) == MZK_E_NOMEM && !h && g_live_bytes == 0);      // prepared points asked for: one rung
  }
  printf("ok b\n");

  // ---- c: an empty handle takes the first rung and no memory; one on context 1 says so
  {
    SrsOwner h;
    const size_t a0 = g_allocs;
    CHECK(make(0, 1, 0, 0, &h) == MZK_OK && !h->own.mem && !h->has_tables && h->table_bytes() == 0 && g_allocs == a0);
    CHECK(make(0, 16, 3, 0, &h) == MZK_OK && !h->own.mem && h->has_tables && h->own.bits == 16 && h->sets == 1 && g_refused == 0);
    CHECK(h->points().d == nullptr && h->points().stride == 0);
    g_cur = 1;
    CHECK(make(300, 1, 0, 0, &h) == MZK_OK && h->ctx_index == 1 && h->own.bits == 8 && h->own.bytes == 32 * 300 * 64);
    g_cur = 0;
    h.reset();
    CHECK(g_live_bytes == 0);
  }
  printf("ok c\n");

  // ---- d: direct tables attached, replaced and dropped: one owner at a time, the bytes counted while they are held
  {
    SrsOwner h;
    CHECK(make(40, 1, 0, 0, &h) == MZK_OK && h->own.bits == 8);
    const size_t own = h->own.bytes;
    const SrsDirectPlan D = srs_direct_plan(40, 8, (size_t)1 << 40);
    CHECK(D.err == SRS_DIRECT_OK);
    DevMem d;
    CHECK(d.alloc(D.bytes, "direct") == MZK_OK);
    void* first = d.get();
    h->direct.attach(std::move(d), D.bits, D.bytes);
    CHECK(!d && h->direct.mem.get() == first && h->direct.bits == 8 && h->table_bytes() == own + D.bytes && g_live_bytes == own + D.bytes);
    const SrsDirectPlan D9 = srs_direct_plan(40, 9, (size_t)1 << 40);
    CHECK(d.alloc(D9.bytes, "direct") == MZK_OK);
    h->direct.attach(std::move(d), D9.bits, D9.bytes);                          // the 8-bit tables go
    CHECK(!g_live.count(first) && h->direct.bits == 9 && g_live_bytes == own + D9.bytes);
    h->direct.drop();
    CHECK(!h->direct.mem && h->direct.bits == 0 && h->table_bytes() == own && g_live_bytes == own);
    h->direct.drop();                                                           // nothing to drop: nothing happens
    CHECK(g_live_bytes == own);
  }
  CHECK(g_live.empty());
  printf("ok d\n");

  // ---- e: wide tables through a const handle: reserved by the first long batch, attached once built, used from then on; a refusal
  // -- device or budget -- is remembered, leaves no message, and is not tried again
  {
    SrsOwner owner;
    CHECK(make((size_t)1 << 14, 1, 0, 0, &owner) == MZK_OK);
    const mzk_srs* h = owner.get();
    const size_t own = h->own.bytes, wb = srs_wide_bytes(h->n);
    DevMem t;
    CHECK(srs_wide_reserve(h, MANY_WIDE_FROM - 1, &t) == SRS_WIDE_USE_OWN && !t && h->wide.state == SRS_WIDE_UNTRIED);
    CHECK(srs_wide_reserve(h, MANY_WIDE_FROM, &t) == SRS_WIDE_ALLOCATE && t && g_live[t.get()] == wb && h->wide.state == SRS_WIDE_UNTRIED);
    t.reset();                                                                  // the build failed: nothing is remembered
    CHECK(srs_wide_reserve(h, MANY_WIDE_FROM, &t) == SRS_WIDE_ALLOCATE && t);
    srs_wide_built(h, std::move(t));
    CHECK(!t && h->wide.state == SRS_WIDE_BUILT && h->wide.bits == MANY_WIDE_BITS && h->table_bytes() == own + wb && g_live_bytes == own + wb);
    const size_t a0 = g_allocs;
    CHECK(srs_wide_reserve(h, MANY_WIDE_FROM, &t) == SRS_WIDE_USE_WIDE && srs_wide_reserve(h, 100, &t) == SRS_WIDE_USE_OWN && !t && g_allocs == a0);
  }
  CHECK(g_live.empty());
  for (int by_budget = 0; by_budget < 2; by_budget++) {
    SrsOwner owner;
    CHECK(make((size_t)1 << 14, 1, 0, 0, &owner) == MZK_OK);
    const mzk_srs* h = owner.get();
    DevMem t;
    if (by_budget) g_table_budget = h->own.bytes + srs_wide_bytes(h->n) - 1;
    else g_refuse = 1;
    g_refused = 0;
    snprintf(g_msg, sizeof g_msg, "untouched");
    CHECK(srs_wide_reserve(h, MANY_WIDE_FROM, &t) == SRS_WIDE_USE_OWN && !t && h->wide.state == SRS_WIDE_REFUSED);
    CHECK(g_refused == (by_budget ? 0u : 1u));
    CHECK(!strcmp(g_msg, by_budget ? "untouched" : ""));                        // the refused allocation's message does not stay
    g_table_budget = 0;
    const size_t a0 = g_allocs;
    CHECK(srs_wide_reserve(h, MANY_WIDE_FROM, &t) == SRS_WIDE_USE_OWN && !t && g_allocs == a0 && h->table_bytes() == h->own.bytes);
  }
  CHECK(g_live.empty() && g_live_bytes == 0);
  printf("ok e\n");

  for (g_cur = 0; g_cur < 2; g_cur++) ws_release_all();
  CHECK(g_live.empty());
  printf("ok all\n");
  return 0;
}
