// mzk_das.hip -- Celestia's commitment on the device (das/celestia.rs:73-169 over algebra/merkle.rs): the Merkle tree of every row and
// every column of a batch of byte squares in ONE launch, the tree over their roots in a second, and a handle that keeps every node so
// that sample proofs are gathers.  The shapes, the trees a workgroup takes and every size are decided in mzk_das_plan.h.
//
// A leaf is one symbol, one byte, and is not hashed itself.  Merkle::commit splits at mid = len / 2, so a tree of n leaves is
// M = 2^floor(log2 n) items of one or two leaves under a full binary tree (mzk_das_plan.h).  Every hashed message is 2 bytes (two
// leaves), 33 bytes (a one-leaf item beside a two-leaf item's digest) or 64 bytes: below the 136-byte rate, so every node is exactly
// one Keccak permutation and a tree is n - 1 of them.  A tree has at most 128 items: it lives in LDS from its items to its root.
#include "mzk_common.h"
#include "mzk_das_plan.h"
#include "mzk_keccak.h"
#include "mzk_keccak_pair.h"

namespace mzk {

// One side of the squares: all row trees or all column trees, flat and square-major (tree t of the rows = row t % rows of square t / rows).
struct DasSide {
  int n, depth, items, g_log;      // leaves, D, M of one tree; log2 of the trees per workgroup G = DAS_WG_ITEMS / M
  size_t trees, wgs;               // trees of this side, workgroups' worth of them
  u8* roots;                       // trees x 32 bytes
  u8* nodes;                       // handle form: level l (0 = items) of all trees at node das_level_offset(trees, M, l); null: roots only
};

// node `i` of LDS level l of a workgroup: the G trees side by side, tree-major, so that the children of node h are nodes 2h and 2h + 1
// of the level below and the G roots end up contiguous
__device__ __forceinline__ int das_lds_level(int l) { return 2 * (int)DAS_WG_ITEMS - ((2 * (int)DAS_WG_ITEMS) >> l); }

// A workgroup takes G trees of one side: G * M = DAS_WG_ITEMS items, two per lane, then G * M / 2^l hashes at level l -- one permutation
// per lane and step, the lanes full down to G * M / 2^l < 256.  A column workgroup takes G ADJACENT columns with the lanes along them, so
// that a step down the rows reads G contiguous bytes.  A power-of-two leaf count is the same code: every item is then one leaf and level 1
// hashes two bytes.
__global__ __launch_bounds__(DAS_TREE_BLOCK) void k_das_trees(const u8* __restrict__ code, size_t row_stride, size_t square_stride, int rows, int cols, DasSide rs,
                                                               DasSide cs, unsigned iters) {
  __shared__ uint4 sh[DAS_TREE_LDS / 16];
  const int tid = threadIdx.x;
  const size_t total = rs.wgs + cs.wgs;
#pragma unroll 1
  for (unsigned it = 0; it < iters; it++) {
    const size_t wg = (size_t)it * gridDim.x + blockIdx.x;
    if (wg >= total) break;                                  // workgroup-uniform
    if (it) __syncthreads();                                 // the copy-out of the round before still reads the LDS
    const bool col = wg >= rs.wgs;
    const int n = col ? cs.n : rs.n, D = col ? cs.depth : rs.depth, M = col ? cs.items : rs.items, g_log = col ? cs.g_log : rs.g_log;
    const size_t trees = col ? cs.trees : rs.trees;
    u8* const roots = col ? cs.roots : rs.roots;
    u8* const nodes = col ? cs.nodes : rs.nodes;
    const size_t first = (col ? wg - rs.wgs : wg) << g_log;
    const int side = col ? cols : rows;                      // trees per square on this side
#pragma unroll 1
    for (int ph = 0; ph <= D; ph++) {
      const int count = (int)DAS_WG_ITEMS >> ph;
#pragma unroll 1
      for (int h = tid; h < count; h += (int)DAS_TREE_BLOCK) {
        int g, out;
        if (ph == 0) {
          int p;
          das_item_slot(col, h, D, g_log, &g, &p);
          out = g * M + p;
        } else {
          g = h >> (D - ph);
          out = das_lds_level(ph) + h;
        }
        const size_t tree = first + (size_t)g;
        if (tree >= trees) continue;
        u64 a[25];
        bool hash = true;
        if (ph == 0) {
          int start, size;
          das_item(n, D, out - g * M, &start, &size);
          const size_t q = tree / (size_t)side, line = tree - q * (size_t)side;
          const u8* at = code + q * square_stride + (col ? (size_t)start * row_stride + line : line * row_stride + (size_t)start);
          const u64 b0 = at[0];
          if (size == 2) {
            const u64 b1 = at[col ? row_stride : 1];
            a[0] = b0 | (b1 << 8) | (0x06ULL << 16);
          } else {
            hash = false;
            a[0] = b0;                                       // a one-leaf item is the byte itself, zeros behind it
          }
          a[1] = a[2] = a[3] = 0;
#pragma unroll
          for (int i = 4; i < 9; i++) a[i] = 0;
        } else {
          const uint4* c = sh + 2 * (das_lds_level(ph - 1) + 2 * h);
          const uint4 l0 = c[0], l1 = c[1], r0 = c[2], r1 = c[3];
          const u64 L[4] = {(u64)l0.x | (u64)l0.y << 32, (u64)l0.z | (u64)l0.w << 32, (u64)l1.x | (u64)l1.y << 32, (u64)l1.z | (u64)l1.w << 32};
          const u64 R[4] = {(u64)r0.x | (u64)r0.y << 32, (u64)r0.z | (u64)r0.w << 32, (u64)r1.x | (u64)r1.y << 32, (u64)r1.z | (u64)r1.w << 32};
          int ll = 32, lr = 32;                              // bytes of the two children: items may be one byte
          if (ph == 1) {
            int start, k;
            das_item(n, D - 1, h & ((M >> 1) - 1), &start, &k);         // the slice of 2, 3 or 4 leaves above the two items
            ll = k / 2 == 1 ? 1 : 32;
            lr = k - k / 2 == 1 ? 1 : 32;
          }
#pragma unroll
          for (int i = 0; i < 9; i++) a[i] = 0;
          if (ll == 32) {                                    // two digests (a digest is never followed by a leaf: the smaller half goes left)
            a[0] = L[0]; a[1] = L[1]; a[2] = L[2]; a[3] = L[3];
            a[4] = R[0]; a[5] = R[1]; a[6] = R[2]; a[7] = R[3]; a[8] = 0x06ULL;
          } else if (lr == 32) {                             // 33 bytes: the leaf, then the digest
            a[0] = (L[0] & 0xff) | (R[0] << 8);
            a[1] = (R[0] >> 56) | (R[1] << 8);
            a[2] = (R[1] >> 56) | (R[2] << 8);
            a[3] = (R[2] >> 56) | (R[3] << 8);
            a[4] = (R[3] >> 56) | (0x06ULL << 8);
          } else {
            a[0] = (L[0] & 0xff) | ((R[0] & 0xff) << 8) | (0x06ULL << 16);
          }
        }
        if (hash) {
#pragma unroll
          for (int i = 9; i < 25; i++) a[i] = 0;
          a[16] = 0x8000000000000000ULL;                     // byte 135 of the one block
          keccak_f(a);
        }
        const uint4 o0 = make_uint4((u32)a[0], (u32)(a[0] >> 32), (u32)a[1], (u32)(a[1] >> 32));
        const uint4 o1 = make_uint4((u32)a[2], (u32)(a[2] >> 32), (u32)a[3], (u32)(a[3] >> 32));
        sh[2 * out] = o0;
        sh[2 * out + 1] = o1;
        if (ph == D) {
          uint4* r = reinterpret_cast<uint4*>(roots + tree * DAS_NODE);
          r[0] = o0;
          r[1] = o1;
        }
      }
      __syncthreads();
    }
    if (nodes != nullptr) {                                  // workgroup-uniform: every level below the roots, 16 bytes per lane and store
      const size_t live = trees - first < ((size_t)1 << g_log) ? trees - first : (size_t)1 << g_log;
      for (int l = 0; l < D; l++) {
        const int per = M >> l;
        uint4* dst = reinterpret_cast<uint4*>(nodes) + 2 * (das_level_offset(trees, M, l) + first * (size_t)per);
        const uint4* src = sh + 2 * das_lds_level(l);
        const int n16 = 2 * (int)live * per;
        for (int i = tid; i < n16; i += (int)DAS_TREE_BLOCK) dst[i] = src[i];
      }
    }
  }
}

// The tree over the rows + cols roots of one square (rows first), one workgroup per square: at most 256 items of one or two 32-byte
// leaves, every message 64 bytes.  A few hundred dependent hashes on one CU is latency, so a hash is a lane PAIR (mzk_keccak_pair.h).
__global__ __launch_bounds__(DAS_ROOT_BLOCK) void k_das_data_roots(const u32* __restrict__ row_roots, const u32* __restrict__ col_roots, int rows, int cols, int depth,
                                                                    size_t squares, u32* __restrict__ data_roots, unsigned iters) {
  __shared__ u32 sh[2][256 * 8];
  const int h = threadIdx.x >> 1, parity = threadIdx.x & 1;
  const int n = rows + cols, M = 1 << depth;
#pragma unroll 1
  for (unsigned it = 0; it < iters; it++) {
    const size_t q = (size_t)it * gridDim.x + blockIdx.x;
    if (q >= squares) break;                                 // workgroup-uniform (a round ends behind a barrier: the LDS is free)
    if (h < M) {                                             // pair-uniform, as every condition below
      int start, size;
      das_item(n, depth, h, &start, &size);
      auto leaf = [&](int i) { return i < rows ? row_roots + (q * (size_t)rows + (size_t)i) * 8 : col_roots + (q * (size_t)cols + (size_t)(i - rows)) * 8; };
      const u32* l0 = leaf(start);
      if (size == 2) {
        const u32* l1 = leaf(start + 1);
        u32 a[25];
#pragma unroll
        for (int i = 0; i < 4; i++) { a[i] = l0[2 * i + parity]; a[4 + i] = l1[2 * i + parity]; }
        a[8] = parity ? 0u : 0x06u;
#pragma unroll
        for (int i = 9; i < 25; i++) a[i] = 0;
        a[16] = parity ? 0x80000000u : 0u;
        keccak_f_pair(a, parity);
#pragma unroll
        for (int i = 0; i < 4; i++) sh[0][8 * h + 2 * i + parity] = a[i];
      } else {
#pragma unroll
        for (int i = 0; i < 4; i++) sh[0][8 * h + 2 * i + parity] = l0[2 * i + parity];
      }
    }
    __syncthreads();
    int cur = 0;
#pragma unroll 1
    for (int cnt = M >> 1; cnt >= 1; cnt >>= 1) {
      if (h < cnt) {
        u32 a[25];
        const u32* c32 = sh[cur] + 16 * h;
#pragma unroll
        for (int i = 0; i < 8; i++) a[i] = c32[2 * i + parity];
        a[8] = parity ? 0u : 0x06u;
#pragma unroll
        for (int i = 9; i < 25; i++) a[i] = 0;
        a[16] = parity ? 0x80000000u : 0u;
        keccak_f_pair(a, parity);
        u32* o = cnt == 1 ? data_roots + q * 8 : sh[cur ^ 1] + 8 * h;
#pragma unroll
        for (int i = 0; i < 4; i++) o[2 * i + parity] = a[i];
      }
      __syncthreads();
      cur ^= 1;
    }
  }
}

// the symbols of a view, dense (what a handle keeps for the leaves of its paths)
__global__ __launch_bounds__(256) void k_das_copy_symbols(const u8* __restrict__ code, size_t row_stride, size_t square_stride, int rows, int cols, size_t total,
                                                           u8* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const size_t per = (size_t)rows * (size_t)cols;
  const size_t q = i / per, rc = i - q * per, r = rc / (size_t)cols, c = rc - r * (size_t)cols;
  out[i] = code[q * square_stride + r * row_stride + c];
}

// What the gather reads of a handle
struct DasGridView {
  int rows, cols;
  size_t squares;
  DasSide rs, cs;                  // nodes and roots of the two sides
  const u8* symbols;               // squares x rows x cols, dense
};

// Merkle::open for `count` samples, one lane per (sample, entry): depth and entry lengths follow from n alone (das_locate), the bytes
// from the stored levels.  Entry 0 of a two-leaf item is the other leaf; then the sibling item (a byte or a digest); then the sibling
// node of every level below the root.
__global__ __launch_bounds__(256) void k_das_gather(DasGridView v, const u64* __restrict__ positions, size_t count, uint4* __restrict__ paths, u8* __restrict__ entry_lens,
                                                     u8* __restrict__ depths, u8* __restrict__ leaves) {
  const size_t gid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t s = gid >> 3;
  const int k = (int)(gid & 7);
  if (s >= count) return;
  const u64 q = positions[4 * s], r = positions[4 * s + 1], c = positions[4 * s + 2], is_row = positions[4 * s + 3];
  if (q >= v.squares || r >= (u64)v.rows || c >= (u64)v.cols || is_row > 1) {
    if (k == 0) depths[s] = 255;
    return;
  }
  const int n = is_row ? v.rs.n : v.cs.n, D = is_row ? v.rs.depth : v.cs.depth, M = is_row ? v.rs.items : v.cs.items;
  const size_t trees = is_row ? v.rs.trees : v.cs.trees;
  const u8* nodes = is_row ? v.rs.nodes : v.cs.nodes;
  const int index = is_row ? (int)c : (int)r;
  const size_t tree = is_row ? q * (size_t)v.rows + r : q * (size_t)v.cols + c;
  int p, start, size, sib;
  das_locate(n, D, index, &p, &start, &size, &sib);
  const int depth = das_path_depth(D, size, sib);
  const u8* sym = v.symbols + q * (size_t)v.rows * (size_t)v.cols;
  if (k == 0) {
    depths[s] = (u8)depth;
    leaves[s] = sym[r * (size_t)v.cols + c];
  }
  uint4 lo = make_uint4(0, 0, 0, 0), hi = lo;
  int len = 0;
  if (k < depth) {
    const int e = size == 2 ? k : k + 1;
    if (e == 0) {
      const int other = start + 1 - (index - start);
      lo.x = is_row ? sym[r * (size_t)v.cols + (size_t)other] : sym[(size_t)other * (size_t)v.cols + c];
      len = 1;
    } else {
      const int l = e - 1;                                   // level 0: the sibling item; level l: node (p >> l) ^ 1
      const size_t node = das_level_offset(trees, M, l) + tree * (size_t)(M >> l) + (size_t)((p >> l) ^ 1);
      const uint4* src = reinterpret_cast<const uint4*>(nodes) + 2 * node;
      lo = src[0];
      hi = src[1];
      len = l == 0 && sib == 1 ? 1 : 32;
    }
  }
  paths[2 * gid] = lo;
  paths[2 * gid + 1] = hi;
  entry_lens[gid] = (u8)len;
}

// ---- host side ------------------------------------------------------------------------------------------------------------------------
static int das_plan_checked(size_t rows, size_t cols, size_t row_stride, size_t square_stride, size_t squares, DasPlan* P) {
  *P = das_plan(rows, cols, row_stride, square_stride, squares);
  if (P->err != MZK_OK) { set_error("%s", P->msg); return P->err; }
  return MZK_OK;
}
static int ilog2_exact(unsigned v) { int l = 0; while ((1u << l) < v) l++; return l; }
static DasSide das_side(const DasTree& t, unsigned g, size_t trees, size_t wgs, void* roots, void* nodes) {
  return DasSide{t.n, t.depth, t.items, ilog2_exact(g), trees, wgs, (u8*)roots, (u8*)nodes};
}

// both launches; d_*_nodes null: roots only
static int das_hash(const DasPlan& P, const void* d_code, size_t row_stride, size_t square_stride, void* d_row_roots, void* d_col_roots, void* d_data_roots,
                    void* d_row_nodes, void* d_col_nodes, hipStream_t s) {
  if (!d_code || !d_row_roots || !d_col_roots || !d_data_roots) { set_error("das: null pointer"); return MZK_E_ARG; }
  if (((uintptr_t)d_row_roots | (uintptr_t)d_col_roots | (uintptr_t)d_data_roots) & 15) { set_error("das: the root outputs must be 16-byte aligned"); return MZK_E_ARG; }
  const DasSide rs = das_side(P.row_tree, P.row_g, P.row_trees, P.row_wgs, d_row_roots, d_row_nodes);
  const DasSide cs = das_side(P.col_tree, P.col_g, P.col_trees, P.col_wgs, d_col_roots, d_col_nodes);
  hipLaunchKernelGGL(k_das_trees, dim3((unsigned)P.trees.grid), dim3(P.trees.block), 0, s, (const u8*)d_code, row_stride, square_stride, (int)P.rows, (int)P.cols, rs, cs,
                     P.trees.iters);
  MZK_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_das_data_roots, dim3((unsigned)P.roots.grid), dim3(P.roots.block), 0, s, (const u32*)d_row_roots, (const u32*)d_col_roots, (int)P.rows, (int)P.cols,
                     P.root_tree.depth, P.squares, (u32*)d_data_roots, P.roots.iters);
  MZK_HIP(hipGetLastError());
  return MZK_OK;
}

static int das_stage_in(WsFrame& ws, WsSlot slot, const void* host, size_t bytes, void** dev, hipStream_t s) {
  MZK_TRY(ws.get(slot, bytes, dev));
  MZK_HIP(hipMemcpyAsync(*dev, host, bytes, hipMemcpyHostToDevice, s));
  return MZK_OK;
}

}  // namespace mzk

using namespace mzk;

struct mzk_das_grid {
  DasPlan plan;
  DevMem mem;                      // row nodes | column nodes | row roots | column roots | data roots | symbols
  u8 *d_row_nodes = nullptr, *d_col_nodes = nullptr, *d_row_roots = nullptr, *d_col_roots = nullptr, *d_data_roots = nullptr, *d_symbols = nullptr;
  // Owner: the context (and its device) whose memory holds the grid, as for a mzk_merkle.  Later operations enter that context and
  // run behind `built`.
  int ctx_index = 0;
  int device = -1;
  hipEvent_t built = nullptr;
};

namespace mzk {

struct DasScope {
  CtxScope sc;
  int rc;
  explicit DasScope(const mzk_das_grid* g) : sc(g->ctx_index), rc(MZK_OK) {
    if (!sc.ok || ctx().device != g->device) {
      set_error("das grid handle was built on context %d (device %d); that context %s", g->ctx_index, g->device, sc.ok ? "drives another device now" : "no longer exists");
      rc = MZK_E_ARG;
    }
  }
  int wait(const mzk_das_grid* g, hipStream_t s) const {
    if (g->built && hipStreamWaitEvent(s, g->built, 0) != hipSuccess) { (void)hipGetLastError(); set_error("das: cannot order behind the build"); return MZK_E_HIP; }
    return MZK_OK;
  }
};

static int das_grid_build_impl(const void* d_code, const DasPlan& P, size_t row_stride, size_t square_stride, mzk_das_grid** out, hipStream_t s) {
  std::unique_ptr<mzk_das_grid> g(new mzk_das_grid());
  g->plan = P;
  MZK_TRY(g->mem.alloc(P.handle_bytes, "das grid"));
  g->d_row_nodes = g->mem.as<u8>();
  g->d_col_nodes = g->d_row_nodes + P.row_node_bytes;
  g->d_row_roots = g->d_col_nodes + P.col_node_bytes;
  g->d_col_roots = g->d_row_roots + P.row_trees * DAS_NODE;
  g->d_data_roots = g->d_col_roots + P.col_trees * DAS_NODE;
  g->d_symbols = g->d_data_roots + P.squares * DAS_NODE;
  g->ctx_index = ctx().index;
  g->device = ctx().device;
  hipLaunchKernelGGL(k_das_copy_symbols, dim3((unsigned)((P.symbol_bytes + 255) / 256)), dim3(256), 0, s, (const u8*)d_code, row_stride, square_stride, (int)P.rows,
                     (int)P.cols, P.symbol_bytes, g->d_symbols);
  int rc = hipGetLastError() == hipSuccess ? MZK_OK : MZK_E_HIP;
  if (rc == MZK_OK) rc = das_hash(P, d_code, row_stride, square_stride, g->d_row_roots, g->d_col_roots, g->d_data_roots, g->d_row_nodes, g->d_col_nodes, s);
  if (rc == MZK_OK && hipEventCreateWithFlags(&g->built, hipEventDisableTiming) != hipSuccess) rc = MZK_E_HIP;
  if (rc == MZK_OK && hipEventRecord(g->built, s) != hipSuccess) rc = MZK_E_HIP;
  if (rc != MZK_OK) {
    if (rc == MZK_E_HIP) { (void)hipGetLastError(); set_error("das grid: launch or event failed"); }
    (void)hipStreamSynchronize(s);       // enqueued work may still write the buffers that go away here
    mzk_das_grid_free(g.release());
    return rc;
  }
  *out = g.release();
  return MZK_OK;
}

static DasGridView das_view(const mzk_das_grid* g) {
  const DasPlan& P = g->plan;
  return DasGridView{(int)P.rows, (int)P.cols, P.squares, das_side(P.row_tree, P.row_g, P.row_trees, P.row_wgs, g->d_row_roots, g->d_row_nodes),
                     das_side(P.col_tree, P.col_g, P.col_trees, P.col_wgs, g->d_col_roots, g->d_col_nodes), g->d_symbols};
}
constexpr size_t DAS_MAX_SAMPLES = (size_t)1 << 28;      // 8 lanes each: the grid stays below 2^31 lanes
static int das_gather(const mzk_das_grid* g, const void* d_positions, size_t count, void* d_paths, void* d_entry_lens, void* d_depths, void* d_leaves, hipStream_t s) {
  hipLaunchKernelGGL(k_das_gather, dim3((unsigned)((count * 8 + 255) / 256)), dim3(256), 0, s, das_view(g), (const u64*)d_positions, count, (uint4*)d_paths,
                     (u8*)d_entry_lens, (u8*)d_depths, (u8*)d_leaves);
  MZK_HIP(hipGetLastError());
  return MZK_OK;
}

}  // namespace mzk

// ---- C ABI (include/mzk.h, "Celestia's commitment") ------------------------------------------------------------------------------------
extern "C" {

int mzk_das_plan_get(size_t rows, size_t cols, size_t squares, uint64_t* plan) {
  DasPlan P;
  MZK_TRY(das_plan_checked(rows, cols, cols, rows * cols, squares, &P));
  if (!plan) { set_error("das_plan: null pointer"); return MZK_E_ARG; }
  das_plan_export(P, plan);
  return MZK_OK;
}

int mzk_das_commit_dev(const void* d_code, size_t rows, size_t cols, size_t row_stride, size_t square_stride, size_t squares, void* d_row_roots, void* d_col_roots,
                       void* d_data_roots, void* stream) {
  MZK_ENTER();
  WsFrame ws("mzk_das_commit_dev");
  WsGuard wsg((hipStream_t)stream);
  DasPlan P;
  MZK_TRY(das_plan_checked(rows, cols, row_stride, square_stride, squares, &P));
  if (!d_row_roots || !d_col_roots) {                        // only the data roots are wanted: the others are scratch
    u8* scratch;
    MZK_TRY(ws.get(WS_MISC_A, (P.row_trees + P.col_trees) * DAS_NODE, (void**)&scratch));
    if (!d_row_roots) d_row_roots = scratch;
    if (!d_col_roots) d_col_roots = scratch + P.row_trees * DAS_NODE;
  }
  return das_hash(P, d_code, row_stride, square_stride, d_row_roots, d_col_roots, d_data_roots, nullptr, nullptr, (hipStream_t)stream);
}

int mzk_das_commit(const uint8_t* code, size_t rows, size_t cols, size_t squares, uint8_t* row_roots, uint8_t* col_roots, uint8_t* data_roots) {
  MZK_ENTER();
  WsFrame ws("mzk_das_commit");
  DasPlan P;
  MZK_TRY(das_plan_checked(rows, cols, cols, rows * cols, squares, &P));
  if (!code || !data_roots) { set_error("das_commit: null pointer"); return MZK_E_ARG; }
  hipStream_t s = ctx().stream;
  WsGuard wsg(s);
  void* d_c;
  u8* d_o;      // row roots | column roots | data roots
  MZK_TRY(das_stage_in(ws, WS_MISC_B, code, P.symbol_bytes, &d_c, s));
  MZK_TRY(ws.get(WS_MISC_C, P.root_bytes, (void**)&d_o));
  u8 *d_r = d_o, *d_l = d_r + P.row_trees * DAS_NODE, *d_d = d_l + P.col_trees * DAS_NODE;
  MZK_TRY(das_hash(P, d_c, cols, rows * cols, d_r, d_l, d_d, nullptr, nullptr, s));
  if (row_roots) MZK_HIP(hipMemcpyAsync(row_roots, d_r, P.row_trees * DAS_NODE, hipMemcpyDeviceToHost, s));
  if (col_roots) MZK_HIP(hipMemcpyAsync(col_roots, d_l, P.col_trees * DAS_NODE, hipMemcpyDeviceToHost, s));
  return d2h_sync(data_roots, d_d, P.squares * DAS_NODE, s);
}

int mzk_das_grid_build_dev(const void* d_code, size_t rows, size_t cols, size_t row_stride, size_t square_stride, size_t squares, mzk_das_grid** out, void* stream) {
  MZK_ENTER();
  if (!out) { set_error("das_grid_build: null output handle"); return MZK_E_ARG; }
  *out = nullptr;
  DasPlan P;
  MZK_TRY(das_plan_checked(rows, cols, row_stride, square_stride, squares, &P));
  if (!d_code) { set_error("das_grid_build: null pointer"); return MZK_E_ARG; }
  return das_grid_build_impl(d_code, P, row_stride, square_stride, out, (hipStream_t)stream);
}

int mzk_das_grid_build(const uint8_t* code, size_t rows, size_t cols, size_t squares, mzk_das_grid** out) {
  MZK_ENTER();
  WsFrame ws("mzk_das_grid_build");
  if (!out) { set_error("das_grid_build: null output handle"); return MZK_E_ARG; }
  *out = nullptr;
  DasPlan P;
  MZK_TRY(das_plan_checked(rows, cols, cols, rows * cols, squares, &P));
  if (!code) { set_error("das_grid_build: null pointer"); return MZK_E_ARG; }
  hipStream_t s = ctx().stream;
  WsGuard wsg(s);
  void* d_c;
  MZK_TRY(das_stage_in(ws, WS_MISC_B, code, P.symbol_bytes, &d_c, s));
  MZK_TRY(das_grid_build_impl(d_c, P, cols, rows * cols, out, s));
  if (hipStreamSynchronize(s) != hipSuccess) {
    (void)hipGetLastError();
    mzk_das_grid_free(*out);
    *out = nullptr;
    set_error("das_grid_build: sync failed");
    return MZK_E_HIP;
  }
  return MZK_OK;
}

int mzk_das_grid_roots(const mzk_das_grid* g, uint8_t* row_roots, uint8_t* col_roots, uint8_t* data_roots) {
  if (!g) { set_error("das_grid_roots: null pointer"); return MZK_E_ARG; }
  MZK_ENTER();
  DasScope ds(g);
  MZK_TRY(ds.rc);
  hipStream_t s = ctx().stream;
  MZK_TRY(ds.wait(g, s));
  const DasPlan& P = g->plan;
  if (row_roots) MZK_HIP(hipMemcpyAsync(row_roots, g->d_row_roots, P.row_trees * DAS_NODE, hipMemcpyDeviceToHost, s));
  if (col_roots) MZK_HIP(hipMemcpyAsync(col_roots, g->d_col_roots, P.col_trees * DAS_NODE, hipMemcpyDeviceToHost, s));
  if (data_roots) MZK_HIP(hipMemcpyAsync(data_roots, g->d_data_roots, P.squares * DAS_NODE, hipMemcpyDeviceToHost, s));
  MZK_HIP(hipStreamSynchronize(s));
  return MZK_OK;
}

int mzk_das_grid_open(const mzk_das_grid* g, const uint64_t* positions, size_t count, uint8_t* paths, uint8_t* entry_lens, uint8_t* depths, uint8_t* leaves) {
  if (!g || ((!positions || !paths || !entry_lens || !depths || !leaves) && count)) { set_error("das_grid_open: null pointer"); return MZK_E_ARG; }
  if (count == 0) return MZK_OK;
  if (count > DAS_MAX_SAMPLES) { set_error("das_grid_open: count = %zu is beyond 2^28 samples a call", count); return MZK_E_ARG; }
  const DasPlan& P = g->plan;
  for (size_t i = 0; i < count; i++) {
    const uint64_t* p = positions + 4 * i;
    if (p[0] >= P.squares || p[1] >= P.rows || p[2] >= P.cols || p[3] > 1) {
      set_error("das_grid_open: position %zu = (square %llu, row %llu, col %llu, is_row %llu) is outside %zu squares of %zu x %zu", i, (unsigned long long)p[0],
                (unsigned long long)p[1], (unsigned long long)p[2], (unsigned long long)p[3], P.squares, P.rows, P.cols);
      return MZK_E_ARG;
    }
  }
  MZK_ENTER();
  WsFrame ws("mzk_das_grid_open");
  DasScope ds(g);
  MZK_TRY(ds.rc);
  hipStream_t s = ctx().stream;
  MZK_TRY(ds.wait(g, s));
  WsGuard wsg(s);
  const size_t path_bytes = count * MZK_DAS_PATH_MAX * DAS_NODE, len_bytes = count * MZK_DAS_PATH_MAX;
  u8* d;        // paths | positions | entry lengths | depths | leaves
  MZK_TRY(ws.get(WS_MISC_C, path_bytes + count * 32 + len_bytes + 2 * count, (void**)&d));
  u8 *d_pos = d + path_bytes, *d_len = d_pos + count * 32, *d_dep = d_len + len_bytes, *d_leaf = d_dep + count;
  MZK_HIP(hipMemcpyAsync(d_pos, positions, count * 32, hipMemcpyHostToDevice, s));
  MZK_TRY(das_gather(g, d_pos, count, d, d_len, d_dep, d_leaf, s));
  MZK_HIP(hipMemcpyAsync(paths, d, path_bytes, hipMemcpyDeviceToHost, s));
  MZK_HIP(hipMemcpyAsync(entry_lens, d_len, len_bytes, hipMemcpyDeviceToHost, s));
  MZK_HIP(hipMemcpyAsync(depths, d_dep, count, hipMemcpyDeviceToHost, s));
  MZK_HIP(hipMemcpyAsync(leaves, d_leaf, count, hipMemcpyDeviceToHost, s));
  MZK_HIP(hipStreamSynchronize(s));
  return MZK_OK;
}

int mzk_das_grid_open_dev(const mzk_das_grid* g, const void* d_positions, size_t count, void* d_paths, void* d_entry_lens, void* d_depths, void* d_leaves,
                          void* stream) {
  if (!g || ((!d_positions || !d_paths || !d_entry_lens || !d_depths || !d_leaves) && count)) { set_error("das_grid_open: null pointer"); return MZK_E_ARG; }
  if (count == 0) return MZK_OK;
  if (count > DAS_MAX_SAMPLES) { set_error("das_grid_open: count = %zu is beyond 2^28 samples a call", count); return MZK_E_ARG; }
  if (((uintptr_t)d_paths & 15) || ((uintptr_t)d_positions & 7)) { set_error("das_grid_open: d_paths must be 16-byte aligned, d_positions 8-byte aligned"); return MZK_E_ARG; }
  MZK_ENTER();
  DasScope ds(g);
  MZK_TRY(ds.rc);
  MZK_TRY(ds.wait(g, (hipStream_t)stream));
  return das_gather(g, d_positions, count, d_paths, d_entry_lens, d_depths, d_leaves, (hipStream_t)stream);
}

void mzk_das_grid_free(mzk_das_grid* g) {
  if (!g) return;
  if (g->built) (void)hipEventDestroy(g->built);
  delete g;
}

}  // extern "C"
