// The layout and the unpack of Merkle openings (myzkp_amd/csrc/mzk_merkle_open_plan.h) run on the host for
// tests/test_hostcheck_merkle_open.py.  Stand-alone: reads cases from the file given as argv[1], each
//   case NAME stride S trees T indices I nodes N leaves L entries E scratch B rc RC bad_entry BE bad_len BL
//   tree FIELD DEPTH COUNT NEG        x T      (NEG: the tree's Sign::Minus flags in hex, or - for none; COUNT 0: a skipped tree)
//   idx  HEX    the I indices, u64 little-endian          hn HEX   the gathered digests, N u64 words
//   hl   HEX    the gathered sibling limbs, L u32 words   paths HEX / lens HEX   what E entries of S bytes / E u64 must hold afterwards
// (- for an empty array), unpacks into buffers of exactly that size pre-filled with 0xA5 and compares every byte, the return code and
// the failing entry; the totals of the layout and the byte size of the scratch are compared with I, N, L, E and B.  Prints "ok <cases>".
// Built plain and with -fsanitize=address,undefined: every array is a heap block of its exact size.
#include <stdio.h>
#include <stdlib.h>
#include <fstream>
#include <string>
#include <vector>
#include "../../myzkp_amd/csrc/mzk_merkle_open_plan.h"

using namespace mzk;

// a heap block of exactly the bytes given (one byte when empty, never read)
struct Block {
  uint8_t* p;
  size_t n;
  explicit Block(const std::string& hex) : p(nullptr), n(hex == "-" ? 0 : hex.size() / 2) {
    p = (uint8_t*)malloc(n ? n : 1);
    for (size_t i = 0; i < n; i++) p[i] = (uint8_t)strtoul(hex.substr(2 * i, 2).c_str(), nullptr, 16);
  }
  Block(size_t bytes, uint8_t fill) : p((uint8_t*)malloc(bytes ? bytes : 1)), n(bytes) { memset(p, fill, bytes ? bytes : 1); }
  Block(const Block&) = delete;
  ~Block() { free(p); }
};

static int fail(const std::string& name, const char* what) { fprintf(stderr, "case %s: %s\n", name.c_str(), what); return 1; }

int main(int argc, char** argv) {
  if (argc < 2) { fprintf(stderr, "usage: merkle_open_shim vectors.txt\n"); return 2; }
  std::ifstream f(argv[1]);
  if (!f) { perror(argv[1]); return 2; }
  std::string key, name, hex;
  size_t cases = 0;
  while (f >> key) {
    if (key != "case") return fail(key, "expected `case`");
    size_t stride, n_trees, I, N, L, E, B, want_entry, want_len;
    int want_rc;
    f >> name >> key >> stride >> key >> n_trees >> key >> I >> key >> N >> key >> L >> key >> E >> key >> B >> key >> want_rc >> key >> want_entry >> key >> want_len;
    std::vector<MerkleOpenTree> trees(n_trees);
    std::vector<Block*> negs;
    for (size_t t = 0; t < n_trees; t++) {
      f >> key >> trees[t].field >> trees[t].depth >> trees[t].count >> hex;
      if (key != "tree") return fail(name, "expected `tree`");
      negs.push_back(new Block(hex));
      trees[t].neg = negs.back()->n ? negs.back()->p : nullptr;
    }
    f >> key >> hex;
    if (key != "idx") return fail(name, "expected `idx`");
    const Block idx(hex);
    f >> key >> hex;
    const Block hn(hex);
    f >> key >> hex;
    const Block hl(hex);
    f >> key >> hex;
    const Block want_paths(hex);
    f >> key >> hex;
    const Block want_lens(hex);
    if (!f || key != "lens") return fail(name, "truncated");
    // the layout: totals and the lease
    const MerkleOpenAt total = merkle_open_totals(trees.data(), n_trees);
    if (total.index != I || total.node != N || total.leaf != L || total.entry != E) return fail(name, "totals of the layout differ");
    if (merkle_open_scratch_bytes(total) != B) return fail(name, "scratch bytes differ");
    if (idx.n != 8 * I || hn.n != 8 * N || hl.n != 4 * L || want_paths.n != E * stride || want_lens.n != 8 * E) return fail(name, "array sizes of the case");
    // the unpack
    Block paths(E * stride, 0xA5), lens(8 * E, 0xA5);
    size_t bad_entry = (size_t)-1, bad_len = (size_t)-1;
    const int rc = merkle_open_unpack(trees.data(), n_trees, (const uint64_t*)idx.p, (const uint64_t*)hn.p, (const uint32_t*)hl.p, paths.p, stride,
                                      (uint64_t*)lens.p, &bad_entry, &bad_len);
    if (rc != want_rc) return fail(name, "return code differs");
    if (rc != MZK_OK && (bad_entry != want_entry || bad_len != want_len)) return fail(name, "failing entry or its length differs");
    if (memcmp(paths.p, want_paths.p, paths.n) != 0) return fail(name, "paths differ");
    if (memcmp(lens.p, want_lens.p, lens.n) != 0) return fail(name, "path_lens differ");
    for (Block* b : negs) delete b;
    cases++;
  }
  printf("ok %zu\n", cases);
  return 0;
}
