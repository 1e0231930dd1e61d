// Merkle::hash and Merkle::verify of the C++ mirror (myzkp_amd/host/myzkp.hpp: plain host code over its own SHA3-256) against vectors
// written by tests/das_model.py, for tests/test_hostcheck_merkle_host.py.  Stand-alone: links nothing of the library.
//   usage: merkle_host_shim <vector file>
//   H <message hex or -> <digest hex>
//   V <root hex> <index> <leaf hex> <expected 0 / 1> <path entry hex> ...
// Prints "ok <hashes> <verifies>" or one line per mismatch and exits 1.  Built once plain and once with -fsanitize=address,undefined.
#include <cstdio>
#include <fstream>
#include <iostream>
#include <sstream>
#include "../../myzkp_amd/host/myzkp.hpp"

static std::vector<uint8_t> unhex(const std::string& s) {
  std::vector<uint8_t> out;
  if (s == "-") return out;
  for (size_t i = 0; i + 1 < s.size(); i += 2) out.push_back((uint8_t)std::stoi(s.substr(i, 2), nullptr, 16));
  return out;
}

int main(int argc, char** argv) {
  if (argc != 2) { fprintf(stderr, "usage: %s <vector file>\n", argv[0]); return 2; }
  std::ifstream in(argv[1]);
  if (!in) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
  std::string line;
  size_t hashes = 0, verifies = 0, bad = 0, at = 0;
  while (std::getline(in, line)) {
    at++;
    std::istringstream f(line);
    std::string kind;
    f >> kind;
    if (kind == "H") {
      std::string msg, digest;
      f >> msg >> digest;
      if (myzkp::Merkle::hash(unhex(msg)) != unhex(digest)) { printf("line %zu: hash differs\n", at); bad++; }
      hashes++;
    } else if (kind == "V") {
      std::string root, leaf, e;
      size_t index;
      int want;
      f >> root >> index >> leaf >> want;
      myzkp::MerklePath path;
      while (f >> e) path.push_back(unhex(e));
      if ((int)myzkp::Merkle::verify(unhex(root), index, path, unhex(leaf)) != want) { printf("line %zu: verify is not %d\n", at, want); bad++; }
      verifies++;
    }
  }
  if (bad) return 1;
  printf("ok %zu %zu\n", hashes, verifies);
  return 0;
}
