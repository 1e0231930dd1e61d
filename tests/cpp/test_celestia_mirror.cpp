// The reference's test_celestia (das/celestia.rs:196-231) through the C++ mirror (myzkp_amd/host/myzkp.hpp: struct Celestia), line for
// line, then the `celestia` arm of examples/da.rs for data sizes 16, 64, 256, 1024.  Prints every commitment as hex for
// tests/test_gpu_celestia_cpp.py, which compares it with tests/das_model.py over the code of tests/rs_model.py.
#include <algorithm>
#include <cstdio>
#include "../../myzkp_amd/host/myzkp.hpp"
using namespace myzkp;

static int failures = 0;
#define CHECK(c) do { if (!(c)) { printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); failures++; } } while (0)

static void put(const char* what, size_t i, const std::vector<uint8_t>& v) {
  printf("%s.%zu", what, i);
  for (uint8_t b : v) printf(" %02x", b);
  printf("\n");
}
static void put_commitment(const char* name, const CommitmentCelestia& c) {
  char what[64];
  snprintf(what, sizeof what, "%s.row", name);
  for (size_t i = 0; i < c.row_roots.size(); i++) put(what, i, c.row_roots[i]);
  snprintf(what, sizeof what, "%s.col", name);
  for (size_t i = 0; i < c.col_roots.size(); i++) put(what, i, c.col_roots[i]);
  snprintf(what, sizeof what, "%s.data", name);
  put(what, 0, c.data_root);
}

static void test_celestia() {
  const auto params = Celestia::setup(8, 2.0, 64);
  CHECK(params.codeword_size == 16 && params.chunk_size == 8);

  std::vector<uint8_t> data;
  for (int i = 0; i < 64; i++) data.push_back((uint8_t)i);
  const auto encoded = Celestia::encode(data, params);
  const auto commit = Celestia::commit(encoded, params);
  put_commitment("test_celestia", commit);

  for (size_t i = 0; i < 10; i++) {
    const SamplePosition position{i / 12, i % 12, false};
    CHECK(Celestia::verify(position, encoded, commit, params));
  }

  const auto reconstructed = Celestia::reconstruct(encoded, params);
  for (size_t i = 0; i < 63; i++) CHECK(data[i] == reconstructed[i]);

  std::vector<uint8_t> mal_data;
  for (int i = 1; i < 65; i++) mal_data.push_back((uint8_t)i);
  const auto mal_encoded = Celestia::encode(mal_data, params);
  const SamplePosition mal_position{0, 0, false};
  CHECK(!Celestia::verify(mal_position, mal_encoded, commit, params));

  // rows as well, every position, and the proof the mirror hands out is the one Merkle::verify accepts
  for (size_t r = 0; r < 16; r++)
    for (size_t c = 0; c < 16; c++) {
      CHECK(Celestia::verify(SamplePosition{r, c, true}, encoded, commit, params));
      CHECK(Celestia::verify(SamplePosition{r, c, false}, encoded, commit, params));
    }
  const ProofCelestia proof = Celestia::open(SamplePosition{3, 5, true}, commit);
  CHECK(proof.is_row && proof.proof.size() == 4 && proof.proof[0].size() == 1 && proof.proof[1].size() == 32);
  // setup computes chunk_size * ceil(expansion_factor)
  CHECK(Celestia::setup(8, 1.5, 64).codeword_size == 16 && Celestia::setup(5, 3.0, 25).codeword_size == 15);
}

static void example_da() {       // examples/da.rs:51-74
  const size_t data_sizes[] = {16, 64, 256, 1024}, sqrt_data_sizes[] = {4, 8, 16, 32};
  for (int t = 0; t < 4; t++) {
    const size_t data_size = data_sizes[t], sqrt_data_size = sqrt_data_sizes[t];
    std::vector<uint8_t> data;
    for (size_t i = 0; i < data_size; i++) data.push_back((uint8_t)(i % 256));
    const size_t expansion_factor = 2, base_num_sampling = 16;
    const auto params = Celestia::setup(sqrt_data_size, (double)expansion_factor, data_size);
    const auto encoded = Celestia::encode(data, params);
    const auto commit = Celestia::commit(encoded, params);
    const size_t side = sqrt_data_size * expansion_factor;
    for (size_t i = 0; i < std::min(side * side, base_num_sampling); i++) {
      const SamplePosition position{i / side, i % side, false};
      CHECK(Celestia::verify(position, encoded, commit, params));
    }
    char name[32];
    snprintf(name, sizeof name, "da%zu", data_size);
    put_commitment(name, commit);
    CHECK(Celestia::reconstruct(encoded, params) == data);
  }
}

int main() {
  try {
    expect(mzk_init(0));
    test_celestia();
    example_da();
  } catch (const Panic& p) {
    printf("FAIL: Panic(%d): %s\n", p.code, p.what());
    return 1;
  }
  if (failures) { printf("%d FAILED\n", failures); return 1; }
  printf("celestia mirror tests passed\n");
  return 0;
}
