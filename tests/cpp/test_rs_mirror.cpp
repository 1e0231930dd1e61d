// The reference's nine Reed-Solomon tests (algebra/reedsolomon.rs:461-570) through the C++ mirror (myzkp_amd/host/myzkp.hpp:
// setup_rs1d / encode_rs1d / decode_rs1d, setup_rs2d / encode_rs2d / decode_rs2d), statement for statement; `code[i] += v` is u8
// addition there and here.  Prints the codes as hex for tests/test_gpu_rs_cpp.py, which compares them with tests/rs_model.py.
#include <cstdio>
#include "../../myzkp_amd/host/myzkp.hpp"
using namespace myzkp;

static int failures = 0;
#define CHECK(c) do { if (!(c)) { printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); failures++; } } while (0)
typedef std::vector<uint8_t> Bytes;

static void put(const char* what, const Bytes& v) {
  printf("%s", what);
  for (uint8_t b : v) printf(" %02x", b);
  printf("\n");
}
static Bytes tail(const Bytes& v, size_t from) { return Bytes(v.begin() + from, v.end()); }

static void test_syndrome_computation_no_error() {
  const auto rs = setup_rs1d(7, 3);
  const Bytes codeword = encode_rs1d({9, 1, 7}, rs);
  uint8_t syndromes[4] = {1, 1, 1, 1};
  expect(mzk_rs_syndromes(7, 3, codeword.data(), 1, syndromes));
  for (uint8_t s : syndromes) CHECK(s == 0);
  put("generator", rs.generator_polynomial());
}
static void test_no_errors() {
  const auto rs = setup_rs1d(7, 3);
  const Bytes message = {9, 1, 7};
  const Bytes code = encode_rs1d(message, rs);
  put("code.9.1.7", code);
  CHECK(tail(code, 4) == message);
  const auto decoded = decode_rs1d(code, rs);
  CHECK(decoded && *decoded == message);
}
static void test_single_error_correction() {
  const auto rs = setup_rs1d(7, 3);
  const Bytes message = {1, 2, 3};
  Bytes code = encode_rs1d(message, rs);
  put("code.1.2.3", code);
  code[3] += 10;
  const auto decoded = decode_rs1d(code, rs);
  CHECK(decoded && *decoded == message);
}
static void test_multiple_error_correction() {
  const auto rs = setup_rs1d(7, 3);
  const Bytes message = {4, 8, 15};
  Bytes code = encode_rs1d(message, rs);
  put("code.4.8.15", code);
  CHECK(tail(code, 4) == message);
  code[1] += 7;
  code[5] += 12;
  const auto decoded = decode_rs1d(code, rs);
  CHECK(decoded && *decoded == message);
}
static void test_too_many_errors() {
  const auto rs = setup_rs1d(7, 3);
  const Bytes message = {2, 4, 6};
  Bytes code = encode_rs1d(message, rs);
  put("code.2.4.6", code);
  CHECK(tail(code, 4) == message);
  code[0] += 3;
  code[3] += 5;
  code[6] += 7;
  CHECK(!decode_rs1d(code, rs));
}
static void test_2d(const char* name, const Bytes& message, const std::vector<std::array<int, 3>>& errors) {
  const auto rs_e = setup_rs2d(4, 4, 3);
  auto code = encode_rs2d(message, rs_e);
  for (size_t r = 0; r < code.size(); r++) {
    char what[64];
    snprintf(what, sizeof what, "%s.row%zu", name, r);
    put(what, code[r]);
  }
  CHECK(code[2][2] == message[0] && code[2][3] == message[1] && code[3][2] == message[2]);
  for (const auto& e : errors) code[e[0]][e[1]] += (uint8_t)e[2];
  const auto rs_d = setup_rs2d(4, 4, 3);
  const auto decoded = decode_rs2d(code, rs_d);
  CHECK(decoded && *decoded == message);
}

int main() {
  expect(mzk_init(0));
  test_syndrome_computation_no_error();
  test_no_errors();
  test_single_error_correction();
  test_multiple_error_correction();
  test_too_many_errors();
  test_2d("no_errors_2d", {2, 4, 6}, {});
  test_2d("single_error_correction_2d", {2, 8, 3}, {{1, 1, 10}});
  test_2d("multiple_error_correction_2d", {5, 4, 16}, {{1, 0, 6}, {1, 1, 5}});
  test_2d("too_many_errors_2d", {8, 2, 3}, {{1, 0, 6}, {0, 1, 5}});          // which, in the reference too, expects success
  // the trimmed form next to the fixed one (reedsolomon.rs:76-77)
  const auto rs = setup_rs1d(7, 3);
  put("trimmed.6.0.0", encode_rs1d({6, 0, 0}, rs));
  put("fixed.6.0.0", encode_rs1d_fixed({6, 0, 0}, rs));
  CHECK(encode_rs1d({0, 0, 0}, rs).empty() && encode_rs1d({6}, rs) == encode_rs1d({6, 0, 0}, rs));
  // the reference's assertions surface as Panic
  try { (void)setup_rs1d(3, 7); CHECK(false); } catch (const Panic& p) { CHECK(p.code == MZK_E_ARG); }
  try { (void)encode_rs1d({1, 2, 3, 4}, rs); CHECK(false); } catch (const Panic& p) { CHECK(p.code == MZK_E_LENGTH); }
  try { (void)encode_rs1d({1}, setup_rs1d(256, 8)); CHECK(false); } catch (const Panic& p) { CHECK(p.code == MZK_E_ARG); }
  if (failures) { printf("%d failure(s)\n", failures); return 1; }
  printf("rs mirror tests passed\n");
  return 0;
}
