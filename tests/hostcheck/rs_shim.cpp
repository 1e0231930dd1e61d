// GF(2^8) arithmetic (myzkp_amd/csrc/mzk_gf256.h) and the Reed-Solomon plan and tables (mzk_rs_plan.h) run on the host for
// tests/test_hostcheck_rs.py.  Stand-alone, no arguments.  Prints
//   M a <256 products a*b as hex>                    for every a
//   I <256 inverses as hex, inv(0) = 0>
//   X <mismatches of the packed forms against the scalar product>
//   T <pts as hex> <inv_pts as hex>                  (the same for every code: checked here against every call)
//   K n k d t form lanes pw pad w spl ppl npad dpad <generator as hex>          for every admitted (n, k)
//   B batch  grid block per_block iters lds  x 3 (encode, syndromes, decode)     for every batch of that (n, k)
//   R n k batch err <message>                        for every refused shape
// then "ok <codes>".  Built once plain and once with -fsanitize=address,undefined.
#include <inttypes.h>
#include <stdio.h>
#include <string.h>
#include "../../myzkp_amd/csrc/mzk_rs_plan.h"

using namespace mzk;

static void hex(const uint8_t* p, int n) {
  for (int i = 0; i < n; i++) printf("%02x", p[i]);
}

static long packed_mismatches() {
  long bad = 0;
  uint32_t x = 0x12345678u;
  for (int rep = 0; rep < 256; rep++) {
    x = x * 1664525u + 1013904223u;
    const uint32_t v = x ^ (x >> 13);
    uint32_t forms[8];
    gf256::shifted8(v, forms);
    bad += gf256::xtime4(v) != (gf256::xtime(v & 0xFF) | gf256::xtime((v >> 8) & 0xFF) << 8 | gf256::xtime((v >> 16) & 0xFF) << 16 | gf256::xtime(v >> 24) << 24);
    for (uint32_t s = 0; s < 256; s++) {
      uint32_t want = 0;
      for (int j = 0; j < 4; j++) want |= gf256::gf_mul((v >> (8 * j)) & 0xFF, s) << (8 * j);
      bad += gf256::mul4_scalar(v, s) != want;
      bad += gf256::mul4_shifted(forms, s) != want;
    }
  }
  for (uint32_t a = 0; a < 256; a++)
    for (uint32_t e = 0; e < 300; e += 7) {
      uint32_t want = 1;
      for (uint32_t i = 0; i < e; i++) want = gf256::gf_mul(want, a);
      bad += gf256::gf_pow(a, e) != want;
    }
  return bad;
}

static void print_launch(const RsLaunch& L) { printf("  %zu %u %u %u %zu", L.grid, L.block, L.per_block, L.iters, L.lds); }

int main() {
  for (uint32_t a = 0; a < 256; a++) {
    uint8_t row[256];
    for (uint32_t b = 0; b < 256; b++) row[b] = (uint8_t)gf256::gf_mul(a, b);
    printf("M %u ", a);
    hex(row, 256);
    printf("\n");
  }
  uint8_t inv[256];
  for (uint32_t a = 0; a < 256; a++) inv[a] = (uint8_t)gf256::gf_inv(a);
  printf("I ");
  hex(inv, 256);
  printf("\nX %ld\n", packed_mismatches());

  const size_t batches[] = {1, 63, 64, 65, (size_t)1 << 20, (size_t)1 << 31};
  static RsTables first, T;
  bool have_first = false;
  size_t codes = 0;
  for (size_t n = 1; n <= RS_MAX_N; n++) {
    for (size_t k = 1; k <= n; k++) {
      const RsPlan P0 = rs_plan(n, k, 1);
      if (P0.err != MZK_OK) { fprintf(stderr, "(%zu, %zu) refused: %s\n", n, k, P0.msg); return 1; }
      rs_tables(n, k, P0.enc_pad, &T);
      if (!have_first) {
        first = T;
        have_first = true;
        printf("T ");
        hex(T.pts, 256);
        printf(" ");
        hex(T.inv_pts, 256);
        printf("\n");
      }
      if (memcmp(first.pts, T.pts, 256) || memcmp(first.inv_pts, T.inv_pts, 256)) { fprintf(stderr, "(%zu, %zu): points differ\n", n, k); return 1; }
      // the shifted forms against the scalar product: byte j of word w of form b = padded generator coefficient 4w + j times x^b
      for (int w = 0; w < 64; w++)
        for (int j = 0; j < 4; j++) {
          const int at = 4 * w + j - P0.enc_pad;
          uint32_t c = at >= 0 && at < P0.d ? T.gen[at] : 0;
          for (int b = 0; b < 8; b++, c = gf256::xtime(c))
            if (((T.gen_shifted[b][w] >> (8 * j)) & 0xFF) != c) { fprintf(stderr, "(%zu, %zu): shifted form %d word %d\n", n, k, b, w); return 1; }
        }
      printf("K %d %d %d %d %d %d %d %d %d %d %d %d %d ", P0.n, P0.k, P0.d, P0.t, P0.form, P0.enc_lanes, P0.enc_pw, P0.enc_pad, P0.dec_w, P0.dec_spl, P0.dec_ppl, P0.dec_npad,
             P0.dec_dpad);
      hex(T.gen, P0.d + 1);
      printf("\n");
      for (size_t batch : batches) {
        const RsPlan P = rs_plan(n, k, batch);
        if (P.err != MZK_OK || P.form != P0.form || P.enc_pw != P0.enc_pw || P.dec_w != P0.dec_w) { fprintf(stderr, "(%zu, %zu, %zu): plan depends on the batch\n", n, k, batch); return 1; }
        printf("B %zu", batch);
        print_launch(P.enc);
        print_launch(P.syn);
        print_launch(P.dec);
        printf("\n");
      }
      codes++;
    }
  }
  const size_t refused[][3] = {{256, 8, 1}, {256, 256, 1}, {16, 0, 1}, {0, 0, 1}, {8, 9, 1}, {1000, 1000, 5}, {16, 8, 0}, {16, 8, ((size_t)1 << 31) + 1}, {255, 1, (size_t)1 << 40}};
  for (const auto& r : refused) {
    const RsPlan P = rs_plan(r[0], r[1], r[2]);
    printf("R %zu %zu %zu %d %s\n", r[0], r[1], r[2], P.err, P.msg);
  }
  printf("ok %zu\n", codes);
  return 0;
}
