// mzk_gl.h (the Goldilocks arithmetic the HIP kernels execute) compiled for the host: one C entry point per group of operations,
// called from tests/test_hostcheck_goldilocks.py and checked there against Python integers.
#include "../../myzkp_amd/csrc/mzk_gl.h"
#include <string.h>

using namespace mzk;

extern "C" {

// base: 0 add, 1 sub, 2 neg, 3 mul, 4 sqr, 5 pow (b = exponent), 6 inv, 7 reduce128 (a = lo, b = hi)
int gl_base_op(int op, uint64_t a, uint64_t b, uint64_t* out) {
  switch (op) {
    case 0: *out = gl::add(a, b); return 0;
    case 1: *out = gl::sub(a, b); return 0;
    case 2: *out = gl::neg(a); return 0;
    case 3: *out = gl::mul(a, b); return 0;
    case 4: *out = gl::sqr(a); return 0;
    case 5: *out = gl::pow(a, b); return 0;
    case 6: *out = gl::inv(a); return 0;
    case 7: *out = gl::reduce128(a, b); return 0;
    default: return -1;
  }
}
// extension: 0 add, 1 sub, 2 neg, 3 mul, 4 scale by the base value b[0]; 5 .. 8 the same add / sub / scale / mul through the
// El<3> forms the kernels use
int gl_ext_op(int op, const uint64_t* a, const uint64_t* b, uint64_t* out) {
  const gl::Ext x = gl::ext_make(a[0], a[1], a[2]), y = gl::ext_make(b[0], b[1], b[2]);
  gl::El<3> ex, ey;
  memcpy(ex.c, a, 24); memcpy(ey.c, b, 24);
  gl::Ext r;
  gl::El<3> e;
  switch (op) {
    case 0: r = gl::ext_add(x, y); break;
    case 1: r = gl::ext_sub(x, y); break;
    case 2: r = gl::ext_neg(x); break;
    case 3: r = gl::ext_mul(x, y); break;
    case 4: r = gl::ext_scale(x, b[0]); break;
    case 5: e = gl::el_add<3>(ex, ey); memcpy(out, e.c, 24); return 0;
    case 6: e = gl::el_sub<3>(ex, ey); memcpy(out, e.c, 24); return 0;
    case 7: e = gl::el_scale<3>(ex, b[0]); memcpy(out, e.c, 24); return 0;
    case 8: e = gl::el_mul(ex, ey); memcpy(out, e.c, 24); return 0;
    default: return -1;
  }
  memcpy(out, r.c, 24);
  return 0;
}
// leaf bytes of one element of nc coefficients; returns the length
int gl_leaf(int nc, const uint64_t* c, uint8_t* out) {
  auto put = [&](int pos, uint32_t byte) { out[pos] = (uint8_t)byte; };
  return nc == 3 ? gl::leaf_bytes<3>(c, 0, put) : gl::leaf_bytes<1>(c, 0, put);
}

}  // extern "C"
