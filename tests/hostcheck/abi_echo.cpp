#include "abi_echo.h"

size_t mzk_echo_usize(size_t v) { return v; }

int mzk_echo_u64(uint64_t v, uint64_t* out) {
  *out = v;
  return 0;
}

int mzk_echo_ptr(const void* p, size_t* out) {
  *out = (size_t)p;
  return 0;
}

void* mzk_echo_handle(void* h) { return h; }

const char* mzk_echo_name(int which) { return which ? "one" : "zero"; }

int mzk_echo_mixed(int a, size_t b, unsigned c, uint64_t d, void* p, uint64_t out[5]) {
  out[0] = (uint64_t)(int64_t)a;
  out[1] = b;
  out[2] = c;
  out[3] = d;
  out[4] = (uint64_t)p;
  return a;
}
