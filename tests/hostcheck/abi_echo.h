/* A six-function C ABI in the style of include/mzk.h that hands its arguments back: tests/test_abi_bind.py reads this header with
 * myzkp_amd/_abi.py, binds the library built from abi_echo.cpp and sends values through it that do not fit in 32 bits. */
#ifndef ABI_ECHO_H
#define ABI_ECHO_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

size_t mzk_echo_usize(size_t v);
int mzk_echo_u64(uint64_t v, uint64_t* out);
int mzk_echo_ptr(const void* p, size_t* out);
void* mzk_echo_handle(void* h);
const char* mzk_echo_name(int which);
/* out = { a, b, c, d, (uint64_t)p } */
int mzk_echo_mixed(int a, size_t b, unsigned c, uint64_t d, void* p, uint64_t out[5]);

#ifdef __cplusplus
}
#endif
#endif
