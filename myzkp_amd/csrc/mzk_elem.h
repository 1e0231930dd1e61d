// mzk_elem.h -- the packed field element at its two boundaries.  A packed element is P::NW canonical little-endian 32-bit words
// (8 for Fr / Fq, 4 for M128).  Global memory <-> registers: fe_gload / fe_gstore (128-bit accesses, so g + idx * NW is 16-byte
// aligned).  Host scalar -> kernel argument: Words8 by value, filled by h_words / h_mont_words (mzk_common.h).
// HIP only (uint4): mzk_field.h stays compilable by a plain host compiler.
#pragma once
#include <hip/hip_runtime.h>
#include "mzk_field.h"

namespace mzk {

struct Words8 { u32 w[8]; };     // one packed element by value (M128 reads w[0..4), the rest is zero)
struct Words16 { u32 w[16]; };   // one packed affine point by value

// the packed words only: a loop that issues the loads of ALL its elements first and unpacks afterwards keeps several requests in flight
template <int NW> __device__ __forceinline__ void gload_words(const u32* __restrict__ g, size_t idx, u32 (&w)[NW]) {
  const uint4* p4 = reinterpret_cast<const uint4*>(g + idx * NW);
#pragma unroll
  for (int q = 0; q < NW / 4; q++) {
    uint4 v = p4[q];
    w[4 * q] = v.x; w[4 * q + 1] = v.y; w[4 * q + 2] = v.z; w[4 * q + 3] = v.w;
  }
}
template <int NW> __device__ __forceinline__ void gstore_words(u32* __restrict__ g, size_t idx, const u32 (&w)[NW]) {
  uint4* p4 = reinterpret_cast<uint4*>(g + idx * NW);
#pragma unroll
  for (int q = 0; q < NW / 4; q++) p4[q] = make_uint4(w[4 * q], w[4 * q + 1], w[4 * q + 2], w[4 * q + 3]);
}
// the fixed 8-word pair at a pointer (a coordinate inside a packed point: the caller's word array is wider than 8)
__device__ __forceinline__ void load_words8(const u32* __restrict__ g, u32* w) {
  const uint4* p4 = reinterpret_cast<const uint4*>(g);
  uint4 a = p4[0], b = p4[1];
  w[0] = a.x; w[1] = a.y; w[2] = a.z; w[3] = a.w; w[4] = b.x; w[5] = b.y; w[6] = b.z; w[7] = b.w;
}
__device__ __forceinline__ void store_words8(u32* __restrict__ g, const u32* w) {
  uint4* p4 = reinterpret_cast<uint4*>(g);
  p4[0] = make_uint4(w[0], w[1], w[2], w[3]);
  p4[1] = make_uint4(w[4], w[5], w[6], w[7]);
}

template <class P> __device__ __forceinline__ Fe<P> fe_gload(const u32* __restrict__ g, size_t idx) {
  u32 w[P::NW];
  gload_words<P::NW>(g, idx, w);
  return fe_unpack<P>(w);
}
template <class P> __device__ __forceinline__ void fe_gstore(u32* __restrict__ g, size_t idx, const Fe<P>& v) {   // v canonical
  u32 w[P::NW];
  fe_pack<P>(v, w);
  gstore_words<P::NW>(g, idx, w);
}

}  // namespace mzk
