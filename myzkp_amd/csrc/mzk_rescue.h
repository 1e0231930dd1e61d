// mzk_rescue.h -- one Rescue-Prime hash chain (zkstark/rescueprime.rs:401-452, :521-591) as the work of ONE lane: plain C++ over
// Fe<P>, so that a host compiler builds the same text with the portable products (tests/hostcheck/rescue_shim.cpp) and hipcc with the
// hand-scheduled ones (FeAsm<P>, mzk_field_asm.h).  The programs, the MDS matrix and the round constants (RescueConsts: one block of
// 32-bit words, mzk_rescue_plan.h) are the same for every lane and are read at wave-uniform addresses.
//
// Values: the state is kept in Montgomery form, canonical after every half-round (fe_reduce), so every product sees normalised
// limbs; the constants are Montgomery form; what leaves (trace rows, outputs) is changed back by a product with 1 and reduced.
// Registers: the m power chains of a half-round run one after another through ONE slot table (four slots), and every loop over the
// state is written as "work on element 0, then rotate" -- the state is only ever indexed by constants, so it stays in registers, and
// the chain interpreter exists once in the kernel whatever m is.
#pragma once
#include "mzk_field.h"
#include "mzk_field_asm.h"
#include "mzk_rescue_plan.h"

namespace mzk {

#if defined(__HIP_DEVICE_COMPILE__)
#define MZK_RS_UNIFORM(x) __builtin_amdgcn_readfirstlane(x)
#else
#define MZK_RS_UNIFORM(x) (x)
#endif

// offsets in words into `words`
struct RescueConsts {
  const u32* words;
  u32 prog[2], steps[2];           // alpha, alphainv
  u32 mds, rc;
  u32 n_rounds;
};

template <class P> MZK_HD Fe<P> rs_uload(const u32* w, u32 off) {
  const u32* at = w + (size_t)off;      // one base: the limbs are at constant offsets from it
  Fe<P> r;
#pragma unroll
  for (int i = 0; i < P::L; i++) r.l[i] = MZK_RS_UNIFORM(at[i]);
  return r;
}

template <class P> struct RsTable { Fe<P> s0, s1, s2, s3; };      // x, x^3, x^5, x^7
// j is wave-uniform: a select between registers, never an indexed array
template <class P> MZK_HD Fe<P> rs_pick(const RsTable<P>& t, u32 j) {
  Fe<P> r = t.s0;
  if (j == 1) r = t.s1;
  else if (j == 2) r = t.s2;
  else if (j == 3) r = t.s3;
  return r;
}

// x^e by program `half` (0: alpha, 1: alphainv); x in Montgomery form with normalised limbs
template <class P> MZK_HD Fe<P> rs_pow(const RescueConsts& c, u32 half, const Fe<P>& x) {
  RsTable<P> t;
  t.s0 = x; t.s1 = x; t.s2 = x; t.s3 = x;
  Fe<P> acc = x;
  const u32 p0 = c.prog[half], p1 = p0 + c.steps[half];
#pragma unroll 1
  for (u32 pc = p0; pc < p1; pc++) {
    const u32 w = MZK_RS_UNIFORM(c.words[pc]);
    const u32 op = w & 0xffu, arg = w >> 8;
    if (op == RS_OP_SQR) {
#pragma unroll 1
      for (u32 k = 0; k < arg; k++) acc = FeAsm<P>::sqr(acc);
    } else if (op == RS_OP_MUL) {
      acc = FeAsm<P>::mul(acc, rs_pick<P>(t, arg));
    } else if (op == RS_OP_LOAD) {
      acc = rs_pick<P>(t, arg);
    } else if (op == RS_OP_TABLE) {
      const Fe<P> x2 = FeAsm<P>::sqr(x);
      t.s1 = FeAsm<P>::mul(x, x2);
      if (arg >= 2) t.s2 = FeAsm<P>::mul(t.s1, x2);
      if (arg >= 3) t.s3 = FeAsm<P>::mul(t.s2, x2);
    } else {
      acc = fe_one<P>();
    }
  }
  return acc;
}

template <class P, int M> MZK_HD void rs_rotate(Fe<P> (&s)[M], const Fe<P> last) {      // by value: `last` may be s[0]
#pragma unroll
  for (int i = 0; i + 1 < M; i++) s[i] = s[i + 1];
  s[M - 1] = last;
}

// row i of mds * s + round constant rc_index, canonical
// (s is rotated all the way round in the one-product form, so that one matrix element is live at a time: nine scalar registers for Fr)
template <class P, int M> MZK_HD Fe<P> rs_mds_row(const RescueConsts& c, u32 i, u32 rc_index, Fe<P> (&s)[M]) {
  constexpr u32 L = (u32)P::L;
  const u32 base = c.mds + i * (u32)M * L;
  Fe<P> acc = rs_uload<P>(c.words, c.rc + rc_index * L);
  if constexpr (SparseMod<P>::value && M % 2 == 0) {
    acc = fe_add<P>(acc, FeAsm<P>::mul_add2(s[0], rs_uload<P>(c.words, base), s[1], rs_uload<P>(c.words, base + L)));
    if constexpr (M == 4) acc = fe_add<P>(acc, FeAsm<P>::mul_add2(s[2], rs_uload<P>(c.words, base + 2 * L), s[3], rs_uload<P>(c.words, base + 3 * L)));
  } else {
#pragma unroll 1
    for (u32 j = 0; j < (u32)M; j++) {
      acc = fe_add<P>(acc, FeAsm<P>::mul(s[0], rs_uload<P>(c.words, base + j * L)));
      rs_rotate<P, M>(s, s[0]);
    }
  }
  return fe_reduce<P>(acc);
}

template <class P> MZK_HD Fe<P> rs_from_mont(const Fe<P>& v) {
  Fe<P> one = fe_zero<P>();
  one.l[0] = 1;
  return fe_reduce<P>(FeAsm<P>::mul(v, one));
}

// A chain of `links` hashes from the canonical plain x.  out.row(link, row, element, value) receives every trace element (TRACE only),
// out.output(link, value) every link's output; values canonical and plain.
template <class P, int M, bool TRACE, class Out> MZK_HD void rs_chain(const RescueConsts& c, const Fe<P>& x, size_t links, Out& out) {
  Fe<P> st[M], nw[M];
  Fe<P> cur = x;
  st[0] = fe_reduce<P>(FeAsm<P>::mul(x, fe_r2<P>()));
#pragma unroll
  for (int i = 1; i < M; i++) st[i] = fe_zero<P>();
#pragma unroll
  for (int i = 0; i < M; i++) nw[i] = fe_zero<P>();
#pragma unroll 1
  for (size_t l = 0; l < links; l++) {
    if (TRACE) {
      out.row(l, 0, 0, cur);
#pragma unroll
      for (int i = 1; i < M; i++) out.row(l, 0, (u32)i, fe_zero<P>());
    }
#pragma unroll 1
    for (u32 r = 0; r < c.n_rounds; r++) {
#pragma unroll 1
      for (u32 half = 0; half < 2; half++) {
#pragma unroll 1
        for (u32 i = 0; i < (u32)M; i++) rs_rotate<P, M>(st, rs_pow<P>(c, half, st[0]));
#pragma unroll 1
        for (u32 i = 0; i < (u32)M; i++) rs_rotate<P, M>(nw, rs_mds_row<P, M>(c, i, (2 * r + half) * (u32)M + i, st));
#pragma unroll
        for (int i = 0; i < M; i++) st[i] = nw[i];
      }
      if (TRACE) {
#pragma unroll 1
        for (u32 i = 0; i < (u32)M; i++) {
          const Fe<P> v = rs_from_mont<P>(st[0]);
          out.row(l, r + 1, i, v);
          if (i == 0) cur = v;
          rs_rotate<P, M>(st, st[0]);
        }
      }
    }
    if (!TRACE) cur = rs_from_mont<P>(st[0]);
    out.output(l, cur);
    // the next link absorbs the output: state[0] is its Montgomery form already
#pragma unroll
    for (int i = 1; i < M; i++) st[i] = fe_zero<P>();
  }
}

}  // namespace mzk
