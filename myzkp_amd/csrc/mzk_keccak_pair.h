// mzk_keccak_pair.h -- Keccak-f[1600] on a pair of lanes and SHAKE256 over a byte stream on top of it, shared by the translation
// units that hash on a nearly empty GPU: the upper levels of a Merkle tree (mzk_merkle.hip), the proof stream of FRI::prove
// (mzk_fri.hip), the proof stream of the product sum-check (mzk_sumcheck.hip).  Device code only; the library is built without relocatable device code,
// so every user compiles its own copy.
#pragma once
#include "mzk_field.h"
#include "mzk_keccak_asm.h"
#include "mzk_transcript.h"

namespace mzk {

typedef uint8_t u8;

// ---- Keccak-f[1600] (FIPS 202 section 3.2/3.3; mzk_merkle.hip has the one-lane form) on a PAIR of lanes ---------------------
// The upper levels of a tree are a few hundred hashes at most: one hash per lane leaves the GPU empty and the level's
// time is the instruction latency of one permutation (24 x 190 dependent-issue instructions).  Here the even lane of a
// pair holds the low halves of the 25 lanes of the state and the odd lane the high halves; xors and chi are local, and
// a rotation needs the partner's half of the same word: one quad_perm DPP move + one v_alignbit_b32, the same formula
// on both lanes.  ~125 instructions per round and lane instead of 190 (1.3 x the total work: only used where the level
// is latency-bound).  Both lanes of a pair must be active (a DPP read of a disabled lane returns 0).
__device__ __forceinline__ void keccak_f_pair(u32 (&a)[25], int parity) {
  // One scheduled asm block per round (mzk_keccak_asm.h, generated): hipcc emitted the round word by word -- xor, s_nop 1,
  // v_mov_b32_dpp, s_nop 0, v_alignbit: 49 wait-state instructions per round, 7.6 cycles per instruction on the lone wave of a
  // tree's upper levels; batched (all xors, all lane exchanges, all funnel shifts) every hazard distance is covered by independent work.
  // Where the round constant comes from (same-box A/B, profiles/round6_keccak_round_constant_ab.txt; FRI round at 2^14 / Merkle commit of 2^16 leaves):
  //   `KECCAK_RC[rnd]` inside its round: s_getpc + address arithmetic + s_load_dwordx2 + s_waitcnt in front of EVERY round of the lone wave
  //      of a tree's upper levels -- a fifth of the round                                                             114 - 116 us / 0.153 ms
  //   the constant of round r + 1 fetched while round r runs (the wait finds it there)                              106 - 108 us / 0.147 ms
  //   all 24 rounds unrolled, the constants literals of the instruction stream (49 KB of code in k_merkle_tail)     104 - 105 us / 0.139 ms
  // The last is the form here: no scalar load, no address arithmetic per round.
  constexpr u64 K[24] = {
      0x0000000000000001ULL, 0x0000000000008082ULL, 0x800000000000808aULL, 0x8000000080008000ULL, 0x000000000000808bULL, 0x0000000080000001ULL,
      0x8000000080008081ULL, 0x8000000000008009ULL, 0x000000000000008aULL, 0x0000000000000088ULL, 0x0000000080008009ULL, 0x000000008000000aULL,
      0x000000008000808bULL, 0x800000000000008bULL, 0x8000000000008089ULL, 0x8000000000008003ULL, 0x8000000000008002ULL, 0x8000000000000080ULL,
      0x000000000000800aULL, 0x800000008000000aULL, 0x8000000080008081ULL, 0x8000000000008080ULL, 0x0000000080000001ULL, 0x8000000080008008ULL};
#pragma unroll
  for (int rnd = 0; rnd < 24; rnd++) keccak_round_pair_asm(a, parity ? (u32)(K[rnd] >> 32) : (u32)K[rnd]);
}
// SHAKE256(msg[0 .. len))[0 .. 32) by the lane pair (lane & 1 = parity) of the calling lanes 0 / 1; out_w32[2 i + parity] = the
// parity half of digest word i.  msg: 8-byte aligned, readable to the next multiple of 8.
__device__ inline void fri_shake256_pair(const u8* msg, size_t len, int parity, u32* out_w32) {
  u32 a[25];
#pragma unroll
  for (int i = 0; i < 25; i++) a[i] = 0;
  const size_t blocks = mzk_tx::shake_blocks(len);
  for (size_t b = 0; b < blocks; b++) {
#pragma unroll
    for (int w = 0; w < mzk_tx::SHAKE_RATE / 8; w++) {
      const u64 v = mzk_tx::shake_word(msg, len, b, w);
      a[w] ^= parity ? (u32)(v >> 32) : (u32)v;
    }
    keccak_f_pair(a, parity);
  }
#pragma unroll
  for (int i = 0; i < 4; i++) out_w32[2 * i + parity] = a[i];
}

}  // namespace mzk
