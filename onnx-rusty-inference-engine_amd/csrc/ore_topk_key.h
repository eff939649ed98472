// The selection order of the top-k kernels as a 64-bit key, and the wave-wide rounds that pick by it: shared by
// ore_topk.hip (rows of a matrix) and ore_nearest.hip (scores that are never stored).  Device code only.
//
// Element i of value x becomes  hi:lo = image(x) : ~i  where image() is the order-preserving unsigned image of
// the float (sign bit set for x >= 0, all bits flipped for x < 0) after folding -0.0 to +0.0, and 0 for a NaN.
// -inf maps to 0x007fffff, so every number's image is above a NaN's; ~i puts the lower index first among equal
// images.  Keys are unique and never 0 (i < 2^31), so 0 is the empty slot, and round j's winner is "the largest
// key strictly below round j - 1's".
#pragma once
#include <hip/hip_runtime.h>

namespace ore {
namespace {

typedef unsigned long long u64;

__device__ __forceinline__ u64 topk_key(unsigned bits, int i) {
  unsigned hi;
  if ((bits & 0x7fffffffu) > 0x7f800000u) {
    hi = 0u;  // NaN of either sign
  } else {
    if (bits == 0x80000000u) bits = 0u;  // -0.0 ties with +0.0
    hi = (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u);
  }
  return (u64(hi) << 32) | u64(~unsigned(i));
}

// the index of a key, and the bits of its value: every number but -0.0 exactly as it went in (-0.0 comes back
// as +0.0), a NaN as the quiet NaN 0x7fc00000
__device__ __forceinline__ int topk_key_index(u64 key) { return int(~unsigned(key)); }
__device__ __forceinline__ unsigned topk_key_bits(u64 key) {
  const unsigned hi = unsigned(key >> 32);
  if (hi == 0u) return 0x7fc00000u;
  return (hi & 0x80000000u) ? (hi & 0x7fffffffu) : ~hi;
}

// The max of v over the wave, in every lane, without the LDS crossbar: six exchange steps in the VALU, each
// moving the two halves of the key and keeping the larger key.  Within a row of 16 lanes by DPP: lane ^ 1
// and lane ^ 2 (quad_perm), then the mirrored half row and the mirrored row (after the quad steps a quad
// holds one value, so a mirror pairs groups as an xor would).  Across rows by the gfx950 swaps of v with
// itself: v_permlane16_swap leaves rows (0,0,2,2) in one result and (1,1,3,3) in the other,
// v_permlane32_swap the lower half twice and the upper half twice.  The wave is fully active here.
template <int CTRL>
__device__ __forceinline__ u64 dpp_max(u64 v) {
  const unsigned lo = unsigned(__builtin_amdgcn_update_dpp(0, int(unsigned(v)), CTRL, 0xf, 0xf, false));
  const unsigned hi = unsigned(__builtin_amdgcn_update_dpp(0, int(unsigned(v >> 32)), CTRL, 0xf, 0xf, false));
  const u64 o = (u64(hi) << 32) | lo;
  return o > v ? o : v;
}

__device__ __forceinline__ u64 wave_max(u64 v) {
  v = dpp_max<0xb1>(v);   // quad_perm [1,0,3,2]
  v = dpp_max<0x4e>(v);   // quad_perm [2,3,0,1]
  v = dpp_max<0x141>(v);  // row_half_mirror
  v = dpp_max<0x140>(v);  // row_mirror
  const unsigned lo = unsigned(v), hi = unsigned(v >> 32);
  auto l16 = __builtin_amdgcn_permlane16_swap(lo, lo, false, false);
  auto h16 = __builtin_amdgcn_permlane16_swap(hi, hi, false, false);
  const u64 a = (u64(h16[0]) << 32) | l16[0], b = (u64(h16[1]) << 32) | l16[1];
  v = a > b ? a : b;
  auto l32 = __builtin_amdgcn_permlane32_swap(unsigned(v), unsigned(v), false, false);
  auto h32 = __builtin_amdgcn_permlane32_swap(unsigned(v >> 32), unsigned(v >> 32), false, false);
  const u64 c = (u64(h32[0]) << 32) | l32[0], d = (u64(h32[1]) << 32) | l32[1];
  return c > d ? c : d;
}

// the k rounds over keys held in registers; returns lane j's key of round j
template <int NE>
__device__ __forceinline__ u64 topk_rounds(const u64 (&key)[NE], int k, int lane) {
  u64 prev = ~0ull, mine = 0ull;
  for (int j = 0; j < k; ++j) {  // wave-uniform trip count
    u64 best = 0ull;
#pragma unroll
    for (int t = 0; t < NE; ++t) {
      const u64 c = key[t] < prev ? key[t] : 0ull;
      best = c > best ? c : best;
    }
    prev = wave_max(best);
    mine = lane == j ? prev : mine;
  }
  return mine;
}

}  // namespace
}  // namespace ore
