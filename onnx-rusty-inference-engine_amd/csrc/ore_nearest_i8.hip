// Nearest neighbours on an int8 gallery with one scale per row (extension, ore_nearest_i8 and ore_gallery_i8;
// DESIGN.md 3.13c): the k best of s[i, j] = fmul(fmul((float)dot, tq[i]), tg[j]), dot = sum_d cq[i, d] cg[j, d] an
// exact int32 sum of v_mfma_i32_16x16x64_i8, cq and tq the query row quantised by include/ore.h's rule inside the
// kernel, under ore_topk_f32's order (ore_topk_key.h) -- and the packer that makes codes and scales by the same rule.
// The kernel is ore_nearest.h's streaming kernel over the format below; split, gallery ring, the place of the scale
// loads and selection are described there.
//
// The format.  A k-group is 64 d, a lane's operand sixteen codes, the accumulators int32.
//
// Queries.  Before the first step a wave takes the maximum |x| of each of its 16 rows over the whole row (NaNs
// skipped: fmaxf), lane-strided and reduced over the wave, and leaves t = a / 127 and 127 / a in LDS.  The codes are
// then written to LDS by the wave that took the maximum, four d per lane: 64 rows of D bytes, D rounded up to a whole
// turn of the ring (512), at a pitch of 16 bytes more (128 m + 4 dwords between rows).  Up to DRES = 1024 d the
// tile is resident for the segment; above it the tile is staged in chunks of 1024 d -- the scales are still those of
// the whole row.  Query rows past n and d past D enter LDS as code 0.  No int8 copy of q reaches memory.
//
// Gallery.  A byte that is not there is made 0 on its bits before the MFMA; the k-groups past D that fill the last
// turn multiply zero codes, which is exact.
//
// Position independence.  The dot product is exact, so the bits of s[i, j] depend on q[i, :], gallery[j, :] and
// tg[j] alone, whatever the order of the d, the load path, resident or chunked.
#include <algorithm>

// every product of the definition is rounded on its own: the format's arithmetic, the packer's and, instantiated
// here, the streaming kernel's
#pragma clang fp contract(off)

#include "ore_nearest.h"
#include "ore_nearest_bins.h"

namespace ore {

namespace {

typedef int intx4 __attribute__((ext_vector_type(4)));
typedef unsigned uintx4 __attribute__((ext_vector_type(4)));

constexpr int NI_DMAX = 131072;  // 127 * 128 * D < 2^31
static_assert(127LL * 128 * NI_DMAX < (1LL << 31), "the dot product stays in int32");

// the maximum over the wave, in every lane
__device__ __forceinline__ float ni_wave_fmax(float a) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) a = fmaxf(a, __shfl_xor(a, m));
  return a;
}

// one code of include/ore.h's rule: x inv rounded on its own, clamped, ties to even; a NaN quotient is 0
__device__ __forceinline__ unsigned ni_code(float x, float inv) {
  const float r = x * inv;
  const int c = r != r ? 0 : int(__builtin_rintf(fminf(fmaxf(r, -127.0f), 127.0f)));
  return unsigned(c) & 0xffu;
}
__device__ __forceinline__ unsigned ni_code4(floatx4 v, float inv) {
  return ni_code(v[0], inv) | ni_code(v[1], inv) << 8 | ni_code(v[2], inv) << 16 | ni_code(v[3], inv) << 24;
}

struct FmtI8 {
  typedef signed char elem;
  typedef intx4 opnd;
  typedef intx4 accum;
  static constexpr int KG = 64, DRES = 1024, DC = 1024, PAD = 16, QX = 8;
  static constexpr bool SCALES = true;

  // The gallery loads sit in the K loop, far ahead of their use, so they are masked without a branch: a byte that is
  // not there is read from `safe` instead (the gallery's first byte, or its first sixteen: always there), and mask
  // makes it 0 when the operand is consumed.
  template <bool VEC>
  static __device__ __forceinline__ intx4 load(bool row_ok, const signed char* __restrict__ row, int d, int D,
                                               const signed char* __restrict__ safe) {
    if (VEC)  // D % 16 == 0: the group is inside the row or outside it
      return *reinterpret_cast<const intx4*>(row_ok && d < D ? row + d : safe);
    intx4 v;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      unsigned x = 0u;
#pragma unroll
      for (int b = 0; b < 4; ++b)
        x |= unsigned(static_cast<unsigned char>(*(row_ok && d + 4 * w + b < D ? row + d + 4 * w + b : safe))) << (8 * b);
      v[w] = int(x);
    }
    return v;
  }

  template <bool VEC>
  static __device__ __forceinline__ intx4 mask(intx4 v, bool row_ok, int d, int D) {
    if (VEC) {
      const unsigned m = row_ok && d < D ? ~0u : 0u;
      return __builtin_bit_cast(intx4, __builtin_bit_cast(uintx4, v) & uintx4{m, m, m, m});
    }
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const int left = row_ok ? D - (d + 4 * w) : 0;  // bytes of this dword that are there
      v[w] &= left >= 4 ? -1 : left <= 0 ? 0 : int((1u << (8 * left)) - 1u);
    }
    return v;
  }

  // the scales of the tile's rows: a wave per row, the maximum over the whole row, NaNs skipped
  template <bool VQ>
  static __device__ __forceinline__ void prologue(const float* q, long long q_stride, int n, int D, long long q0, int wave,
                                                  int lane, float* stq, float* sinv) {
    for (int r = wave; r < NN_QT; r += 4) {
      const long long qi = q0 + r;
      const float* const row = q + qi * q_stride;
      float a = 0.0f;
      for (int d = 4 * lane; d < D; d += 256) {
        const floatx4 v = nn_load4<VQ>(qi < n, row, d, D);
#pragma unroll
        for (int e = 0; e < 4; ++e) a = fmaxf(a, fabsf(v[e]));
      }
      a = ni_wave_fmax(a);
      if (lane == 0) {
        stq[r] = a / 127.0f;
        sinv[r] = 127.0f / a;
      }
    }
  }

  static __device__ __forceinline__ void stage4(signed char* dst, floatx4 v, float inv) {
    *reinterpret_cast<unsigned*>(dst) = ni_code4(v, inv);
  }

  static __device__ __forceinline__ intx4 mfma(intx4 a, intx4 b, intx4 c) {
    return __builtin_amdgcn_mfma_i32_16x16x64_i8(a, b, c, 0, 0, 0);
  }

  // two roundings, nothing to fuse them with
  static __device__ __forceinline__ float score(int acc, float tq, float tg) { return (float(acc) * tq) * tg; }
};
static_assert(ns_lds_bytes<FmtI8>(FmtI8::DRES, 64) <= 160 * 1024 &&
              ns_lds_bytes<FmtI8>(FmtI8::DRES + 1, 64) <= ns_lds_bytes<FmtI8>(FmtI8::DRES, 64), "LDS");
static_assert(ns_lds_bytes<FmtI8>(FmtI8::DRES, 64) + size_t(NN_QT) * FmtI8::KG * NS_PF > 160 * 1024,
              "a resident tile one turn longer does not fit");

// f32 rows -> codes and a scale per row by include/ore.h's rule: a wave per row, four rows per workgroup.  Pass 1 takes
// the row's maximum, pass 2 writes the codes (the row comes from the cache) and lane 0 the scale.  VEC (D % 4 == 0,
// src 16-byte and dst 4-byte aligned): a lane takes four elements, one 16-byte load and one packed store; otherwise one
template <bool VEC>
__global__ __launch_bounds__(256) void gallery_i8_kernel(const float* __restrict__ src, signed char* __restrict__ dst,
                                                         float* __restrict__ scales, long long G, long long D) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (long long r = 4LL * blockIdx.x + wave; r < G; r += 4LL * gridDim.x) {
    const float* const row = src + r * D;
    signed char* const out = dst + r * D;
    float a = 0.0f;
    if (VEC) {
      for (long long d = 4 * lane; d < D; d += 256) {
        const floatx4 v = *reinterpret_cast<const floatx4*>(row + d);
#pragma unroll
        for (int e = 0; e < 4; ++e) a = fmaxf(a, fabsf(v[e]));
      }
    } else {
      for (long long d = lane; d < D; d += 64) a = fmaxf(a, fabsf(row[d]));
    }
    a = ni_wave_fmax(a);
    const float inv = 127.0f / a;
    if (VEC) {
      for (long long d = 4 * lane; d < D; d += 256)
        *reinterpret_cast<unsigned*>(out + d) = ni_code4(*reinterpret_cast<const floatx4*>(row + d), inv);
    } else {
      for (long long d = lane; d < D; d += 64) out[d] = static_cast<signed char>(ni_code(row[d], inv));
    }
    if (lane == 0) scales[r] = a / 127.0f;
  }
}

}  // namespace

int nearest_i8_max_d() { return NI_DMAX; }

void launch_gallery_i8(const float* src, long long G, long long D, void* dst, float* scales, hipStream_t s) {
  const bool vec = D % 4 == 0 && (reinterpret_cast<uintptr_t>(src) & 15) == 0 && (reinterpret_cast<uintptr_t>(dst) & 3) == 0;
  const dim3 grid((unsigned)std::min<long long>((G + 3) / 4, 1 << 20));
  if (vec) hipLaunchKernelGGL(gallery_i8_kernel<true>, grid, dim3(256), 0, s, src, static_cast<signed char*>(dst), scales, G, D);
  else hipLaunchKernelGGL(gallery_i8_kernel<false>, grid, dim3(256), 0, s, src, static_cast<signed char*>(dst), scales, G, D);
}

void launch_nearest_i8(const float* q, long long q_stride, int n, int D, const void* gallery, const float* scales, long long G,
                       int k, int S, void* part, float* values, int* indices, hipStream_t s) {
  nearest_launch<NearestStream<FmtI8>>(q, q_stride, n, D, gallery, scales, G, k, S, part, values, indices, s);
}

// ore_nearest_bins.h's kernel over the same format: 64 rows of 1040 codes and the queries' scales twice on a compute unit
void launch_nearest_bins_i8(const float* q, long long q_stride, int n, int D, const void* gallery, const float* scales, long long G,
                            int bin_rows, int S, void* win, hipStream_t s) {
  nearest_bins_launch<FmtI8, 1024>(q, q_stride, n, D, gallery, scales, G, bin_rows, S, win, s);
}

}  // namespace ore
