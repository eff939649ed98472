// Nearest neighbours on an f16 gallery (extension, ore_nearest_f16 and ore_gallery_f16): the k best
// of s[i, j] = sum_d RNE_f16(q[i, d]) g[j, d] per query row, products exact in f32, accumulated in f32 by
// v_mfma_f32_16x16x32_f16, under ore_topk_f32's order (ore_topk_key.h) -- and the packer that makes the gallery.
// The kernel is ore_nearest.h's streaming kernel over the format below; split, data movement and selection are
// described there.
//
// The format.  A k-group is 32 d, a lane's operand eight halves.  The query tile is rounded to f16 once per workgroup:
// 64 rows of D halves at a pitch of 8 halves more (16 m + 4 dwords between rows).  It is resident up to D = 512;
// above that it is staged in chunks of 512 d.  A gallery element that is not there becomes +0 on its bits, so a NaN or
// an inf that is masked never meets a multiplication; a padded product is +0 and leaves the accumulator, which
// starts at +0 and is never -0, unchanged.  The MFMA takes d = 32 kg + 8 (l >> 4) + e from lane l.
#include <algorithm>

#include "ore_nearest.h"
#include "ore_nearest_bins.h"

namespace ore {

namespace {

typedef _Float16 halfx4 __attribute__((ext_vector_type(4)));
typedef _Float16 halfx8 __attribute__((ext_vector_type(8)));

struct FmtF16 {
  typedef _Float16 elem;
  typedef halfx8 opnd;
  typedef floatx4 accum;
  static constexpr int KG = 32, DRES = 512, DC = 512, PAD = 8, QX = 0;
  static constexpr bool SCALES = false;

  // The gallery loads sit in the K loop, far ahead of their use, so they are masked without a branch: an element that
  // is not there is read from `safe` instead (the gallery's first element, or its first eight: always there), and
  // mask makes it +0 when the operand is consumed.
  template <bool VEC>
  static __device__ __forceinline__ halfx8 load(bool row_ok, const _Float16* __restrict__ row, int d, int D,
                                                const _Float16* __restrict__ safe) {
    halfx8 v;
    if (VEC) {  // D % 8 == 0: the group is inside the row or outside it
      v = *reinterpret_cast<const halfx8*>(row_ok && d < D ? row + d : safe);
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = *(row_ok && d + e < D ? row + d + e : safe);
    }
    return v;
  }

  template <bool VEC>
  static __device__ __forceinline__ halfx8 mask(halfx8 v, bool row_ok, int d, int D) {
    typedef unsigned uintx4 __attribute__((ext_vector_type(4)));
    if (VEC) {
      const unsigned m = row_ok && d < D ? ~0u : 0u;  // on the bits: a NaN or an inf that is masked becomes +0 too
      return __builtin_bit_cast(halfx8, __builtin_bit_cast(uintx4, v) & uintx4{m, m, m, m});
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = row_ok && d + e < D ? v[e] : (_Float16)0.0f;
    return v;
  }

  template <bool VQ>
  static __device__ __forceinline__ void prologue(const float*, long long, int, int, long long, int, int, float*, float*) {}

  static __device__ __forceinline__ void stage4(_Float16* dst, floatx4 v, float) {
    *reinterpret_cast<halfx4*>(dst) = halfx4{(_Float16)v[0], (_Float16)v[1], (_Float16)v[2], (_Float16)v[3]};
  }

  static __device__ __forceinline__ floatx4 mfma(halfx8 a, halfx8 b, floatx4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
  }

  static __device__ __forceinline__ float score(float acc) { return acc; }
};
static_assert(ns_lds_bytes<FmtF16>(FmtF16::DRES, 64) <= 160 * 1024 &&
              ns_lds_bytes<FmtF16>(FmtF16::DRES + 1, 64) <= ns_lds_bytes<FmtF16>(FmtF16::DRES, 64), "LDS");

// f32 -> f16, round to nearest even, no clamp.  VEC (D % 8 == 0, both bases 16-byte aligned): a thread takes eight
// elements, two 16-byte loads and one 16-byte store; otherwise one element
template <bool VEC>
__global__ __launch_bounds__(256) void gallery_f16_kernel(const float* __restrict__ src, _Float16* __restrict__ dst, long long total) {
  const long long t0 = (long long)blockIdx.x * 256 + threadIdx.x, stride = (long long)gridDim.x * 256;
  if (VEC) {
    for (long long i = 8 * t0; i < total; i += 8 * stride) {
      const floatx4 a = *reinterpret_cast<const floatx4*>(src + i), b = *reinterpret_cast<const floatx4*>(src + i + 4);
      *reinterpret_cast<halfx8*>(dst + i) = halfx8{(_Float16)a[0], (_Float16)a[1], (_Float16)a[2], (_Float16)a[3],
                                                   (_Float16)b[0], (_Float16)b[1], (_Float16)b[2], (_Float16)b[3]};
    }
  } else {
    for (long long i = t0; i < total; i += stride) dst[i] = (_Float16)src[i];
  }
}

}  // namespace

void launch_gallery_f16(const float* src, long long G, long long D, void* dst, hipStream_t s) {
  const long long total = G * D;
  const bool vec = D % 8 == 0 && ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 15) == 0;
  const dim3 grid((unsigned)std::min<long long>(((vec ? total / 8 : total) + 255) / 256, 1 << 16));
  if (vec) hipLaunchKernelGGL(gallery_f16_kernel<true>, grid, dim3(256), 0, s, src, static_cast<_Float16*>(dst), total);
  else hipLaunchKernelGGL(gallery_f16_kernel<false>, grid, dim3(256), 0, s, src, static_cast<_Float16*>(dst), total);
}

void launch_nearest_f16(const float* q, long long q_stride, int n, int D, const void* gallery, const float* scales, long long G,
                        int k, int S, void* part, float* values, int* indices, hipStream_t s) {
  nearest_launch<NearestStream<FmtF16>>(q, q_stride, n, D, gallery, scales, G, k, S, part, values, indices, s);
}

// ore_nearest_bins.h's kernel over the same format: 64 rows of 520 halves twice on a compute unit
void launch_nearest_bins_f16(const float* q, long long q_stride, int n, int D, const void* gallery, const float* scales, long long G,
                             int bin_rows, int S, void* win, hipStream_t s) {
  nearest_bins_launch<FmtF16, 512>(q, q_stride, n, D, gallery, scales, G, bin_rows, S, win, s);
}

}  // namespace ore
