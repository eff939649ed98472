// Input preprocessing (extension, ore_preprocess_u8 / ore_model_run_u8): uint8 NHWC image batches, as a
// decoder leaves them, to the float32 NCHW planes every model entry point consumes, in one launch:
//   y[i][c][h][w] = fadd_rn(fmul_rn(float(x[i][h][w][cs]), scale[c]), shift[c])
// The multiply and the add round separately (never an FMA), so the host reproduces the result bit for bit
// with (x.astype(float32) * scale) + shift.  The channel reversal is resolved on the host into the plane
// each source channel writes (PreprocParams::plane), so the kernels know only source channels.
//
// One pass over memory: 4 C bytes read and 16 C bytes written per 4 pixels, no LDS.
//  * preproc_u8_vec_kernel<C>: one thread per group of 4 consecutive pixels of one image.  It loads the
//    group's 4 C bytes as C dwords (C = 3: 12 bytes per lane, a wave reads 768 contiguous bytes), converts
//    each byte in registers and issues C float4 stores, one per plane (a wave writes 1 KiB contiguous per
//    plane).  Needs H W % 4 == 0, a 4-byte aligned x and 16-byte aligned planes (y and its image stride).
//  * preproc_u8_scalar_kernel: one thread per pixel, byte loads and float stores; any size and alignment.
// Image bases are 64-bit; offsets inside one image stay below 2^31 elements (checked by the caller).
#include <hip/hip_runtime.h>

#include "ore_kernels.h"

namespace ore {

namespace {

__device__ __forceinline__ float norm_rn(float v, float scale, float shift) {
#pragma clang fp contract(off)
  const float p = v * scale;
  return p + shift;
}

template <int C>
struct alignas(4) PixelGroup {
  unsigned w[C];  // 4 pixels x C channels, interleaved
};

// byte b (0 .. 4 C - 1) of a group: a compile-time word and shift after unrolling (v_cvt_f32_ubyte0..3)
template <int C>
__device__ __forceinline__ float group_byte(const PixelGroup<C>& g, int b) {
  return float((g.w[b >> 2] >> ((b & 3) * 8)) & 0xffu);
}

template <int C>
__global__ __launch_bounds__(256) void preproc_u8_vec_kernel(PreprocParams p) {
  const int q = blockIdx.x * 256 + threadIdx.x;  // pixel group inside the image
  if (q >= (p.HW >> 2)) return;
  for (long long i = blockIdx.y; i < p.N; i += gridDim.y) {
    const PixelGroup<C> g =
        reinterpret_cast<const PixelGroup<C>*>(p.x + size_t(i) * size_t(p.HW) * C)[q];
    float* yi = p.y + size_t(i) * size_t(p.y_nstride);
#pragma unroll
    for (int s = 0; s < C; ++s) {
      float4 v;
      v.x = norm_rn(group_byte<C>(g, s), p.scale[s], p.shift[s]);
      v.y = norm_rn(group_byte<C>(g, C + s), p.scale[s], p.shift[s]);
      v.z = norm_rn(group_byte<C>(g, 2 * C + s), p.scale[s], p.shift[s]);
      v.w = norm_rn(group_byte<C>(g, 3 * C + s), p.scale[s], p.shift[s]);
      reinterpret_cast<float4*>(yi + size_t(p.plane[s]) * size_t(p.HW))[q] = v;
    }
  }
}

__global__ __launch_bounds__(256) void preproc_u8_scalar_kernel(PreprocParams p) {
  const int px = blockIdx.x * 256 + threadIdx.x;
  if (px >= p.HW) return;
  for (long long i = blockIdx.y; i < p.N; i += gridDim.y) {
    const unsigned char* xi = p.x + size_t(i) * size_t(p.HW) * size_t(p.C) + size_t(px) * size_t(p.C);
    float* yi = p.y + size_t(i) * size_t(p.y_nstride) + px;
    for (int s = 0; s < p.C; ++s)
      yi[size_t(p.plane[s]) * size_t(p.HW)] = norm_rn(float(xi[s]), p.scale[s], p.shift[s]);
  }
}

// every image's bytes start on a dword and every plane on 16 bytes
bool vectorised(const PreprocParams& p) {
  return (p.HW & 3) == 0 && (reinterpret_cast<uintptr_t>(p.x) & 3) == 0 && (reinterpret_cast<uintptr_t>(p.y) & 15) == 0 &&
         (p.y_nstride & 3) == 0;
}

}  // namespace

void launch_preproc_u8(const PreprocParams& p, hipStream_t s) {
  if (p.N <= 0 || p.HW <= 0) return;
  const unsigned gy = unsigned(p.N < 65535 ? p.N : 65535);
  if (vectorised(p)) {
    const dim3 grid(unsigned(((p.HW >> 2) + 255) / 256), gy);
    switch (p.C) {
      case 1: hipLaunchKernelGGL(preproc_u8_vec_kernel<1>, grid, dim3(256), 0, s, p); break;
      case 2: hipLaunchKernelGGL(preproc_u8_vec_kernel<2>, grid, dim3(256), 0, s, p); break;
      case 3: hipLaunchKernelGGL(preproc_u8_vec_kernel<3>, grid, dim3(256), 0, s, p); break;
      default: hipLaunchKernelGGL(preproc_u8_vec_kernel<4>, grid, dim3(256), 0, s, p); break;
    }
  } else {
    hipLaunchKernelGGL(preproc_u8_scalar_kernel, dim3(unsigned((p.HW + 255) / 256), gy), dim3(256), 0, s, p);
  }
}

}  // namespace ore
