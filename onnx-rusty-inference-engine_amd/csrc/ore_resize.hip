// Resize + crop in front of the graph (extension, ore_preprocess_resize_u8 / ore_model_set_input_resize):
// uint8 NHWC images of any size to the float32 NCHW planes the model consumes, in the launch that converts
// and normalises.  Per output element, with a, b the bytes at (y0, x0), (y0, x1) and c, d at (y1, x0),
// (y1, x1) of the source channel, tx / ty the column / row weights (resize_tap, ore_resize_geom.h):
//     top = a + (b - a) tx;  bot = c + (d - c) tx;  v = top + (bot - top) ty;  y = v scale + shift
// Every operation rounds on its own (never an FMA), so numpy reproduces the result bit for bit.
//
// resize_u8_generic_kernel: one thread per output pixel, byte loads of the 2 x 2 x C taps from global memory,
// C float stores (a wave writes 256 contiguous bytes per plane).  Any size, alignment and y stride.  It is the
// only dense kernel (resize_u8_list_kernel below is the same arithmetic over an image list): an LDS-staged one (a workgroup staging a band's source rows with 16-byte loads, 4 pixels x C
// channels per thread, float4 stores) ran 2.0x faster at 375 x 500 -> 224 but lost at 1080 x 1920 -> 224,
// where this kernel already moves its bytes at the device-to-device copy rate, and was removed
// (DESIGN.md 3.8b has the numbers).
// Image bases are 64-bit; offsets inside one image stay below 2^31 (sizes <= RESIZE_MAX, C <= 4).
#include <hip/hip_runtime.h>

#include "ore_kernels.h"
#include "ore_resize_geom.h"

namespace ore {

namespace {

constexpr int RS_THREADS = 256;

__device__ __forceinline__ float lerp_rn(float a, float b, float t) {
#pragma clang fp contract(off)
  const float d = b - a;
  const float p = d * t;
  return a + p;
}

__device__ __forceinline__ float norm_rn(float v, float scale, float shift) {
#pragma clang fp contract(off)
  const float p = v * scale;
  return p + shift;
}

__global__ __launch_bounds__(RS_THREADS) void resize_u8_generic_kernel(ResizeParams p) {
  const int px = blockIdx.x * RS_THREADS + threadIdx.x;
  const int HW = p.H * p.W;
  if (px >= HW) return;
  const int r = px / p.W, q = px - r * p.W;
  const ResizeTap ty = resize_tap(p.Hs, p.Rh, p.top + r);
  const ResizeTap tx = resize_tap(p.Ws, p.Rw, p.left + q);
  const size_t row = size_t(p.Ws) * size_t(p.C);
  const size_t o00 = size_t(ty.i0) * row + size_t(tx.i0) * p.C, o01 = size_t(ty.i0) * row + size_t(tx.i1) * p.C;
  const size_t o10 = size_t(ty.i1) * row + size_t(tx.i0) * p.C, o11 = size_t(ty.i1) * row + size_t(tx.i1) * p.C;
  for (long long i = blockIdx.y; i < p.N; i += gridDim.y) {
    const unsigned char* xi = p.x + size_t(i) * size_t(p.Hs) * row;
    float* yi = p.y + size_t(i) * size_t(p.y_nstride) + px;
    for (int s = 0; s < p.C; ++s) {
      const float up = lerp_rn(float(xi[o00 + s]), float(xi[o01 + s]), tx.t);
      const float lo = lerp_rn(float(xi[o10 + s]), float(xi[o11 + s]), tx.t);
      yi[size_t(p.plane[s]) * size_t(HW)] = norm_rn(lerp_rn(up, lo, ty.t), p.scale[s], p.shift[s]);
    }
  }
}

// resize_u8_list_kernel: the same thread-per-pixel arithmetic over an image list (ore_image_list): image i of
// the launch takes its base, size, row stride and geometry from table[i].  The table is a const __restrict__
// kernel argument indexed by the block index alone, so the descriptor is one scalar load per workgroup and
// lives in SGPRs; the taps, which the dense kernel computes once per thread, are computed per image (one
// image per thread unless the list passes the grid's 65,535).  Every output pixel costs the same work
// whatever its source size, so mixed sizes bring no load imbalance.
__global__ __launch_bounds__(RS_THREADS) void resize_u8_list_kernel(const ResizeImage* __restrict__ table,
                                                                    ResizeListParams p) {
  const int px = blockIdx.x * RS_THREADS + threadIdx.x;
  const int HW = p.H * p.W;
  if (px >= HW) return;
  const int r = px / p.W, q = px - r * p.W;
  for (long long i = blockIdx.y; i < p.N; i += gridDim.y) {
    const ResizeImage d = table[i];
    const ResizeTap ty = resize_tap(d.Hs, d.Rh, d.top + r);
    const ResizeTap tx = resize_tap(d.Ws, d.Rw, d.left + q);
    const size_t r0 = size_t(ty.i0) * size_t(d.row), r1 = size_t(ty.i1) * size_t(d.row);
    const size_t c0 = size_t(tx.i0) * p.C, c1 = size_t(tx.i1) * p.C;
    const unsigned char* xi = d.x;
    float* yi = p.y + size_t(i) * size_t(p.y_nstride) + px;
    for (int s = 0; s < p.C; ++s) {
      const float up = lerp_rn(float(xi[r0 + c0 + s]), float(xi[r0 + c1 + s]), tx.t);
      const float lo = lerp_rn(float(xi[r1 + c0 + s]), float(xi[r1 + c1 + s]), tx.t);
      yi[size_t(p.plane[s]) * size_t(HW)] = norm_rn(lerp_rn(up, lo, ty.t), p.scale[s], p.shift[s]);
    }
  }
}

}  // namespace

void launch_resize_u8_list(const ResizeListParams& p, hipStream_t s) {
  if (p.N <= 0 || p.H <= 0 || p.W <= 0) return;
  const unsigned gy = unsigned(p.N < 65535 ? p.N : 65535);
  const long long hw = (long long)p.H * p.W;
  hipLaunchKernelGGL(resize_u8_list_kernel, dim3(unsigned((hw + RS_THREADS - 1) / RS_THREADS), gy), dim3(RS_THREADS), 0, s,
                     p.table + p.first, p);
}

void launch_resize_u8(const ResizeParams& p, hipStream_t s) {
  if (p.N <= 0 || p.H <= 0 || p.W <= 0) return;
  const unsigned gy = unsigned(p.N < 65535 ? p.N : 65535);
  const long long hw = (long long)p.H * p.W;
  hipLaunchKernelGGL(resize_u8_generic_kernel, dim3(unsigned((hw + RS_THREADS - 1) / RS_THREADS), gy), dim3(RS_THREADS), 0, s, p);
}

}  // namespace ore
