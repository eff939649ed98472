// Class activation maps of the selected classes (extension, ore_class_maps_f32 / ore_model_set_cam): a gathered
// 1x1 conv.  A GAP-headed classifier ends  Conv 1x1 (C -> M) -> [Relu] -> GlobalAveragePool -> [Softmax]; the
// pool's input T [n, M, H, W] is, class by class, the class activation map (Zhou et al. 2016).  For the k <= 64
// classes c[g, j] that the top-k selection kept (group g = image i / views) these kernels recompute
//     maps[i, j, r, q] = T[i, c[i / views, j], r, q]        float32, contiguous [n, k, H, W]
// from the conv's input, with the bits the model's unfused plan stores for T:
//   f32: the conv kernels' k-ordered f32 fma chain on v_mfma_f32_16x16x4_f32 (lane (lc, kq) feeds k = 4 s + kq
//        of k-step s, k-steps ascending from a zero accumulator), then + bias, then Relu -- the chain
//        conv1x1_gap_f32_kernel states (ore_conv_gap.hip);
//   f16: RNE_f16(relu?(sum f16(x) f16(w) [f32 acc] + b)) widened to f32, on v_mfma_f32_32x32x16_f16 with
//        conv_f16_kernel's assignment: k-step t covers channels 16 t .. 16 t + 15, lane l feeds the eight
//        channels 16 t + 8 (l >> 5) .. + 7 of row / pixel l & 31, K padded with zeros to a multiple of 32.
// A tail of a k-step multiplies zeros by zeros on both sides, as the conv kernels' padded tiles do.
//
// One wavefront is one task: an image x a block of 32 pixels x all k rows (k padded with zero rows to whole
// MFMA row tiles; the padded rows are computed and never stored).  Four tasks per 256-thread block, no LDS and no
// barrier; the tasks of an image are consecutive, P = H W is walked in blocks and is not bounded.  A small n still
// gives n ceil(P / 32) wavefronts.  The activations are read exactly once, straight from HBM into the B
// operand; A is gathered per k-step from the row-major [M][C] f32 weights (the k rows of an image stay in L2:
// k C 4 bytes), the class ids read from the device array and clamped to 0 .. M - 1 so that no id reads outside
// w.  Bounds: a pixel past P loads pixel P - 1 and is not stored, a channel past C loads channel 0 and
// enters as zero, every store is inside [n, k, H, W].  The f32 kernel takes planes of any stride and alignment by
// 4-byte loads (16 consecutive pixels per channel and instruction); the f16 kernel takes one 16-B load per pixel
// and k-step where C % 8 == 0 and the pixels are 16-B aligned, 2-byte loads otherwise.
#include <hip/hip_runtime.h>

#include "ore_kernels.h"

namespace ore {

namespace {

typedef float cm4 __attribute__((ext_vector_type(4)));
typedef float cm16 __attribute__((ext_vector_type(16)));
typedef _Float16 cmh8 __attribute__((ext_vector_type(8)));
typedef unsigned cmu4 __attribute__((ext_vector_type(4)));

constexpr int CM_PB = 32;  // pixels per task (wavefront)

// the task of this wavefront: image and first pixel; false past the last one (wave-uniform)
__device__ __forceinline__ bool cm_task(const ClassMaps& p, int* img, int* p0) {
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int pblocks = (p.P + CM_PB - 1) / CM_PB;
  const long long task = (long long)blockIdx.x * 4 + wave;
  if (task >= (long long)p.N * pblocks) return false;
  *img = int(task / pblocks);
  *p0 = int(task - (long long)*img * pblocks) * CM_PB;
  return true;
}

// the class of slot j of this image's group, clamped into the weights
__device__ __forceinline__ int cm_class(const ClassMaps& p, int img, int j) {
  const int c = p.classes[(long long)(img / p.views) * p.k + j];
  return c < 0 ? 0 : c >= p.M ? p.M - 1 : c;
}

template <int RT>  // 16-row tiles: k <= 16 RT
__global__ __launch_bounds__(256) void class_maps_f32_kernel(ClassMaps p) {
  int img, p0;
  if (!cm_task(p, &img, &p0)) return;  // wave-uniform; no barrier in this kernel
  const int lane = threadIdx.x & 63, lc = lane & 15, kq = lane >> 4;
  const float* __restrict__ xi = static_cast<const float*>(p.x) + (long long)img * p.x_nstride;
  // A: lane (lc, kq) holds row 16 r + lc, k = 4 s + kq of k-step s
  const float* wrow[RT];
  bool rok[RT];
#pragma unroll
  for (int r = 0; r < RT; ++r) {
    const int j = 16 * r + lc;
    rok[r] = j < p.k;
    wrow[r] = p.w + (long long)cm_class(p, img, rok[r] ? j : 0) * p.C;
  }
  // B: lane (lc, kq) holds channel 4 s + kq of pixel p0 + 16 f + lc
  const float* xp[2];
#pragma unroll
  for (int f = 0; f < 2; ++f) {
    const int px = p0 + 16 * f + lc;
    xp[f] = xi + (px < p.P ? px : p.P - 1);
  }
  cm4 acc[RT][2];
#pragma unroll
  for (int r = 0; r < RT; ++r)
#pragma unroll
    for (int f = 0; f < 2; ++f) acc[r][f] = cm4{0.0f, 0.0f, 0.0f, 0.0f};
  // every load is unconditional (a clamped address) and a row past k or a channel past C is zeroed by a bit mask,
  // not a select: the k loop stays free of branches, unrolls, and keeps its loads in flight under the MFMAs
  unsigned rmask[RT];
#pragma unroll
  for (int r = 0; r < RT; ++r) rmask[r] = rok[r] ? 0xffffffffu : 0u;
  auto kstep = [&](int cc, unsigned cmask) __attribute__((always_inline)) {
    float a[RT], b[2];
#pragma unroll
    for (int r = 0; r < RT; ++r) a[r] = __uint_as_float(__float_as_uint(wrow[r][cc]) & rmask[r] & cmask);
#pragma unroll
    for (int f = 0; f < 2; ++f) b[f] = __uint_as_float(__float_as_uint(xp[f][(long long)cc * p.x_ps]) & cmask);
#pragma unroll
    for (int r = 0; r < RT; ++r)
#pragma unroll
      for (int f = 0; f < 2; ++f) acc[r][f] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[r], b[f], acc[r][f], 0, 0, 0);
  };
  const int nfull = p.C / 4;
  int s = 0;
  for (; s + 8 <= nfull; s += 8) {  // eight k-steps' loads in flight
#pragma unroll
    for (int u = 0; u < 8; ++u) kstep(4 * (s + u) + kq, 0xffffffffu);
  }
  for (; s < nfull; ++s) kstep(4 * s + kq, 0xffffffffu);
  if (p.C % 4) {  // the tail k-step: channels past C enter as zero on both sides
    const int c = 4 * nfull + kq;
    kstep(c < p.C ? c : 0, c < p.C ? 0xffffffffu : 0u);
  }
  // lane (lc, kq) holds rows 16 r + 4 kq + e of pixel p0 + 16 f + lc
#pragma unroll
  for (int r = 0; r < RT; ++r)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int j = 16 * r + 4 * kq + e;
      if (j >= p.k) continue;
      const float bv = p.bias ? p.bias[cm_class(p, img, j)] : 0.0f;
      float* __restrict__ out = p.maps + ((long long)img * p.k + j) * p.P;
#pragma unroll
      for (int f = 0; f < 2; ++f) {
        const int px = p0 + 16 * f + lc;
        float v = acc[r][f][e] + bv;
        if (p.relu) v = fmaxf(v, 0.0f);
        if (px < p.P) out[px] = v;
      }
    }
}

// VEC: C % 8 == 0 and 16-B aligned pixels: one 16-B load per lane and k-step
template <int RT, bool VEC>  // 32-row tiles: k <= 32 RT
__global__ __launch_bounds__(256) void class_maps_f16_kernel(ClassMaps p) {
  int img, p0;
  if (!cm_task(p, &img, &p0)) return;  // wave-uniform; no barrier in this kernel
  const int lane = threadIdx.x & 63, lcol = lane & 31, lrow = lane >> 5;
  const int px = p0 + lcol;
  const _Float16* __restrict__ xp = static_cast<const _Float16*>(p.x) + (long long)img * p.x_nstride +
                                    (long long)(px < p.P ? px : p.P - 1) * p.x_ps;
  const float* wrow[RT];
  bool rok[RT];
#pragma unroll
  for (int r = 0; r < RT; ++r) {
    const int j = 32 * r + lcol;
    rok[r] = j < p.k;
    wrow[r] = p.w + (long long)cm_class(p, img, rok[r] ? j : 0) * p.C;
  }
  cm16 acc[RT];
#pragma unroll
  for (int r = 0; r < RT; ++r)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[r][e] = 0.0f;
  // as in the f32 kernel: unconditional loads from clamped addresses, zeros by bit masks, no branch in the k loop
  unsigned rmask[RT];
#pragma unroll
  for (int r = 0; r < RT; ++r) rmask[r] = rok[r] ? 0xffffffffu : 0u;
  auto kstep = [&](int ks) __attribute__((always_inline)) {
    const int c0 = ks + 8 * lrow;
    cmh8 b, a[RT];
    if constexpr (VEC) {  // the lane's eight channels are all inside C or all past it
      const unsigned cmask = c0 < p.C ? 0xffffffffu : 0u;
      const int cc = c0 < p.C ? c0 : 0;
      cmu4 bb = *reinterpret_cast<const cmu4*>(xp + cc);
#pragma unroll
      for (int e = 0; e < 4; ++e) bb[e] &= cmask;
      b = __builtin_bit_cast(cmh8, bb);
#pragma unroll
      for (int r = 0; r < RT; ++r) {
        const cm4 w0 = *reinterpret_cast<const cm4*>(wrow[r] + cc), w1 = *reinterpret_cast<const cm4*>(wrow[r] + cc + 4);
#pragma unroll
        for (int e = 0; e < 8; ++e)  // RNE, as the weight pack rounds
          a[r][e] = (_Float16)__uint_as_float(__float_as_uint(e < 4 ? w0[e & 3] : w1[e & 3]) & rmask[r] & cmask);
      }
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const unsigned cmask = c0 + e < p.C ? 0xffffffffu : 0u;
        const int cc = c0 + e < p.C ? c0 + e : 0;
        const unsigned short hb = (unsigned short)(reinterpret_cast<const unsigned short*>(xp)[cc] & cmask);
        b[e] = __builtin_bit_cast(_Float16, hb);
#pragma unroll
        for (int r = 0; r < RT; ++r) a[r][e] = (_Float16)__uint_as_float(__float_as_uint(wrow[r][cc]) & rmask[r] & cmask);
      }
    }
#pragma unroll
    for (int r = 0; r < RT; ++r) acc[r] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[r], b, acc[r], 0, 0, 0);
  };
  const int Kp = (p.C + 31) & ~31;  // conv_f16_kernel's padded K: the same number of k-steps, two per stage
  for (int ks = 0; ks < Kp; ks += 32) {
    kstep(ks);
    kstep(ks + 16);
  }
  // lane (lcol, lrow) holds rows 32 r + 8 q + 4 lrow + e of pixel p0 + lcol
#pragma unroll
  for (int r = 0; r < RT; ++r)
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int j = 32 * r + 8 * q + 4 * lrow + e;
        if (j >= p.k) continue;
        const float bv = p.bias ? p.bias[cm_class(p, img, j)] : 0.0f;
        float v = acc[r][4 * q + e] + bv;
        if (p.relu) v = fmaxf(v, 0.0f);
        if (px < p.P) p.maps[((long long)img * p.k + j) * p.P + px] = (float)(_Float16)v;  // the stored f16, widened
      }
}

unsigned cm_blocks(const ClassMaps& p) {
  const long long tasks = (long long)p.N * ((p.P + CM_PB - 1) / CM_PB);
  return (unsigned)((tasks + 3) / 4);
}

}  // namespace

bool class_maps_eligible(const ClassMaps& p) {
  return p.x && p.w && p.classes && p.maps && p.N >= 1 && p.C >= 1 && p.P >= 1 && p.M >= 1 && p.k >= 1 && p.k <= 64 &&
         p.k <= p.M && p.views >= 1 && p.N % p.views == 0 && p.x_ps >= 1 &&
         ((long long)p.N * ((p.P + CM_PB - 1) / CM_PB) + 3) / 4 < (1LL << 31);
}

void launch_class_maps_f32(const ClassMaps& p, hipStream_t s) {
  const dim3 grid(cm_blocks(p));
  switch ((p.k + 15) / 16) {
    case 1: hipLaunchKernelGGL(class_maps_f32_kernel<1>, grid, dim3(256), 0, s, p); break;
    case 2: hipLaunchKernelGGL(class_maps_f32_kernel<2>, grid, dim3(256), 0, s, p); break;
    case 3: hipLaunchKernelGGL(class_maps_f32_kernel<3>, grid, dim3(256), 0, s, p); break;
    default: hipLaunchKernelGGL(class_maps_f32_kernel<4>, grid, dim3(256), 0, s, p); break;
  }
}

void launch_class_maps_f16(const ClassMaps& p, hipStream_t s) {
  const dim3 grid(cm_blocks(p));
  const bool vec = p.C % 8 == 0 && p.x_ps % 8 == 0 && p.x_nstride % 8 == 0 &&
                   ((reinterpret_cast<uintptr_t>(p.x) | reinterpret_cast<uintptr_t>(p.w)) & 15) == 0;
  if (p.k <= 32) {
    if (vec) hipLaunchKernelGGL((class_maps_f16_kernel<1, true>), grid, dim3(256), 0, s, p);
    else hipLaunchKernelGGL((class_maps_f16_kernel<1, false>), grid, dim3(256), 0, s, p);
  } else {
    if (vec) hipLaunchKernelGGL((class_maps_f16_kernel<2, true>), grid, dim3(256), 0, s, p);
    else hipLaunchKernelGGL((class_maps_f16_kernel<2, false>), grid, dim3(256), 0, s, p);
  }
}

}  // namespace ore
