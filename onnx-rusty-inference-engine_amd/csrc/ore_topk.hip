// Row-wise top-k (extension, ore_topk_f32 / ore_model_classify): the k best elements of every row of a
// float32 matrix [rows][D] (row stride >= D), values and int32 indices, in one launch.  One wavefront per
// row, four rows per 256-thread block, no LDS and no barrier (the row-to-wave mapping of softmax_kernel).
//
// Order (fully specified, the host reproduces it with np.argsort(-x, kind="stable")[:, :k]): larger value
// first; equal values (-0.0 == +0.0) by ascending index; every NaN after every number, -inf included, NaNs
// among themselves by ascending index.
//
// Element i becomes the 64-bit key  hi:lo = image(x[i]) : ~i  where image() is the order-preserving unsigned
// image of the float (sign bit set for x >= 0, all bits flipped for x < 0) after folding -0.0 to +0.0, and 0
// for a NaN.  -inf maps to 0x007fffff, so every number's image is above a NaN's; ~i puts the lower index
// first among equal images.  Keys are unique and never 0 (i < 2^31), so 0 pads the slots past D and
// round j's winner is simply "the largest key strictly below round j - 1's": a lane-local max over the lane's
// keys, then a 6-step xor butterfly on the two halves.  Nothing is removed between rounds and no register
// is indexed dynamically.  Lane j keeps round j's key, so after k <= 64 rounds lane j holds output j and
// the row's k values and k indices go out as one coalesced store each.  values are copied as bits from
// x[index]: the sign of a zero and a NaN's payload survive.
//  * topk_kernel<NE>: D <= 64 NE, the keys stay in registers (one read of the row); NE = 4 and 16.
//  * topk_long_kernel: any D; every round re-reads the row (it stays in cache) and rebuilds the keys.
//
// View-mean top-k (extension, ore_topk_mean_f32 / ore_model_set_views): rows come in groups of V consecutive
// rows (the views of one subject); the selection runs over the mean row of each group, one wavefront per group.
// Element i of group g is
//     acc = x[gV, i];  for v = 1 .. V-1: acc = fadd_rn(acc, x[gV+v, i]);  m_i = fdiv_rn(acc, (float)V)
// in ascending view order, every operation rounded on its own, division IEEE, subnormals kept: numpy float32
// reproduces m bit for bit.  The keys are those of m; the stored value is m recomputed at the winning index by
// the same chain (the same bits: the sign of a zero survives, a NaN mean ranks as a NaN).  V == 1 is launch_topk.
//  * topk_mean_kernel<NE>: D <= 64 NE; V reads of the group's rows build the means, their keys stay in registers.
//  * topk_mean_long_kernel: any D; every round recomputes the means, so it reads k V D elements per group where
//    the register kernel reads V D (the rows stay in cache; at D = 4100, V = 10, k = 5 that is 50 reads and 45
//    adds per element against 10 and 9).  Correctness over speed past D = 1024.
#include <hip/hip_runtime.h>

#include "ore_kernels.h"

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

// lane j < k holds output j's key: the index is ~lo, the value a bit copy of the row's element
__device__ __forceinline__ void topk_store(const unsigned* xr, u64 mine, int lane, int k, long long row,
                                           float* values, int* indices) {
  if (lane < k && mine != 0ull) {  // mine == 0 only if k > D, which the callers reject
    const int idx = int(~unsigned(mine));
    reinterpret_cast<unsigned*>(values)[row * k + lane] = xr[idx];
    indices[row * k + lane] = idx;
  }
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

template <int NE>  // elements per lane held in registers: D <= 64 NE
__global__ __launch_bounds__(256) void topk_kernel(const float* __restrict__ x, long long stride, long long rows,
                                                   int D, int k, float* __restrict__ values,
                                                   int* __restrict__ indices) {
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;  // wave-uniform; no barrier in this kernel
  const unsigned* xr = reinterpret_cast<const unsigned*>(x) + row * stride;
  u64 key[NE];
#pragma unroll
  for (int t = 0; t < NE; ++t) {
    const int i = 64 * t + lane;
    key[t] = i < D ? topk_key(xr[i], i) : 0ull;
  }
  topk_store(xr, topk_rounds<NE>(key, k, lane), lane, k, row, values, indices);
}

__global__ __launch_bounds__(256) void topk_long_kernel(const float* __restrict__ x, long long stride,
                                                        long long rows, int D, int k, float* __restrict__ values,
                                                        int* __restrict__ indices) {
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const unsigned* xr = reinterpret_cast<const unsigned*>(x) + row * stride;
  u64 prev = ~0ull, mine = 0ull;
  for (int j = 0; j < k; ++j) {
    u64 best = 0ull;
    for (int i = lane; i < D; i += 64) {
      const u64 key = topk_key(xr[i], i);
      const u64 c = key < prev ? key : 0ull;
      best = c > best ? c : best;
    }
    prev = wave_max(best);
    mine = lane == j ? prev : mine;
  }
  topk_store(xr, mine, lane, k, row, values, indices);
}

// element i of the mean row of a group (xg: its first row)
__device__ __forceinline__ float view_mean(const float* __restrict__ xg, long long stride, int V, float fv, int i) {
#pragma clang fp contract(off)
  float acc = xg[i];
#pragma unroll 4  // the loads of four views in flight; the additions stay in view order
  for (int v = 1; v < V; ++v) acc = acc + xg[v * stride + i];
  return acc / fv;
}

// lane j < k holds output j's key: the value is the mean at its index, recomputed
__device__ __forceinline__ void topk_mean_store(const float* xg, long long stride, int V, float fv, u64 mine, int lane,
                                                int k, long long g, float* values, int* indices) {
  if (lane < k && mine != 0ull) {
    const int idx = int(~unsigned(mine));
    values[g * k + lane] = view_mean(xg, stride, V, fv, idx);
    indices[g * k + lane] = idx;
  }
}

template <int NE>  // topk_kernel<NE> whose key build reads V rows
__global__ __launch_bounds__(256) void topk_mean_kernel(const float* __restrict__ x, long long stride, long long groups,
                                                        int V, int D, int k, float* __restrict__ values,
                                                        int* __restrict__ indices) {
  const int lane = threadIdx.x & 63;
  const long long g = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (g >= groups) return;  // wave-uniform; no barrier in this kernel
  const float* xg = x + g * V * stride;
  const float fv = float(V);
  u64 key[NE];
  {
#pragma clang fp contract(off)
    // the slots past D read element 0 (D >= 1) and are never used: every load is unconditional, no divergence
    float acc[NE];
#pragma unroll
    for (int t = 0; t < NE; ++t) {
      const int i = 64 * t + lane;
      acc[t] = xg[i < D ? i : 0];
    }
#pragma unroll 2  // two views' loads in flight
    for (int v = 1; v < V; ++v) {  // ascending view order; the NE chains of a lane are independent
      const float* xv = xg + v * stride;
#pragma unroll
      for (int t = 0; t < NE; ++t) {
        const int i = 64 * t + lane;
        acc[t] = acc[t] + xv[i < D ? i : 0];
      }
    }
#pragma unroll
    for (int t = 0; t < NE; ++t) {
      const int i = 64 * t + lane;
      key[t] = i < D ? topk_key(__float_as_uint(acc[t] / fv), i) : 0ull;
    }
  }
  topk_mean_store(xg, stride, V, fv, topk_rounds<NE>(key, k, lane), lane, k, g, values, indices);
}

__global__ __launch_bounds__(256) void topk_mean_long_kernel(const float* __restrict__ x, long long stride,
                                                             long long groups, int V, int D, int k,
                                                             float* __restrict__ values, int* __restrict__ indices) {
  const int lane = threadIdx.x & 63;
  const long long g = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (g >= groups) return;
  const float* xg = x + g * V * stride;
  const float fv = float(V);
  u64 prev = ~0ull, mine = 0ull;
  for (int j = 0; j < k; ++j) {
    u64 best = 0ull;
    for (int i = lane; i < D; i += 64) {
      const u64 key = topk_key(__float_as_uint(view_mean(xg, stride, V, fv, i)), i);
      const u64 c = key < prev ? key : 0ull;
      best = c > best ? c : best;
    }
    prev = wave_max(best);
    mine = lane == j ? prev : mine;
  }
  topk_mean_store(xg, stride, V, fv, mine, lane, k, g, values, indices);
}

}  // namespace

void launch_topk_mean(const float* x, long long stride, long long groups, int V, int D, int k, float* values,
                      int* indices, hipStream_t s) {
  if (groups <= 0) return;
  if (V == 1) return launch_topk(x, stride, groups, D, k, values, indices, s);
  const dim3 grid((unsigned)((groups + 3) / 4));
  if (D <= 256)
    hipLaunchKernelGGL(topk_mean_kernel<4>, grid, dim3(256), 0, s, x, stride, groups, V, D, k, values, indices);
  else if (D <= 1024)
    hipLaunchKernelGGL(topk_mean_kernel<16>, grid, dim3(256), 0, s, x, stride, groups, V, D, k, values, indices);
  else
    hipLaunchKernelGGL(topk_mean_long_kernel, grid, dim3(256), 0, s, x, stride, groups, V, D, k, values, indices);
}

void launch_topk(const float* x, long long stride, long long rows, int D, int k, float* values, int* indices,
                 hipStream_t s) {
  if (rows <= 0) return;
  const dim3 grid((unsigned)((rows + 3) / 4));
  if (D <= 256)
    hipLaunchKernelGGL(topk_kernel<4>, grid, dim3(256), 0, s, x, stride, rows, D, k, values, indices);
  else if (D <= 1024)
    hipLaunchKernelGGL(topk_kernel<16>, grid, dim3(256), 0, s, x, stride, rows, D, k, values, indices);
  else
    hipLaunchKernelGGL(topk_long_kernel, grid, dim3(256), 0, s, x, stride, rows, D, k, values, indices);
}

}  // namespace ore
