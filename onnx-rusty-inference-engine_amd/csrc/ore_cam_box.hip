// Localisation from class activation maps (extension, ore_upsample_maps_f32 / ore_cam_boxes_f32 /
// ore_model_set_cam_boxes; include/ore.h states the arithmetic): a map plane m [Hm, Wm] resized to the image's
// H x W with the project's bilinear filter on floats, and the bounding box of the largest 8-connected component of
// what lies at or above  lo + frac (hi - lo)  of the resized plane (Zhou et al. 2016).
//
// cam_upsampled() is the one statement of the resized value: the taps of resize_tap (ore_resize_geom.h) and three
// resize_lerp_rn, every operation rounded on its own.  Both kernels call it.
//
// upsample_maps_f32_kernel: one thread per output pixel, its two taps computed once and reused for every plane
// the thread walks (blockIdx.y strides the planes); a wave stores 256 contiguous bytes per plane.  The 2 x 2
// source samples come from global memory (a plane is a few hundred bytes and stays in cache).
//
// cam_boxes_f32_kernel: one workgroup of 256 threads per plane, everything in LDS, nothing global but the plane
// read once and 5 ints written.  The H x W plane is never stored: it is evaluated twice from the staged Hm x Wm
// plane and two tap tables, once for lo / hi, once for the mask, a bitmap of Wd = ceil(W / 32) words per row.
// Components are taken one at a time by a bit-parallel flood fill (DESIGN.md 3.12 says why not label propagation:
// labels would need 4 H W bytes, 1 MB at the caps, against 2 bitmaps of H Wd words):
//   seed  = the first pixel of the remaining mask in raster order, so components come in the order of the tie rule;
//   sweep = every word of the component takes the OR of its 3 x 3 word neighbourhood, dilated by one bit, ANDed
//           with the mask, and filled along the mask's runs inside the word by two carry chains (cb_fill);
//   a sweep that changes no word is the fixed point; then the popcount, the box, and the component leaves the mask.
// A thread owns `chunk` consecutive (row, word) items in column-major order, that is consecutive rows of one
// word column, and walks them down and then up in place: a sweep carries a bit through a whole chunk of rows,
// not one row.  Words only ever gain bits that belong to the component, so reading a neighbour another thread is
// updating is harmless.  The row stride and the chunk are odd, so the threads of a wave start in different banks.
// Trip bounds: a sweep that is not the last sets at least one bit, so a component of c pixels takes at most c + 1
// sweeps (bounded by H W + 1); each component removes at least one pixel, so there are at most H W of them; the
// loop also ends as soon as the pixels left cannot beat the best count.  Every barrier is outside divergent
// code: the loop conditions are values every thread read from LDS behind a barrier, or __syncthreads_or itself.
#include <hip/hip_runtime.h>

#include <atomic>
#include <climits>

#include "ore_kernels.h"
#include "ore_resize_geom.h"

namespace ore {

namespace {

constexpr int CB_THREADS = 256;
constexpr int CB_RED = 16;  // reduction slots behind the bitmaps

// element (r, q) of the resized plane from its taps: top = a + (b - a) tx, bot = c + (d - c) tx, top + (bot - top) ty
__device__ __forceinline__ float cam_upsampled(const float* m, int wm, const ResizeTap& ty, const ResizeTap& tx) {
  const float* r0 = m + ty.i0 * wm;
  const float* r1 = m + ty.i1 * wm;
  const float top = resize_lerp_rn(r0[tx.i0], r0[tx.i1], tx.t);
  const float bot = resize_lerp_rn(r1[tx.i0], r1[tx.i1], tx.t);
  return resize_lerp_rn(top, bot, ty.t);
}

__global__ __launch_bounds__(CB_THREADS) void upsample_maps_f32_kernel(const float* __restrict__ maps, float* __restrict__ out,
                                                                       long long planes, int hm, int wm, int h, int w) {
  const int px = blockIdx.x * CB_THREADS + threadIdx.x;
  const int hw = h * w;
  if (px >= hw) return;  // no barrier in this kernel
  const int r = px / w, q = px - r * w;
  const ResizeTap ty = resize_tap(hm, h, r);
  const ResizeTap tx = resize_tap(wm, w, q);
  for (long long i = blockIdx.y; i < planes; i += gridDim.y)
    out[i * hw + px] = cam_upsampled(maps + i * (hm * wm), wm, ty, tx);
}

// the mask's runs that hold a seed, inside one word: m + s carries from a seed to the end of its run, the
// changed bits (and the seeds a carry ran over) are the run above the seed; the same on the reversed bits fills
// downwards.  s is a subset of m.
__device__ __forceinline__ unsigned cb_fill(unsigned m, unsigned s) {
  const unsigned up = (((m + s) ^ m) | s) & m;
  const unsigned rm = __brev(m), rs = __brev(up);
  return __brev((((rm + rs) ^ rm) | rs) & rm);
}

struct CamBoxes {
  const float* maps;  // [planes][hm][wm]
  int* boxes;         // [planes][4]
  int* areas;         // [planes] or null
  int hm, wm, h, w;
  float frac;
};

enum { R_CNT = 0, R_RMIN, R_RMAX, R_CMIN, R_CMAX, R_SEED, R_TOTAL, R_LO = 8, R_HI = 12 };

__global__ __launch_bounds__(CB_THREADS) void cam_boxes_f32_kernel(CamBoxes p) {
  extern __shared__ unsigned cb_lds[];
  const int tid = threadIdx.x;
  const int H = p.h, W = p.w, wm = p.wm, P = p.hm * p.wm;
  const int Wd = (W + 31) >> 5, RS = Wd | 1;
  float* plane = reinterpret_cast<float*>(cb_lds);             // [P]
  int* tapi = reinterpret_cast<int*>(cb_lds + P);              // [H + W]: i0 | i1 << 16, rows then columns
  float* tapt = reinterpret_cast<float*>(cb_lds + P + H + W);  // [H + W]: the weight of i1
  unsigned* mask = cb_lds + P + 2 * (H + W);                   // [H][RS]: what is left of the mask
  unsigned* comp = mask + H * RS;                              // [H][RS]: the component being filled
  int* red = reinterpret_cast<int*>(comp + H * RS);            // [CB_RED]
  float* redf = reinterpret_cast<float*>(red);

  const float* __restrict__ src = p.maps + (long long)blockIdx.x * P;
  for (int i = tid; i < P; i += CB_THREADS) plane[i] = src[i];
  for (int i = tid; i < H + W; i += CB_THREADS) {
    const ResizeTap t = i < H ? resize_tap(p.hm, H, i) : resize_tap(wm, W, i - H);
    tapi[i] = t.i0 | (t.i1 << 16);
    tapt[i] = t.t;
  }
  for (int i = tid; i < 2 * H * RS; i += CB_THREADS) mask[i] = 0u;  // mask and comp, the pad words too
  if (tid == 0) {
    red[R_TOTAL] = 0;
    red[R_SEED] = INT_MAX;
  }
  __syncthreads();

  auto tap = [&](int i) {
    const int v = tapi[i];
    ResizeTap t;
    t.i0 = v & 0xffff;
    t.i1 = v >> 16;
    t.t = tapt[i];
    return t;
  };
  // this thread's items [i0, i1) of the H * Wd words in column-major order: item i is word i / H of row i % H
  const int T = H * Wd;
  const int chunk = ((T + CB_THREADS - 1) / CB_THREADS) | 1;
  const int i0 = min(T, tid * chunk), i1 = min(T, i0 + chunk);
  const int wd0 = i0 / H, r0 = i0 - wd0 * H;

  // lo, hi over the non-NaN resized values: a comparison with a NaN is false, so a NaN never enters
  float lo = INFINITY, hi = -INFINITY;
  for (int i = i0, r = r0, wd = wd0; i < i1; ++i) {
    const ResizeTap ty = tap(r);
    const int q0 = wd << 5, nb = min(32, W - q0);
    for (int b = 0; b < nb; ++b) {
      const float u = cam_upsampled(plane, wm, ty, tap(H + q0 + b));
      if (u < lo) lo = u;
      if (u > hi) hi = u;
    }
    if (++r == H) r = 0, ++wd;
  }
  for (int o = 32; o >= 1; o >>= 1) {
    const float l2 = __shfl_xor(lo, o), h2 = __shfl_xor(hi, o);
    if (l2 < lo) lo = l2;
    if (h2 > hi) hi = h2;
  }
  if ((tid & 63) == 0) {
    redf[R_LO + (tid >> 6)] = lo;
    redf[R_HI + (tid >> 6)] = hi;
  }
  __syncthreads();
  for (int k = 0; k < CB_THREADS / 64; ++k) {
    const float l2 = redf[R_LO + k], h2 = redf[R_HI + k];
    if (l2 < lo) lo = l2;
    if (h2 > hi) hi = h2;
  }
  // no value at all leaves lo = +inf, hi = -inf: thr = inf + frac * (-inf) is NaN and the mask is empty
  const float thr = resize_lerp_rn(lo, hi, p.frac);

  // the mask, its pixel count and its first pixel
  {
    int cnt = 0, key = INT_MAX;
    for (int i = i0, r = r0, wd = wd0; i < i1; ++i) {
      const ResizeTap ty = tap(r);
      const int q0 = wd << 5, nb = min(32, W - q0);
      unsigned bits = 0u;
      for (int b = 0; b < nb; ++b)
        if (cam_upsampled(plane, wm, ty, tap(H + q0 + b)) >= thr) bits |= 1u << b;
      mask[r * RS + wd] = bits;
      if (bits) {
        cnt += __popc(bits);
        key = min(key, r * W + q0 + (__ffs(bits) - 1));
      }
      if (++r == H) r = 0, ++wd;
    }
    if (cnt) {
      atomicAdd(&red[R_TOTAL], cnt);
      atomicMin(&red[R_SEED], key);
    }
  }
  __syncthreads();
  int remaining = red[R_TOTAL], seed = red[R_SEED];
  __syncthreads();  // every thread has read them before thread 0 resets the slots

  // one item of a sweep: 1 when the word gained a bit
  auto step = [&](int r, int wd) -> int {
    const int idx = r * RS + wd;
    const unsigned m = mask[idx];
    if (!m) return 0;
    const unsigned old = comp[idx];
    if (old == m) return 0;
    const bool left = wd > 0, right = wd + 1 < Wd;
    unsigned n = old, nl = left ? comp[idx - 1] : 0u, nr = right ? comp[idx + 1] : 0u;
    if (r > 0) {
      n |= comp[idx - RS];
      if (left) nl |= comp[idx - RS - 1];
      if (right) nr |= comp[idx - RS + 1];
    }
    if (r + 1 < H) {
      n |= comp[idx + RS];
      if (left) nl |= comp[idx + RS - 1];
      if (right) nr |= comp[idx + RS + 1];
    }
    const unsigned s = (n | (n << 1) | (n >> 1) | (nl >> 31) | (nr << 31)) & m;
    if (!s) return 0;
    const unsigned now = old | cb_fill(m, s);
    if (now == old) return 0;
    comp[idx] = now;
    return 1;
  };

  int best_cnt = 0, best_t = 0, best_l = 0, best_b = 0, best_r = 0;
  const int HW = H * W;
  for (int c = 0; c < HW; ++c) {                        // at most one component per pixel
    if (seed == INT_MAX || remaining <= best_cnt) break;  // uniform: both came out of LDS behind a barrier
    if (tid == 0) {
      const int sr = seed / W, sc = seed - sr * W;
      comp[sr * RS + (sc >> 5)] = 1u << (sc & 31);
      red[R_CNT] = 0;
      red[R_RMIN] = INT_MAX;
      red[R_RMAX] = -1;
      red[R_CMIN] = INT_MAX;
      red[R_CMAX] = -1;
      red[R_SEED] = INT_MAX;
    }
    __syncthreads();
    for (int sweep = 0; sweep <= HW; ++sweep) {  // a sweep that is not the last adds a pixel
      int changed = 0;
      int r = r0, wd = wd0;
      for (int i = i0; i < i1; ++i) {  // down the chunk's rows
        changed |= step(r, wd);
        if (++r == H) r = 0, ++wd;
      }
      for (int i = i1 - 1; i >= i0; --i) {  // and back up
        if (--r < 0) r = H - 1, --wd;
        changed |= step(r, wd);
      }
      if (!__syncthreads_or(changed)) break;
    }
    // the component's count and box; it leaves the mask, and the next seed is the first pixel still there
    {
      int cnt = 0, rmin = INT_MAX, rmax = -1, cmin = INT_MAX, cmax = -1, key = INT_MAX;
      for (int i = i0, r = r0, wd = wd0; i < i1; ++i) {
        const int idx = r * RS + wd, q0 = wd << 5;
        const unsigned cw = comp[idx];
        unsigned mw = mask[idx];
        if (cw) {
          cnt += __popc(cw);
          rmin = min(rmin, r);
          rmax = max(rmax, r);
          cmin = min(cmin, q0 + (__ffs(cw) - 1));
          cmax = max(cmax, q0 + 31 - __clz(cw));
          mw &= ~cw;
          mask[idx] = mw;
          comp[idx] = 0u;
        }
        if (mw) key = min(key, r * W + q0 + (__ffs(mw) - 1));
        if (++r == H) r = 0, ++wd;
      }
      if (cnt) {
        atomicAdd(&red[R_CNT], cnt);
        atomicMin(&red[R_RMIN], rmin);
        atomicMax(&red[R_RMAX], rmax);
        atomicMin(&red[R_CMIN], cmin);
        atomicMax(&red[R_CMAX], cmax);
      }
      if (key != INT_MAX) atomicMin(&red[R_SEED], key);
    }
    __syncthreads();
    const int cnt = red[R_CNT];
    if (cnt > best_cnt) {  // an equal count keeps the earlier component
      best_cnt = cnt;
      best_t = red[R_RMIN];
      best_b = red[R_RMAX] + 1;
      best_l = red[R_CMIN];
      best_r = red[R_CMAX] + 1;
    }
    remaining -= cnt;
    seed = red[R_SEED];
    __syncthreads();  // read before thread 0 resets the slots
  }
  if (tid == 0) {
    int* box = p.boxes + (long long)blockIdx.x * 4;
    box[0] = best_t;
    box[1] = best_l;
    box[2] = best_b;
    box[3] = best_r;
    if (p.areas) p.areas[blockIdx.x] = best_cnt;
  }
}

int cb_lds_bytes(int hm, int wm, int h, int w) {
  const int rs = ((w + 31) >> 5) | 1;
  return (hm * wm + 2 * (h + w) + 2 * h * rs + CB_RED) * 4;
}

}  // namespace

const char* cam_boxes_unsupported(long long hm, long long wm, long long h, long long w) {
  if (hm < 1 || wm < 1 || hm * wm > CAM_BOX_MAX_MAP || hm > CAM_BOX_MAX_MAP || wm > CAM_BOX_MAX_MAP) return "map";
  if (h < 1 || h > CAM_BOX_MAX_SIDE) return "h";
  if (w < 1 || w > CAM_BOX_MAX_SIDE) return "w";
  return nullptr;
}

void launch_upsample_maps_f32(const float* maps, long long planes, int hm, int wm, int h, int w, float* out, hipStream_t s) {
  const dim3 grid((unsigned)((h * w + CB_THREADS - 1) / CB_THREADS), (unsigned)std::min<long long>(planes, 65535));
  hipLaunchKernelGGL(upsample_maps_f32_kernel, grid, dim3(CB_THREADS), 0, s, maps, out, planes, hm, wm, h, w);
}

void launch_cam_boxes_f32(const float* maps, long long planes, int hm, int wm, int h, int w, float frac, int* boxes, int* areas,
                          hipStream_t s) {
  // the largest shape: 4096 + 2 * 1024 + 2 * 512 * 17 + 16 words, 94,272 bytes
  static std::atomic<unsigned long long> raised{0};
  ore_raise_lds_once(raised, reinterpret_cast<const void*>(&cam_boxes_f32_kernel),
                     cb_lds_bytes(1, CAM_BOX_MAX_MAP, CAM_BOX_MAX_SIDE, CAM_BOX_MAX_SIDE));
  const CamBoxes p{maps, boxes, areas, hm, wm, h, w, frac};
  hipLaunchKernelGGL(cam_boxes_f32_kernel, dim3((unsigned)planes), dim3(CB_THREADS), cb_lds_bytes(hm, wm, h, w), s, p);
}

}  // namespace ore
