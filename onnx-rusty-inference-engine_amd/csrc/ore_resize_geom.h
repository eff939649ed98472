// The tap map of the bilinear resize (ore_preprocess_resize_u8, ore_resize.hip): for one axis, which two
// source samples an output sample blends and with what weight.  Half-pixel centres, no antialiasing (the
// convention of cv2.INTER_LINEAR and of F.interpolate(mode="bilinear", align_corners=False)), stated in
// integers so that the kernels, the host checks and ore_resize_taps agree bit for bit.  Plain C++ besides
// the __host__ __device__ marks (as ore_wino_geom.h), so a host program can compile it alone.
#pragma once

#if defined(__HIPCC__)
#define ORE_RS_HD __host__ __device__
#else
#define ORE_RS_HD
#endif

namespace ore {

constexpr int RESIZE_MAX = 16384;  // source and resized sizes: (2 o + 1) S < 2^30, rem < 2 D <= 2^15

struct ResizeTap {
  int i0, i1;  // source samples, i0 <= i1 <= S - 1
  float t;     // weight of i1, 0 <= t < 1: sample = s[i0] + (s[i1] - s[i0]) t
};

// Resized index o (0 <= o < D) of an axis of S source samples resized to D.  The source coordinate is
// (o + 1/2) S / D - 1/2 = ((2 o + 1) S - D) / 2 D, clamped at 0: its floor is i0, its fraction rem / 2 D,
// one correctly rounded float32 division of two exactly representable integers.  At and past the last
// sample both taps are S - 1 and the weight is 0.
ORE_RS_HD inline ResizeTap resize_tap(int S, int D, int o) {
  int num = (2 * o + 1) * S - D;
  if (num < 0) num = 0;
  const unsigned d2 = 2u * unsigned(D);
  int i0 = int(unsigned(num) / d2);
  int rem = int(unsigned(num) - unsigned(i0) * d2);
  if (i0 >= S - 1) {
    i0 = S - 1;
    rem = 0;
  }
  ResizeTap r;
  r.i0 = i0;
  r.i1 = i0 + 1 < S ? i0 + 1 : S - 1;
  r.t = float(rem) / float(d2);
  return r;
}

// one axis of a geometry: S source samples resized to D, of which [origin, origin + count) are produced
ORE_RS_HD inline bool resize_axis_ok(long long S, long long D, long long origin, long long count) {
  return S >= 1 && S <= RESIZE_MAX && D >= 1 && D <= RESIZE_MAX && origin >= 0 && count >= 1 && count <= D &&
         origin <= D - count;
}

}  // namespace ore
