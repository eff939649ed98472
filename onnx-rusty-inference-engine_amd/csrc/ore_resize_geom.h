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

// ---------------------------------------------------------------- antialiased axes (ORE_FILTER_BILINEAR_AA)
// An axis that shrinks (S > D) under the antialiasing filter takes the triangle filter stretched by S / D
// (PIL's BILINEAR, F.interpolate(antialias=True)), in integers: with c = (2 o + 1) S the taps of resized
// index o are the source samples j of [0, S - 1] with |(2 j + 1) D - c| < 2 S, a contiguous and never empty
// run, and tap j weighs u_j = 2 S - |(2 j + 1) D - c| out of their sum U (taken over the clipped run, so the
// edges renormalise).  An axis with S <= D keeps resize_tap.  S <= 32 D bounds the run at 64 taps, u_j below
// 2^15, U at 2^21 and the sum of u_j * byte below 2^29.
constexpr int RESIZE_AA_MAX_RATIO = 32;  // ORE_AA_MAX_RATIO
constexpr int RESIZE_AA_MAX_TAPS = 64;   // ORE_AA_MAX_TAPS

struct ResizeSpan {
  int first, n;  // taps first .. first + n - 1, 1 <= n <= RESIZE_AA_MAX_TAPS
  int sum;       // U
};

ORE_RS_HD inline bool resize_axis_shrinks(long long S, long long D) { return S > D; }

// the ratio rule: an axis the antialiasing filter leaves alone, or one that shrinks by at most 32
ORE_RS_HD inline bool resize_axis_aa_ok(long long S, long long D) { return S <= D || S <= RESIZE_AA_MAX_RATIO * D; }

// weight of source sample j for resized index o; positive exactly on the taps of o
ORE_RS_HD inline int resize_aa_weight(int S, int D, int o, int j) {
  const int a = (2 * j + 1) * D - (2 * o + 1) * S;
  return 2 * S - (a < 0 ? -a : a);
}

// The run and its weight sum in closed form (S > D, S <= 32 D, 0 <= o < D).  (2 j + 1) D > c - 2 S gives
// first = floor((c - 2 S - D) / 2 D) + 1, whose numerator is negative only at o = 0, where the run starts at
// sample 0; (2 j + 1) D < c + 2 S gives last = floor((c + 2 S - D - 1) / 2 D), clipped to S - 1.  The
// distances a_j = (2 j + 1) D - c step by 2 D: the first k of them are negative (j <= floor((c - D - 1) / 2 D)),
// so the sum of |a_j| is two arithmetic series.
ORE_RS_HD inline ResizeSpan resize_aa_span(int S, int D, int o) {
  const int c = (2 * o + 1) * S;
  const unsigned d2 = 2u * unsigned(D);
  const int lo = c - 2 * S - D;
  const int first = lo < 0 ? 0 : int(unsigned(lo) / d2) + 1;
  int last = int(unsigned(c + 2 * S - D - 1) / d2);
  if (last > S - 1) last = S - 1;
  const int n = last - first + 1;
  int k = int(unsigned(c - D - 1) / d2) - first + 1;  // taps left of the centre
  k = k < 0 ? 0 : (k > n ? n : k);
  const int a0 = (2 * first + 1) * D - c;
  const int neg = k * a0 + D * k * (k - 1);                          // sum of the k negative a_j
  const int pos = (n - k) * a0 + D * (n * (n - 1) - k * (k - 1));    // sum of the others
  ResizeSpan r;
  r.first = first;
  r.n = n;
  r.sum = 2 * S * n - (pos - neg);
  return r;
}

}  // namespace ore
