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

// The blend of two samples under a tap's weight, every operation rounded on its own (never an FMA): a + (b - a) t.
// The float resizes (the class activation maps of ore_cam_box.hip and their host restatement ore_cam_box_host) take
// it from here; ore_resize.hip keeps its own lerp_rn, the same three operations.
ORE_RS_HD inline float resize_lerp_rn(float a, float b, float t) {
#pragma clang fp contract(off)
  const float d = b - a;
  const float p = d * t;
  return a + p;
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

// ---------------------------------------------------------------- cubic axes (ORE_FILTER_BICUBIC / _BICUBIC_AA)
// The Keys cubic convolution kernel, its weights in float32 with every operation rounded on its own (never an
// FMA, IEEE division), so that the kernels, ore_resize_cubic_taps and a numpy restatement agree bit for bit.
// include/ore.h states both filters; the integer part and the weights are here for host and device alike.
constexpr int RESIZE_CUBIC_AA_MAX_RATIO = 16;  // ORE_CUBIC_AA_MAX_RATIO: a run is then at most RESIZE_AA_MAX_TAPS

// |z| <= 1 and 1 <= |z| <= 2 of the kernel, in Horner form: ((a z + b) z) z + 1 and ((a z + b) z + c) z + d
ORE_RS_HD inline float cubic_near_rn(float a, float b, float z) {
#pragma clang fp contract(off)
  float r = a * z;
  r = r + b;
  r = r * z;
  r = r * z;
  return r + 1.0f;
}

ORE_RS_HD inline float cubic_far_rn(float a, float b, float c, float d, float z) {
#pragma clang fp contract(off)
  float r = a * z;
  r = r + b;
  r = r * z;
  r = r + c;
  r = r * z;
  return r + d;
}

// ORE_FILTER_BICUBIC (a = -0.75; cv2.INTER_CUBIC, F.interpolate(mode="bicubic")): resized index o reads the four
// samples clamp(first + k, 0, S - 1), k = 0..3, with weights w[k].  The source coordinate is that of resize_tap,
// NOT clamped at 0: its floor i is -1 where (2 o + 1) S < D, so first = i - 1 lies in [-2, S - 2].
struct ResizeCubicTap {
  int first;
  float w[4];
};

ORE_RS_HD inline ResizeCubicTap resize_cubic_tap(int S, int D, int o) {
  const int num = (2 * o + 1) * S - D;  // > -2 D
  const unsigned d2 = 2u * unsigned(D);
  const int i = num < 0 ? -1 : int(unsigned(num) / d2);
  const int rem = num - int(d2) * i;
  const float t = float(rem) / float(d2);
  const float s = 1.0f - t;
  ResizeCubicTap r;
  r.first = i - 1;
  r.w[0] = cubic_far_rn(-0.75f, 3.75f, -6.0f, 3.0f, t + 1.0f);
  r.w[1] = cubic_near_rn(1.25f, -2.25f, t);
  r.w[2] = cubic_near_rn(1.25f, -2.25f, s);
  r.w[3] = cubic_far_rn(-0.75f, 3.75f, -6.0f, 3.0f, s + 1.0f);
  return r;
}

ORE_RS_HD inline int resize_clamp(int j, int S) { return j < 0 ? 0 : (j > S - 1 ? S - 1 : j); }

// ORE_FILTER_BICUBIC_AA (a = -0.5; PIL's BICUBIC, F.interpolate(mode="bicubic", antialias=True)): with
// F = max(S, D), G = 2 F and c = (2 o + 1) S the taps of resized index o are the samples j of [0, S - 1] with
// a_j = |(2 j + 1) D - c| < 2 G, tap j weighing the kernel at a_j / G; the weights are divided by their sum over
// the clipped run, so the edges renormalise.  S <= 16 D bounds a run at 64 taps; an axis that does not shrink
// has at most 4.
struct ResizeCubicSpan {
  int first, n;  // taps first .. first + n - 1, 1 <= n <= resize_cubic_aa_max_taps(S, D)
};

ORE_RS_HD inline bool resize_axis_cubic_aa_ok(long long S, long long D) { return S <= RESIZE_CUBIC_AA_MAX_RATIO * D; }

// The run in closed form, as resize_aa_span: (2 j + 1) D > c - 4 F gives first = floor((c - 4 F - D) / 2 D) + 1,
// at least 0 (a negative numerator starts the run at sample 0); (2 j + 1) D < c + 4 F gives
// last = floor((c + 4 F - D - 1) / 2 D), clipped to S - 1.
ORE_RS_HD inline ResizeCubicSpan resize_cubic_aa_span(int S, int D, int o) {
  const int F = S > D ? S : D;
  const int c = (2 * o + 1) * S;
  const unsigned d2 = 2u * unsigned(D);
  const int lo = c - 4 * F - D;
  const int first = lo < 0 ? 0 : int(unsigned(lo) / d2) + 1;
  int last = int(unsigned(c + 4 * F - D - 1) / d2);
  if (last > S - 1) last = S - 1;
  ResizeCubicSpan r;
  r.first = first;
  r.n = last - first + 1;
  return r;
}

// no run of the axis is longer: the odd numbers 2 j + 1 of an open interval of length 8 F / D
ORE_RS_HD inline int resize_cubic_aa_max_taps(int S, int D) {
  const int F = S > D ? S : D;
  const int n = (4 * F + D - 1) / D;
  return n < RESIZE_AA_MAX_TAPS ? n : RESIZE_AA_MAX_TAPS;
}

// weight of source sample j (a tap of o) before the division by the run's sum
ORE_RS_HD inline float resize_cubic_aa_weight(int S, int D, int o, int j) {
  const int G = 2 * (S > D ? S : D);
  const int d = (2 * j + 1) * D - (2 * o + 1) * S;
  const int a = d < 0 ? -d : d;
  const float z = float(a) / float(G);
  return a < G ? cubic_near_rn(1.5f, -2.5f, z) : cubic_far_rn(-0.5f, 2.5f, -4.0f, 2.0f, z);
}

}  // namespace ore
