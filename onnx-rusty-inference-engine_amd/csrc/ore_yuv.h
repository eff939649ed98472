// The colour conversion of the NV12 image lists (ore_image_list_create_nv12, the *_nv12_* kernels in
// ore_resize.hip, ore_yuv_to_rgb): one (Y, U, V) triple of bytes to one (R, G, B) triple of bytes, fixed in
// integers so that the kernels, the host entry and a numpy restatement agree bit for bit.  With U' = U - 128,
// V' = V - 128, a matrix {yoff, cy, cvr, cug, cvg, cub} of round(k * 2^20) coefficients and >> an arithmetic
// shift (floor):
//     y = max(Y - yoff, 0) * cy + 2^19
//     R = clamp((y + cvr V') >> 20, 0, 255)
//     G = clamp((y - cug U' - cvg V') >> 20, 0, 255)
//     B = clamp((y + cub U') >> 20, 0, 255)
// Every accumulator stays below 5.8e8 in magnitude over all 2^24 triples, so int32 holds it.  The three terms
// of U' and V' (yuv_chroma) depend on the chroma pair alone: a kernel computes them once per pair and adds
// them to each of the pair's luma samples (yuv_rgb); integer arithmetic, so the split changes no result.
// Plain C++ besides the __host__ __device__ marks (as ore_resize_geom.h), so a host program can compile it alone.
#pragma once

#if defined(__HIPCC__)
#define ORE_YUV_HD __host__ __device__
#else
#define ORE_YUV_HD
#endif

namespace ore {

struct YuvMatrix {
  int yoff, cy, cvr, cug, cvg, cub;
};

constexpr int YUV_MATRICES = 3;  // ORE_YUV_BT601, ORE_YUV_BT709, ORE_YUV_BT601_FULL

// the matrix of an ore_yuv_matrix id; false for an unknown id
inline bool yuv_matrix(int id, YuvMatrix* m) {
  static const YuvMatrix table[YUV_MATRICES] = {
      {16, 1220542, 1673527, 409993, 852492, 2116026},  // BT.601 limited range: 1.164, 1.596, 0.391, 0.813, 2.018
      {16, 1220542, 1880097, 223347, 558891, 2214593},  // BT.709 limited range: 1.164, 1.793, 0.213, 0.533, 2.112
      {0, 1048576, 1470104, 360853, 748826, 1858077},   // BT.601 full range:    1,     1.402, 0.344, 0.714, 1.772
  };
  if (id < 0 || id >= YUV_MATRICES) return false;
  *m = table[id];
  return true;
}

// what a chroma pair adds to the luma term of R, G and B
struct YuvChroma {
  int r, g, b;
};

ORE_YUV_HD inline YuvChroma yuv_chroma(const YuvMatrix& m, int U, int V) {
  const int u = U - 128, v = V - 128;
  YuvChroma c;
  c.r = m.cvr * v;
  c.g = -(m.cug * u) - m.cvg * v;
  c.b = m.cub * u;
  return c;
}

ORE_YUV_HD inline int yuv_clamp(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// rgb: R, G, B of luma byte Y under the chroma terms c
ORE_YUV_HD inline void yuv_rgb(const YuvMatrix& m, int Y, const YuvChroma& c, int (&rgb)[3]) {
  const int d = Y - m.yoff;
  const int y = (d < 0 ? 0 : d) * m.cy + (1 << 19);
  rgb[0] = yuv_clamp((y + c.r) >> 20);
  rgb[1] = yuv_clamp((y + c.g) >> 20);
  rgb[2] = yuv_clamp((y + c.b) >> 20);
}

}  // namespace ore
