// Resize + crop in front of the graph (extension, ore_preprocess_resize_u8 / ore_model_set_input_resize):
// uint8 NHWC images of any size to the float32 NCHW planes the model consumes, in the launch that converts
// and normalises.  Per output element, with a, b the bytes at (y0, x0), (y0, x1) and c, d at (y1, x0),
// (y1, x1) of the source channel, tx / ty the column / row weights (resize_tap, ore_resize_geom.h):
//     top = a + (b - a) tx;  bot = c + (d - c) tx;  v = top + (bot - top) ty;  y = v scale + shift
// Every operation rounds on its own (never an FMA), so numpy reproduces the result bit for bit.
//
// resize_u8_generic_kernel: one thread per output pixel, byte loads of the 2 x 2 x C taps from global memory,
// C float stores (a wave writes 256 contiguous bytes per plane).  Any size, alignment and y stride.  It is the
// only dense bilinear kernel: an LDS-staged one (a workgroup staging a band's source rows with 16-byte loads,
// 4 pixels x C channels per thread, float4 stores) ran 2.0x faster at 375 x 500 -> 224 but lost at
// 1080 x 1920 -> 224, where this kernel already moves its bytes at the device-to-device copy rate, and was
// removed (DESIGN.md 3.8b has the numbers).
// Image bases are 64-bit; offsets inside one image stay below 2^31 (sizes <= RESIZE_MAX, C <= 4).
//
// Everything else in this file is three parts that meet in two kernel templates:
//  - the list skeleton (list_pixels): which output pixel a thread computes for which descriptor, line by line or, for
//    a transposing descriptor, tile by tile through LDS;
//  - the sources (SrcU8<C>, SrcNv12, SrcYuv<F>): where a row of an image starts and the C ints of its pixels, whether
//    they are interleaved bytes, NV12 planes converted on the fly or the strided planes every YUV format reduces to;
//  - the four filter bodies (bilinear_pixel, aa_pixel, cubic_pixel, cubic_aa_pixel) over a source and a ResizeGeom.
// resize_list_kernel<FILTER, C, MODE> is the skeleton around a body over the descriptor's source, and
// resize_dense_kernel<FILTER, C> the body over image i of a batch.  One body reads no source: the plain filter over
// interleaved descriptors keeps its channel count at run time (bilinear_u8_pixel), one instance per mode.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "../../include/ore.h"
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

// ---------------------------------------------------------------------------------------------------------
// The list skeleton.  An image list (ore_image_list) is a device table of descriptors: image i of the launch takes
// its base, size, row stride and geometry from table[i].  The table is a const __restrict__ kernel argument indexed
// by the block index alone, so the descriptor is one scalar load per workgroup and lives in SGPRs; the taps, which
// the dense bilinear kernel computes once per thread, are computed per image (one image per thread unless the list
// passes the grid's 65,535).  Every output pixel costs the same work whatever its source size, so mixed sizes bring
// no load imbalance.
//
// A descriptor's flip (ORE_IMAGE_FLIP_H, ore_image_list_set_ex) mirrors its window: output column q takes resized
// column left + W - 1 - q, the store position stays q, so the image is the unflipped one with its columns
// reversed, bit for bit.  The flag comes with the descriptor: wave-uniform, one scalar select per image.  The list
// kernel exists per ListMode: LIST_FLIP reads the flag; LIST_PLAIN does not, and is the one launched when no
// descriptor of the list is flipped (ResizeListParams::flips), so that such a launch pays nothing for the feature.
//
// A descriptor's orientation (ore_image_list_set_oriented, EXIF codes 1..8) is three more bits of the same word
// (LIST_REV_ROWS / LIST_REV_COLS / LIST_TRANSPOSE, ore_kernels.h); the descriptor's geometry is then the STORED
// image's (ore_orient_geometry).  Output pixel (r, q) -- after the flip -- takes row u and column v of the stored
// window of Hz x Wz = (H, W), or (W, H) under the transpose: (u, v) = (r, q) or (q, r), each reversed in its extent
// where its bit is set.  The taps and every float operation stay those of the stored window, so the image is the
// unoriented one of shape (Hz, Wz) permuted, bit for bit.  The bits are wave-uniform like the flag; a third instance
// (LIST_ORIENT) reads them, launched only for a list that holds a code other than 1 (or, inside a capture, a list
// marked by a first oriented set), so that the two instances above pay nothing for them either.
enum ListMode { LIST_PLAIN = 0, LIST_FLIP = 1, LIST_ORIENT = 2 };

struct ListRQ {
  int r, q;  // row and column of the descriptor's (stored) window
};

template <int MODE>
__device__ __forceinline__ ListRQ list_rq(int word, int H, int W, int r, int q) {
  if constexpr (MODE == LIST_PLAIN) return ListRQ{r, q};
  if constexpr (MODE == LIST_FLIP) return ListRQ{r, word ? W - 1 - q : q};
  if (word & LIST_FLIP_H) q = W - 1 - q;
  const bool tr = (word & LIST_TRANSPOSE) != 0;
  const int u = tr ? q : r, v = tr ? r : q;
  const int Hz = tr ? W : H, Wz = tr ? H : W;
  return ListRQ{word & LIST_REV_ROWS ? Hz - 1 - u : u, word & LIST_REV_COLS ? Wz - 1 - v : v};
}

// Under the transpose a wave's 64 adjacent output columns are 64 stored rows: with the index map alone every tap
// read of a wave scatters over 64 rows, which measured 2.6 - 10 times the upright launch (that instance
// was removed).  LIST_ORIENT therefore maps transposing descriptors by tiles.  A workgroup of T threads takes a tile of
// T / 16 output rows x 16 output columns.  Its lanes compute adjacent along the output ROW index, which under the
// transpose is the stored column, so a wave's tap reads cover 4 stored rows (8 where T = 128) instead of 64; the results pass through
// LDS ([plane][column][row], pitch rows + 1: both the writes and the reads are conflict-free) and are stored with
// lanes adjacent along the output column.  Descriptors that do not transpose keep the line mapping (block b: pixels
// b T ..), so the branch is per descriptor: block- and wave-uniform, and every thread of the block reaches the two
// barriers.  The grid has one block per tile, which is never fewer than the line mapping needs.
// pixel(pp, yo, hw, px, r, q) computes output pixel (r, q) of the image and stores channel s at
// yo[pp.plane[s] * hw + px]: the tile path hands it the LDS tile, which is therefore laid out by OUTPUT plane (the
// plane map is a permutation of 0 .. C-1).
constexpr int TILE_W = 16;

template <int T, class P, class F>
__device__ __forceinline__ void list_image(int word, const P& p, int C, float* __restrict__ yimg, F&& pixel) {
  const int HW = p.H * p.W;
  const int tid = threadIdx.x;
  if (!(word & LIST_TRANSPOSE)) {
    const int px = blockIdx.x * T + tid;
    if (px < HW) {
      const int r = px / p.W;
      pixel(p, yimg, HW, px, r, px - r * p.W);
    }
    return;
  }
  constexpr int TH = T / TILE_W, PITCH = TH + 1, PLANE = TILE_W * PITCH;
  __shared__ float tile[4 * PLANE];
  const int tw = (p.W + TILE_W - 1) / TILE_W;
  const int tr = blockIdx.x / tw, tc = blockIdx.x - tr * tw;  // the grid is exactly the tiles: tr * TH < H
  if (tr * TH >= p.H) return;  // block-uniform, as everything up to here
  {
    const int il = tid % TH, jl = tid / TH;
    const int r = tr * TH + il, q = tc * TILE_W + jl;
    if (r < p.H && q < p.W) pixel(p, tile, PLANE, jl * PITCH + il, r, q);
  }
  __syncthreads();
  {
    const int jl = tid % TILE_W, il = tid / TILE_W;
    const int r = tr * TH + il, q = tc * TILE_W + jl;
    if (r < p.H && q < p.W)  // ragged tile edges: nothing outside the image's H x W elements is stored
      for (int k = 0; k < C; ++k) yimg[size_t(k) * size_t(HW) + size_t(r) * p.W + q] = tile[k * PLANE + jl * PITCH + il];
  }
  __syncthreads();  // the tile is free for the next image of this block
}

// The skeleton of every list kernel, for workgroups of T threads: the images blockIdx.y walks, and for each the
// output pixel of this thread.  body(d, pp, yo, hw, px, r, q) is the kernel's pixel: row r and column q of descriptor
// d's window, stored at yo[pp.plane[s] * hw + px].  LIST_PLAIN and LIST_FLIP: thread t of block b has pixel b T + t of
// every image; LIST_ORIENT: every image through list_image.
template <int T, int MODE, class D, class P, class F>
__device__ __forceinline__ void list_pixels(const D* __restrict__ table, const P& p, int C, F&& body) {
  if constexpr (MODE == LIST_ORIENT) {
    for (long long i = blockIdx.y; i < p.N; i += gridDim.y) {
      const D d = table[i];
      list_image<T>(d.flip, p, C, p.y + size_t(i) * size_t(p.y_nstride), [&](const P& pp, float* yo, int hw, int px, int r, int q) {
        const ListRQ m = list_rq<LIST_ORIENT>(d.flip, p.H, p.W, r, q);
        body(d, pp, yo, hw, px, m.r, m.q);
      });
    }
  } else {
    const int px = blockIdx.x * T + threadIdx.x;
    const int HW = p.H * p.W;
    if (px >= HW) return;
    const int r = px / p.W, q = px - r * p.W;
    for (long long i = blockIdx.y; i < p.N; i += gridDim.y) {
      const D d = table[i];
      const ListRQ m = list_rq<MODE>(d.flip, p.H, p.W, r, q);
      body(d, p, p.y + size_t(i) * size_t(p.y_nstride), HW, px, m.r, m.q);
    }
  }
}

// ---------------------------------------------------------------------------------------------------------
// The sources.  A filter body reads an image through a source: where a row starts (at), the C ints of one of its
// pixels (px) and of four neighbours at once (px4: interleaved bytes as C dwords), and through the image's geometry
// (ResizeGeom), which a dense batch, the three descriptors and nothing else supply.  The three kinds of source differ
// in nothing else; the antialiased bilinear filter, whose column runs are integer sums over grouped loads, has one
// aa_row per kind beside them (further down).

struct ResizeGeom {
  int Hs, Ws, Rh, Rw, top, left;
};

template <class T>
__device__ __forceinline__ ResizeGeom resize_geom(const T& t) {
  ResizeGeom g;
  g.Hs = t.Hs; g.Ws = t.Ws; g.Rh = t.Rh; g.Rw = t.Rw; g.top = t.top; g.left = t.left;
  return g;
}

template <int C>
struct SrcU8 {
  const unsigned char* x;
  int row;  // bytes between rows
  using Row = const unsigned char*;
  __device__ __forceinline__ Row at(int r) const { return x + size_t(r) * size_t(row); }
  __device__ __forceinline__ void px(Row w, int j, int (&v)[C]) const {
#pragma unroll
    for (int s = 0; s < C; ++s) v[s] = int(w[j * C + s]);
  }
  // pixels j .. j + 3, all inside the row: their 4 C bytes as C dword loads at the pixels' own (any) alignment
  __device__ __forceinline__ void px4(Row w, int j, int (&v)[4][C]) const {
    unsigned d[C];
#pragma unroll
    for (int i = 0; i < C; ++i) __builtin_memcpy(&d[i], w + j * C + 4 * i, 4);
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int s = 0; s < C; ++s) {
        const int k = t * C + s;
        v[t][s] = int((d[k >> 2] >> (8 * (k & 3))) & 0xffu);
      }
  }
};

// NV12 sources (ore_image_list_create_nv12): the pixel fetch replaced by fetch and convert.  Source pixel (r, j) is
// the Y byte at (r, j) and the UV pair at (r >> 1, j >> 1), converted by ore_yuv.h to the R, G, B bytes an
// interleaved source would hold with C = 3; everything after the fetch is the same code.  The six matrix integers
// are kernel arguments (SGPRs).  The clamp makes the conversion non-linear, so it is done per tap and cannot leave
// the sums; what depends on the chroma pair alone (yuv_chroma) is computed once per pair.

// the chroma terms of pair c of UV row ur: two bytes at any alignment
__device__ __forceinline__ YuvChroma nv12_chroma(const YuvMatrix& m, const unsigned char* __restrict__ ur, int c) {
  unsigned short uv;
  __builtin_memcpy(&uv, ur + 2 * c, 2);
  return yuv_chroma(m, int(uv & 0xffu), int(uv >> 8));
}

// R, G, B of source pixel j of a row (yr: its Y bytes, ur: its UV pairs)
__device__ __forceinline__ void nv12_pixel(const YuvMatrix& m, const unsigned char* __restrict__ yr,
                                           const unsigned char* __restrict__ ur, int j, int (&rgb)[3]) {
  yuv_rgb(m, int(yr[j]), nv12_chroma(m, ur, j >> 1), rgb);
}

struct SrcNv12 {
  const unsigned char* y;
  const unsigned char* uv;
  int yrow, uvrow;
  YuvMatrix m;
  struct Row {
    const unsigned char* yr;
    const unsigned char* ur;
  };
  __device__ __forceinline__ Row at(int r) const {
    return Row{y + size_t(r) * size_t(yrow), uv + size_t(r >> 1) * size_t(uvrow)};
  }
  __device__ __forceinline__ void px(const Row& w, int j, int (&v)[3]) const { nv12_pixel(m, w.yr, w.ur, j, v); }
  __device__ __forceinline__ void px4(const Row& w, int j, int (&v)[4][3]) const {
#pragma unroll
    for (int t = 0; t < 4; ++t) px(w, j + t, v[t]);
  }
};

// YUV sources of any ore_yuv_format (ore_image_list_create_yuv): the NV12 fetch generalised to strided planes
// (YuvImage, ore_kernels.h).  ore_image_list_set_yuv reduced the format to three bases, three pitches, a luma and
// a chroma byte step and the two subsampling shifts, so nothing here reads the format.  Those fields leave four ways
// to fetch a pixel (YuvFetch), and the source is templated on them: the way is chosen from the descriptor -- one
// scalar load per workgroup, so the branch is wave-uniform -- in one place, yuv_fetch_as, and the body it selects is
// branch-free, so that its loads issue together.  Where a filter makes the choice was measured per filter (DESIGN.md
// 3.8f) and is kept: once per image around the whole pixel for the bilinear and cubic bodies, once per tap row for
// the antialiased bilinear one.  (Choosing per pixel fetched instead, inside the fetch, put each of the four taps'
// loads behind a wait of its own: 162 us against 109 us for 256 NV12 frames of 1080 x 1920 under the plain filter.)
enum YuvFetch {
  YUV_GREY = 0,    // u == null: Y alone, every chroma term zero
  YUV_PLANES = 1,  // cstep == 1: Y, U and V by a byte load each
  YUV_PAIRS = 2,   // cstep == 2: NV12's interleaved pairs, v == u + 1: Y by a byte, (U, V) by one two-byte load
  YUV_PACKED = 3,  // ystep == 2: YUYV, a pixel's group Y0 U Y1 V is one dword
};

// the three rows source row r reads; u and v are null in a grey frame
struct YuvRow {
  const unsigned char* y;
  const unsigned char* u;
  const unsigned char* v;
};

__device__ __forceinline__ YuvRow yuv_row(const YuvImage& d, int r) {
  YuvRow w;
  w.y = d.y + size_t(r) * size_t(d.yrow);
  w.u = nullptr; w.v = nullptr;
  if (d.u) {
    const size_t cr = size_t(r >> d.sy);
    w.u = d.u + cr * size_t(d.urow);
    w.v = d.v + cr * size_t(d.vrow);
  }
  return w;
}

// the chroma terms of sample c of a row of planes or pairs; the pair is two bytes at any alignment, as nv12_chroma
template <int F>
__device__ __forceinline__ YuvChroma yuv_sample(const YuvMatrix& m, const YuvRow& w, int c) {
  static_assert(F == YUV_PLANES || F == YUV_PAIRS, "grey rows have no chroma, packed rows carry it beside the luma");
  if (F == YUV_PAIRS) {
    unsigned short uv;
    __builtin_memcpy(&uv, w.u + 2 * c, 2);
    return yuv_chroma(m, int(uv & 0xffu), int(uv >> 8));
  }
  return yuv_chroma(m, int(w.u[c]), int(w.v[c]));
}

template <int F>
struct SrcYuv {
  YuvImage d;
  YuvMatrix m;
  using Row = YuvRow;
  __device__ __forceinline__ Row at(int r) const { return yuv_row(d, r); }
  __device__ __forceinline__ void px(const Row& w, int j, int (&rgb)[3]) const {
    if constexpr (F == YUV_PACKED) {
      unsigned g;
      __builtin_memcpy(&g, w.y + 4 * (j >> 1), 4);
      yuv_rgb(m, int((g >> (16 * (j & 1))) & 0xffu), yuv_chroma(m, int((g >> 8) & 0xffu), int(g >> 24)), rgb);
    } else if constexpr (F == YUV_GREY) {
      yuv_rgb(m, int(w.y[j]), YuvChroma{0, 0, 0}, rgb);  // U = V = 128
    } else {
      yuv_rgb(m, int(w.y[j]), yuv_sample<F>(m, w, j >> d.sx), rgb);
    }
  }
  __device__ __forceinline__ void px4(const Row& w, int j, int (&v)[4][3]) const {
#pragma unroll
    for (int t = 0; t < 4; ++t) px(w, j + t, v[t]);
  }
};

// a YUV descriptor whose way to fetch is not chosen yet: its rows start where every SrcYuv<F>'s do
struct SrcYuvAny {
  YuvImage d;
  YuvMatrix m;
  using Row = YuvRow;
  __device__ __forceinline__ Row at(int r) const { return yuv_row(d, r); }
};

// f(the source to read through): the descriptor's SrcYuv<F>, or a source of the other kinds as it is
template <class Fn>
__device__ __forceinline__ void yuv_fetch_as(const SrcYuvAny& src, Fn&& f) {
  const YuvImage& d = src.d;
  switch (d.ystep != 1 ? YUV_PACKED : !d.u ? YUV_GREY : d.cstep == 2 ? YUV_PAIRS : YUV_PLANES) {
    case YUV_PACKED: return f(SrcYuv<YUV_PACKED>{d, src.m});
    case YUV_PAIRS: return f(SrcYuv<YUV_PAIRS>{d, src.m});
    case YUV_PLANES: return f(SrcYuv<YUV_PLANES>{d, src.m});
    default: return f(SrcYuv<YUV_GREY>{d, src.m});
  }
}

template <class Src, class Fn>
__device__ __forceinline__ void yuv_fetch_as(const Src& src, Fn&& f) {
  f(src);
}

// the source of image i of a dense batch, and of a list descriptor under its list's parameters
template <int C>
__device__ __forceinline__ SrcU8<C> src_of(const ResizeParams& p, long long i) {
  const int row = p.Ws * p.C;
  return SrcU8<C>{p.x + size_t(i) * size_t(p.Hs) * size_t(row), row};
}

template <int C>
__device__ __forceinline__ SrcU8<C> src_of(const ResizeImage& d, const ResizeListParams&) {
  return SrcU8<C>{d.x, d.row};
}

template <int C>
__device__ __forceinline__ SrcNv12 src_of(const Nv12Image& d, const Nv12ListParams& p) {
  static_assert(C == 3, "an NV12 frame converts to three channels");
  return SrcNv12{d.y, d.uv, d.yrow, d.uvrow, p.m};
}

template <int C>
__device__ __forceinline__ SrcYuvAny src_of(const YuvImage& d, const YuvListParams& p) {
  static_assert(C == 3, "a YUV frame converts to three channels");
  return SrcYuvAny{d, p.m};
}

// ---------------------------------------------------------------------------------------------------------
// ORE_FILTER_BILINEAR over a source: the arithmetic at the top of the file.  One output pixel: row r and column q of
// the window, stored at yi[plane * HW] (yi: the pixel in plane 0).  A YUV descriptor's way to fetch is chosen once per
// image around the four fetches alone; the taps before them and the lerps and stores after them exist once.
template <int C, class Src, class P>
__device__ __forceinline__ void bilinear_pixel(const Src& src, const ResizeGeom& g, const P& p, float* yi, int HW, int r, int q) {
  const ResizeTap ty = resize_tap(g.Hs, g.Rh, g.top + r);
  const ResizeTap tx = resize_tap(g.Ws, g.Rw, g.left + q);
  const typename Src::Row w0 = src.at(ty.i0), w1 = src.at(ty.i1);
  int a[C], b[C], c[C], e[C];
  yuv_fetch_as(src, [&](const auto& s) {
    s.px(w0, tx.i0, a);
    s.px(w0, tx.i1, b);
    s.px(w1, tx.i0, c);
    s.px(w1, tx.i1, e);
  });
#pragma unroll
  for (int s = 0; s < C; ++s) {
    const float up = lerp_rn(float(a[s]), float(b[s]), tx.t);
    const float lo = lerp_rn(float(c[s]), float(e[s]), tx.t);
    yi[size_t(p.plane[s]) * size_t(HW)] = norm_rn(lerp_rn(up, lo, ty.t), p.scale[s], p.shift[s]);
  }
}

// The same pixel of an interleaved descriptor with the channel count at run time (p.C), each channel loaded and
// stored in turn: the list kernel's one bilinear instance per mode for C = 1..4 (C = 0 in its template arguments).
// A body over SrcU8<C> loads all 4 C bytes before the first store, which is another schedule -- as declaring yi
// __restrict__ is -- and wants a measurement of its own.
__device__ __forceinline__ void bilinear_u8_pixel(const ResizeImage& d, const ResizeListParams& p, float* yi, int HW,
                                                  int r, int q) {
  const ResizeTap ty = resize_tap(d.Hs, d.Rh, d.top + r);
  const ResizeTap tx = resize_tap(d.Ws, d.Rw, d.left + q);
  const size_t r0 = size_t(ty.i0) * size_t(d.row), r1 = size_t(ty.i1) * size_t(d.row);
  const size_t c0 = size_t(tx.i0) * p.C, c1 = size_t(tx.i1) * p.C;
  const unsigned char* xi = d.x;
  for (int s = 0; s < p.C; ++s) {
    const float up = lerp_rn(float(xi[r0 + c0 + s]), float(xi[r0 + c1 + s]), tx.t);
    const float lo = lerp_rn(float(xi[r1 + c0 + s]), float(xi[r1 + c1 + s]), tx.t);
    yi[size_t(p.plane[s]) * size_t(HW)] = norm_rn(lerp_rn(up, lo, ty.t), p.scale[s], p.shift[s]);
  }
}

// ---------------------------------------------------------------------------------------------------------
// ORE_FILTER_BILINEAR_AA (include/ore.h has the arithmetic): an axis that shrinks sums every source sample of
// the stretched triangle (resize_aa_span / resize_aa_weight), the other axis keeps resize_tap.  Per output
// element: per tap row the column sum in integers (exact, one conversion) or the column lerp; then the row
// taps in ascending order, fmul and fadd each rounded on its own, one division by the row weight sum (or the
// row lerp); one division by the column weight sum; scale and shift.  The divisions are IEEE (hipcc's default
// correctly rounded fdiv); they are the only place the ISA holds v_fma.  A run of column taps is read four
// taps (4 C bytes) at a time as C dwords at the run's own alignment, the rest by bytes.
//
// One device body (aa_pixel), templated on the channel count so that the per-channel sums live in registers: one
// thread per output pixel walks its taps_y x taps_x window in global memory, any size, alignment, row stride and y
// stride, 64-bit image bases only.  What it asks of a source is one tap row's column sums: aa_row, one overload per
// kind of source, each with the grouped loads its layout allows.  A band kernel (a workgroup computing the horizontal
// sums of a band's source rows once into LDS, then the vertical chains from LDS) gave the same bits but was slower at
// both bench geometries and was removed (DESIGN.md 3.8d has the numbers).

__device__ __forceinline__ float macc_rn(float acc, float v, float g) {
#pragma clang fp contract(off)
  const float p = v * g;
  return acc + p;
}

// the taps of one axis for resized index o: a run (shrinking) or the two samples of resize_tap
struct AaAxis {
  int first, n, sum;  // shrinking: resize_aa_span
  int i1;             // plain: samples first and i1, weight t
  float t;
};

__device__ __forceinline__ AaAxis aa_axis(bool shrinks, int S, int D, int o) {
  AaAxis a;
  if (shrinks) {
    const ResizeSpan sp = resize_aa_span(S, D, o);
    a.first = sp.first; a.n = sp.n; a.sum = sp.sum;
    a.i1 = sp.first; a.t = 0.f;
  } else {
    const ResizeTap tp = resize_tap(S, D, o);
    a.first = tp.i0; a.n = 2; a.sum = 1;
    a.i1 = tp.i1; a.t = tp.t;
  }
  return a;
}

// g of source row r of interleaved bytes for resized column ox
template <int C>
__device__ __forceinline__ void aa_row(const SrcU8<C>& src, const ResizeGeom& d, int r, bool sx, const AaAxis& ax, int ox,
                                       float (&g)[C]) {
  const unsigned char* __restrict__ xr = src.at(r);
  if (sx) {
    int acc[C];
#pragma unroll
    for (int s = 0; s < C; ++s) acc[s] = 0;
    const unsigned char* pp = xr + ax.first * C;
    int j = 0;
    // four taps at a time: their 4 C bytes as C dword loads at the window's own (any) alignment, all inside it
    for (; j + 4 <= ax.n; j += 4) {
      unsigned dw[C];
#pragma unroll
      for (int i = 0; i < C; ++i) __builtin_memcpy(&dw[i], pp + j * C + 4 * i, 4);
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int u = resize_aa_weight(d.Ws, d.Rw, ox, ax.first + j + t);
#pragma unroll
        for (int s = 0; s < C; ++s) {
          const int k = t * C + s;
          acc[s] += __mul24(u, int((dw[k >> 2] >> (8 * (k & 3))) & 0xffu));
        }
      }
    }
    for (; j < ax.n; ++j) {
      const int u = resize_aa_weight(d.Ws, d.Rw, ox, ax.first + j);
#pragma unroll
      for (int s = 0; s < C; ++s) acc[s] += __mul24(u, int(pp[j * C + s]));
    }
#pragma unroll
    for (int s = 0; s < C; ++s) g[s] = float(acc[s]);
  } else {
#pragma unroll
    for (int s = 0; s < C; ++s) g[s] = lerp_rn(float(xr[ax.first * C + s]), float(xr[ax.i1 * C + s]), ax.t);
  }
}

// after the vertical step: the column division, scale and shift, and the C stores of pixel px
template <int C, class P>
__device__ __forceinline__ void aa_store(const P& p, float* __restrict__ yi, int HW, int px, bool sx, int U, float (&w)[C]) {
  const float uf = float(U);
#pragma unroll
  for (int s = 0; s < C; ++s) {
    const float v = sx ? w[s] / uf : w[s];
    yi[size_t(p.plane[s]) * size_t(HW) + px] = norm_rn(v, p.scale[s], p.shift[s]);
  }
}

// g of NV12 source row r for resized column ox: the row above over converted pixels.  A run of column taps reads its
// Y bytes four taps at a time as one dword at the run's own alignment, and the two chroma pairs those four taps
// share -- three where the run starts on an odd column, the first and the last then serving one tap each.
__device__ __forceinline__ void aa_row(const SrcNv12& src, const ResizeGeom& d, int r, bool sx, const AaAxis& ax, int ox,
                                       float (&g)[3]) {
  const unsigned char* yr = src.y + size_t(r) * size_t(src.yrow);
  const unsigned char* ur = src.uv + size_t(r >> 1) * size_t(src.uvrow);
  if (sx) {
    int acc[3] = {0, 0, 0};
    const unsigned char* pp = yr + ax.first;
    const bool odd = (ax.first & 1) != 0;  // j steps by four: every group of the run starts on the same parity
    int j = 0;
    for (; j + 4 <= ax.n; j += 4) {
      unsigned yy;
      __builtin_memcpy(&yy, pp + j, 4);
      const int c0 = (ax.first + j) >> 1;
      const YuvChroma k0 = nv12_chroma(src.m, ur, c0), k1 = nv12_chroma(src.m, ur, c0 + 1);
      // tap t takes pair (odd + t) >> 1; the third pair exists where it is needed: tap 3 of an odd start is inside the row
      const YuvChroma k2 = odd ? nv12_chroma(src.m, ur, c0 + 2) : k1;
      const YuvChroma kt[4] = {k0, odd ? k1 : k0, k1, k2};
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int u = resize_aa_weight(d.Ws, d.Rw, ox, ax.first + j + t);
        int rgb[3];
        yuv_rgb(src.m, int((yy >> (8 * t)) & 0xffu), kt[t], rgb);
#pragma unroll
        for (int s = 0; s < 3; ++s) acc[s] += __mul24(u, rgb[s]);
      }
    }
    for (; j < ax.n; ++j) {
      const int u = resize_aa_weight(d.Ws, d.Rw, ox, ax.first + j);
      int rgb[3];
      nv12_pixel(src.m, yr, ur, ax.first + j, rgb);
#pragma unroll
      for (int s = 0; s < 3; ++s) acc[s] += __mul24(u, rgb[s]);
    }
#pragma unroll
    for (int s = 0; s < 3; ++s) g[s] = float(acc[s]);
  } else {
    int a[3], b[3];
    nv12_pixel(src.m, yr, ur, ax.first, a);
    nv12_pixel(src.m, yr, ur, ax.i1, b);
#pragma unroll
    for (int s = 0; s < 3; ++s) g[s] = lerp_rn(float(a[s]), float(b[s]), ax.t);
  }
}

__device__ __forceinline__ void yuv_tap(const YuvMatrix& m, const ResizeGeom& d, int ox, int col, int Y, const YuvChroma& k,
                                        int (&acc)[3]) {
  const int u = resize_aa_weight(d.Ws, d.Rw, ox, col);
  int rgb[3];
  yuv_rgb(m, Y, k, rgb);
#pragma unroll
  for (int s = 0; s < 3; ++s) acc[s] += __mul24(u, rgb[s]);
}

// The groups of four taps of a run over planes whose luma step is 1 (every format but YUYV), as the NV12 row does
// them: the four Y bytes as one dword at the run's own alignment, and each chroma sample those taps touch fetched
// and multiplied out once -- four samples under SX = 0; two under SX = 1, three where the run starts on an odd
// column; one under SX = 2, two where it does not start on a multiple of four; none for grey (SX = -1).  j steps
// by four, so every group of the run starts on the same phase.  Returns the taps done; the rest go one by one.
template <int F, int SX>
__device__ __forceinline__ int aa_run_planar(const YuvMatrix& m, const ResizeGeom& d, const YuvRow& w, const AaAxis& ax, int ox,
                                             int (&acc)[3]) {
  static_assert((F == YUV_GREY) == (SX < 0), "SX = -1 stands for no chroma");
  constexpr int S = SX < 0 ? 0 : SX;
  constexpr int NK = SX < 0 ? 1 : ((2 + (1 << S)) >> S) + 1;
  const int ph = ax.first & ((1 << S) - 1);
  int j = 0;
  for (; j + 4 <= ax.n; j += 4) {
    const int col = ax.first + j;
    unsigned yy;
    __builtin_memcpy(&yy, w.y + col, 4);
    YuvChroma k[NK];
    if constexpr (SX < 0) {
      k[0] = YuvChroma{0, 0, 0};
    } else {
      const int c0 = col >> S;
      k[0] = yuv_sample<F>(m, w, c0);
      // sample c0 + s exists where a tap of the group needs it: the last tap takes sample c0 + ((ph + 3) >> S)
#pragma unroll
      for (int s = 1; s < NK; ++s) k[s] = ((ph + 3) >> S) >= s ? yuv_sample<F>(m, w, c0 + s) : k[s - 1];
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      constexpr int last = NK - 1;
      const int lo = t >> S, hi = lo + 1 < last ? lo + 1 : last;  // tap t takes sample (ph + t) >> S: lo or the next
      const YuvChroma kt = ((ph + t) >> S) != lo ? k[hi] : k[lo < last ? lo : last];
      yuv_tap(m, d, ox, col + t, int((yy >> (8 * t)) & 0xffu), kt, acc);
    }
  }
  return j;
}

// The same groups of a YUYV row (luma step 2): row bytes are groups Y0 U Y1 V of two columns.  The two groups of
// four taps from an even column carry their four lumas and both chroma pairs: two dword loads and nothing else; from
// an odd column the taps reach into a third group, which is inside the row because its first column is a tap.
__device__ __forceinline__ int aa_run_yuyv(const YuvMatrix& m, const ResizeGeom& d, const YuvRow& w, const AaAxis& ax, int ox,
                                           int (&acc)[3]) {
  const bool odd = (ax.first & 1) != 0;
  int j = 0;
  for (; j + 4 <= ax.n; j += 4) {
    const int col = ax.first + j;
    const unsigned char* gp = w.y + 4 * (col >> 1);
    unsigned g0, g1, g2;
    __builtin_memcpy(&g0, gp, 4);
    __builtin_memcpy(&g1, gp + 4, 4);
    g2 = g1;
    if (odd) __builtin_memcpy(&g2, gp + 8, 4);
    const YuvChroma k0 = yuv_chroma(m, int((g0 >> 8) & 0xffu), int(g0 >> 24));
    const YuvChroma k1 = yuv_chroma(m, int((g1 >> 8) & 0xffu), int(g1 >> 24));
    const YuvChroma k2 = odd ? yuv_chroma(m, int((g2 >> 8) & 0xffu), int(g2 >> 24)) : k1;
    const YuvChroma kt[4] = {k0, odd ? k1 : k0, k1, k2};
    const unsigned yt[4] = {odd ? g0 >> 16 : g0, odd ? g1 : g0 >> 16, odd ? g1 >> 16 : g1, odd ? g2 : g1 >> 16};
#pragma unroll
    for (int t = 0; t < 4; ++t) yuv_tap(m, d, ox, col + t, int(yt[t] & 0xffu), kt[t], acc);
  }
  return j;
}

// g of source row r for resized column ox under one way to fetch and, for planes, one horizontal chroma shift
template <int SX, int F>
__device__ __forceinline__ void aa_row_yuv_as(const SrcYuv<F>& src, const ResizeGeom& d, int r, bool sx, const AaAxis& ax, int ox,
                                              float (&g)[3]) {
  const YuvRow w = src.at(r);
  if (sx) {
    int acc[3] = {0, 0, 0};
    int j;
    if constexpr (F == YUV_PACKED)
      j = aa_run_yuyv(src.m, d, w, ax, ox, acc);
    else
      j = aa_run_planar<F, SX>(src.m, d, w, ax, ox, acc);
    for (; j < ax.n; ++j) {
      const int u = resize_aa_weight(d.Ws, d.Rw, ox, ax.first + j);
      int rgb[3];
      src.px(w, ax.first + j, rgb);
#pragma unroll
      for (int s = 0; s < 3; ++s) acc[s] += __mul24(u, rgb[s]);
    }
#pragma unroll
    for (int s = 0; s < 3; ++s) g[s] = float(acc[s]);
  } else {
    int a[3], b[3];
    src.px(w, ax.first, a);
    src.px(w, ax.i1, b);
#pragma unroll
    for (int s = 0; s < 3; ++s) g[s] = lerp_rn(float(a[s]), float(b[s]), ax.t);
  }
}

// g of YUV source row r: the row above over converted pixels, by the chroma shift of the source's way to fetch
template <int F>
__device__ __forceinline__ void aa_row(const SrcYuv<F>& src, const ResizeGeom& d, int r, bool sx, const AaAxis& ax, int ox,
                                       float (&g)[3]) {
  if constexpr (F == YUV_GREY)
    aa_row_yuv_as<-1>(src, d, r, sx, ax, ox, g);
  else if constexpr (F != YUV_PLANES)
    aa_row_yuv_as<1>(src, d, r, sx, ax, ox, g);  // YUYV, and pairs are NV12: sx = 1
  else if (src.d.sx == 0)
    aa_row_yuv_as<0>(src, d, r, sx, ax, ox, g);
  else if (src.d.sx == 1)
    aa_row_yuv_as<1>(src, d, r, sx, ax, ox, g);
  else
    aa_row_yuv_as<2>(src, d, r, sx, ax, ox, g);
}

// output pixel px of an image from global memory: row r and column q of the window (not px's row and column where a
// list descriptor is flipped or oriented)
template <int C, class Src, class P>
__device__ __forceinline__ void aa_pixel(const Src& src, const ResizeGeom& d, const P& p, float* __restrict__ yi, int HW, int px,
                                         int r, int q) {
  const bool sx = d.Ws > d.Rw, sy = d.Hs > d.Rh;
  const int oy = d.top + r, ox = d.left + q;
  const AaAxis ax = aa_axis(sx, d.Ws, d.Rw, ox);
  const AaAxis ay = aa_axis(sy, d.Hs, d.Rh, oy);
  const auto row = [&](int sr, float (&g)[C]) {  // a YUV descriptor's way to fetch is chosen here, per tap row
    yuv_fetch_as(src, [&](const auto& s) { aa_row(s, d, sr, sx, ax, ox, g); });
  };
  float w[C];
  if (sy) {
#pragma unroll
    for (int s = 0; s < C; ++s) w[s] = 0.f;
    for (int i = 0; i < ay.n; ++i) {
      float g[C];
      row(ay.first + i, g);
      const float v = float(resize_aa_weight(d.Hs, d.Rh, oy, ay.first + i));
#pragma unroll
      for (int s = 0; s < C; ++s) w[s] = macc_rn(w[s], v, g[s]);
    }
    const float vf = float(ay.sum);
#pragma unroll
    for (int s = 0; s < C; ++s) w[s] = w[s] / vf;
  } else {
    float g0[C], g1[C];
    row(ay.first, g0);
    row(ay.i1, g1);
#pragma unroll
    for (int s = 0; s < C; ++s) w[s] = lerp_rn(g0[s], g1[s], ay.t);
  }
  aa_store<C>(p, yi, HW, px, sx, ax.sum, w);
}

// ---------------------------------------------------------------------------------------------------------
// ORE_FILTER_BICUBIC and ORE_FILTER_BICUBIC_AA (include/ore.h has the arithmetic, ore_resize_geom.h the taps and
// weights): float weights, every operation rounded on its own, no integer sums -- so nothing of the triangle
// filter's run code above applies, and a source's at, px and px4 are all they read.  One thread per output pixel.
//
// The antialiased filter's column weights are the same for every tap row of a pixel: they are computed once per
// pixel into LDS, laid out [tap][thread] (stride 1 in the thread index: conflict-free; a thread reads only what it
// wrote, so there is no barrier), while the row weight costs one division and one cubic per tap row.  The launch
// sizes the LDS to the longest run its geometry can have (resize_cubic_aa_max_taps); workgroups are 128 threads so
// that 64 taps are 32 KB.  DESIGN.md 3.8g has the variants measured.

constexpr int CUBIC_AA_THREADS = 128;

__device__ __forceinline__ float mul_rn(float a, float b) {
#pragma clang fp contract(off)
  return a * b;
}

__device__ __forceinline__ float add_rn(float a, float b) {
#pragma clang fp contract(off)
  return a + b;
}

// ORE_FILTER_BICUBIC: 4 x 4 taps, the border replicated; the tap columns are clamped once, outside the rows
template <int C, class Src, class P>
__device__ __forceinline__ void cubic_pixel(const Src& src, const ResizeGeom& g, const P& p, float* __restrict__ yi, int HW,
                                            int px, int r, int q) {
  const ResizeCubicTap ty = resize_cubic_tap(g.Hs, g.Rh, g.top + r);
  const ResizeCubicTap tx = resize_cubic_tap(g.Ws, g.Rw, g.left + q);
  int cj[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) cj[j] = resize_clamp(tx.first + j, g.Ws);
  float v[C];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const typename Src::Row w = src.at(resize_clamp(ty.first + k, g.Hs));
    float gk[C];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      int x[C];
      src.px(w, cj[j], x);
#pragma unroll
      for (int s = 0; s < C; ++s) gk[s] = j == 0 ? mul_rn(tx.w[0], float(x[s])) : macc_rn(gk[s], tx.w[j], float(x[s]));
    }
#pragma unroll
    for (int s = 0; s < C; ++s) v[s] = k == 0 ? mul_rn(ty.w[0], gk[s]) : macc_rn(v[s], ty.w[k], gk[s]);
  }
#pragma unroll
  for (int s = 0; s < C; ++s) yi[size_t(p.plane[s]) * size_t(HW) + px] = norm_rn(v[s], p.scale[s], p.shift[s]);
}

// ORE_FILTER_BICUBIC_AA: u is this thread's column of the LDS weight table, tap j at u[j * CUBIC_AA_THREADS]
template <int C, class Src, class P>
__device__ __forceinline__ void cubic_aa_pixel(const Src& src, const ResizeGeom& g, const P& p, float* __restrict__ yi, int HW,
                                               int px, int r, int q, float* __restrict__ u) {
  const int oy = g.top + r, ox = g.left + q;
  const ResizeCubicSpan sx = resize_cubic_aa_span(g.Ws, g.Rw, ox);
  const ResizeCubicSpan sy = resize_cubic_aa_span(g.Hs, g.Rh, oy);
  float U = 0.f;
  for (int j = 0; j < sx.n; ++j) {
    const float w = resize_cubic_aa_weight(g.Ws, g.Rw, ox, sx.first + j);
    u[j * CUBIC_AA_THREADS] = w;
    U = add_rn(U, w);
  }
  float acc[C];
#pragma unroll
  for (int s = 0; s < C; ++s) acc[s] = 0.f;
  float V = 0.f;
  for (int i = 0; i < sy.n; ++i) {
    const typename Src::Row w = src.at(sy.first + i);
    const float v = resize_cubic_aa_weight(g.Hs, g.Rh, oy, sy.first + i);
    V = add_rn(V, v);
    float gs[C];
#pragma unroll
    for (int s = 0; s < C; ++s) gs[s] = 0.f;
    int j = 0;
    for (; j + 4 <= sx.n; j += 4) {  // four taps' fetches issue together; the sums stay in ascending order
      int x[4][C];
      src.px4(w, sx.first + j, x);
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const float uj = u[(j + t) * CUBIC_AA_THREADS];
#pragma unroll
        for (int s = 0; s < C; ++s) gs[s] = macc_rn(gs[s], uj, float(x[t][s]));
      }
    }
    for (; j < sx.n; ++j) {
      int x[C];
      src.px(w, sx.first + j, x);
      const float uj = u[j * CUBIC_AA_THREADS];
#pragma unroll
      for (int s = 0; s < C; ++s) gs[s] = macc_rn(gs[s], uj, float(x[s]));
    }
#pragma unroll
    for (int s = 0; s < C; ++s) acc[s] = macc_rn(acc[s], v, gs[s]);
  }
#pragma unroll
  for (int s = 0; s < C; ++s) {
    const float t = acc[s] / V;
    yi[size_t(p.plane[s]) * size_t(HW) + px] = norm_rn(t / U, p.scale[s], p.shift[s]);
  }
}

// ---------------------------------------------------------------------------------------------------------
// The kernels.  FILTER is an ore_resize_filter; it selects the body and with it the workgroup's size.

constexpr int filter_threads(int filter) { return filter == ORE_FILTER_BICUBIC_AA ? CUBIC_AA_THREADS : RS_THREADS; }

// output pixel px under FILTER: row r and column q of the window of src, channel s stored at yo[p.plane[s] * HW + px];
// u as in cubic_aa_pixel.  The way to fetch a YUV descriptor selects is chosen where 3.8f measured it for each filter:
// around the whole pixel for the cubic bodies (here), around the four fetches in bilinear_pixel, per tap row in aa_pixel.
template <int FILTER, int C, class Src, class P>
__device__ __forceinline__ void filter_pixel(const Src& src, const ResizeGeom& g, const P& p, float* yo, int HW, int px, int r,
                                             int q, float* u) {
  if constexpr (FILTER == ORE_FILTER_BILINEAR_AA)
    aa_pixel<C>(src, g, p, yo, HW, px, r, q);
  else if constexpr (FILTER == ORE_FILTER_BILINEAR)
    bilinear_pixel<C>(src, g, p, yo + px, HW, r, q);
  else
    yuv_fetch_as(src, [&](const auto& s) {
      if constexpr (FILTER == ORE_FILTER_BICUBIC_AA)
        cubic_aa_pixel<C>(s, g, p, yo, HW, px, r, q, u);
      else
        cubic_pixel<C>(s, g, p, yo, HW, px, r, q);
    });
}

// the dense batch under every filter but the plain one (resize_u8_generic_kernel, whose taps stay outside the image loop)
template <int FILTER, int C>
__global__ __launch_bounds__(filter_threads(FILTER)) void resize_dense_kernel(ResizeParams p) {
  extern __shared__ float cubic_lds[];
  const int px = blockIdx.x * filter_threads(FILTER) + threadIdx.x;
  const int HW = p.H * p.W;
  if (px >= HW) return;
  const int r = px / p.W, q = px - r * p.W;
  const ResizeGeom g = resize_geom(p);
  for (long long i = blockIdx.y; i < p.N; i += gridDim.y)
    filter_pixel<FILTER, C>(src_of<C>(p, i), g, p, p.y + size_t(i) * size_t(p.y_nstride), HW, px, r, q, cubic_lds + threadIdx.x);
}

// the list of descriptors D under parameters P (interleaved bytes: C = 1..4, or 0 under the plain filter, which takes
// p.C at run time; NV12 and YUV frames: C = 3)
template <int FILTER, int C, int MODE, class D, class P>
__global__ __launch_bounds__(filter_threads(FILTER)) void resize_list_kernel(const D* __restrict__ table, P p) {
  extern __shared__ float cubic_lds[];
  int channels = C;
  if constexpr (C == 0) channels = p.C;
  list_pixels<filter_threads(FILTER), MODE>(table, p, channels, [&](const D& d, const P& pp, float* yo, int hw, int px, int r, int q) {
    if constexpr (C == 0)
      bilinear_u8_pixel(d, pp, yo + px, hw, r, q);
    else
      filter_pixel<FILTER, C>(src_of<C>(d, pp), resize_geom(d), pp, yo, hw, px, r, q, cubic_lds + threadIdx.x);
  });
}

// ---------------------------------------------------------------------------------------------------------
// The launches.

// blocks of T threads for an H x W output: one per T pixels, or under LIST_ORIENT one per tile of T / 16 rows x 16 columns
inline dim3 list_grid(int H, int W, long long N, int T, int mode = LIST_PLAIN) {
  const unsigned gy = unsigned(N < 65535 ? N : 65535);
  if (mode == LIST_ORIENT) return dim3(unsigned(((H + T / TILE_W - 1) / (T / TILE_W)) * ((W + TILE_W - 1) / TILE_W)), gy);
  return dim3(unsigned(((long long)H * W + T - 1) / T), gy);
}

// the antialiased cubic filter's weight table: `taps` bounds its column runs; the other filters take no dynamic LDS
inline size_t filter_lds(int filter, int taps) {
  return filter == ORE_FILTER_BICUBIC_AA ? size_t(taps) * CUBIC_AA_THREADS * sizeof(float) : 0;
}

template <int V>
using Int = std::integral_constant<int, V>;

// f(Int<FILTER>) for an ore_resize_filter the caller's checks have seen, f(Int<C>) for a channel count 1..4
template <class F>
void with_filter(int32_t filter, F&& f) {
  if (filter & ORE_FILTER_CUBIC_BIT)
    filter == ORE_FILTER_BICUBIC_AA ? f(Int<ORE_FILTER_BICUBIC_AA>{}) : f(Int<ORE_FILTER_BICUBIC>{});
  else
    filter == ORE_FILTER_BILINEAR_AA ? f(Int<ORE_FILTER_BILINEAR_AA>{}) : f(Int<ORE_FILTER_BILINEAR>{});
}

template <class F>
void with_channels(int C, F&& f) {
  switch (C) {
    case 1: return f(Int<1>{});
    case 2: return f(Int<2>{});
    case 3: return f(Int<3>{});
    default: return f(Int<4>{});
  }
}

// One list launch: the instance for p.flips (a ListMode), its grid, and the LDS sized by p.taps: the longest column
// run of the list's last set, or, where a captured launch may meet the descriptors of a later set, the longest the
// ratio rule allows.
template <int FILTER, int C, class D, class P>
void list_launch(const D* table, const P& p, hipStream_t s) {
  constexpr int T = filter_threads(FILTER);
  const auto k = p.flips == LIST_ORIENT ? resize_list_kernel<FILTER, C, LIST_ORIENT, D, P>
                 : p.flips              ? resize_list_kernel<FILTER, C, LIST_FLIP, D, P>
                                        : resize_list_kernel<FILTER, C, LIST_PLAIN, D, P>;
  hipLaunchKernelGGL(k, list_grid(p.H, p.W, p.N, T, p.flips), dim3(T), filter_lds(FILTER, p.taps), s, table, p);
}

template <class P>
void resize_list(const P& p, int32_t filter, hipStream_t s) {
  if (p.N <= 0 || p.H <= 0 || p.W <= 0) return;
  with_filter(filter, [&](auto f) {
    constexpr int FILTER = decltype(f)::value;
    if constexpr (!std::is_same_v<P, ResizeListParams>)
      list_launch<FILTER, 3>(p.table + p.first, p, s);
    else if constexpr (FILTER == ORE_FILTER_BILINEAR)
      list_launch<FILTER, 0>(p.table + p.first, p, s);  // one instance for every channel count
    else
      with_channels(p.C, [&](auto c) { list_launch<FILTER, decltype(c)::value>(p.table + p.first, p, s); });
  });
}

}  // namespace

void launch_resize_list(const ResizeListParams& p, int32_t filter, hipStream_t s) { resize_list(p, filter, s); }
void launch_resize_list(const Nv12ListParams& p, int32_t filter, hipStream_t s) { resize_list(p, filter, s); }
void launch_resize_list(const YuvListParams& p, int32_t filter, hipStream_t s) { resize_list(p, filter, s); }

void launch_resize_dense(const ResizeParams& p, int32_t filter, hipStream_t s) {
  if (p.N <= 0 || p.H <= 0 || p.W <= 0) return;
  if (filter == ORE_FILTER_BILINEAR_AA && p.Hs <= p.Rh && p.Ws <= p.Rw) filter = ORE_FILTER_BILINEAR;  // nothing shrinks: the plain filter, bit for bit
  with_filter(filter, [&](auto f) {
    constexpr int FILTER = decltype(f)::value;
    if constexpr (FILTER == ORE_FILTER_BILINEAR) {
      hipLaunchKernelGGL(resize_u8_generic_kernel, list_grid(p.H, p.W, p.N, RS_THREADS), dim3(RS_THREADS), 0, s, p);
    } else {
      constexpr int T = filter_threads(FILTER);
      const size_t lds = FILTER == ORE_FILTER_BICUBIC_AA ? filter_lds(FILTER, resize_cubic_aa_max_taps(p.Ws, p.Rw)) : 0;
      with_channels(p.C, [&](auto c) {
        hipLaunchKernelGGL((resize_dense_kernel<FILTER, decltype(c)::value>), list_grid(p.H, p.W, p.N, T), dim3(T), lds, s, p);
      });
    }
  });
}

}  // namespace ore
