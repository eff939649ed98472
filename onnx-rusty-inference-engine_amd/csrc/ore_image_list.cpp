// C ABI of the image lists (include/ore.h): the descriptor checks, the lists and their set entries, and the list
// conversion's launch, for the three descriptor formats -- interleaved uint8 images, NV12 frames, YUV frames.
// What a format has of its own is its ListFormat below and its launch_resize_list overload (ore_resize.hip);
// the rule chain (check_list), the set (list_set) and the launch (launch_list) are written once over it.
#include <algorithm>

#include "ore_internal.h"
#include "ore_resize_geom.h"

namespace ore {

// An EXIF orientation code 1..8 as the three permutation bits of ore_orient_geometry; false: not a code
static bool orient_bits(int code, bool* rev_rows, bool* rev_cols, bool* transpose) {
  if (code < 1 || code > 8) return false;
  *rev_rows = code == 3 || code == 4 || code == 6 || code == 7;
  *rev_cols = code == 2 || code == 3 || code == 7 || code == 8;
  *transpose = code >= 5;
  return true;
}

// the descriptor's geometry and the list's output shape in stored space (include/ore.h: ore_orient_geometry);
// returns the LIST_* bits of the kernels' descriptor word
static int orient_stored(int code, const ore_resize& g, int64_t h, int64_t w, ore_resize* sg, int64_t* hz, int64_t* wz) {
  bool rr = false, rc = false, tr = false;
  orient_bits(code, &rr, &rc, &tr);
  *hz = tr ? w : h;
  *wz = tr ? h : w;
  sg->rh = tr ? g.rw : g.rh;
  sg->rw = tr ? g.rh : g.rw;
  const int64_t a0 = tr ? g.left : g.top, b0 = tr ? g.top : g.left;
  sg->top = rr ? sg->rh - *hz - a0 : a0;
  sg->left = rc ? sg->rw - *wz - b0 : b0;
  return (rr ? LIST_REV_ROWS : 0) | (rc ? LIST_REV_COLS : 0) | (tr ? LIST_TRANSPOSE : 0);
}

// What an ore_yuv_format is, for ore_image_check_yuv and for ore_image_list_set_yuv's reduction to strided planes
// (YuvImage): the planes in use, the chroma shifts, and the bytes between the luma and the chroma samples of a row.
struct YuvLayout {
  const char* name;
  int planes;  // plane[0 .. planes) are in use
  int sx, sy;
  int ystep, cstep;
};

static const YuvLayout* yuv_layout(int32_t format) {
  static const YuvLayout table[] = {
      {"NV12", 2, 1, 1, 1, 2}, {"YUYV", 1, 1, 0, 2, 4}, {"I444", 3, 0, 0, 1, 1}, {"I440", 3, 0, 1, 1, 1},
      {"I422", 3, 1, 0, 1, 1}, {"I420", 3, 1, 1, 1, 1}, {"I411", 3, 2, 0, 1, 1}, {"GRAY", 1, 0, 0, 1, 0},
  };
  return format >= 0 && format < int32_t(sizeof(table) / sizeof(table[0])) ? &table[format] : nullptr;
}

// rows of plane k of an hs x ws frame, and the bytes of one
static long long yuv_plane_rows(const YuvLayout& f, int k, long long hs) { return k == 0 ? hs : (hs + (1 << f.sy) - 1) >> f.sy; }
static long long yuv_plane_row_bytes(const YuvLayout& f, int k, long long ws) {
  if (k == 0) return f.ystep == 2 ? 4 * ((ws + 1) / 2) : ws;
  return ((ws + (1 << f.sx) - 1) >> f.sx) * f.cstep;
}

// ---------------------------------------------------------------- the three formats
// A ListFormat is what one descriptor format has of its own; a new format is one more of these, a launch_resize_list
// overload for its parameter block, and its thin entries at the end of this file.
//   Desc, Image   the ABI's descriptor and the kernels' packed one (Hs .. flip under the same names in all)
//   format        the ore_image_format of its lists; list_formats[] has how messages call it
//   pointers      the rules between the orientation code and the size range: pointers, format words
//   planes        the planes of a descriptor that passed those: rows, bytes of a row, stride (0: dense)
//   below, reach  the two messages of a plane: its stride is below its row; its rows reach past 2^31 bytes
//   fill          Image's own fields (pointers, pitches, steps, shifts) from a checked descriptor
struct Plane {
  long long rows, row_bytes, stride;
  long long pitch() const { return rows > 1 && stride ? stride : row_bytes; }  // dense where 0, and where no row is ever stepped
};
static const struct { const char* kind; const char* entry; } list_formats[] = {
    {"a list of interleaved images", "ore_image_list_set"}, {"an NV12 list", "ore_image_list_set_nv12"}, {"a YUV list", "ore_image_list_set_yuv"}};

struct U8Format {
  using Desc = ore_image_u8;
  using Image = ResizeImage;
  static constexpr int32_t format = ORE_IMAGE_INTERLEAVED;
  static ore_status pointers(long long i, const Desc& d) {
    return d.data ? ORE_OK : set_error(nullptr, ORE_ERR_INVALID, "image %lld: null data pointer", i);
  }
  static int planes(const Desc& d, int64_t c, Plane p[3]) {
    p[0] = {d.hs, d.ws * c, d.row_stride};
    return 1;
  }
  static ore_status below(long long i, int, const Plane& p) {
    return set_error(nullptr, ORE_ERR_INVALID, "image %lld: row stride %lld below ws*c = %lld", i, p.stride, p.row_bytes);
  }
  static ore_status reach(long long i, int, const Plane& p) {
    return set_error(nullptr, ORE_ERR_INVALID, "image %lld: %lld rows at a stride of %lld bytes reach past 2^31 bytes", i, p.rows, p.stride);
  }
  static void fill(const Desc& d, int64_t c, Image* r) {
    Plane p[3];
    planes(d, c, p);
    r->x = d.data;
    r->row = int(p[0].pitch());
  }
};

struct Nv12Format {
  using Desc = ore_image_nv12;
  using Image = Nv12Image;
  static constexpr int32_t format = ORE_IMAGE_NV12;
  static ore_status pointers(long long i, const Desc& d) {
    return d.y && d.uv ? ORE_OK : set_error(nullptr, ORE_ERR_INVALID, "image %lld: null %s pointer", i, d.y ? "uv" : "y");
  }
  static int planes(const Desc& d, int64_t, Plane p[3]) {
    p[0] = {d.hs, d.ws, d.y_stride};
    p[1] = {(d.hs + 1) / 2, 2 * ((d.ws + 1) / 2), d.uv_stride};  // UV rows, and the bytes of one
    return 2;
  }
  static ore_status below(long long i, int k, const Plane& p) {
    return set_error(nullptr, ORE_ERR_INVALID, k ? "image %lld: uv stride %lld below 2*ceil(ws/2) = %lld" : "image %lld: y stride %lld below ws = %lld",
                     i, p.stride, p.row_bytes);
  }
  static ore_status reach(long long i, int k, const Plane& p) {
    return set_error(nullptr, ORE_ERR_INVALID, "image %lld: %lld %s rows at a stride of %lld bytes reach past 2^31 bytes", i, p.rows,
                     k ? "uv" : "y", p.stride);
  }
  static void fill(const Desc& d, int64_t c, Image* r) {
    Plane p[3];
    planes(d, c, p);
    r->y = d.y; r->uv = d.uv;
    r->yrow = int(p[0].pitch());
    r->uvrow = int(p[1].pitch());
  }
};

static_assert(sizeof(ore_image_yuv) == 104, "ore_image_yuv is part of the ABI");
static_assert(sizeof(YuvImage) == 80 && sizeof(YuvImage) % 8 == 0, "the pointers of a YuvImage table stay aligned");

struct YuvFormat {
  using Desc = ore_image_yuv;
  using Image = YuvImage;
  static constexpr int32_t format = ORE_IMAGE_YUV;
  static ore_status pointers(long long i, const Desc& d) {
    const YuvLayout* f = yuv_layout(d.format);
    if (!f) return set_error(nullptr, ORE_ERR_INVALID, "image %lld: unknown YUV format %d", i, int(d.format));
    if (d.reserved != 0) return set_error(nullptr, ORE_ERR_INVALID, "image %lld: reserved is %d, it must be 0", i, int(d.reserved));
    for (int k = 0; k < 3; ++k) {
      if (k < f->planes && !d.plane[k])
        return set_error(nullptr, ORE_ERR_INVALID, "image %lld: null plane %d pointer (%s has %d)", i, k, f->name, f->planes);
      if (k >= f->planes && d.plane[k])
        return set_error(nullptr, ORE_ERR_INVALID, "image %lld: plane %d must be null (%s has %d)", i, k, f->name, f->planes);
    }
    return ORE_OK;
  }
  static int planes(const Desc& d, int64_t, Plane p[3]) {
    const YuvLayout& f = *yuv_layout(d.format);  // checked
    for (int k = 0; k < f.planes; ++k) p[k] = {yuv_plane_rows(f, k, d.hs), yuv_plane_row_bytes(f, k, d.ws), d.stride[k]};
    return f.planes;
  }
  static ore_status below(long long i, int k, const Plane& p) {
    return set_error(nullptr, ORE_ERR_INVALID, "image %lld: plane %d stride %lld below its %lld row bytes", i, k, p.stride, p.row_bytes);
  }
  static ore_status reach(long long i, int k, const Plane& p) {
    return set_error(nullptr, ORE_ERR_INVALID, "image %lld: plane %d: %lld rows at a stride of %lld bytes reach past 2^31 bytes", i, k,
                     p.rows, p.stride);
  }
  // the format ends here: the kernels see three strided planes
  static void fill(const Desc& d, int64_t c, Image* r) {
    const YuvLayout& f = *yuv_layout(d.format);  // checked
    Plane p[3];
    const int n = planes(d, c, p);
    r->y = d.plane[0];
    r->yrow = int(p[0].pitch());
    if (f.ystep == 2) {  // YUYV: U and V inside the luma plane's groups
      r->u = d.plane[0] + 1; r->v = d.plane[0] + 3;
      r->urow = r->vrow = r->yrow;
    } else if (n == 2) {  // NV12: V one byte after U
      r->u = d.plane[1]; r->v = d.plane[1] + 1;
      r->urow = r->vrow = int(p[1].pitch());
    } else if (n == 3) {
      r->u = d.plane[1]; r->v = d.plane[2];
      r->urow = int(p[1].pitch()); r->vrow = int(p[2].pitch());
    }  // grey: no chroma, u and v stay null
    r->ystep = f.ystep; r->cstep = f.cstep;
    r->sx = f.sx; r->sy = f.sy;
  }
};

// ---------------------------------------------------------------- one check
// The rule chain of the three ore_image_check*_oriented entries.  Of the call: filter, count, output shape (c = 3 of
// the frame formats), imgs.  Of each descriptor, in this order: its orientation code, F::pointers, the size range,
// the crop window, every plane's stride against its row, every plane's reach, the antialiasing ratio.  A descriptor
// is judged in stored space: its geometry and the output shape as orient_stored gives them.  The crop rule there is
// the displayed-space rule (top_s + hz <= rh_s is top + h <= rh or left + w <= rw).
template <class F>
static ore_status check_descriptor(const typename F::Desc& d, long long i, int64_t c, int64_t h, int64_t w, int32_t filter, const uint8_t* code) {
  if (code && (*code < 1 || *code > 8))  // null orientations are all 1; a bad code: the descriptor's geometry is not looked at
    return set_error(nullptr, ORE_ERR_INVALID, "image %lld: orientation %d is not an EXIF code 1..8", i, int(*code));
  ore_resize g = d.g;
  if (code) orient_stored(*code, d.g, h, w, &g, &h, &w);
  if (ore_status st = F::pointers(i, d)) return st;
  if (ore_status st = check_resize_window(nullptr, i, d.hs, d.ws, h, w, g)) return st;
  Plane p[3];
  const int n = F::planes(d, c, p);
  for (int k = 0; k < n; ++k)
    if (p[k].stride != 0 && p[k].stride < p[k].row_bytes) return F::below(i, k, p[k]);
  for (int k = 0; k < n; ++k)  // a one-row plane never steps a row
    if (p[k].rows > 1 && (!fits_i32(p[k].stride) || !fits_i32((p[k].rows - 1) * p[k].pitch() + p[k].row_bytes))) return F::reach(i, k, p[k]);
  return check_resize_ratio(nullptr, i, filter, d.hs, d.ws, g);
}

template <class F>
static ore_status check_list(const typename F::Desc* imgs, int64_t n, int64_t c, int64_t h, int64_t w, int32_t filter,
                             const uint8_t* orientations, int64_t* bad_index) {
  if (!filter_known(filter))
    return set_error(nullptr, ORE_ERR_INVALID, "unknown resize filter %d", int(filter));
  if (n < 0) return set_error(nullptr, ORE_ERR_INVALID, "negative image count %lld", (long long)n);
  PreprocParams q;  // c and the output size: the direct conversion's checks
  if (ore_status st = preproc_params(nullptr, h, w, c, nullptr, nullptr, 0, &q)) return st;
  if (n == 0) return ORE_OK;
  if (!imgs) return set_error(nullptr, ORE_ERR_INVALID, "null argument");
  for (int64_t i = 0; i < n; ++i)
    if (ore_status st = check_descriptor<F>(imgs[i], i, c, h, w, filter, orientations ? orientations + i : nullptr)) {
      if (bad_index) *bad_index = i;
      return st;
    }
  return ORE_OK;
}

// ---------------------------------------------------------------- the lists
// ore_image_list_create_ex, _create_nv12 and _create_yuv: the list and the table and mirror of its format
static ore_status list_create(ore_ctx* ctx, int64_t capacity, int64_t c, int64_t h, int64_t w, int32_t filter, int32_t format,
                              int32_t matrix, ore_image_list** out) {
  if (!ctx || !out) return set_error(ctx, ORE_ERR_INVALID, "null argument");
  if (!filter_known(filter))
    return set_error(ctx, ORE_ERR_INVALID, "unknown resize filter %d", int(filter));
  YuvMatrix ym;
  if (format != ORE_IMAGE_INTERLEAVED && !yuv_matrix(matrix, &ym))
    return set_error(ctx, ORE_ERR_INVALID, "unknown YUV matrix %d", int(matrix));
  PreprocParams q;
  if (ore_status st = preproc_params(ctx, h, w, c, nullptr, nullptr, 0, &q)) return st;
  if (capacity < 1 || !fits_i32(capacity))
    return set_error(ctx, ORE_ERR_INVALID, "image list capacity %lld (1..2^31-1)", (long long)capacity);
  ORE_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  ore_image_list* l = new ore_image_list();
  l->ctx = ctx;
  l->capacity = capacity;
  l->c = c; l->h = h; l->w = w;
  l->filter = filter;
  l->format = format;
  l->matrix = format != ORE_IMAGE_INTERLEAVED ? matrix : 0;
  l->desc_bytes = format == ORE_IMAGE_YUV ? sizeof(YuvImage) : format == ORE_IMAGE_NV12 ? sizeof(Nv12Image) : sizeof(ResizeImage);
  const size_t bytes = size_t(capacity) * l->desc_bytes;
  // the table holds device addresses and geometry: never filled (device_alloc, own = false)
  if (device_alloc(ctx, &l->table, bytes, false) != hipSuccess || hipHostMalloc(&l->mirror, bytes, hipHostMallocDefault) != hipSuccess ||
      hipEventCreateWithFlags(&l->uploaded, hipEventDisableTiming) != hipSuccess) {
    (void)hipGetLastError();
    (void)ore_image_list_destroy(l);
    return set_error(ctx, ORE_ERR_OOM, "image list of %lld descriptors (%zu bytes) allocation failed", (long long)capacity, bytes);
  }
  *out = l;
  return ORE_OK;
}

// A set between the descriptors' check and the mirror's rewrite: the capacity, the capture rule, and the
// wait for the previous upload to have read the mirror.  n == 0 empties the list here.
static ore_status list_set_begin(ore_image_list* l, int64_t n) {
  ore_ctx* ctx = l->ctx;
  if (n > l->capacity)
    return set_error(ctx, ORE_ERR_INVALID, "%lld images exceed the list's capacity %lld", (long long)n, (long long)l->capacity);
  ORE_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  if (ctx->stream && hipStreamIsCapturing(ctx->stream, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone)
    return set_error(ctx, ORE_ERR_INVALID, "ore_image_list_set inside a stream capture: a captured graph reads the table at "
                                           "replay, set it before or after the capture");
  if (n == 0) {
    l->count = 0;
    return ORE_OK;
  }
  ORE_HIP_CHECK(ctx, hipEventSynchronize(l->uploaded));  // the previous upload has read the mirror
  return ORE_OK;
}

// the per-descriptor flag words of the _ex sets (null: all zero): ORE_IMAGE_FLIP_H is the only bit
static ore_status list_check_flags(ore_ctx* ctx, const uint32_t* flags, int64_t n) {
  for (int64_t i = 0; flags && i < n; ++i)
    if (flags[i] & ~uint32_t(ORE_IMAGE_FLIP_H))
      return set_error(ctx, ORE_ERR_INVALID, "image %lld: unknown flag bits 0x%x (ORE_IMAGE_FLIP_H is the only one)", (long long)i,
                       unsigned(flags[i] & ~uint32_t(ORE_IMAGE_FLIP_H)));
  return ORE_OK;
}

// ---------------------------------------------------------------- one set
// Every set entry: the descriptors checked and packed into the mirror (F::fill, then the geometry and the flip word
// all formats share), and the mirror uploaded.  A rejected set leaves the list as it was.
template <class F>
static ore_status list_set(ore_image_list* l, const typename F::Desc* imgs, const uint32_t* flags, const uint8_t* orientations, int64_t n,
                           bool oriented_entry) {
  if (!l) return set_error(nullptr, ORE_ERR_INVALID, "null image list");
  ore_ctx* ctx = l->ctx;
  if (l->format != F::format)
    return set_error(ctx, ORE_ERR_INVALID, "%s on %s: %s is its entry", list_formats[F::format].entry, list_formats[l->format].kind,
                     list_formats[l->format].entry);
  int64_t bad = -1;
  if (check_list<F>(imgs, n, l->c, l->h, l->w, l->filter, orientations, &bad)) {
    ctx->err = ore_last_error(nullptr);
    return ORE_ERR_INVALID;
  }
  if (ore_status st = list_check_flags(ctx, flags, n)) return st;
  if (ore_status st = list_set_begin(l, n)) return st;
  if (oriented_entry) l->oriented = true;  // for good: captures of the list record the orientation-reading kernels
  if (n == 0) return ORE_OK;
  bool any_flip = false, any_orient = false;
  int taps = 0;
  typename F::Image* mirror = static_cast<typename F::Image*>(l->mirror);
  for (int64_t i = 0; i < n; ++i) {
    const typename F::Desc& d = imgs[i];
    typename F::Image& r = mirror[i];
    r = typename F::Image{};
    F::fill(d, l->c, &r);
    r.Hs = int(d.hs); r.Ws = int(d.ws);
    ore_resize g = d.g;  // an oriented descriptor carries the stored image's geometry and the permutation bits
    int64_t hz, wz;
    const int bits = orientations ? orient_stored(orientations[i], d.g, l->h, l->w, &g, &hz, &wz) : 0;
    r.Rh = int(g.rh); r.Rw = int(g.rw); r.top = int(g.top); r.left = int(g.left);
    r.flip = (flags ? int(flags[i] & ORE_IMAGE_FLIP_H) : 0) | bits;
    any_flip |= r.flip != 0;
    any_orient |= bits != 0;
    if (l->filter == ORE_FILTER_BICUBIC_AA) taps = std::max(taps, resize_cubic_aa_max_taps(r.Ws, r.Rw));
  }
  // stream-ordered: launches submitted earlier read the old table, later ones the new
  ORE_HIP_CHECK(ctx, hipMemcpyAsync(l->table, l->mirror, size_t(n) * sizeof(typename F::Image), hipMemcpyHostToDevice, ctx->stream));
  ORE_HIP_CHECK(ctx, hipEventRecord(l->uploaded, ctx->stream));
  l->count = n;
  l->any_flip = any_flip;
  l->any_orient = any_orient;
  l->taps = taps;
  return ORE_OK;
}

// ---------------------------------------------------------------- one launch choice
ore_status list_params(ore_ctx* ctx, const ore_image_list* l, const float* scale, const float* shift, int32_t flags,
                       ResizeListParams* p) {
  PreprocParams q;
  if (ore_status st = preproc_params(ctx, l->h, l->w, l->c, scale, shift, flags, &q)) return st;
  *p = ResizeListParams{};
  p->table = l->format == ORE_IMAGE_INTERLEAVED ? static_cast<const ResizeImage*>(l->table) : nullptr;
  p->N = l->count;
  p->C = int(l->c); p->H = int(l->h); p->W = int(l->w);
  copy_norm(q, p);
  return ORE_OK;
}

// the parameter block of a frame format's kernels: p's launch with the list's table and matrix
template <class Q, class Image>
static Q planar_params(const ore_image_list* l, const ResizeListParams& p) {
  Q q{};
  q.table = static_cast<const Image*>(l->table);
  q.first = p.first; q.y = p.y; q.N = p.N; q.y_nstride = p.y_nstride;
  q.H = p.H; q.W = p.W;
  q.flips = p.flips;
  q.taps = p.taps;
  yuv_matrix(l->matrix, &q.m);  // checked at creation
  for (int s = 0; s < 3; ++s) {
    q.plane[s] = p.plane[s];
    q.scale[s] = p.scale[s];
    q.shift[s] = p.shift[s];
  }
  return q;
}

void launch_list(ore_ctx* ctx, const ore_image_list* l, const ResizeListParams& p0) {
  // The flag-free instance of the kernel when no descriptor of the list is flipped.  Not inside a stream capture:
  // a captured graph reads at replay whatever table a later set uploaded, flags included.
  ResizeListParams p = p0;
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  const bool capturing = ctx->stream && hipStreamIsCapturing(ctx->stream, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone;
  // The orientation-reading instance when the last set held a code other than 1; a capture records it for a list
  // that an oriented set has marked, and otherwise what it recorded before there were orientations.
  p.flips = capturing ? (l->oriented ? 2 : 1) : l->any_orient ? 2 : l->any_flip ? 1 : 0;
  p.taps = capturing || l->taps < 1 ? RESIZE_AA_MAX_TAPS : l->taps;  // likewise: a later set may bring longer runs
  if (l->format == ORE_IMAGE_YUV)
    launch_resize_list(planar_params<YuvListParams, YuvImage>(l, p), l->filter, ctx->stream);
  else if (l->format == ORE_IMAGE_NV12)
    launch_resize_list(planar_params<Nv12ListParams, Nv12Image>(l, p), l->filter, ctx->stream);
  else
    launch_resize_list(p, l->filter, ctx->stream);
}

}  // namespace ore

using namespace ore;

extern "C" {

ore_status ore_orient_geometry(int32_t orientation, const ore_resize* g, int64_t h, int64_t w, ore_resize* stored_g, int64_t* hz,
                               int64_t* wz, int32_t* rev_rows, int32_t* rev_cols, int32_t* transpose) {
  bool rr, rc, tr;
  if (!orient_bits(orientation, &rr, &rc, &tr))
    return set_error(nullptr, ORE_ERR_INVALID, "orientation %d is not an EXIF code 1..8", int(orientation));
  if (!g) return set_error(nullptr, ORE_ERR_INVALID, "null resize geometry");
  ore_resize sg;
  int64_t hh, ww;
  orient_stored(orientation, *g, h, w, &sg, &hh, &ww);
  if (stored_g) *stored_g = sg;
  if (hz) *hz = hh;
  if (wz) *wz = ww;
  if (rev_rows) *rev_rows = rr;
  if (rev_cols) *rev_cols = rc;
  if (transpose) *transpose = tr;
  return ORE_OK;
}

ore_status ore_yuv_to_rgb(int32_t matrix, const uint8_t* y, const uint8_t* u, const uint8_t* v, int64_t n, uint8_t* rgb) {
  YuvMatrix m;
  if (!yuv_matrix(matrix, &m)) return set_error(nullptr, ORE_ERR_INVALID, "unknown YUV matrix %d", int(matrix));
  if (n < 0) return set_error(nullptr, ORE_ERR_INVALID, "negative count %lld", (long long)n);
  if (n == 0) return ORE_OK;
  if (!y || !u || !v || !rgb) return set_error(nullptr, ORE_ERR_INVALID, "null argument");
  for (int64_t i = 0; i < n; ++i) {
    int c[3];
    yuv_rgb(m, y[i], yuv_chroma(m, u[i], v[i]), c);
    for (int s = 0; s < 3; ++s) rgb[3 * i + s] = uint8_t(c[s]);
  }
  return ORE_OK;
}

// ---- the checks
ore_status ore_image_check(const ore_image_u8* imgs, int64_t n, int64_t c, int64_t h, int64_t w, int64_t* bad_index) {
  return check_list<U8Format>(imgs, n, c, h, w, ORE_FILTER_BILINEAR, nullptr, bad_index);
}
ore_status ore_image_check_ex(const ore_image_u8* imgs, int64_t n, int64_t c, int64_t h, int64_t w, int32_t filter,
                              int64_t* bad_index) {
  return check_list<U8Format>(imgs, n, c, h, w, filter, nullptr, bad_index);
}
ore_status ore_image_check_oriented(const ore_image_u8* imgs, int64_t n, int64_t c, int64_t h, int64_t w, int32_t filter,
                                    const uint8_t* orientations, int64_t* bad_index) {
  return check_list<U8Format>(imgs, n, c, h, w, filter, orientations, bad_index);
}
ore_status ore_image_check_nv12(const ore_image_nv12* imgs, int64_t n, int64_t h, int64_t w, int32_t filter, int64_t* bad_index) {
  return check_list<Nv12Format>(imgs, n, 3, h, w, filter, nullptr, bad_index);
}
ore_status ore_image_check_nv12_oriented(const ore_image_nv12* imgs, int64_t n, int64_t h, int64_t w, int32_t filter,
                                         const uint8_t* orientations, int64_t* bad_index) {
  return check_list<Nv12Format>(imgs, n, 3, h, w, filter, orientations, bad_index);
}
ore_status ore_image_check_yuv(const ore_image_yuv* imgs, int64_t n, int64_t h, int64_t w, int32_t filter, int64_t* bad_index) {
  return check_list<YuvFormat>(imgs, n, 3, h, w, filter, nullptr, bad_index);
}
ore_status ore_image_check_yuv_oriented(const ore_image_yuv* imgs, int64_t n, int64_t h, int64_t w, int32_t filter,
                                        const uint8_t* orientations, int64_t* bad_index) {
  return check_list<YuvFormat>(imgs, n, 3, h, w, filter, orientations, bad_index);
}

// ---- the lists
ore_status ore_image_list_create(ore_ctx* ctx, int64_t capacity, int64_t c, int64_t h, int64_t w, ore_image_list** out) {
  return list_create(ctx, capacity, c, h, w, ORE_FILTER_BILINEAR, ORE_IMAGE_INTERLEAVED, 0, out);
}
ore_status ore_image_list_create_ex(ore_ctx* ctx, int64_t capacity, int64_t c, int64_t h, int64_t w, int32_t filter,
                                    ore_image_list** out) {
  return list_create(ctx, capacity, c, h, w, filter, ORE_IMAGE_INTERLEAVED, 0, out);
}
ore_status ore_image_list_create_nv12(ore_ctx* ctx, int64_t capacity, int64_t h, int64_t w, int32_t filter, int32_t matrix,
                                      ore_image_list** out) {
  return list_create(ctx, capacity, 3, h, w, filter, ORE_IMAGE_NV12, matrix, out);
}
ore_status ore_image_list_create_yuv(ore_ctx* ctx, int64_t capacity, int64_t h, int64_t w, int32_t filter, int32_t matrix,
                                     ore_image_list** out) {
  return list_create(ctx, capacity, 3, h, w, filter, ORE_IMAGE_YUV, matrix, out);
}

ore_status ore_image_list_destroy(ore_image_list* l) {
  if (!l) return ORE_OK;
  (void)hipSetDevice(l->ctx->device);
  if (l->uploaded) {  // a pending upload still reads the mirror; launches that read the table are the caller's to finish
    (void)hipEventSynchronize(l->uploaded);
    (void)hipEventDestroy(l->uploaded);
  }
  if (l->mirror) (void)hipHostFree(l->mirror);
  if (l->table) (void)hipFree(l->table);
  delete l;
  return ORE_OK;
}

int32_t ore_image_list_filter(ore_image_list* l) { return l ? l->filter : ORE_FILTER_BILINEAR; }
int32_t ore_image_list_format(ore_image_list* l) { return l ? l->format : ORE_IMAGE_INTERLEAVED; }
int32_t ore_image_list_matrix(ore_image_list* l) { return l ? l->matrix : ORE_YUV_BT601; }
int64_t ore_image_list_count(ore_image_list* l) { return l ? l->count : 0; }
int32_t ore_image_list_oriented(ore_image_list* l) { return l && l->oriented ? 1 : 0; }

// ---- the sets: plain, with flag words, with flag words and orientation codes
ore_status ore_image_list_set(ore_image_list* l, const ore_image_u8* imgs, int64_t n) {
  return list_set<U8Format>(l, imgs, nullptr, nullptr, n, false);
}
ore_status ore_image_list_set_ex(ore_image_list* l, const ore_image_u8* imgs, const uint32_t* flags, int64_t n) {
  return list_set<U8Format>(l, imgs, flags, nullptr, n, false);
}
ore_status ore_image_list_set_oriented(ore_image_list* l, const ore_image_u8* imgs, const uint32_t* flags,
                                       const uint8_t* orientations, int64_t n) {
  return list_set<U8Format>(l, imgs, flags, orientations, n, true);
}
ore_status ore_image_list_set_nv12(ore_image_list* l, const ore_image_nv12* imgs, int64_t n) {
  return list_set<Nv12Format>(l, imgs, nullptr, nullptr, n, false);
}
ore_status ore_image_list_set_nv12_ex(ore_image_list* l, const ore_image_nv12* imgs, const uint32_t* flags, int64_t n) {
  return list_set<Nv12Format>(l, imgs, flags, nullptr, n, false);
}
ore_status ore_image_list_set_nv12_oriented(ore_image_list* l, const ore_image_nv12* imgs, const uint32_t* flags,
                                            const uint8_t* orientations, int64_t n) {
  return list_set<Nv12Format>(l, imgs, flags, orientations, n, true);
}
ore_status ore_image_list_set_yuv(ore_image_list* l, const ore_image_yuv* imgs, int64_t n) {
  return list_set<YuvFormat>(l, imgs, nullptr, nullptr, n, false);
}
ore_status ore_image_list_set_yuv_ex(ore_image_list* l, const ore_image_yuv* imgs, const uint32_t* flags, int64_t n) {
  return list_set<YuvFormat>(l, imgs, flags, nullptr, n, false);
}
ore_status ore_image_list_set_yuv_oriented(ore_image_list* l, const ore_image_yuv* imgs, const uint32_t* flags,
                                           const uint8_t* orientations, int64_t n) {
  return list_set<YuvFormat>(l, imgs, flags, orientations, n, true);
}

ore_status ore_preprocess_list_u8(ore_ctx* ctx, ore_image_list* l, const float* scale, const float* shift, int32_t flags,
                                  ore_tensor* y) {
  // the arguments first and the context last, as ore_preprocess_resize_u8
  if (!l || !y || !y->data) return set_error(ctx, ORE_ERR_INVALID, "null argument");
  if (y->ndim != 4 || y->dims[0] != l->count || y->dims[1] != l->c || y->dims[2] != l->h || y->dims[3] != l->w)
    return set_error(ctx, ORE_ERR_INVALID, "list output must be [count,c,H,W] of the image list (%lld x %lld x %lld x %lld)",
                     (long long)l->count, (long long)l->c, (long long)l->h, (long long)l->w);
  ResizeListParams p;
  if (ore_status st = list_params(ctx, l, scale, shift, flags, &p)) return st;
  if (nstride_of(y) < l->c * l->h * l->w)
    return set_error(ctx, ORE_ERR_INVALID, "list output: image stride %lld below c*H*W", (long long)nstride_of(y));
  if (!ctx) return set_error(ctx, ORE_ERR_INVALID, "null context");
  if (l->ctx != ctx) return set_error(ctx, ORE_ERR_INVALID, "the image list belongs to another context");
  if (l->count == 0) return ORE_OK;
  p.y = y->data;
  p.y_nstride = nstride_of(y);
  ORE_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  launch_list(ctx, l, p);
  ORE_HIP_CHECK(ctx, hipGetLastError());
  return ORE_OK;
}

}  // extern "C"
