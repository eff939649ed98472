// C ABI: context, memory, reference geometry and the per-op entry points that replace the
// functions behind `node_inference` (model_inference.rs:137-161).
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <vector>

#include "ore_chunk.h"
#include "ore_internal.h"
#include "ore_resize_geom.h"

namespace {
thread_local std::string g_global_err;
}

namespace ore {

ore_status set_error(ore_ctx* ctx, ore_status st, const char* fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  if (ctx) ctx->err = buf;
  g_global_err = buf;
  return st;
}

// get_padding_size (convolution_op.rs:519-557 == max_pool_op.rs:363-401).  The reference
// returns (pad_h, pad_w, pad_bottom, pad_top, pad_right, pad_left) into variables named
// (pad_num_h, pad_num_w, pad_top, pad_bottom, pad_left, pad_right): the larger half lands on
// the top/left, for SAME_UPPER and SAME_LOWER alike.
static ore_status same_padding(ore_ctx* ctx, int64_t H, int64_t W, int64_t sh, int64_t sw, int64_t kh, int64_t kw,
                               Window* w) {
  const int64_t ph = (H % sh == 0) ? kh - sh : kh - (H % sh);
  const int64_t pw = (W % sw == 0) ? kw - sw : kw - (W % sw);
  if (ph < 0 || pw < 0)  // usize underflow in the reference
    return set_error(ctx, ORE_ERR_UNSUPPORTED, "SAME padding with kernel smaller than stride/remainder");
  w->pb = ph / 2;
  w->pt = ph - w->pb;
  w->pr = pw / 2;
  w->pl = pw - w->pr;
  return ORE_OK;
}

ore_status resolve_window(ore_ctx* ctx, int auto_pad, const int64_t* pads, int n_pads, int64_t H, int64_t W,
                          int64_t kh, int64_t kw, int64_t sh, int64_t sw, Window* out) {
  *out = Window{};
  if (sh <= 0 || sw <= 0 || kh <= 0 || kw <= 0)
    return set_error(ctx, ORE_ERR_INVALID, "non-positive kernel/stride");
  switch (auto_pad) {
    case ORE_PAD_SAME_UPPER:
    case ORE_PAD_SAME_LOWER:
      // H' = ceil(H / stride), computed in f32 as the reference does (:297-310)
      out->Ho = int64_t(std::ceil(float(H) / float(sh)));
      out->Wo = int64_t(std::ceil(float(W) / float(sw)));
      return same_padding(ctx, H, W, sh, sw, kh, kw, out);
    case ORE_PAD_NOTSET: {
      if (n_pads < 4) return set_error(ctx, ORE_ERR_INVALID, "auto_pad NOTSET needs 4 pads");
      out->pt = pads[0]; out->pl = pads[1]; out->pb = pads[2]; out->pr = pads[3];
      if (out->pt < 0 || out->pl < 0 || out->pb < 0 || out->pr < 0)
        return set_error(ctx, ORE_ERR_INVALID, "negative pads");
      if (H + out->pt + out->pb < kh || W + out->pl + out->pr < kw)
        return set_error(ctx, ORE_ERR_INVALID, "window larger than padded input");
      out->Ho = (H - kh + out->pt + out->pb) / sh + 1;  // floor (:312-317)
      out->Wo = (W - kw + out->pl + out->pr) / sw + 1;
      return ORE_OK;
    }
    case ORE_PAD_VALID:
      if (H < kh || W < kw) return set_error(ctx, ORE_ERR_INVALID, "window larger than input");
      out->Ho = (H - kh) / sh + 1;
      out->Wo = (W - kw) / sw + 1;
      return ORE_OK;
    default:
      return set_error(ctx, ORE_ERR_UNSUPPORTED, "unknown auto_pad %d", auto_pad);
  }
}

int64_t nstride_of(const ore_tensor* t) {
  if (t->nstride) return t->nstride;
  int64_t s = 1;
  for (int i = 1; i < t->ndim; ++i) s *= t->dims[i];
  return s;
}

// a per-op f32 tensor as the runners take it (dense planes)
static Ref ref_of(const ore_tensor* t) { return {t->data, nstride_of(t), 0, 4}; }

static int64_t numel(const ore_tensor* t) {
  int64_t s = 1;
  for (int i = 0; i < t->ndim; ++i) s *= t->dims[i];
  return s;
}

static bool contiguous(const ore_tensor* t) {
  if (!t->nstride) return true;
  int64_t s = 1;
  for (int i = 1; i < t->ndim; ++i) s *= t->dims[i];
  return t->nstride == s;
}

// The image stride of a 4-D activation that may be a slice (Conv's and MaxPool's x and y): 0 (contiguous) or at
// least one image's elements -- below that the images overlap and one image's outputs overwrite another's --
// and, for the kernels' 32-bit image offsets, nstride * N + 256 below 2^31.  Host only.
static ore_status check_image_stride(ore_ctx* ctx, const char* op, const char* name, const ore_tensor* t) {
  const int64_t img = t->dims[1] * t->dims[2] * t->dims[3], lim = int64_t(1) << 31;
  if (t->nstride < 0 || (t->nstride && t->nstride < img))
    return set_error(ctx, ORE_ERR_INVALID, "%s: %s->nstride %lld is below the image size %lld (images would overlap)", op,
                     name, (long long)t->nstride, (long long)img);
  const int64_t s = t->nstride ? t->nstride : img, n = std::max<int64_t>(t->dims[0], 1);
  if (s >= lim || n >= lim || !fits_i32(s * n + 256))
    return set_error(ctx, ORE_ERR_INVALID, "%s: %s spans %lld images of stride %lld, past 32-bit indexing", op, name,
                     (long long)t->dims[0], (long long)s);
  return ORE_OK;
}

// mapped bytes before x: the rest of x's 4 KiB page, or the walker's arena lead where x lies inside the
// context's mapped range.  The streaming 3x3 conv, the row-walking pooled conv and the f32 fire kernels
// read a few of them, masked, instead of issuing negative buffer offsets.
static int x_guard_bytes(const ore_ctx* ctx, const void* x) {
  const char* xc = static_cast<const char*>(x);
  int64_t g = int64_t(reinterpret_cast<uintptr_t>(x) & 4095);
  if (ctx->mapped_lo && xc >= ctx->mapped_lo && xc < ctx->mapped_hi)
    g = std::max<int64_t>(g, std::min<int64_t>(xc - ctx->mapped_lo, 1 << 20));
  return int(g);
}

ore_status preproc_params(ore_ctx* ctx, int64_t h, int64_t w, int64_t c, const float* scale, const float* shift,
                          int32_t flags, PreprocParams* p) {
  if (c < 1 || c > 4) return set_error(ctx, ORE_ERR_INVALID, "uint8 input: %lld channels (1..4 supported)", (long long)c);
  if (flags & ~ORE_PRE_REVERSE_CHANNELS)
    return set_error(ctx, ORE_ERR_INVALID, "unknown preprocess flags 0x%x", unsigned(flags & ~ORE_PRE_REVERSE_CHANNELS));
  const bool rev = (flags & ORE_PRE_REVERSE_CHANNELS) != 0;
  if (rev && c != 3) return set_error(ctx, ORE_ERR_INVALID, "ORE_PRE_REVERSE_CHANNELS needs 3 channels, not %lld", (long long)c);
  if (h <= 0 || w <= 0 || !fits_i32(h) || !fits_i32(w) || !fits_i32(h * w) || !fits_i32(h * w * c))
    return set_error(ctx, ORE_ERR_INVALID, "uint8 input: image of %lld x %lld x %lld", (long long)h, (long long)w, (long long)c);
  *p = PreprocParams{};
  p->HW = int(h * w);
  p->C = int(c);
  for (int s = 0; s < int(c); ++s) {  // source channel s is output channel ch
    const int ch = rev ? int(c) - 1 - s : s;
    p->plane[s] = ch;
    p->scale[s] = scale ? scale[ch] : 1.0f;
    p->shift[s] = shift ? shift[ch] : 0.0f;
  }
  return ORE_OK;
}

bool filter_known(int32_t filter) {
  return filter == ORE_FILTER_BILINEAR || filter == ORE_FILTER_BILINEAR_AA || filter == ORE_FILTER_BICUBIC ||
         filter == ORE_FILTER_BICUBIC_AA;
}

// the most an antialiasing filter shrinks an axis (ORE_AA_MAX_RATIO, ORE_CUBIC_AA_MAX_RATIO); 0: no ratio rule
static int filter_max_ratio(int32_t filter) {
  return filter == ORE_FILTER_BILINEAR_AA ? ORE_AA_MAX_RATIO : filter == ORE_FILTER_BICUBIC_AA ? ORE_CUBIC_AA_MAX_RATIO : 0;
}

// the axis on which the filter would shrink by more than its ratio, or null
static const char* aa_bad_axis(int32_t filter, int64_t hs, int64_t ws, const ore_resize& g) {
  const int ratio = filter_max_ratio(filter);
  if (!ratio) return nullptr;
  if (hs > ratio * g.rh) return "rows";
  if (ws > ratio * g.rw) return "columns";
  return nullptr;
}

// what a geometry message opens with: "resize" of a dense conversion (i < 0), "image i" of a list's descriptor
struct Subject {
  char s[32];
  explicit Subject(int64_t i) {
    if (i < 0) snprintf(s, sizeof s, "resize");
    else snprintf(s, sizeof s, "image %lld", (long long)i);
  }
};

ore_status check_resize_window(ore_ctx* ctx, int64_t i, int64_t hs, int64_t ws, int64_t h, int64_t w, const ore_resize& g) {
  if (hs < 1 || ws < 1 || hs > RESIZE_MAX || ws > RESIZE_MAX || g.rh < 1 || g.rw < 1 || g.rh > RESIZE_MAX || g.rw > RESIZE_MAX)
    return set_error(ctx, ORE_ERR_INVALID, "%s: source %lld x %lld resized to %lld x %lld (each 1..%d)", Subject(i).s, (long long)hs,
                     (long long)ws, (long long)g.rh, (long long)g.rw, RESIZE_MAX);
  if (!resize_axis_ok(hs, g.rh, g.top, h) || !resize_axis_ok(ws, g.rw, g.left, w))
    return set_error(ctx, ORE_ERR_INVALID, "%s: the %lld x %lld crop at (%lld, %lld) lies outside the %lld x %lld resized image",
                     Subject(i).s, (long long)h, (long long)w, (long long)g.top, (long long)g.left, (long long)g.rh, (long long)g.rw);
  return ORE_OK;
}

ore_status check_resize_ratio(ore_ctx* ctx, int64_t i, int32_t filter, int64_t hs, int64_t ws, const ore_resize& g) {
  if (const char* axis = aa_bad_axis(filter, hs, ws, g))
    return set_error(ctx, ORE_ERR_INVALID, "%s: the antialiasing filter shrinks an axis at most %d times, the %s go %lld -> %lld",
                     Subject(i).s, filter_max_ratio(filter), axis, (long long)(axis[0] == 'r' ? hs : ws),
                     (long long)(axis[0] == 'r' ? g.rh : g.rw));
  return ORE_OK;
}

ore_status resize_params(ore_ctx* ctx, int64_t hs, int64_t ws, int64_t c, int64_t h, int64_t w, const ore_resize* g,
                         const float* scale, const float* shift, int32_t flags, ResizeParams* p, int32_t filter) {
  if (!g) return set_error(ctx, ORE_ERR_INVALID, "null resize geometry");
  if (!filter_known(filter))
    return set_error(ctx, ORE_ERR_INVALID, "unknown resize filter %d", int(filter));
  PreprocParams q;  // c, the flags, the reversal and the output size: the direct conversion's checks
  if (ore_status st = preproc_params(ctx, h, w, c, scale, shift, flags, &q)) return st;
  if (ore_status st = check_resize_window(ctx, -1, hs, ws, h, w, *g)) return st;
  if (ore_status st = check_resize_ratio(ctx, -1, filter, hs, ws, *g)) return st;
  *p = ResizeParams{};
  p->Hs = int(hs); p->Ws = int(ws); p->C = int(c);
  p->Rh = int(g->rh); p->Rw = int(g->rw); p->top = int(g->top); p->left = int(g->left);
  p->H = int(h); p->W = int(w);
  copy_norm(q, p);
  return ORE_OK;
}

ConvPlan conv_plan(int64_t M, int64_t C, int64_t H, int64_t W, int64_t kh, int64_t kw, int64_t sh, int64_t sw,
                   const Window& win, bool f16, int xmode, bool wino, int forced) {
  return plan_conv(int(M), int(C), int(H), int(W), int(kh), int(kw), int(sh), int(sw), int(win.pt), int(win.pl),
                   int(win.Ho), int(win.Wo), kh == 1 && kw == 1, f16, xmode, wino, forced);
}

hipError_t device_fill(ore_ctx* ctx, void* dptr, size_t bytes, uint32_t pattern) {
  char* p = static_cast<char*>(dptr);
  const size_t words = bytes / 4;
  if (words)
    if (hipError_t e = hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(p), int(pattern), words, ctx->stream)) return e;
  for (size_t i = words * 4; i < bytes; ++i)
    if (hipError_t e = hipMemsetAsync(p + i, int((pattern >> (8 * (i & 3))) & 0xff), 1, ctx->stream)) return e;
  return hipSuccess;
}

hipError_t device_alloc(ore_ctx* ctx, void** dptr, size_t bytes, bool own) {
  *dptr = nullptr;
  if (hipError_t e = hipMalloc(dptr, bytes)) return e;
  if (!own || !ctx->alloc_fill) return hipSuccess;
  const hipError_t e = device_fill(ctx, *dptr, bytes, ctx->alloc_pattern);
  if (e != hipSuccess) {
    (void)hipFree(*dptr);
    *dptr = nullptr;
  }
  return e;
}

size_t packed_bytes(const ConvPlan& pln) { return conv_packed_bytes(pln) + size_t(pln.krows) * sizeof(int2); }

float* pack_to_scratch(ore_ctx* ctx, const ConvPlan& pln, const float* w, bool kmajor_src, int64_t M, int64_t C,
                       int64_t kh, int64_t kw, int64_t H, int64_t W, const int2** ktab) {
  const size_t need = packed_bytes(pln);
  if (need > ctx->scratch_bytes) {
    if (ctx->scratch) {
      (void)hipStreamSynchronize(ctx->stream);
      (void)hipFree(ctx->scratch);
    }
    ctx->scratch = nullptr;
    ctx->scratch_bytes = 0;
    if (device_alloc(ctx, reinterpret_cast<void**>(&ctx->scratch), need, true) != hipSuccess) {
      set_error(ctx, ORE_ERR_OOM, "weight scratch allocation (%zu bytes) failed", need);
      return nullptr;
    }
    ctx->scratch_bytes = need;
  }
  launch_pack(w, kmajor_src, int(M), int(C), int(kh), int(kw), pln, ctx->scratch, ctx->stream);
  int2* kt = reinterpret_cast<int2*>(reinterpret_cast<char*>(ctx->scratch) + conv_packed_bytes(pln));
  launch_ktab(kt, int(C * kh * kw), int(kh), int(kw), int(H * W), int(W), ctx->stream);
  if (hipGetLastError() != hipSuccess) {
    set_error(ctx, ORE_ERR_HIP, "weight packing launch failed");
    return nullptr;
  }
  *ktab = kt;
  return ctx->scratch;
}

// kh = kw = 1, stride 1, no padding, the output plane the input's
static bool pointwise(const ConvGeom& g) {
  return g.kh == 1 && g.kw == 1 && g.sh == 1 && g.sw == 1 && g.win.pt == 0 && g.win.pl == 0 && g.win.Ho == g.H &&
         g.win.Wo == g.W;
}

// The ConvParams fields the four conv paths fill alike; x_ps / y_ps: the strides as the path's layouts
// resolve them; ep: the pool of a pooled form.  false: not a pool the pooled epilogues take (epool_tile).
// Each path then sets what is its own: P, Ntot, is1x1, vec_out, x_guard, and per chunk x_bytes.
static bool conv_params(ConvParams* out, const ConvPlan& pln, const Ref& x, const Ref& y, int64_t N, const ConvGeom& g,
                        const ConvOperands& w, int64_t x_ps, int64_t y_ps, const PoolGeom* ep) {
  ConvParams p{};
  p.x = x.p; p.wp = w.wp; p.ktab = w.ktab; p.bias = w.bias; p.y = y.p;
  p.N = int(N); p.C = int(g.C); p.H = int(g.H); p.W = int(g.W);
  p.M = int(g.M); p.kh = int(g.kh); p.kw = int(g.kw); p.sh = int(g.sh); p.sw = int(g.sw);
  p.pt = int(g.win.pt); p.pl = int(g.win.pl);
  p.Ho = int(g.win.Ho); p.Wo = int(g.win.Wo);
  // the GEMM's K: the f16 packings pad taps and channels per xmode
  p.K = pln.f16 ? f16_conv_k(pln.xmode, int(g.C), int(g.kh), int(g.kw)) : int(g.C * g.kh * g.kw);
  p.x_ps = int(x_ps);
  p.y_ps = int(y_ps);
  p.x_nstride = x.nstride;
  p.y_nstride = y.nstride;
  p.relu = g.relu ? 1 : 0;
  p.Mp = pln.Mp;
  p.x_f32 = (!pln.f16 || pln.xmode == F16_X_NCHW32) ? 1 : 0;  // x is f32 NCHW; else NHWC f16
  if (ep) {
    if (epool_tile(g.win.Ho, g.win.Wo, ep->kh, ep->kw, ep->sh, ep->sw, ep->win, &p.ep_tr, &p.ep_tc) == 0.0) return false;
    p.ep_pt = int(ep->win.pt); p.ep_pl = int(ep->win.pl); p.ep_Ho = int(ep->win.Ho); p.ep_Wo = int(ep->win.Wo);
  }
  *out = p;
  return true;
}

// columns of a pooled form: whole patches of conv outputs, ep_tr x ep_tc per image
static int64_t epool_columns(const ConvParams& p, int64_t n) { return n * int64_t(p.ep_tr) * p.ep_tc * CONV_EPOOL_BN; }

ConvRun run_conv(ore_ctx* ctx, const ConvPlan& pln, const Ref& x, const Ref& y, int64_t N, const ConvGeom& g,
                 const ConvOperands& w) {
  if (N == 0) return ORE_OK;
  if (pln.f16 || x.es != 4) return set_error(ctx, ORE_ERR_INVALID, "internal: run_conv takes f32 plans and inputs");
  const int64_t x_ps = plane_stride(x, g.H * g.W), y_ps = plane_stride(y, g.win.Ho * g.win.Wo);
  ConvParams p;
  conv_params(&p, pln, x, y, N, g, w, x_ps, y_ps, nullptr);
  p.P = int(g.win.Ho * g.win.Wo);
  p.Ntot = N * y_ps;  // a column per element of y's (padded) planes
  // 16-B epilogue stores of 4 floats
  p.vec_out = (y_ps % 4 == 0 && y.nstride % 4 == 0 && (reinterpret_cast<uintptr_t>(y.p) & 15) == 0) ? 1 : 0;
  p.is1x1 = pointwise(g) && x_ps == y_ps;  // the 1x1 kernels take column j of y from column j of x: equal plane strides
  p.x_guard = x_guard_bytes(ctx, x.p);
  if (x_ps < g.H * g.W || y_ps < g.win.Ho * g.win.Wo) return set_error(ctx, ORE_ERR_INVALID, "plane stride below plane size");
  if (!fits_i32(x.nstride * N + 256) || !fits_i32(y.nstride * N + 256) || !fits_i32(int64_t(pln.krows) * pln.Mp) ||
      !fits_i32(p.Ntot + 256) || (p.Ntot + 127) / 128 * ((g.M + 31) / 32) >= (int64_t(1) << 31))
    return set_error(ctx, ORE_ERR_INVALID, "conv geometry exceeds 32-bit indexing");
  if (!pln.wino && !p.is1x1 && !w.ktab) return set_error(ctx, ORE_ERR_INVALID, "internal: gather table missing");
  // the output may be a slice of a wider concat buffer (y.nstride above M * y_ps), e.g. an expand3x3
  // writing channels 256..511 of 512
  const ChunkSide xs{x.nstride, g.C * x_ps * 4, 4}, ys{y.nstride, g.M * y_ps * 4, 4};
  const int64_t nb = image_chunk(N, xs, ys);
  if (nb == 0) return set_error(ctx, ORE_ERR_UNSUPPORTED, "conv: one image exceeds 2 GiB");
  int tile = -1;
  for (Chunk c = chunk_at(0, N, nb); c.nc > 0; c = chunk_at(c.i0 + c.nc, N, nb)) {
    ConvParams q = p;
    q.x = x.p + c.i0 * x.nstride;
    q.y = y.p + c.i0 * y.nstride;
    q.N = int(c.nc);
    q.Ntot = c.nc * y_ps;
    q.x_bytes = xs.bytes(c.nc);
    ConvPlan qp = pln;
    if (pln.wino && !conv_wino_eligible(q, qp.cfg - WINO_TILE_BASE)) {  // the first tile that takes it
      int t = 0;
      while (t < WINO_TILES_N && !conv_wino_eligible(q, t)) ++t;
      if (t == WINO_TILES_N) return set_error(ctx, ORE_ERR_UNSUPPORTED, "Winograd conv: no tile takes this layout");
      qp.cfg = WINO_TILE_BASE + t;
    }
    tile = launch_conv(q, qp, ctx->stream);
    ORE_HIP_CHECK(ctx, hipGetLastError());
  }
  return {ORE_OK, tile};
}

ore_status run_fire(ore_ctx* ctx, const Ref& x, const Ref& y, int64_t N, int64_t H, int64_t W, const FireOperands& f,
                    const Window* pool) {
  if (N == 0) return ORE_OK;
  const int64_t yplane = pool ? pool->Ho * pool->Wo : H * W;
  const int64_t x_ps = plane_stride(x, H * W), y_ps = plane_stride(y, yplane);
  FireParams p{};
  p.x = x.p; p.y = y.p;
  p.w1 = static_cast<const float*>(f.w1); p.b1 = f.b1; p.w3 = static_cast<const float*>(f.w3); p.b3 = f.b3;
  p.ws = static_cast<const float*>(f.ws); p.bs = f.bs;
  p.N = int(N); p.C = int(f.C); p.H = int(H); p.W = int(W);
  p.E1 = int(f.E1); p.E3 = int(f.E3); p.Ms = int(f.Ms); p.Msp = int(f.Msp);
  p.x_ps = int(x_ps); p.y_ps = int(y_ps);
  p.x_nstride = x.nstride; p.y_nstride = y.nstride;
  p.Ntot = N * y_ps;
  if (pool) {
    p.pool = 1;
    p.Hp = int(pool->Ho); p.Wp = int(pool->Wo); p.ppt = int(pool->pt); p.ppl = int(pool->pl);
    if (!fire_pool_plan(&p)) return set_error(ctx, ORE_ERR_INVALID, "internal: no band shape for the pooled fire module");
  }
  p.x_guard = x_guard_bytes(ctx, x.p);
  p.x_lead = int(((W + 1) * 4 + 15) & ~int64_t(15));
  if (x_ps < H * W || y_ps < yplane || !fits_i32(x.nstride * N + 256) || !fits_i32(y.nstride * N + 256) ||
      !fits_i32(p.Ntot + 256))
    return set_error(ctx, ORE_ERR_INVALID, "fire geometry exceeds 32-bit indexing");
  // x is addressed through a buffer resource, x_lead bytes before it included
  const ChunkSide xs{x.nstride, f.C * x_ps * 4, 4}, ys{y.nstride, f.Ms * y_ps * 4, 4};
  const int64_t nb = image_chunk(N, xs, ys);
  if (nb == 0) return set_error(ctx, ORE_ERR_UNSUPPORTED, "fused fire module: one image exceeds 2 GiB");
  for (Chunk c = chunk_at(0, N, nb); c.nc > 0; c = chunk_at(c.i0 + c.nc, N, nb)) {
    FireParams q = p;
    q.x = x.p + c.i0 * x.nstride;
    q.y = y.p + c.i0 * y.nstride;
    q.N = int(c.nc);
    q.Ntot = c.nc * y_ps;
    q.x_bytes = xs.bytes(c.nc);
    if (!fire_eligible(q)) return set_error(ctx, ORE_ERR_INVALID, "internal: fused fire module on an unsupported layout");
    launch_fire(q, ctx->stream);
    ORE_HIP_CHECK(ctx, hipGetLastError());
  }
  return ORE_OK;
}

ore_status run_fire_f16(ore_ctx* ctx, const Ref& x, const Ref& y, int64_t N, int64_t H, int64_t W,
                        const FireOperands& f, const Window* pool) {
  if (N == 0) return ORE_OK;
  const int64_t x_cs = pixel_stride(x, f.C), y_cs = pixel_stride(y, f.Ms ? f.Ms : f.E1 + f.E3);
  if (!fits_i32(N) || !fits_i32(H * W) || !fits_i32(x_cs) || !fits_i32(y_cs))
    return set_error(ctx, ORE_ERR_INVALID, "fire geometry exceeds 32-bit indexing");
  FireF16Params p{};
  p.x = x.p; p.w1 = f.w1; p.b1 = f.b1; p.w3 = f.w3; p.b3 = f.b3; p.ws = f.ws; p.bs = f.bs; p.y = y.p;
  p.N = int(N); p.C = int(f.C); p.H = int(H); p.W = int(W);
  p.E1 = int(f.E1); p.E3 = int(f.E3); p.Ms = int(f.Ms); p.Msp = int((f.Ms + 31) / 32 * 32);
  p.x_cs = int(x_cs); p.y_cs = int(y_cs);
  p.x_nstride = x.nstride; p.y_nstride = y.nstride;
  if (pool) {
    p.pool = 1;
    p.Hp = int(pool->Ho); p.Wp = int(pool->Wo); p.ppt = int(pool->pt); p.ppl = int(pool->pl);
    if (!fire_pool_f16_plan(&p)) return set_error(ctx, ORE_ERR_INVALID, "internal: no band shape for the pooled f16 fire module");
  }
  if (!fire_f16_eligible(p)) return set_error(ctx, ORE_ERR_INVALID, "internal: f16 fire module on an unsupported layout");
  launch_fire_f16(p, ctx->stream);
  ORE_HIP_CHECK(ctx, hipGetLastError());
  return ORE_OK;
}

double epool_tile(int64_t Ho, int64_t Wo, int64_t pkh, int64_t pkw, int64_t psh, int64_t psw, const Window& pwin,
                  int* tr, int* tc) {
  // the kernel's pooled epilogue is specialised for 3x3 / stride-2 windows (every SqueezeNet pool)
  if (pkh != 3 || pkw != 3 || psh != 2 || psw != 2 || Ho * Wo == 0 || pwin.Ho <= 0 || pwin.Wo <= 0) return 0.0;
  *tr = int((pwin.Ho + EPOOL_TILE_PR - 1) / EPOOL_TILE_PR);
  *tc = int((pwin.Wo + EPOOL_TILE_PC - 1) / EPOOL_TILE_PC);
  return double(int64_t(*tr) * *tc * CONV_EPOOL_BN) / double(Ho * Wo);
}

ConvRun run_conv_epool(ore_ctx* ctx, const ConvPlan& pln, const Ref& x, const Ref& y, int64_t N, const ConvGeom& g,
                       const ConvOperands& w, const PoolGeom& ep) {
  if (N == 0) return ORE_OK;
  if (pln.f16) return set_error(ctx, ORE_ERR_INVALID, "internal: the pooled epilogue is f32 gather only");
  const int64_t x_ps = plane_stride(x, g.H * g.W), y_ps = plane_stride(y, ep.win.Ho * ep.win.Wo);
  ConvParams p;
  if (!conv_params(&p, pln, x, y, N, g, w, x_ps, y_ps, &ep))
    return set_error(ctx, ORE_ERR_INVALID, "internal: the pooled epilogue takes 3x3 / stride-2 pools");
  p.P = int(g.win.Ho * g.win.Wo);
  p.Ntot = epool_columns(p, N);
  // vec_out stays 0: the pooled epilogues store single pooled values
  p.is1x1 = pointwise(g) && x_ps == g.H * g.W;  // y is the pooled plane, never x's: dense input planes instead
  p.x_guard = x_guard_bytes(ctx, x.p);
  p.ep_variant = pln.epv;
  p.wc1 = w.wc1;
  p.sq1 = w.sq1;
  if (x_ps < g.H * g.W || y_ps < ep.win.Ho * ep.win.Wo) return set_error(ctx, ORE_ERR_INVALID, "plane stride below plane size");
  if (!fits_i32(x.nstride * N + 256) || !fits_i32(y.nstride * N + 256) || !fits_i32(int64_t(pln.krows) * pln.Mp) ||
      !fits_i32(p.Ntot + 256) || N * p.ep_tr * p.ep_tc * ((g.M + 31) / 32) >= (int64_t(1) << 31))
    return set_error(ctx, ORE_ERR_INVALID, "conv geometry exceeds 32-bit indexing");
  if (!p.is1x1 && !w.ktab) return set_error(ctx, ORE_ERR_INVALID, "internal: gather table missing");
  // with the next 1x1 conv fused in, what the launch writes is that conv's output
  const C1SqueezeF32* sq1 = w.sq1;
  const ChunkSide xs{x.nstride, g.C * x_ps * 4, 4};
  const ChunkSide ys = sq1 ? ChunkSide{sq1->y_nstride, sq1->M * int64_t(sq1->y_ps) * 4, 4} : ChunkSide{y.nstride, g.M * y_ps * 4, 4};
  const int64_t nb = image_chunk(N, xs, ys);
  if (nb == 0) return set_error(ctx, ORE_ERR_UNSUPPORTED, "pooled conv: one image exceeds 2 GiB");
  int tile = -1;
  for (Chunk c = chunk_at(0, N, nb); c.nc > 0; c = chunk_at(c.i0 + c.nc, N, nb)) {
    ConvParams q = p;
    C1SqueezeF32 sq{};
    q.x = x.p + c.i0 * x.nstride;
    if (y.p) q.y = y.p + c.i0 * y.nstride;
    if (sq1) {
      sq = *sq1;
      sq.y = sq1->y + c.i0 * sq1->y_nstride;
      q.sq1 = &sq;
    }
    q.N = int(c.nc);
    q.Ntot = epool_columns(p, c.nc);
    q.x_bytes = xs.bytes(c.nc);
    tile = launch_conv_epool(q, ctx->stream);
    ORE_HIP_CHECK(ctx, hipGetLastError());
    if (sq1 && tile < 0)
      return set_error(ctx, ORE_ERR_INVALID, "internal: the fused first conv + squeeze declined its launch");
  }
  return {ORE_OK, tile};
}

ore_status run_conv_pool(ore_ctx* ctx, const ConvPlan& pln, const Ref& x, const Ref& y, int64_t N, const ConvGeom& g,
                         const ConvOperands& w, const PoolGeom& pool) {
  if (N == 0) return ORE_OK;
  const Window& pwin = pool.win;
  const int64_t x_ps = plane_stride(x, g.H * g.W), y_ps = plane_stride(y, pwin.Ho * pwin.Wo);
  if (pln.f16 || pln.wino || x.es != 4)
    return set_error(ctx, ORE_ERR_INVALID, "internal: the pooled 1x1 conv is f32 direct only");
  // 3x3 / stride-2 pools (the window is implied by the walker's pass, kernel_shape 3x3):
  // pool_conv1x1_f32_kernel (LDS-staged rows, MFMA squeeze)
  PoolConvParams q{};
  q.x = x.p; q.wp = w.wp; q.bias = w.bias; q.y = y.p;
  q.N = int(N); q.C = int(g.C); q.H = int(g.H); q.W = int(g.W); q.Hp = int(pwin.Ho); q.Wp = int(pwin.Wo);
  q.pt = int(pwin.pt); q.pl = int(pwin.pl); q.M = int(g.M); q.Mp = pln.Mp; q.Kp = pln.krows;
  q.x_ps = int(x_ps); q.y_ps = int(y_ps); q.x_nstride = x.nstride; q.y_nstride = y.nstride;
  q.relu = g.relu ? 1 : 0;
  if (const PoolExpand* pe = w.pe) {
    q.s = pe->s; q.w1 = pe->w1; q.b1 = pe->b1; q.C1 = pe->C1; q.E1 = pe->E1; q.w1_Mp = pe->w1_Mp;
    q.s_ps = int(pe->s_ps); q.s_nstride = pe->s_nstride;
    if (!fits_i32(pe->s_nstride * N + 256) || !fits_i32(pe->s_ps))
      return set_error(ctx, ORE_ERR_INVALID, "internal: recomputed expand input past 2 GiB");
  }
  if (pool.sh != 2 || pool.sw != 2 || pwin.Ho <= 0 || !fits_i32(x.nstride * N + 256) || !fits_i32(y.nstride * N + 256) ||
      !pool_conv1x1_f32_eligible(q))
    return set_error(ctx, ORE_ERR_INVALID, "internal: pooled 1x1 conv outside pool_conv1x1_f32_kernel's limits");
  launch_pool_conv1x1_f32(q, ctx->stream);
  ORE_HIP_CHECK(ctx, hipGetLastError());
  return ORE_OK;
}

ConvRun run_conv_pair_pool_f16(ore_ctx* ctx, const ConvPlan& pln, const Ref& x, const Ref& y, int64_t N,
                               const ConvGeom& g, const ConvOperands& w, const PoolGeom& ep) {
  // every `return ORE_OK` before the launch is a quiet decline (tile -1): the caller takes the two-launch path
  if (N == 0 || !pln.f16 || pln.xmode != F16_X_NHWC_PAIR) return ORE_OK;
  const int64_t x_ps = plane_stride(x, g.H * g.W), y_ps = pixel_stride(y, g.M);
  ConvParams p;
  if (!conv_params(&p, pln, x, y, N, g, w, x_ps, y_ps, &ep)) return ORE_OK;
  if (!fits_i32(N * int64_t(p.ep_tr) * p.ep_tc) || !fits_i32(g.C * x_ps) || !fits_i32(y_ps * ep.win.Ho * ep.win.Wo) ||
      x_ps < g.H * g.W)
    return ORE_OK;
  // P, Ntot, vec_out, is1x1 stay 0: the persistent kernels walk pooled tiles, not GEMM columns, and
  // gather the 7x7 taps themselves; no x_guard: an f16 model's input is not read through the arena
  const C1Squeeze* sq = w.sq16;
  if (!conv_pair_pool_f16_eligible(p, sq)) return ORE_OK;
  int tile;
  if (pln.epv == C1_BAND_F16_VARIANT && sq && conv_band_pool_f16_eligible(p, sq)) {  // the band walker (round 6)
    launch_conv_band_pool_f16(p, *sq, ctx->stream);
    tile = C1_BAND_F16_TILE;
  } else {
    launch_conv_pair_pool_f16(p, sq, ctx->stream);
    tile = C1_POOL_F16_TILE;
  }
  ORE_HIP_CHECK(ctx, hipGetLastError());
  return {ORE_OK, tile};
}

ConvRun run_conv_f16(ore_ctx* ctx, const ConvPlan& pln, const Ref& x, const Ref& y, int64_t N, const ConvGeom& g,
                     const ConvOperands& w, const PoolGeom* ep) {
  if (N == 0) return ORE_OK;
  if (!pln.f16) return set_error(ctx, ORE_ERR_INVALID, "internal: run_conv_f16 needs an f16 plan");
  const bool nchw = pln.xmode == F16_X_NCHW32;
  const int64_t x_ps = nchw ? plane_stride(x, g.H * g.W) : pixel_stride(x, g.C), y_ps = pixel_stride(y, g.M);
  if (nchw ? x_ps < g.H * g.W : x_ps < g.C) return set_error(ctx, ORE_ERR_INVALID, "input stride below its extent");
  if (y_ps < g.M) return set_error(ctx, ORE_ERR_INVALID, "output pixel stride below the channel count");
  if (pln.xmode == F16_X_NHWC_VEC &&
      (g.C % 8 || x_ps % 8 || x.nstride % 8 || (reinterpret_cast<uintptr_t>(x.p) & 15)))
    return set_error(ctx, ORE_ERR_INVALID, "internal: 16-B NHWC gather needs C, strides %% 8 == 0 and an aligned input");
  if (pln.xmode == F16_X_NHWC_PAIR && (g.C > 4 || x_ps != 4 || x.nstride % 4 || (reinterpret_cast<uintptr_t>(x.p) & 7)))
    return set_error(ctx, ORE_ERR_INVALID, "internal: the tap-pair gather needs an NHWC4 input");
  if (!w.ktab) return set_error(ctx, ORE_ERR_INVALID, "internal: gather table missing");
  ConvParams p;
  if (!conv_params(&p, pln, x, y, N, g, w, x_ps, y_ps, ep))  // y is then the pool's NHWC output [ep->win.Ho][ep->win.Wo]
    return set_error(ctx, ORE_ERR_INVALID, "internal: the pooled epilogue takes 3x3 / stride-2 pools");
  p.P = int(g.win.Ho * g.win.Wo);
  p.Ntot = ep ? epool_columns(p, N) : N * p.P;  // NHWC output: columns dense over the Ho x Wo pixels
  // 16-B epilogue stores of 8 halves along the channels
  p.vec_out = (g.M % 8 == 0 && y_ps % 8 == 0 && y.nstride % 8 == 0 && (reinterpret_cast<uintptr_t>(y.p) & 15) == 0) ? 1 : 0;
  // is1x1 stays 0: the f16 kernels always gather through ktab; no x_guard: they read nothing before x
  if (!fits_i32(x.nstride * N + 256) || !fits_i32(y.nstride * N + 256) || !fits_i32(int64_t(pln.krows) * pln.Mp) ||
      !fits_i32(p.Ntot + 256) || (p.Ntot + 127) / 128 * ((g.M + 31) / 32) >= (int64_t(1) << 31))
    return set_error(ctx, ORE_ERR_INVALID, "conv geometry exceeds 32-bit indexing");
  // the NHWC_VEC kernel reads x through a buffer resource
  const int xes = nchw ? 4 : 2;
  const ChunkSide xs{x.nstride, (nchw ? g.C * x_ps : g.H * g.W * x_ps) * xes, xes};
  const ChunkSide ys{y.nstride, (ep ? ep->win.Ho * ep->win.Wo : g.win.Ho * g.win.Wo) * y_ps * 2, 2};
  const int64_t nb = image_chunk(N, xs, ys);
  if (nb == 0) return set_error(ctx, ORE_ERR_UNSUPPORTED, "f16 conv: one image exceeds 2 GiB");
  int tile = -1;
  for (Chunk c = chunk_at(0, N, nb); c.nc > 0; c = chunk_at(c.i0 + c.nc, N, nb)) {
    ConvParams q = p;
    q.x = reinterpret_cast<const float*>(reinterpret_cast<const char*>(x.p) + c.i0 * x.nstride * xes);
    q.y = reinterpret_cast<float*>(reinterpret_cast<char*>(y.p) + c.i0 * y.nstride * 2);
    q.N = int(c.nc);
    q.Ntot = ep ? epool_columns(p, c.nc) : c.nc * p.P;
    q.x_bytes = xs.bytes(c.nc);
    if (ep)
      launch_conv_f16_epool(q, pln.xmode, ctx->stream);
    else
      tile = launch_conv(q, pln, ctx->stream);
    ORE_HIP_CHECK(ctx, hipGetLastError());
  }
  return {ORE_OK, tile};
}

// the PoolParams / NhwcPoolParams fields the two MaxPool layouts share
template <class P>
static void pool_params(P* p, int64_t N, int64_t C, int64_t H, int64_t W, const PoolGeom& g) {
  p->N = int(N); p->C = int(C); p->H = int(H); p->W = int(W);
  p->kh = int(g.kh); p->kw = int(g.kw); p->sh = int(g.sh); p->sw = int(g.sw);
  p->pt = int(g.win.pt); p->pl = int(g.win.pl);
  p->Ho = int(g.win.Ho); p->Wo = int(g.win.Wo);
}

ore_status run_maxpool(ore_ctx* ctx, const Ref& x, const Ref& y, int64_t N, int64_t C, int64_t H, int64_t W,
                       const PoolGeom& pool) {
  if (N == 0) return ORE_OK;
  if (x.es == 2) {
    NhwcPoolParams p{};
    pool_params(&p, N, C, H, W, pool);
    p.x = reinterpret_cast<const _Float16*>(x.p); p.y = reinterpret_cast<_Float16*>(y.p);
    p.x_cs = int(pixel_stride(x, C)); p.y_cs = int(pixel_stride(y, C));
    p.x_nstride = x.nstride; p.y_nstride = y.nstride;
    launch_maxpool_nhwc(p, ctx->stream);
  } else {
    PoolParams p{};
    pool_params(&p, N, C, H, W, pool);
    p.es = x.es;
    p.variant = ctx->pool_variant;
    p.x_ps = int(plane_stride(x, H * W));
    p.y_ps = int(plane_stride(y, pool.win.Ho * pool.win.Wo));
    p.x = x.p; p.y = y.p;
    p.x_nstride = x.nstride; p.y_nstride = y.nstride;
    launch_maxpool(p, ctx->stream);
  }
  ORE_HIP_CHECK(ctx, hipGetLastError());
  return ORE_OK;
}

}  // namespace ore

using namespace ore;

// =================================================================================== C ABI
extern "C" {

int32_t ore_abi_version(void) { return ORE_ABI_VERSION; }

const char* ore_last_error(ore_ctx* ctx) { return ctx ? ctx->err.c_str() : g_global_err.c_str(); }

ore_status ore_ctx_create(int32_t device, ore_ctx** out) {
  if (!out) return set_error(nullptr, ORE_ERR_INVALID, "null out");
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n <= 0) return set_error(nullptr, ORE_ERR_HIP, "no HIP device available");
  if (device < 0 || device >= n) return set_error(nullptr, ORE_ERR_INVALID, "device %d out of range", device);
  ORE_HIP_CHECK(nullptr, hipSetDevice(device));
  ore_ctx* c = new ore_ctx();
  c->device = device;
  if (hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking) != hipSuccess) {
    delete c;
    return set_error(nullptr, ORE_ERR_HIP, "hipStreamCreate failed");
  }
  c->stream = c->own_stream;
  *out = c;
  return ORE_OK;
}

ore_status ore_ctx_destroy(ore_ctx* ctx) {
  if (!ctx) return ORE_OK;
  (void)hipSetDevice(ctx->device);
  if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
  else (void)hipDeviceSynchronize();
  if (ctx->scratch) (void)hipFree(ctx->scratch);
  if (ctx->own_stream) {
    (void)hipStreamSynchronize(ctx->own_stream);
    (void)hipStreamDestroy(ctx->own_stream);
  }
  delete ctx;
  return ORE_OK;
}

ore_status ore_ctx_set_conv_algo(ore_ctx* ctx, int32_t algo) {
  if (!ctx) return set_error(nullptr, ORE_ERR_INVALID, "null context");
  if (algo != ORE_CONV_ALGO_DIRECT && algo != ORE_CONV_ALGO_WINOGRAD)
    return set_error(ctx, ORE_ERR_INVALID, "unknown conv algorithm %d", int(algo));
  ctx->conv_algo = algo;
  return ORE_OK;
}

ore_status ore_ctx_set_conv_tile(ore_ctx* ctx, int32_t tile) {
  if (!ctx) return set_error(nullptr, ORE_ERR_INVALID, "null context");
  const bool sp = tile >= CONV_TILE_SP && tile < CONV_TILE_SP + CONV_TILES_SP;
  if (conv_tile_retired(tile)) return set_error(ctx, ORE_ERR_UNSUPPORTED, "conv tile %d was retired (ABI 2)", int(tile));
  if (!sp && (tile < -1 || tile >= WINO_TILE_BASE + WINO_TILES_N))
    return set_error(ctx, ORE_ERR_INVALID, "conv tile %d is not a conv tile id", int(tile));
  ctx->conv_tile = tile;
  return ORE_OK;
}

ore_status ore_ctx_set_pool_variant(ore_ctx* ctx, int32_t variant) {
  if (!ctx) return set_error(nullptr, ORE_ERR_INVALID, "null context");
  if (variant == 1) return set_error(ctx, ORE_ERR_UNSUPPORTED, "MaxPool variant 1 was retired (ABI 2)");
  if (variant != 0 && (variant < 2 || variant > 5)) return set_error(ctx, ORE_ERR_INVALID, "unknown MaxPool variant %d", int(variant));
  ctx->pool_variant = variant;
  return ORE_OK;
}

ore_status ore_ctx_set_resize_variant(ore_ctx* ctx, int32_t variant) {
  if (!ctx) return set_error(nullptr, ORE_ERR_INVALID, "null context");
  if (variant < 0 || variant > 1) return set_error(ctx, ORE_ERR_INVALID, "unknown resize variant %d", int(variant));
  ctx->resize_variant = variant;
  return ORE_OK;
}

ore_status ore_ctx_set_alloc_fill(ore_ctx* ctx, int32_t on, uint32_t pattern) {
  if (!ctx) return set_error(nullptr, ORE_ERR_INVALID, "null context");
  ctx->alloc_fill = on != 0;
  ctx->alloc_pattern = pattern;
  return ORE_OK;
}

ore_status ore_ctx_set_stream(ore_ctx* ctx, void* s) {
  if (!ctx) return set_error(nullptr, ORE_ERR_INVALID, "null ctx");
  ctx->stream = reinterpret_cast<hipStream_t>(s);
  return ORE_OK;
}

void* ore_ctx_get_stream(ore_ctx* ctx) { return ctx ? reinterpret_cast<void*>(ctx->stream) : nullptr; }

ore_status ore_sync(ore_ctx* ctx) {
  if (!ctx) return set_error(nullptr, ORE_ERR_INVALID, "null ctx");
  ORE_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  ORE_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  return ORE_OK;
}

ore_status ore_malloc(ore_ctx* ctx, size_t bytes, void** dptr) {
  if (!ctx || !dptr) return set_error(ctx, ORE_ERR_INVALID, "null argument");
  ORE_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  if (device_alloc(ctx, dptr, bytes ? bytes : 1, false) != hipSuccess) return set_error(ctx, ORE_ERR_OOM, "hipMalloc(%zu) failed", bytes);
  return ORE_OK;
}

ore_status ore_free(ore_ctx* ctx, void* dptr) {
  if (!ctx) return set_error(nullptr, ORE_ERR_INVALID, "null ctx");
  if (dptr) ORE_HIP_CHECK(ctx, hipFree(dptr));
  return ORE_OK;
}

ore_status ore_upload(ore_ctx* ctx, void* dst, const void* src, size_t bytes) {
  if (!ctx) return set_error(nullptr, ORE_ERR_INVALID, "null ctx");
  ORE_HIP_CHECK(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, ctx->stream));
  ORE_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  return ORE_OK;
}

ore_status ore_download(ore_ctx* ctx, void* dst, const void* src, size_t bytes) {
  if (!ctx) return set_error(nullptr, ORE_ERR_INVALID, "null ctx");
  ORE_HIP_CHECK(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ctx->stream));
  ORE_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  return ORE_OK;
}

// ----------------------------------------------------------------------------- shapes
static ore_status conv_geometry(ore_ctx* ctx, const int64_t xd[4], const int64_t wd[4], const ore_conv_attrs* a,
                                Window* win) {
  if (!a) return set_error(ctx, ORE_ERR_INVALID, "null conv attrs");
  if (a->group != 1 || xd[1] != wd[1])  // assert at convolution_op.rs:252
    return set_error(ctx, ORE_ERR_UNSUPPORTED, "Conv: group must be 1 and Cin must match the weights");
  if (a->dilations[0] != 1 || a->dilations[1] != 1)
    return set_error(ctx, ORE_ERR_UNSUPPORTED, "Conv: dilation > 1 is not supported by the reference path");
  int auto_pad = a->auto_pad;
  if (a->n_pads >= 4 && (a->pads[0] > 0 || a->pads[1] > 0 || a->pads[2] > 0 || a->pads[3] > 0))
    auto_pad = ORE_PAD_NOTSET;  // convolution_op.rs:169-173
  return resolve_window(ctx, auto_pad, a->pads, a->n_pads, xd[2], xd[3], wd[2], wd[3], a->strides[0],
                        a->strides[1], win);
}

ore_status ore_conv_out_shape(const int64_t x_dims[4], const int64_t w_dims[4], const ore_conv_attrs* a,
                              int64_t y_dims[4], int64_t pads_tlbr[4]) {
  Window win;
  ore_status st = conv_geometry(nullptr, x_dims, w_dims, a, &win);
  if (st) return st;
  y_dims[0] = x_dims[0]; y_dims[1] = w_dims[0]; y_dims[2] = win.Ho; y_dims[3] = win.Wo;
  if (pads_tlbr) { pads_tlbr[0] = win.pt; pads_tlbr[1] = win.pl; pads_tlbr[2] = win.pb; pads_tlbr[3] = win.pr; }
  return ORE_OK;
}

ore_status ore_pool_out_shape(const int64_t x_dims[4], const ore_pool_attrs* a, int64_t y_dims[4],
                              int64_t pads_tlbr[4]) {
  if (!a) return set_error(nullptr, ORE_ERR_INVALID, "null pool attrs");
  Window win;
  ore_status st = resolve_window(nullptr, a->auto_pad, a->pads, a->n_pads, x_dims[2], x_dims[3], a->kernel[0],
                                 a->kernel[1], a->strides[0], a->strides[1], &win);
  if (st) return st;
  y_dims[0] = x_dims[0]; y_dims[1] = x_dims[1]; y_dims[2] = win.Ho; y_dims[3] = win.Wo;
  if (pads_tlbr) { pads_tlbr[0] = win.pt; pads_tlbr[1] = win.pl; pads_tlbr[2] = win.pb; pads_tlbr[3] = win.pr; }
  return ORE_OK;
}

// ----------------------------------------------------------------------------- ops
ore_status ore_conv2d_f32(ore_ctx* ctx, const ore_tensor* x, const ore_tensor* w, const ore_tensor* bias,
                          const ore_conv_attrs* a, ore_tensor* y) {
  if (!ctx || !x || !w || !y || !a) return set_error(ctx, ORE_ERR_INVALID, "null argument");
  if (x->ndim != 4 || w->ndim != 4 || y->ndim != 4) return set_error(ctx, ORE_ERR_INVALID, "Conv expects 4-D x, w, y");
  if (!contiguous(w)) return set_error(ctx, ORE_ERR_INVALID, "Conv weights must be contiguous");
  Window win;
  ore_status st = conv_geometry(ctx, x->dims, w->dims, a, &win);
  if (st) return st;
  if (bias && (bias->ndim != 1 || bias->dims[0] != w->dims[0]))
    return set_error(ctx, ORE_ERR_INVALID, "Bias array has the wrong shape");  // add_bias :710
  if (y->dims[0] != x->dims[0] || y->dims[1] != w->dims[0] || y->dims[2] != win.Ho || y->dims[3] != win.Wo)
    return set_error(ctx, ORE_ERR_INVALID, "Conv output dims mismatch: expected [%lld,%lld,%lld,%lld]",
                     (long long)x->dims[0], (long long)w->dims[0], (long long)win.Ho, (long long)win.Wo);
  if (ore_status sx = check_image_stride(ctx, "Conv", "x", x)) return sx;
  if (ore_status sy = check_image_stride(ctx, "Conv", "y", y)) return sy;
  if (x->dims[0] == 0) return ORE_OK;
  const int2* kt = nullptr;
  const ConvGeom g{x->dims[1], x->dims[2], x->dims[3], w->dims[0], w->dims[2], w->dims[3], a->strides[0], a->strides[1],
                   win, a->fuse_relu != 0};
  const ConvPlan pln = conv_plan(g.M, g.C, g.H, g.W, g.kh, g.kw, g.sh, g.sw, win, false, 0,
                                 ctx->conv_algo == ORE_CONV_ALGO_WINOGRAD, ctx->conv_tile);
  float* wp = pack_to_scratch(ctx, pln, w->data, false, g.M, g.C, g.kh, g.kw, g.H, g.W, &kt);
  if (!wp) return ORE_ERR_OOM;
  return run_conv(ctx, pln, ref_of(x), ref_of(y), x->dims[0], g, {wp, kt, bias ? bias->data : nullptr}).st;
}

ore_status ore_maxpool2d_f32(ore_ctx* ctx, const ore_tensor* x, const ore_pool_attrs* a, ore_tensor* y) {
  if (!ctx || !x || !y || !a) return set_error(ctx, ORE_ERR_INVALID, "null argument");
  if (x->ndim != 4 || y->ndim != 4) return set_error(ctx, ORE_ERR_INVALID, "MaxPool expects 4-D tensors");
  Window win;
  ore_status st = resolve_window(ctx, a->auto_pad, a->pads, a->n_pads, x->dims[2], x->dims[3], a->kernel[0],
                                 a->kernel[1], a->strides[0], a->strides[1], &win);
  if (st) return st;
  if (y->dims[0] != x->dims[0] || y->dims[1] != x->dims[1] || y->dims[2] != win.Ho || y->dims[3] != win.Wo)
    return set_error(ctx, ORE_ERR_INVALID, "MaxPool output dims mismatch");
  if (ore_status sx = check_image_stride(ctx, "MaxPool", "x", x)) return sx;
  if (ore_status sy = check_image_stride(ctx, "MaxPool", "y", y)) return sy;
  return run_maxpool(ctx, ref_of(x), ref_of(y), x->dims[0], x->dims[1], x->dims[2], x->dims[3],
                     {a->kernel[0], a->kernel[1], a->strides[0], a->strides[1], win});
}

ore_status ore_relu_f32(ore_ctx* ctx, const ore_tensor* x, ore_tensor* y) {
  if (!ctx || !x || !y) return set_error(ctx, ORE_ERR_INVALID, "null argument");
  if (numel(x) != numel(y)) return set_error(ctx, ORE_ERR_INVALID, "Relu size mismatch");
  if (!contiguous(x) || !contiguous(y)) return set_error(ctx, ORE_ERR_INVALID, "Relu expects contiguous tensors");
  launch_relu(x->data, y->data, numel(x), ctx->stream);
  ORE_HIP_CHECK(ctx, hipGetLastError());
  return ORE_OK;
}

ore_status ore_add_f32(ore_ctx* ctx, const ore_tensor* a, const ore_tensor* b, ore_tensor* y) {
  if (!ctx || !a || !b || !y) return set_error(ctx, ORE_ERR_INVALID, "null argument");
  if (b->ndim > a->ndim || a->ndim > 4 || a->ndim < 1) return set_error(ctx, ORE_ERR_INVALID, "Add: rank mismatch");
  if (!contiguous(a) || !contiguous(b) || !contiguous(y) || numel(a) != numel(y))
    return set_error(ctx, ORE_ERR_INVALID, "Add expects contiguous, same-size a and y");
  AddParams p{};
  p.a = a->data; p.b = b->data; p.y = y->data;
  int64_t bd[4] = {1, 1, 1, 1};
  for (int i = 0; i < 4; ++i) p.d[i] = 1;
  for (int i = 0; i < a->ndim; ++i) p.d[4 - a->ndim + i] = a->dims[i];
  for (int i = 0; i < b->ndim; ++i) bd[4 - b->ndim + i] = b->dims[i];
  int64_t s = 1;
  for (int i = 3; i >= 0; --i) {
    if (bd[i] != 1 && bd[i] != p.d[i]) return set_error(ctx, ORE_ERR_INVALID, "Add: shapes not broadcastable");
    p.bs[i] = bd[i] == 1 ? 0 : s;
    s *= bd[i];
  }
  if (numel(a) == 0) return ORE_OK;
  launch_add_bcast(p, ctx->stream);
  ORE_HIP_CHECK(ctx, hipGetLastError());
  return ORE_OK;
}

ore_status ore_softmax_f32(ore_ctx* ctx, const ore_tensor* x, ore_tensor* y) {
  if (!ctx || !x || !y) return set_error(ctx, ORE_ERR_INVALID, "null argument");
  if (!contiguous(x) || !contiguous(y) || numel(x) != numel(y))
    return set_error(ctx, ORE_ERR_INVALID, "Softmax expects contiguous same-size tensors");
  const int64_t rows = x->dims[0];
  if (rows == 0) return ORE_OK;
  const int64_t D = numel(x) / rows;
  if (D <= 0 || D >= (int64_t(1) << 31)) return set_error(ctx, ORE_ERR_INVALID, "Softmax row length");
  launch_softmax(x->data, y->data, rows, int(D), ctx->stream);
  ORE_HIP_CHECK(ctx, hipGetLastError());
  return ORE_OK;
}

ore_status ore_topk_f32(ore_ctx* ctx, const ore_tensor* x, int32_t k, float* values, int32_t* indices) {
  return ore_topk_mean_f32(ctx, x, 1, k, values, indices);  // one view: launch_topk_mean hands it to launch_topk
}

ore_status ore_topk_mean_f32(ore_ctx* ctx, const ore_tensor* x, int32_t views, int32_t k, float* values, int32_t* indices) {
  // the context last: what can be judged without one is (a null context still gets the message)
  if (!x || !x->data || !values || !indices) return set_error(ctx, ORE_ERR_INVALID, "null argument");
  if (x->ndim < 1 || x->ndim > 4) return set_error(ctx, ORE_ERR_INVALID, "top-k input of %d dims", int(x->ndim));
  const int64_t rows = x->dims[0];
  int64_t D = 1;
  for (int i = 1; i < x->ndim; ++i) D *= x->dims[i];
  if (rows < 0 || D <= 0 || !fits_i32(D) || nstride_of(x) < D) return set_error(ctx, ORE_ERR_INVALID, "top-k row length");
  if (views < 1 || views > ORE_MAX_VIEWS)
    return set_error(ctx, ORE_ERR_INVALID, "top-k views = %d outside 1..%d (ORE_MAX_VIEWS)", int(views), ORE_MAX_VIEWS);
  if (rows % views != 0)
    return set_error(ctx, ORE_ERR_INVALID, "top-k of %lld rows: not a multiple of views = %d", (long long)rows, int(views));
  if (k < 1 || k > std::min<int64_t>(D, 64))
    return set_error(ctx, ORE_ERR_INVALID, "top-k k = %d outside 1..%lld (min(row length, 64))", int(k),
                     (long long)std::min<int64_t>(D, 64));
  if (!ctx) return set_error(ctx, ORE_ERR_INVALID, "null argument");
  if (rows == 0) return ORE_OK;
  ORE_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  launch_topk_mean(x->data, nstride_of(x), rows / views, int(views), int(D), int(k), values, indices, ctx->stream);
  ORE_HIP_CHECK(ctx, hipGetLastError());
  return ORE_OK;
}

ore_status ore_class_maps_f32(ore_ctx* ctx, const ore_tensor* x, const float* w, const float* bias, int64_t M, int32_t relu,
                              const int32_t* classes, int32_t k, int32_t views, float* maps) {
  // the context last, as ore_topk_mean_f32: what can be judged without one is
  if (!x || !x->data || !w || !classes || !maps) return set_error(ctx, ORE_ERR_INVALID, "null argument");
  if (x->ndim != 4) return set_error(ctx, ORE_ERR_INVALID, "class maps: x of %d dims, expected [n, C, H, W]", int(x->ndim));
  const int64_t n = x->dims[0], C = x->dims[1], P = x->dims[2] * x->dims[3];
  if (n < 0 || C <= 0 || x->dims[2] <= 0 || x->dims[3] <= 0 || M <= 0 || !fits_i32(C) || !fits_i32(P) || !fits_i32(M))
    return set_error(ctx, ORE_ERR_INVALID, "class maps: x [%lld, %lld, %lld, %lld] and M = %lld", (long long)n, (long long)C,
                     (long long)x->dims[2], (long long)x->dims[3], (long long)M);
  if (k < 1 || k > std::min<int64_t>(M, 64))
    return set_error(ctx, ORE_ERR_INVALID, "class maps: k = %d outside 1..%lld (min(M, 64))", int(k),
                     (long long)std::min<int64_t>(M, 64));
  if (views < 1 || views > ORE_MAX_VIEWS)
    return set_error(ctx, ORE_ERR_INVALID, "class maps: views = %d outside 1..%d (ORE_MAX_VIEWS)", int(views), ORE_MAX_VIEWS);
  if (n % views != 0)
    return set_error(ctx, ORE_ERR_INVALID, "class maps of %lld images: not a multiple of views = %d", (long long)n, int(views));
  if (ore_status st = check_image_stride(ctx, "class maps", "x", x)) return st;
  if (!ctx) return set_error(ctx, ORE_ERR_INVALID, "null argument");
  if (n == 0) return ORE_OK;
  const ClassMaps p{x->data, w, bias, classes, maps, nstride_of(x), int(n), int(C), int(P), int(M), int(k), int(views),
                    relu ? 1 : 0, int(P)};
  if (!class_maps_eligible(p)) return set_error(ctx, ORE_ERR_INVALID, "class maps: %lld images of %lld pixels exceed one launch",
                                                (long long)n, (long long)P);
  ORE_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  launch_class_maps_f32(p, ctx->stream);
  ORE_HIP_CHECK(ctx, hipGetLastError());
  return ORE_OK;
}

static_assert(CAM_BOX_MAX_MAP == ORE_CAM_BOX_MAX_MAP && CAM_BOX_MAX_SIDE == ORE_CAM_BOX_MAX_SIDE, "ore.h and ore_kernels.h");

// the rules that ore_cam_boxes_f32 and ore_cam_box_host share, behind their pointer checks, in the header's order
static ore_status check_cam_box_shape(ore_ctx* ctx, int64_t hm, int64_t wm, int64_t h, int64_t w, float frac) {
  if (const char* what = cam_boxes_unsupported(hm, wm, h, w)) {
    if (what[0] == 'm')
      return set_error(ctx, ORE_ERR_INVALID, "cam boxes: a map of hm x wm = %lld x %lld, expected hm, wm >= 1 and hm * wm <= %d "
                       "(ORE_CAM_BOX_MAX_MAP)", (long long)hm, (long long)wm, ORE_CAM_BOX_MAX_MAP);
    return set_error(ctx, ORE_ERR_INVALID, "cam boxes: %s = %lld outside 1..%d (ORE_CAM_BOX_MAX_SIDE)", what,
                     (long long)(what[0] == 'h' ? h : w), ORE_CAM_BOX_MAX_SIDE);
  }
  if (h < hm) return set_error(ctx, ORE_ERR_INVALID, "cam boxes: h = %lld below hm = %lld (the map is only enlarged)", (long long)h, (long long)hm);
  if (w < wm) return set_error(ctx, ORE_ERR_INVALID, "cam boxes: w = %lld below wm = %lld (the map is only enlarged)", (long long)w, (long long)wm);
  if (!(frac >= 0.0f && frac <= 1.0f)) return set_error(ctx, ORE_ERR_INVALID, "cam boxes: frac = %g outside [0, 1]", double(frac));
  return ORE_OK;
}

ore_status ore_upsample_maps_f32(ore_ctx* ctx, const float* maps, int64_t planes, int64_t hm, int64_t wm, int64_t h, int64_t w,
                                 float* out) {
  if (!maps || !out) return set_error(ctx, ORE_ERR_INVALID, "null argument");
  if (planes < 0) return set_error(ctx, ORE_ERR_INVALID, "upsample maps: planes = %lld", (long long)planes);
  const int64_t sides[4] = {hm, wm, h, w};
  const char* const names[4] = {"hm", "wm", "h", "w"};
  for (int i = 0; i < 4; ++i)
    if (sides[i] < 1 || sides[i] > RESIZE_MAX)
      return set_error(ctx, ORE_ERR_INVALID, "upsample maps: %s = %lld outside 1..%d", names[i], (long long)sides[i], RESIZE_MAX);
  if (h < hm) return set_error(ctx, ORE_ERR_INVALID, "upsample maps: h = %lld below hm = %lld (the map is only enlarged)", (long long)h, (long long)hm);
  if (w < wm) return set_error(ctx, ORE_ERR_INVALID, "upsample maps: w = %lld below wm = %lld (the map is only enlarged)", (long long)w, (long long)wm);
  if (planes > ((int64_t(1) << 31) - 1) / (h * w))
    return set_error(ctx, ORE_ERR_INVALID, "upsample maps: planes * h * w = %lld * %lld * %lld is not below 2^31", (long long)planes,
                     (long long)h, (long long)w);
  if (!ctx) return set_error(ctx, ORE_ERR_INVALID, "null argument");
  if (planes == 0) return ORE_OK;
  ORE_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  launch_upsample_maps_f32(maps, planes, int(hm), int(wm), int(h), int(w), out, ctx->stream);
  ORE_HIP_CHECK(ctx, hipGetLastError());
  return ORE_OK;
}

ore_status ore_cam_boxes_f32(ore_ctx* ctx, const float* maps, int64_t planes, int64_t hm, int64_t wm, int64_t h, int64_t w,
                             float frac, int32_t* boxes, int32_t* areas) {
  if (!maps || !boxes) return set_error(ctx, ORE_ERR_INVALID, "null argument");
  if (planes < 0 || !fits_i32(planes)) return set_error(ctx, ORE_ERR_INVALID, "cam boxes: planes = %lld", (long long)planes);
  if (ore_status st = check_cam_box_shape(ctx, hm, wm, h, w, frac)) return st;
  if (!ctx) return set_error(ctx, ORE_ERR_INVALID, "null argument");
  if (planes == 0) return ORE_OK;
  ORE_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  launch_cam_boxes_f32(maps, planes, int(hm), int(wm), int(h), int(w), frac, boxes, areas, ctx->stream);
  ORE_HIP_CHECK(ctx, hipGetLastError());
  return ORE_OK;
}

// The arithmetic of include/ore.h in plain C++: the resized plane from resize_tap and resize_lerp_rn, lo / hi by
// comparisons (a NaN never enters), the mask, and a queue flood fill over the pixels in raster order, so that the
// components come in the order of their first pixels and a later one must be strictly larger to win.
ore_status ore_cam_box_host(const float* map, int64_t hm, int64_t wm, int64_t h, int64_t w, float frac, int32_t box[4],
                            int32_t* area) {
  if (!map || !box) return set_error(nullptr, ORE_ERR_INVALID, "null argument");
  if (ore_status st = check_cam_box_shape(nullptr, hm, wm, h, w, frac)) return st;
  const int H = int(h), W = int(w), Wm = int(wm);
  std::vector<ResizeTap> ty(H), tx(W);
  for (int r = 0; r < H; ++r) ty[r] = resize_tap(int(hm), H, r);
  for (int q = 0; q < W; ++q) tx[q] = resize_tap(Wm, W, q);
  std::vector<float> u(size_t(H) * W);
  float lo = INFINITY, hi = -INFINITY;
  for (int r = 0; r < H; ++r)
    for (int q = 0; q < W; ++q) {
      const float* r0 = map + ty[r].i0 * Wm;
      const float* r1 = map + ty[r].i1 * Wm;
      const float top = resize_lerp_rn(r0[tx[q].i0], r0[tx[q].i1], tx[q].t);
      const float bot = resize_lerp_rn(r1[tx[q].i0], r1[tx[q].i1], tx[q].t);
      const float v = resize_lerp_rn(top, bot, ty[r].t);
      u[size_t(r) * W + q] = v;
      if (v < lo) lo = v;
      if (v > hi) hi = v;
    }
  // no non-NaN value leaves lo = +inf, hi = -inf: the threshold is then NaN, as that of the NaN reductions is
  const float thr = resize_lerp_rn(lo, hi, frac);
  std::vector<uint8_t> todo(size_t(H) * W);
  for (size_t i = 0; i < todo.size(); ++i) todo[i] = u[i] >= thr;
  std::vector<int> queue;
  int best = 0, bt = 0, bl = 0, bb = 0, br = 0;
  for (int s = 0; s < H * W; ++s) {
    if (!todo[s]) continue;
    queue.assign(1, s);
    todo[s] = 0;
    int t = H, l = W, b = -1, rr = -1;
    for (size_t k = 0; k < queue.size(); ++k) {
      const int r = queue[k] / W, q = queue[k] - r * W;
      t = std::min(t, r), b = std::max(b, r), l = std::min(l, q), rr = std::max(rr, q);
      for (int dr = -1; dr <= 1; ++dr)
        for (int dq = -1; dq <= 1; ++dq) {
          const int r2 = r + dr, q2 = q + dq;
          if (r2 < 0 || r2 >= H || q2 < 0 || q2 >= W || !todo[r2 * W + q2]) continue;
          todo[r2 * W + q2] = 0;
          queue.push_back(r2 * W + q2);
        }
    }
    if (int(queue.size()) > best) best = int(queue.size()), bt = t, bl = l, bb = b + 1, br = rr + 1;
  }
  box[0] = bt, box[1] = bl, box[2] = bb, box[3] = br;
  if (area) *area = best;
  return ORE_OK;
}

ore_status ore_matmul_f32(ore_ctx* ctx, const ore_tensor* a, const ore_tensor* b, ore_tensor* y) {
  if (!ctx || !a || !b || !y) return set_error(ctx, ORE_ERR_INVALID, "null argument");
  if (a->ndim != 2 || b->ndim != 2 || y->ndim != 2 || a->dims[1] != b->dims[0] || y->dims[0] != a->dims[0] ||
      y->dims[1] != b->dims[1])
    return set_error(ctx, ORE_ERR_INVALID, "MatMul expects a[M,K] . b[K,N] -> y[M,N]");
  if (!contiguous(a) || !contiguous(b) || !contiguous(y))
    return set_error(ctx, ORE_ERR_INVALID, "MatMul expects contiguous tensors");
  // y[m][n] = sum_k a[m][k] b[k][n]  ==  1x1 conv over "images" m with Cin = K, Cout = N and
  // K-major weights b: the MFMA implicit-GEMM kernel, columns = rows of a.
  Window win;
  win.Ho = 1; win.Wo = 1;
  if (a->dims[0] == 0) return ORE_OK;
  const int2* kt = nullptr;
  const ConvPlan pln = conv_plan(b->dims[1], b->dims[0], 1, 1, 1, 1, 1, 1, win, false, 0, false, ctx->conv_tile);
  float* wp = pack_to_scratch(ctx, pln, b->data, true, b->dims[1], b->dims[0], 1, 1, 1, 1, &kt);
  if (!wp) return ORE_ERR_OOM;
  const ConvGeom g{a->dims[1], 1, 1, b->dims[1], 1, 1, 1, 1, win, false};
  return run_conv(ctx, pln, ref_of(a), ref_of(y), a->dims[0], g, {wp, kt, nullptr}).st;
}

ore_status ore_gap_f32(ore_ctx* ctx, const ore_tensor* x, ore_tensor* y) {
  if (!ctx || !x || !y) return set_error(ctx, ORE_ERR_INVALID, "null argument");
  if (x->ndim != 4 || !contiguous(x) || !contiguous(y) || numel(y) != x->dims[0] * x->dims[1])
    return set_error(ctx, ORE_ERR_INVALID, "GlobalAveragePool expects contiguous [N,C,H,W] -> [N,C,1,1]");
  const int64_t HW = x->dims[2] * x->dims[3];
  if (HW <= 0 || HW >= (int64_t(1) << 31)) return set_error(ctx, ORE_ERR_INVALID, "GAP spatial size");
  launch_gap(x->data, 4, y->data, x->dims[0] * x->dims[1], int(HW), int(HW), ctx->stream);
  ORE_HIP_CHECK(ctx, hipGetLastError());
  return ORE_OK;
}

ore_status ore_concat_f32(ore_ctx* ctx, const ore_tensor* a, const ore_tensor* b, int64_t axis, ore_tensor* y) {
  if (!ctx || !a || !b || !y) return set_error(ctx, ORE_ERR_INVALID, "null argument");
  if (a->ndim != 4 || b->ndim != 4 || y->ndim != 4 || axis < 0 || axis > 3)
    return set_error(ctx, ORE_ERR_INVALID, "Concat expects 4-D tensors and axis in [0,3]");
  for (int i = 0; i < 4; ++i) {
    const int64_t want = (i == axis) ? a->dims[i] + b->dims[i] : a->dims[i];
    if ((i != axis && a->dims[i] != b->dims[i]) || y->dims[i] != want)
      return set_error(ctx, ORE_ERR_INVALID, "Concat shape mismatch");
  }
  if (!contiguous(a) || !contiguous(b) || !contiguous(y))
    return set_error(ctx, ORE_ERR_INVALID, "Concat expects contiguous tensors");
  int64_t outer = 1, ia = 1, ib = 1;
  for (int i = 0; i < axis; ++i) outer *= a->dims[i];
  for (int i = int(axis); i < 4; ++i) { ia *= a->dims[i]; ib *= b->dims[i]; }
  if (outer * (ia + ib) == 0) return ORE_OK;
  launch_concat(a->data, b->data, y->data, 4, outer, ia, ib, ctx->stream);
  ORE_HIP_CHECK(ctx, hipGetLastError());
  return ORE_OK;
}

ore_status ore_dropout_f32(ore_ctx* ctx, const ore_tensor* x, ore_tensor* y) {
  if (!ctx || !x || !y) return set_error(ctx, ORE_ERR_INVALID, "null argument");
  if (numel(x) != numel(y) || !contiguous(x) || !contiguous(y))
    return set_error(ctx, ORE_ERR_INVALID, "Dropout size mismatch");
  if (x->data == y->data) return ORE_OK;
  ORE_HIP_CHECK(ctx, hipMemcpyAsync(y->data, x->data, size_t(numel(x)) * 4, hipMemcpyDeviceToDevice, ctx->stream));
  return ORE_OK;
}

ore_status ore_preprocess_u8(ore_ctx* ctx, const uint8_t* x, int64_t n, int64_t h, int64_t w, int64_t c, const float* scale,
                             const float* shift, int32_t flags, ore_tensor* y) {
  if (!ctx || !x || !y || !y->data) return set_error(ctx, ORE_ERR_INVALID, "null argument");
  PreprocParams p;
  if (ore_status st = preproc_params(ctx, h, w, c, scale, shift, flags, &p)) return st;
  if (n < 0) return set_error(ctx, ORE_ERR_INVALID, "negative batch %lld", (long long)n);
  if (y->ndim != 4 || y->dims[0] != n || y->dims[1] != c || y->dims[2] != h || y->dims[3] != w || nstride_of(y) < c * h * w)
    return set_error(ctx, ORE_ERR_INVALID, "preprocess output must be a [n,c,h,w] view of the [n,h,w,c] input");
  if (n == 0) return ORE_OK;
  p.x = x;
  p.y = y->data;
  p.N = n;
  p.y_nstride = nstride_of(y);
  ORE_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  launch_preproc_u8(p, ctx->stream);
  ORE_HIP_CHECK(ctx, hipGetLastError());
  return ORE_OK;
}

ore_status ore_resize_taps(int64_t src, int64_t resized, int64_t origin, int64_t count, int32_t* i0, int32_t* i1, float* t) {
  if (!i0 || !i1 || !t) return set_error(nullptr, ORE_ERR_INVALID, "null argument");
  if (!resize_axis_ok(src, resized, origin, count))
    return set_error(nullptr, ORE_ERR_INVALID, "resize taps: %lld samples resized to %lld (each 1..%d), [%lld, %lld + %lld) of them",
                     (long long)src, (long long)resized, RESIZE_MAX, (long long)origin, (long long)origin, (long long)count);
  for (int64_t k = 0; k < count; ++k) {
    const ResizeTap r = resize_tap(int(src), int(resized), int(origin + k));
    i0[k] = r.i0;
    i1[k] = r.i1;
    t[k] = r.t;
  }
  return ORE_OK;
}

ore_status ore_resize_aa_taps(int64_t src, int64_t resized, int64_t origin, int64_t count, int32_t* first, int32_t* ntaps,
                              int32_t* sum, int32_t* weights) {
  if (!first || !ntaps || !sum) return set_error(nullptr, ORE_ERR_INVALID, "null argument");
  if (!resize_axis_ok(src, resized, origin, count))
    return set_error(nullptr, ORE_ERR_INVALID, "resize taps: %lld samples resized to %lld (each 1..%d), [%lld, %lld + %lld) of them",
                     (long long)src, (long long)resized, RESIZE_MAX, (long long)origin, (long long)origin, (long long)count);
  if (!resize_axis_shrinks(src, resized))
    return set_error(nullptr, ORE_ERR_INVALID, "resize taps: the axis does not shrink (%lld -> %lld): the antialiasing filter leaves "
                                               "it to ore_resize_taps", (long long)src, (long long)resized);
  if (!resize_axis_aa_ok(src, resized))
    return set_error(nullptr, ORE_ERR_INVALID, "resize taps: the antialiasing filter shrinks an axis at most %d times, not %lld -> %lld",
                     ORE_AA_MAX_RATIO, (long long)src, (long long)resized);
  for (int64_t k = 0; k < count; ++k) {
    const ResizeSpan r = resize_aa_span(int(src), int(resized), int(origin + k));
    first[k] = r.first;
    ntaps[k] = r.n;
    sum[k] = r.sum;
    if (weights)
      for (int j = 0; j < ORE_AA_MAX_TAPS; ++j)
        weights[k * ORE_AA_MAX_TAPS + j] = j < r.n ? resize_aa_weight(int(src), int(resized), int(origin + k), r.first + j) : 0;
  }
  return ORE_OK;
}

ore_status ore_resize_cubic_taps(int64_t src, int64_t resized, int64_t origin, int64_t count, int32_t filter, int32_t* first,
                                 int32_t* ntaps, float* weights, float* sum) {
  if (!first || !ntaps || !sum) return set_error(nullptr, ORE_ERR_INVALID, "null argument");
  if (filter != ORE_FILTER_BICUBIC && filter != ORE_FILTER_BICUBIC_AA)
    return set_error(nullptr, ORE_ERR_INVALID, "resize taps: filter %d is not a cubic filter", int(filter));
  if (!resize_axis_ok(src, resized, origin, count))
    return set_error(nullptr, ORE_ERR_INVALID, "resize taps: %lld samples resized to %lld (each 1..%d), [%lld, %lld + %lld) of them",
                     (long long)src, (long long)resized, RESIZE_MAX, (long long)origin, (long long)origin, (long long)count);
  if (filter == ORE_FILTER_BICUBIC_AA && !resize_axis_cubic_aa_ok(src, resized))
    return set_error(nullptr, ORE_ERR_INVALID, "resize taps: the antialiasing filter shrinks an axis at most %d times, not %lld -> %lld",
                     ORE_CUBIC_AA_MAX_RATIO, (long long)src, (long long)resized);
  const int S = int(src), D = int(resized);
  for (int64_t k = 0; k < count; ++k) {
    const int o = int(origin + k);
    float* w = weights ? weights + k * ORE_AA_MAX_TAPS : nullptr;
    if (w)
      for (int j = 0; j < ORE_AA_MAX_TAPS; ++j) w[j] = 0.f;
    if (filter == ORE_FILTER_BICUBIC) {
      const ResizeCubicTap r = resize_cubic_tap(S, D, o);
      first[k] = r.first;
      ntaps[k] = 4;
      sum[k] = 1.0f;
      if (w)
        for (int j = 0; j < 4; ++j) w[j] = r.w[j];
    } else {
      const ResizeCubicSpan r = resize_cubic_aa_span(S, D, o);
      first[k] = r.first;
      ntaps[k] = r.n;
      float W = 0.f;  // one rounded addition per tap, in ascending order
      for (int j = 0; j < r.n; ++j) {
        const float u = resize_cubic_aa_weight(S, D, o, r.first + j);
        if (w) w[j] = u;
        W = W + u;
      }
      sum[k] = W;
    }
  }
  return ORE_OK;
}

ore_status ore_preprocess_resize_u8(ore_ctx* ctx, const uint8_t* x, int64_t n, int64_t hs, int64_t ws, int64_t c,
                                    const ore_resize* g, const float* scale, const float* shift, int32_t flags, ore_tensor* y) {
  return ore_preprocess_resize_u8_ex(ctx, x, n, hs, ws, c, g, ORE_FILTER_BILINEAR, scale, shift, flags, y);
}

ore_status ore_preprocess_resize_u8_ex(ore_ctx* ctx, const uint8_t* x, int64_t n, int64_t hs, int64_t ws, int64_t c,
                                       const ore_resize* g, int32_t filter, const float* scale, const float* shift,
                                       int32_t flags, ore_tensor* y) {
  // the pointers, then the geometry, then the context: a host can exercise every check without a device
  if (!x || !g || !y || !y->data) return set_error(ctx, ORE_ERR_INVALID, "null argument");
  if (n < 0) return set_error(ctx, ORE_ERR_INVALID, "negative batch %lld", (long long)n);
  if (y->ndim != 4 || y->dims[0] != n || y->dims[1] != c)
    return set_error(ctx, ORE_ERR_INVALID, "resize output must be [n,c,H,W] for the [n,hs,ws,c] input");
  ResizeParams p;
  if (ore_status st = resize_params(ctx, hs, ws, c, y->dims[2], y->dims[3], g, scale, shift, flags, &p, filter)) return st;
  if (nstride_of(y) < c * y->dims[2] * y->dims[3])
    return set_error(ctx, ORE_ERR_INVALID, "resize output: image stride %lld below c*H*W", (long long)nstride_of(y));
  if (!ctx) return set_error(ctx, ORE_ERR_INVALID, "null context");
  if (n == 0) return ORE_OK;
  p.x = x;
  p.y = y->data;
  p.N = n;
  p.y_nstride = nstride_of(y);
  ORE_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  launch_resize_dense(p, filter, ctx->stream);
  ORE_HIP_CHECK(ctx, hipGetLastError());
  return ORE_OK;
}

ore_status ore_reshape(const ore_tensor* x, const int64_t* shape, int32_t n_shape, ore_tensor* y) {
  if (!x || !shape || !y) return set_error(nullptr, ORE_ERR_INVALID, "null argument");
  if (n_shape != 2) return set_error(nullptr, ORE_ERR_UNSUPPORTED, "Reshape produces 2-D only (reshape_op.rs:87-91)");
  if (!contiguous(x)) return set_error(nullptr, ORE_ERR_INVALID, "Reshape of a strided view");
  int64_t ns[2] = {shape[0], shape[1]};
  for (int i = 0; i < 2; ++i)
    if (ns[i] == 0) ns[i] = x->dims[i];  // allowzero = 0 (:69-83)
  if (ns[0] < 0 || ns[1] < 0 || ns[0] * ns[1] != numel(x))
    return set_error(nullptr, ORE_ERR_INVALID, "Reshape element count mismatch");
  *y = ore_tensor{};
  y->data = x->data;
  y->ndim = 2;
  y->dims[0] = ns[0];
  y->dims[1] = ns[1];
  return ORE_OK;
}

}  // extern "C"
