// Host-side internals shared by the C ABI implementation files.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <map>
#include <string>
#include <vector>

#include "../../include/ore.h"
#include "ore_kernels.h"

struct ore_ctx {
  int device = 0;
  hipStream_t own_stream = nullptr;
  hipStream_t stream = nullptr;
  std::string err;
  float* scratch = nullptr;  // per-op weight packing (stream-ordered reuse)
  size_t scratch_bytes = 0;
  // a device range known to be mapped, set by the model walker around its conv launches (its arena,
  // which has a 4 KiB lead): the streaming conv may read a few bytes before an input inside it
  const char* mapped_lo = nullptr;
  const char* mapped_hi = nullptr;
  int conv_algo = 0;     // ore_ctx_set_conv_algo (per-op ore_conv2d_f32 only)
  int conv_tile = -1;    // ore_ctx_set_conv_tile: a forced tile id (-1: per-layer heuristic / autotune)
  int pool_variant = 0;  // ore_ctx_set_pool_variant: a forced MaxPool kernel (0: by layout)
  int resize_variant = 0;  // ore_ctx_set_resize_variant: 0 by geometry, 1 thread per pixel -- one kernel today, so nothing reads it
  bool alloc_fill = false;         // ore_ctx_set_alloc_fill (debug): device_alloc fills what the library allocates for itself
  uint32_t alloc_pattern = 0;
};

// ore_image_list: a device table of `capacity` packed descriptors for one output shape and its pinned host
// mirror, both allocated at creation; table[0, count) is what the list's set entry uploaded last.  The descriptors
// are of the list's format, desc_bytes each: ResizeImage (ORE_IMAGE_INTERLEAVED), Nv12Image (ORE_IMAGE_NV12, c = 3)
// or YuvImage (ORE_IMAGE_YUV, c = 3); only the format's own set entry writes them (ore_image_list.cpp)
struct ore_image_list {
  ore_ctx* ctx = nullptr;
  int64_t capacity = 0, count = 0;
  int64_t c = 0, h = 0, w = 0;
  int32_t filter = 0;                  // ore_resize_filter, fixed at creation
  int32_t format = 0;                  // ore_image_format, fixed at creation
  int32_t matrix = 0;                  // ore_yuv_matrix of an NV12 or YUV list, fixed at creation
  bool any_flip = false;               // the last set flipped a descriptor: launches take the kernels' flag-reading instance
  bool any_orient = false;             // the last set held an orientation other than 1: launches take the orientation-reading instance
  bool oriented = false;               // ore_image_list_oriented: an oriented set has succeeded once; captures record that instance
  int taps = 0;                        // ORE_FILTER_BICUBIC_AA: no column run of the last set is longer (sizes the kernels' LDS)
  size_t desc_bytes = 0;               // of one descriptor of the list's format
  void* table = nullptr;               // device
  void* mirror = nullptr;              // pinned host: the source of the stream-ordered upload
  hipEvent_t uploaded = nullptr;       // recorded after each upload; the next set waits on it before it rewrites the mirror
};

namespace ore {

// ---------------------------------------------------------------- errors
ore_status set_error(ore_ctx* ctx, ore_status st, const char* fmt, ...);
#define ORE_HIP_CHECK(ctx, expr)                                                          \
  do {                                                                                    \
    hipError_t e_ = (expr);                                                               \
    if (e_ != hipSuccess)                                                                 \
      return ::ore::set_error((ctx), ORE_ERR_HIP, "%s: %s", #expr, hipGetErrorString(e_)); \
  } while (0)

// ---------------------------------------------------------------- device memory
// Every device allocation of the library goes through here.  own: memory the library keeps for itself (arena,
// conversion / staging / rows buffers, weight packs, the weight scratch) -- under ore_ctx_set_alloc_fill it is
// filled with the context's pattern on the context's stream before the caller gets the pointer, so whatever
// the caller launches on that stream afterwards is ordered behind the fill.  Not own: the caller's memory
// (ore_malloc) and the image-list tables, which hold addresses and geometry and are never filled.
hipError_t device_alloc(ore_ctx* ctx, void** dptr, size_t bytes, bool own);
// `bytes` of device memory set to the 32-bit pattern, stream-ordered (a tail of bytes % 4 takes its low bytes)
hipError_t device_fill(ore_ctx* ctx, void* dptr, size_t bytes, uint32_t pattern);

// ---------------------------------------------------------------- ONNX subset (onnx.proto)
struct Attr {
  std::string name;
  int type = 0;
  float f = 0.f;
  int64_t i = 0;
  std::string s;
  std::vector<int64_t> ints;
  std::vector<float> floats;
  bool has_i = false, has_f = false, has_s = false;
};

struct Node {
  std::string op_type, name;
  std::vector<std::string> inputs, outputs;
  std::vector<Attr> attrs;
};

struct Initializer {
  std::string name;
  std::vector<int64_t> dims;
  int dtype = 0;
  std::vector<float> f32;
  std::vector<int64_t> i64;
};

struct ValueInfo {
  std::string name;
  std::vector<int64_t> shape;
};

struct Graph {
  std::vector<Node> nodes;
  std::vector<Initializer> inits;
  std::vector<ValueInfo> inputs, outputs;
};

// Parses a ModelProto; returns false with a message on malformed input.
bool parse_model(const uint8_t* data, size_t len, Graph* g, std::string* err);

// ---------------------------------------------------------------- reference geometry
// Resolved window geometry (convolution_op.rs:266-350, max_pool_op.rs:188-264).
struct Window {
  int64_t pt = 0, pl = 0, pb = 0, pr = 0;
  int64_t Ho = 0, Wo = 0;
};
// auto_pad as ore_auto_pad; pads in ONNX order.  Returns ORE_OK or an error status.
ore_status resolve_window(ore_ctx* ctx, int auto_pad, const int64_t* pads, int n_pads, int64_t H, int64_t W,
                          int64_t kh, int64_t kw, int64_t sh, int64_t sw, Window* out);

// ---------------------------------------------------------------- runners over resolved geometry
// The layer between a planned Step (or a per-op entry) and the kernels' launch_* entry points: each
// run_* checks its limits, fills the kernel's parameter struct and launches, in image chunks where
// the batch's extent needs it (ore_chunk.h).

// An activation as a runner takes it: storage of es-byte elements, pointer to image 0, elements
// between images, and the channel-plane stride (NCHW) or pixel stride (NHWC); ps 0 = dense.
struct Ref { float* p; int64_t nstride; int64_t ps; int es; };
// ps resolved, once per layout: a plane of `plane` elements (NCHW), a pixel of C channels (NHWC)
inline int64_t plane_stride(const Ref& r, int64_t plane) { return r.ps ? r.ps : plane; }
inline int64_t pixel_stride(const Ref& r, int64_t C) { return r.ps ? r.ps : C; }

// a conv (or MatMul as a 1x1 conv) over x [C][H][W] per image
struct ConvGeom {
  int64_t C, H, W, M, kh, kw, sh, sw;
  Window win;
  bool relu;
};
// a MaxPool's kernel, strides and resolved window: a pool of its own (run_maxpool*), the pool in a conv's
// epilogue (win over the conv output) or the pool in front of a 1x1 conv (run_conv_pool)
struct PoolGeom {
  int64_t kh, kw, sh, sw;
  Window win;
};
// the pooled squeeze's recomputed expand1x1 (walker pass pool_expand): x's first E1 channels are
// relu(w1 s + b1) of s [C1][pH][pW] (plane stride s_ps, image stride s_nstride), w1 K-major [k][w1_Mp]
struct PoolExpand {
  const float* s;
  const float* w1;
  const float* b1;
  int C1, E1, w1_Mp;
  int64_t s_ps, s_nstride;
};
// what a conv kernel reads besides x.  wp: weights packed by launch_pack for the plan (f16 plans: f16
// storage); ktab: the gather table (launch_ktab / launch_ktab_nhwc) where the kernel gathers
struct ConvOperands {
  const float* wp;
  const int2* ktab;
  const float* bias;
  // the fused forms' extras, null without them
  const float* wc1 = nullptr;         // run_conv_epool: the weights again, for the window / band kernels (launch_pack_c1_f32)
  const C1SqueezeF32* sq1 = nullptr;  // run_conv_epool: the next 1x1 conv fused in; y is then unused (p null)
  const C1Squeeze* sq16 = nullptr;    // run_conv_pair_pool_f16: the same
  const PoolExpand* pe = nullptr;     // run_conv_pool
};
// a conv runner's status and the tile id its last launch ran (-1: nothing launched, or a kernel without one)
struct ConvRun {
  ore_status st;
  int tile;
  ConvRun(ore_status s, int t = -1) : st(s), tile(t) {}
};

// Kernel plan of a conv (or MatMul as a 1x1 conv) over resolved geometry.
ConvPlan conv_plan(int64_t M, int64_t C, int64_t H, int64_t W, int64_t kh, int64_t kw, int64_t sh, int64_t sw,
                   const Window& win, bool f16 = false, int xmode = 0, bool wino = false, int forced = -1);
// f32 plans, NCHW x and y
ConvRun run_conv(ore_ctx* ctx, const ConvPlan& pln, const Ref& x, const Ref& y, int64_t N, const ConvGeom& g,
                 const ConvOperands& w);
// f16 first conv + pooled epilogue straight from the f32 NCHW input (ore_conv1_f16.hip) when its
// geometry allows; tile -1 (and ORE_OK) otherwise, for the two-launch path.  y: the pooled NHWC output
ConvRun run_conv_pair_pool_f16(ore_ctx* ctx, const ConvPlan& pln, const Ref& x, const Ref& y, int64_t N,
                               const ConvGeom& g, const ConvOperands& w, const PoolGeom& ep);
// f16 plan (f16 models): y is NHWC f16; x is the f32 NCHW model input (F16_X_NCHW32) or NHWC f16.
// ktab per plan.xmode.  ep: the following MaxPool in the epilogue (y is then the pooled NHWC output;
// that kernel has no tile id)
ConvRun run_conv_f16(ore_ctx* ctx, const ConvPlan& pln, const Ref& x, const Ref& y, int64_t N, const ConvGeom& g,
                     const ConvOperands& w, const PoolGeom* ep = nullptr);
// Conv (+ Relu) and the MaxPool ep (over the conv's Ho x Wo output) in one launch, f32: y is the pooled output
ConvRun run_conv_epool(ore_ctx* ctx, const ConvPlan& pln, const Ref& x, const Ref& y, int64_t N, const ConvGeom& g,
                       const ConvOperands& w, const PoolGeom& ep);
// the operands of a fire module fused with the next squeeze: S of C channels, e1 = Relu(W1 S + b1) (E1
// channels), e3 = Relu(W3 * S + b3) (E3), S' = Relu(Ws [e1; e3] + bs) (Ms; 0: no squeeze, f16 only).
// f32 (run_fire): w1 / w3 in launch_fire_pack layout, ws the squeeze's launch_pack layout of row stride
// Msp; f16 (run_fire_f16): all three in launch_fire_pack_f16 layout
struct FireOperands {
  int64_t C, E1, E3, Ms, Msp;
  const void *w1, *w3, *ws;
  const float *b1, *b3, *bs;
};
// a fire module fused with the next squeeze (ORE_FUSE_FIRE, ore_fire.hip): x = S [C][H][W], y = S'
// [Ms][H][W] (its plane stride is the column count per image); pool: a 3x3 / stride-2 MaxPool (window
// over the H x W conv plane) between the Concat and the squeeze, y on its plane
ore_status run_fire(ore_ctx* ctx, const Ref& x, const Ref& y, int64_t N, int64_t H, int64_t W, const FireOperands& f,
                    const Window* pool = nullptr);
// the f16 fused fire module (ore_fire_f16.hip): x = S, y = S' NHWC f16
ore_status run_fire_f16(ore_ctx* ctx, const Ref& x, const Ref& y, int64_t N, int64_t H, int64_t W,
                        const FireOperands& f, const Window* pool = nullptr);
// pooled-epilogue tiling of a conv output (Ho x Wo) and its pool (3x3 / stride 2 only): *tr x *tc
// tiles of 6 x 9 pooled outputs per image; returns the work factor tiles * CONV_EPOOL_BN / (Ho * Wo)
// (the conv columns computed, recomputed overlap and padding included), 0 for other pools
double epool_tile(int64_t Ho, int64_t Wo, int64_t pkh, int64_t pkw, int64_t psh, int64_t psw, const Window& pwin,
                  int* tr, int* tc);
// 1x1 conv over the MaxPool `pool` (3x3 / stride 2) of x [C][H][W] on pool_conv1x1_f32_kernel: the pooled
// tensor is never materialised (walker pass fuse_pool_squeeze); g: the conv over x's planes, w.pe optional
ore_status run_conv_pool(ore_ctx* ctx, const ConvPlan& pln, const Ref& x, const Ref& y, int64_t N, const ConvGeom& g,
                         const ConvOperands& w, const PoolGeom& pool);
// packs w (and the gather table for an input of H x W) into the context scratch buffer;
// returns the packed weights (or null with the error set), *ktab receives the table
float* pack_to_scratch(ore_ctx* ctx, const ConvPlan& pln, const float* w, bool kmajor_src, int64_t M, int64_t C,
                       int64_t kh, int64_t kw, int64_t H, int64_t W, const int2** ktab);
// bytes of packed weights + gather table for one conv
size_t packed_bytes(const ConvPlan& pln);
// x [C][H][W]: f32 NCHW (ctx->pool_variant selects a kernel) or, of 2-byte elements, NHWC f16 (f16 models)
ore_status run_maxpool(ore_ctx* ctx, const Ref& x, const Ref& y, int64_t N, int64_t C, int64_t H, int64_t W,
                       const PoolGeom& pool);
// the geometry and normalisation of a uint8 [.,h,w,c] -> f32 NCHW conversion (ore_preprocess_u8 and the
// model's _u8 entries): checks c, h, w and flags, and resolves the channel reversal into p->plane;
// scale / shift: host arrays of c floats or null (1 / 0).  x, y, N and y_nstride are the caller's to set.
ore_status preproc_params(ore_ctx* ctx, int64_t h, int64_t w, int64_t c, const float* scale, const float* shift,
                          int32_t flags, PreprocParams* p);
// the plane map, scale and shift preproc_params resolved, for the resizing conversions' parameter structs
template <class P>
void copy_norm(const PreprocParams& q, P* p) {
  for (int s = 0; s < q.C; ++s) {
    p->plane[s] = q.plane[s];
    p->scale[s] = q.scale[s];
    p->shift[s] = q.shift[s];
  }
}
inline bool fits_i32(int64_t v) { return v >= 0 && v < (int64_t(1) << 31); }
// elements between the images of t: its nstride, or dense
int64_t nstride_of(const ore_tensor* t);
bool filter_known(int32_t filter);  // an ore_resize_filter
// The geometry rules every resizing conversion shares, each message written once: the sizes within RESIZE_MAX and
// the h x w crop inside the resized image; then, after the caller's own rules, the antialiasing filter's ratio.
// i: the descriptor of an image list the messages name ("image i: ..."); below 0 a dense conversion ("resize: ...")
ore_status check_resize_window(ore_ctx* ctx, int64_t i, int64_t hs, int64_t ws, int64_t h, int64_t w, const ore_resize& g);
ore_status check_resize_ratio(ore_ctx* ctx, int64_t i, int32_t filter, int64_t hs, int64_t ws, const ore_resize& g);
// as preproc_params for the resizing conversion of [.,hs,ws,c] images to h x w (ore_preprocess_resize_u8 and
// the model's _u8 entries after ore_model_set_input_resize): also checks the sizes against RESIZE_MAX and
// that the crop lies inside the resized image
ore_status resize_params(ore_ctx* ctx, int64_t hs, int64_t ws, int64_t c, int64_t h, int64_t w, const ore_resize* g,
                         const float* scale, const float* shift, int32_t flags, ResizeParams* p,
                         int32_t filter = ORE_FILTER_BILINEAR);
// as preproc_params for the conversion of an image list (ore_preprocess_list_u8 and the model's _u8_list
// entries): the list's output shape and table with the caller's normalisation; first 0, N the list's count.
// y and y_nstride are the caller's to set.
ore_status list_params(ore_ctx* ctx, const ore_image_list* l, const float* scale, const float* shift, int32_t flags,
                       ResizeListParams* p);
// the list conversion's launch under the list's format and filter (ore_preprocess_list_u8 and the model's
// _u8_list entries); of an NV12 or YUV list p carries everything but the table and the matrix, which are the list's
void launch_list(ore_ctx* ctx, const ore_image_list* l, const ResizeListParams& p);

}  // namespace ore
