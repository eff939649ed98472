/*
 * ore.h — C ABI of the MI355X-native (gfx950) fp32 ONNX op executor.
 *
 * Drop-in boundary for the fp32 op path of jackperlo/onnx-rusty-inference-engine.  The
 * reference dispatches every node through `node_inference`
 * (src/inference_engine/model_inference.rs:128-162, match at :137-161) into one Rust function
 * per op in src/inference_fp32_ops/.  Each entry point below replaces one of those functions
 * (cited on the declaration), operating on device tensors that stay resident in HBM.  The
 * graph-level entry points (ore_model_*) replace `inference()` (model_inference.rs:29-120)
 * together with the tensor plumbing of src/inference_engine/utils.rs.
 *
 * Conventions
 *  - Every function returns an ore_status (0 = ORE_OK).  Nothing throws or aborts across the
 *    ABI; the message of the last failure on a context is ore_last_error(ctx) (or
 *    ore_last_error(NULL) for failures before a context exists).  The reference panics in the
 *    same situations (unknown op / attribute / auto_pad string, missing input, shape mismatch).
 *  - Tensors are fp32, NCHW row-major, device memory.  `nstride` is the element distance
 *    between consecutive images (0 = contiguous); it lets an op write a channel slice of a
 *    wider tensor (Concat in place).  A non-zero nstride is at least one image's elements (the
 *    product of dims[1..]) with nstride * dims[0] + 256 below 2^31, or ore_conv2d_f32 and
 *    ore_maxpool2d_f32 -- the ops that take slices, as x and as y -- return ORE_ERR_INVALID naming
 *    the tensor before any device call.  (The other ops take contiguous tensors only.)  Any 4-byte
 *    aligned base is accepted; no op writes outside y's elements, and no element outside x's
 *    reaches a result (tests/test_slices_gpu.py).
 *  - Launches are asynchronous on the context's HIP stream; ore_sync() joins.  A context is
 *    bound to one device and is not thread-safe (one per host thread / device).
 *  - Padding is resolved exactly as the reference does (including its SAME split with the
 *    larger half at the top/left, convolution_op.rs:519-557) before any kernel is launched.
 */
#ifndef ORE_H
#define ORE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ABI 2 (round 4) against ABI 1: the opt-in bf16x3 kernels are gone -- load flags 2 / 8 (ABI 1's
 * ORE_LOAD_X3 / ORE_LOAD_X3_ALL) and conv tile ids 28-35 are rejected with ORE_ERR_UNSUPPORTED; so are
 * ABI 1's retired fusion bit 16 (ORE_FUSE_POOL_CONV), MaxPool variant 1 and conv tile ids 4-11, which
 * ABI 1 builds already refused.  ore_model_load accepts any max_batch: a batch whose activations
 * would pass the kernels' 32-bit offsets runs in image chunks inside ore_model_run.  Every other
 * entry point and value is unchanged. */
#define ORE_ABI_VERSION 2

typedef enum ore_status {
  ORE_OK = 0,
  ORE_ERR_INVALID = 1,     /* bad argument / shape mismatch (reference: assert / unwrap panic) */
  ORE_ERR_UNSUPPORTED = 2, /* op, attribute or mode the reference does not implement (panic!) */
  ORE_ERR_HIP = 3,         /* HIP runtime failure */
  ORE_ERR_OOM = 4,         /* device allocation failed */
  ORE_ERR_PARSE = 5        /* malformed ONNX protobuf */
} ore_status;

typedef enum ore_auto_pad {
  ORE_PAD_NOTSET = 0,     /* explicit `pads` */
  ORE_PAD_SAME_UPPER = 1,
  ORE_PAD_SAME_LOWER = 2,
  ORE_PAD_VALID = 3
} ore_auto_pad;

typedef struct ore_ctx ore_ctx;
typedef struct ore_model ore_model;

typedef struct ore_tensor {
  float* data;      /* device pointer to element [0,0,0,0] */
  int32_t ndim;     /* 1..4 */
  int64_t dims[4];
  int64_t nstride;  /* elements between images (dims[0] steps); 0 = contiguous, else >= one image */
} ore_tensor;

/* Conv attributes (convolution_op.rs:132-173).  pads use ONNX order
 * [h_begin, w_begin, h_end, w_end]; n_pads = 0 when the attribute is absent.  As in the
 * reference, any positive pad forces NOTSET (:169-173) and kernel_shape is ignored (:151). */
typedef struct ore_conv_attrs {
  int32_t auto_pad;      /* ore_auto_pad; reference default VALID (:134) */
  int32_t n_pads;
  int64_t pads[4];
  int64_t strides[2];    /* required (the reference unwraps them, :285-290) */
  int64_t dilations[2];  /* must be 1 (dilation > 1 is not a working path in the reference) */
  int64_t group;         /* must be 1 (asserted, :252) */
  int32_t fuse_relu;     /* extension: apply Relu in the epilogue (a following Relu node) */
} ore_conv_attrs;

/* MaxPool attributes (max_pool_op.rs:85-114).  Unlike Conv, pads do NOT force NOTSET: with
 * the default auto_pad (VALID) the pads are ignored, as in the reference. */
typedef struct ore_pool_attrs {
  int32_t auto_pad;
  int32_t n_pads;
  int64_t pads[4];
  int64_t kernel[2];
  int64_t strides[2];
} ore_pool_attrs;

/* ------------------------------------------------------------------ context & memory */
int32_t ore_abi_version(void);
ore_status ore_ctx_create(int32_t device, ore_ctx** out);
ore_status ore_ctx_destroy(ore_ctx* ctx);
/* Launch on an external HIP stream (e.g. the caller's framework stream).  NULL selects the
 * legacy default (null) stream; the context starts on a stream of its own. */
ore_status ore_ctx_set_stream(ore_ctx* ctx, void* hip_stream);
void* ore_ctx_get_stream(ore_ctx* ctx);
ore_status ore_sync(ore_ctx* ctx);
const char* ore_last_error(ore_ctx* ctx);
/* Conv algorithm of the per-op entry ore_conv2d_f32 on this context (extension; the reference has
 * one algorithm, im2col + per-channel dots, convolution_op.rs:224-517).  ORE_CONV_ALGO_DIRECT (the
 * default): the implicit GEMM in the reference's k order.  ORE_CONV_ALGO_WINOGRAD: 3x3 / stride-1 /
 * pad-1 convs with C % 16 == 0 by Winograd F(2x2, 3x3) in f32 (2.25x fewer MFMAs; its error against a
 * float64 reference is at or below the direct f32 conv's, but results are not bit-identical to it);
 * other geometries stay direct.  Models choose per ORE_LOAD_NO_WINOGRAD instead. */
#define ORE_CONV_ALGO_DIRECT 0
#define ORE_CONV_ALGO_WINOGRAD 1
ore_status ore_ctx_set_conv_algo(ore_ctx* ctx, int32_t algo);
/* Kernel selection for parity tests and tuning (extension).  Results never depend on it: every conv
 * tile of one algorithm computes each output by the same k-ordered chain, every MaxPool kernel the
 * same max.
 *  ore_ctx_set_conv_tile: every conv planned on this context afterwards -- ore_conv2d_f32 /
 *    ore_matmul_f32 calls, and models loaded later -- uses tile id `tile` where it belongs to the
 *    layer's kernel family (else the per-layer heuristic); -1 (default) = the heuristic.  Ids as
 *    ore_model_step_tile reports them (0-3 LDS-staged, 12-20 streaming, 36-40 Winograd, 46-48
 *    persistent streaming 1x1); the retired ids 4-11 and 28-35 return ORE_ERR_UNSUPPORTED.
 *  ore_ctx_set_pool_variant: MaxPool kernel of ore_maxpool2d_f32 and of the walker's MaxPool steps:
 *    0 (default) = by layout, 2 one thread per output, 3 column strips, 4 plane-staged, 5
 *    chunk-staged (1 is retired: ORE_ERR_UNSUPPORTED).
 *  ore_ctx_set_resize_variant: kernel of the antialiased resize (ORE_FILTER_BILINEAR_AA) in every entry that
 *    runs it on this context afterwards, captures included: 0 (default) = by geometry, 1 one thread per
 *    output pixel.  That is the only kernel today (the band kernel that was variant 2 lost to it and was
 *    removed), so both select it; anything else is ORE_ERR_INVALID.  The two bilinear
 *    kernels are not affected. */
ore_status ore_ctx_set_conv_tile(ore_ctx* ctx, int32_t tile);
ore_status ore_ctx_set_pool_variant(ore_ctx* ctx, int32_t variant);
ore_status ore_ctx_set_resize_variant(ore_ctx* ctx, int32_t variant);

ore_status ore_malloc(ore_ctx* ctx, size_t bytes, void** dptr);
ore_status ore_free(ore_ctx* ctx, void* dptr);
ore_status ore_upload(ore_ctx* ctx, void* dst, const void* src, size_t bytes);
ore_status ore_download(ore_ctx* ctx, void* dst, const void* src, size_t bytes);

/* ------------------------------------------------------------------ shape inference
 * Output geometry exactly as the reference computes it (convolution_op.rs:292-324,
 * max_pool_op.rs:214-246); pads_tlbr receives the resolved [top, left, bottom, right]. */
ore_status ore_conv_out_shape(const int64_t x_dims[4], const int64_t w_dims[4], const ore_conv_attrs* a,
                              int64_t y_dims[4], int64_t pads_tlbr[4]);
ore_status ore_pool_out_shape(const int64_t x_dims[4], const ore_pool_attrs* a, int64_t y_dims[4],
                              int64_t pads_tlbr[4]);

/* ------------------------------------------------------------------ ops (node_inference arms) */
/* "Conv"     convolution()  convolution_op.rs:94-193 (conv2d :224-517).  x [N,C,H,W],
 *            w [M,C,kh,kw] (ONNX layout), bias [M] or NULL, y [N,M,Ho,Wo] (may be a slice). */
ore_status ore_conv2d_f32(ore_ctx* ctx, const ore_tensor* x, const ore_tensor* w, const ore_tensor* bias,
                          const ore_conv_attrs* a, ore_tensor* y);
/* "MaxPool"  max_pool()  max_pool_op.rs:65-129 (max_pool2d :157-360). */
ore_status ore_maxpool2d_f32(ore_ctx* ctx, const ore_tensor* x, const ore_pool_attrs* a, ore_tensor* y);
/* "Relu"     relu()  relu_op.rs:11-29 (relu_wrapper :31-33).  y may alias x. */
ore_status ore_relu_f32(ore_ctx* ctx, const ore_tensor* x, ore_tensor* y);
/* "Add"      add()  add_op.rs:16-107: a + b with b broadcast right-aligned onto a
 *            ([N,C,H,W] + [C,1,1], or [N,K] + [1,K]). */
ore_status ore_add_f32(ore_ctx* ctx, const ore_tensor* a, const ore_tensor* b, ore_tensor* y);
/* "Softmax"  softmax()  softmax_op.rs:13-42 (softmax_wrapper :45-57): rows = dims[0],
 *            row length = product of the remaining dims; y is [rows, D]. */
ore_status ore_softmax_f32(ore_ctx* ctx, const ore_tensor* x, ore_tensor* y);
/* "MatMul"   mul()  mul_op.rs:11-32: y[M,N] = a[M,K] . b[K,N] (MFMA). */
ore_status ore_matmul_f32(ore_ctx* ctx, const ore_tensor* a, const ore_tensor* b, ore_tensor* y);
/* "GlobalAveragePool"  global_average_pool()  global_average_pool_op.rs:11-51: y [N,C,1,1]. */
ore_status ore_gap_f32(ore_ctx* ctx, const ore_tensor* x, ore_tensor* y);
/* "Concat"   concatenation()  concatenate_op.rs:11-41: exactly two inputs on `axis`. */
ore_status ore_concat_f32(ore_ctx* ctx, const ore_tensor* a, const ore_tensor* b, int64_t axis, ore_tensor* y);
/* "Dropout"  drop_out()  dropout_op.rs:12-89: inference identity (training_mode = false).
 *            Copies when y != x, no-op when they alias. */
ore_status ore_dropout_f32(ore_ctx* ctx, const ore_tensor* x, ore_tensor* y);
/* "Reshape"  reshape()  reshape_op.rs:16-92: metadata only (row-major reinterpretation to
 *            2-D; a 0 in `shape` copies the input dim).  Writes the resulting view to y. */
ore_status ore_reshape(const ore_tensor* x, const int64_t* shape, int32_t n_shape, ore_tensor* y);
/* Input preprocessing (extension; no reference counterpart -- the reference reads a float TensorProto from
 * a .pb file, main.rs): a batch of uint8 images as a decoder leaves them, interleaved [n,h,w,c] and
 * contiguous with 1 <= c <= 4, to the float32 NCHW tensor the entry points above and ore_model_run take,
 * in one launch (ore_preproc.hip):
 *     y[i,ch,r,q] = fadd_rn(fmul_rn((float)x[i,r,q,cs], scale[ch]), shift[ch])
 * with cs = ch, or cs = c-1-ch under ORE_PRE_REVERSE_CHANNELS (RGB <-> BGR; c == 3 only, ORE_ERR_INVALID
 * otherwise).  The multiply and the add round separately, never as one FMA, so a host computes the same
 * bits with (float)x * scale + shift in two float32 operations.  x is a DEVICE pointer; scale / shift are
 * HOST arrays of c floats, read before the call returns (NULL: 1 / 0).  y is a [n,c,h,w] view and may be
 * a slice (nstride >= c*h*w; the elements between images are not written).  h*w a multiple of 4, x
 * 4-byte aligned and y's planes 16-byte aligned take the vector kernel; anything else a scalar one with
 * the same results.  n == 0 is ORE_OK and launches nothing. */
#define ORE_PRE_REVERSE_CHANNELS 1
ore_status ore_preprocess_u8(ore_ctx* ctx, const uint8_t* x, int64_t n, int64_t h, int64_t w, int64_t c,
                             const float* scale, const float* shift, int32_t flags, ore_tensor* y);
/* Resize and crop in front of the conversion (extension, ore_resize.hip): the images are [n,hs,ws,c], of any
 * size up to 16384 x 16384, and y is [n,c,H,W].  The geometry is four integers: the whole source image is
 * resized to rh x rw (each 1..16384), and y is the H x W window of that resized image whose first sample is
 * (top, left): 0 <= top, top + H <= rh, 0 <= left, left + W <= rw.  Resize(256) + CenterCrop(224) of a
 * 375 x 500 image is {256, 341, 16, 58}; a plain resize {H, W, 0, 0}; a plain crop {hs, ws, top, left}.
 * The filter is bilinear with half-pixel centres and no antialiasing (cv2.INTER_LINEAR;
 * F.interpolate(mode="bilinear", align_corners=False, antialias=False)), stated in integers.  Per axis, for
 * S source samples resized to D and resized index o (top + r for rows, left + q for columns):
 *     num = max((2 o + 1) S - D, 0);  i0 = num div 2 D;  rem = num mod 2 D;
 *     if (i0 >= S - 1) { i0 = S - 1; rem = 0; }   i1 = min(i0 + 1, S - 1);   t = fdiv_rn((float)rem, (float)(2 D))
 * and per output element, with a, b the bytes at (y0, x0), (y0, x1) and c, d those at (y1, x0), (y1, x1) of
 * source channel cs, converted to float32:
 *     top = a + (b - a) tx;  bot = c + (d - c) tx;  v = top + (bot - top) ty;  y = v scale[ch] + shift[ch]
 * where every -, * and + rounds on its own (never an FMA): numpy float32 arrays reproduce it bit for bit,
 * and with rh, rw = hs, ws it is ore_preprocess_u8 of the cropped bytes exactly.
 *  ore_resize_taps: one axis's table (i0, i1, t for the `count` resized indices from `origin`) into HOST
 *    arrays; host only, it touches no device.  It is the map the kernels use (csrc/ore_resize_geom.h).
 *  ore_preprocess_resize_u8: x, scale, shift, flags and y as for ore_preprocess_u8 (y may be a slice, of any
 *    alignment); H, W are y->dims[2], y->dims[3].  One launch, one thread per output pixel.  The pointers and
 *    the geometry are checked first and the context last, all before any device call (ORE_ERR_INVALID);
 *    n == 0 is ORE_OK and launches nothing.  Every image of a call has the same size; rows are dense (no
 *    row stride); an image list (below) lifts both. */
typedef struct ore_resize {
  int64_t rh, rw, top, left;
} ore_resize;
ore_status ore_resize_taps(int64_t src, int64_t resized, int64_t origin, int64_t count, int32_t* i0, int32_t* i1,
                           float* t);
ore_status ore_preprocess_resize_u8(ore_ctx* ctx, const uint8_t* x, int64_t n, int64_t hs, int64_t ws, int64_t c,
                                    const ore_resize* g, const float* scale, const float* shift, int32_t flags,
                                    ore_tensor* y);
/* Image lists (extension, resize_u8_list_kernel in ore_resize.hip): uint8 images of different sizes and row
 * strides in one launch.  A descriptor names one image -- its pointer, size, row stride and its own geometry
 * -- and image i of the result is, bit for bit, what ore_preprocess_resize_u8 gives for a dense copy of that
 * image alone (n = 1, geometry imgs[i].g).  Two descriptors may name the same or overlapping bytes (two
 * regions of interest of one frame).
 *  ore_image_check: host only, it touches no device (as ore_resize_taps).  Every descriptor, for a c-channel
 *    h x w output: data non-null; hs, ws, g.rh, g.rw each 1..16384 and the h x w crop at (g.top, g.left)
 *    inside the resized image; row_stride 0 or >= ws*c; (hs-1)*row_stride + ws*c < 2^31 (offsets inside one
 *    image stay below 2^31, only image bases are 64-bit).  The first failing descriptor gives ORE_ERR_INVALID,
 *    a message with its index and the reason, and *bad_index (when non-null).  n == 0 is ORE_OK.  The
 *    library cannot validate the DEVICE pointers: that data..data + (hs-1)*row_stride + ws*c is readable
 *    device memory is the caller's to guarantee.
 *  ore_image_list_create: a list for one context and one output shape (1 <= c <= 4; h, w >= 1): a device table
 *    of `capacity` packed descriptors and a pinned host mirror, both allocated here.  Nothing is allocated
 *    later, so every use of the list is legal inside a stream capture -- except ore_image_list_set.
 *  ore_image_list_set: ore_image_check, then copy into the mirror, upload the table on the context's stream
 *    and set the count to n.  On a failed check or n > capacity (ORE_ERR_INVALID) the list keeps its previous
 *    content and count.  The upload is stream-ordered: work submitted earlier that reads the old table
 *    finishes first, work submitted later sees the new table; imgs may be reused as soon as the call
 *    returns (a set waits for the previous set's upload before it rewrites the mirror).  n == 0 empties the
 *    list.  ORE_ERR_INVALID while the context's stream is capturing.
 *  ore_image_list_destroy: after the work that reads the list has finished (ore_sync), and after any model
 *    graph captured on it was re-captured or destroyed.
 *  ore_preprocess_list_u8: scale, shift and flags as for ore_preprocess_u8; y is [count,c,h,w] of the list
 *    and may be a slice of any alignment (nstride >= c*h*w, the gaps are not written).  The arguments are
 *    checked first and the context last (l must belong to ctx), all before any device call; count == 0 is
 *    ORE_OK and launches nothing. */
typedef struct ore_image_u8 {
  const uint8_t* data; /* DEVICE pointer to row 0, column 0, channel 0; any alignment */
  int64_t hs, ws;      /* source size, each 1..16384 */
  int64_t row_stride;  /* bytes from a row to the next, >= ws*c; 0 means dense (ws*c) */
  ore_resize g;        /* this image's own {rh, rw, top, left}, as for ore_preprocess_resize_u8 */
} ore_image_u8;        /* 64 bytes */
typedef struct ore_image_list ore_image_list;
ore_status ore_image_check(const ore_image_u8* imgs, int64_t n, int64_t c, int64_t h, int64_t w, int64_t* bad_index);
ore_status ore_image_list_create(ore_ctx* ctx, int64_t capacity, int64_t c, int64_t h, int64_t w, ore_image_list** out);
ore_status ore_image_list_destroy(ore_image_list* l);
ore_status ore_image_list_set(ore_image_list* l, const ore_image_u8* imgs, int64_t n);
int64_t ore_image_list_count(ore_image_list* l);
ore_status ore_preprocess_list_u8(ore_ctx* ctx, ore_image_list* l, const float* scale, const float* shift, int32_t flags,
                                  ore_tensor* y);
/* Antialiased resize (extension, the resize_aa_* kernels in ore_resize.hip): the filter of torchvision's Resize
 * on tensors with antialias=True, of F.interpolate(mode="bilinear", antialias=True) and, up to its rounding to
 * bytes, of PIL's BILINEAR.  The geometry is the same ore_resize; the filter is chosen per axis.  An axis with
 * S <= D (it does not shrink) is computed exactly as above (i0, i1, t and the lerp).  An axis with S > D takes
 * the triangle filter stretched by S / D, in integers: for resized index o, with c = (2 o + 1) S,
 *     taps: every source index j of [0, S - 1] with |(2 j + 1) D - c| < 2 S   (a contiguous, never empty run)
 *     u_j = 2 S - |(2 j + 1) D - c|;   U = the sum of u_j over the taps        (so the edges renormalise)
 * and S <= 32 D is required of every shrinking axis (ORE_AA_MAX_RATIO; ORE_ERR_INVALID with a message naming
 * the axis otherwise): a run is then at most 64 taps (ORE_AA_MAX_TAPS), u_j < 2^15, U <= 2^21 and the sum of
 * u_j * byte < 2^29, and the work of one output pixel is bounded.  Per output element of source channel cs,
 * with v_r, V the row weights and sum, u_j, U the column ones:
 *   1. per tap row r:  columns shrink: g_r = (float)(sum_j u_j x[r,j,cs])   (exact integer sum, one rounding)
 *                      else:           g_r = lerp(x[r,x0,cs], x[r,x1,cs], tx)
 *   2. rows shrink:    acc = +0; for r ascending: acc = fadd_rn(acc, fmul_rn((float)v_r, g_r));
 *                      w = fdiv_rn(acc, (float)V)
 *      else:           w = lerp(g_y0, g_y1, ty)
 *   3. columns shrink: w = fdiv_rn(w, (float)U)
 *   4. y = fadd_rn(fmul_rn(w, scale[ch]), shift[ch])
 * Every float operation rounds on its own (no FMA, IEEE division), so numpy float32 arrays reproduce it bit
 * for bit; where neither axis shrinks it is the ORE_FILTER_BILINEAR result bit for bit.
 *  ore_resize_aa_taps: one shrinking axis's table into HOST arrays (host only, as ore_resize_taps): first tap,
 *    tap count and weight sum of the `count` resized indices from `origin`; weights, when non-null, is
 *    [count][ORE_AA_MAX_TAPS], zero-padded.  ORE_ERR_INVALID when src <= resized (the axis does not shrink:
 *    ore_resize_taps is its table) and when src > 32 resized.
 *  ore_preprocess_resize_u8_ex: ore_preprocess_resize_u8 with the filter; the same order of checks (arguments
 *    and geometry, the ratio rule included, then the context, all before any device call); an unknown filter
 *    is ORE_ERR_INVALID.  ORE_FILTER_BILINEAR is ore_preprocess_resize_u8 itself.
 *  ore_image_check_ex: ore_image_check plus, under ORE_FILTER_BILINEAR_AA, the ratio rule per descriptor.
 *  ore_image_list_create_ex: the filter is a property of the list, fixed at creation like its output shape
 *    (ore_image_list_filter reads it; ore_image_list_create makes a bilinear list).  ore_image_list_set checks
 *    with it, and ore_preprocess_list_u8 and the model's _u8_list entries run it. */
typedef enum { ORE_FILTER_BILINEAR = 0, ORE_FILTER_BILINEAR_AA = 1 } ore_resize_filter;
#define ORE_AA_MAX_RATIO 32
#define ORE_AA_MAX_TAPS 64
ore_status ore_resize_aa_taps(int64_t src, int64_t resized, int64_t origin, int64_t count, int32_t* first,
                              int32_t* ntaps, int32_t* sum, int32_t* weights);
ore_status ore_preprocess_resize_u8_ex(ore_ctx* ctx, const uint8_t* x, int64_t n, int64_t hs, int64_t ws, int64_t c,
                                       const ore_resize* g, int32_t filter, const float* scale, const float* shift,
                                       int32_t flags, ore_tensor* y);
ore_status ore_image_check_ex(const ore_image_u8* imgs, int64_t n, int64_t c, int64_t h, int64_t w, int32_t filter,
                              int64_t* bad_index);
ore_status ore_image_list_create_ex(ore_ctx* ctx, int64_t capacity, int64_t c, int64_t h, int64_t w, int32_t filter,
                                    ore_image_list** out);
int32_t ore_image_list_filter(ore_image_list* l);
/* Cubic resize (extension, the resize_cubic_* kernels in ore_resize.hip): the Keys cubic convolution kernel, plain
 * and antialiased.  The two filters are values of the `filter` word next to ore_resize_filter, not members of it:
 * bit 8 (ORE_FILTER_CUBIC_BIT) selects the cubic kernel, bit 0 stays "antialiased".  Every entry that takes a
 * filter (ore_preprocess_resize_u8_ex, ore_image_check_ex / _nv12 / _yuv, ore_image_list_create_ex / _nv12 / _yuv,
 * ore_model_set_input_resize_ex) accepts 0, 1, 256 and 257 and nothing else; ore_image_list_filter returns the
 * whole word.  Geometry, descriptors, flips, NV12 / YUV conversion per tap, ORE_PRE_REVERSE_CHANNELS, output
 * slices, staging, chunks, captures and views are those of the bilinear filters; ore_ctx_set_resize_variant does
 * not concern these.  Every float operation below is rounded on its own (no FMA, IEEE division) and every constant
 * is exact in binary, so numpy float32 reproduces the results bit for bit.
 *
 * ORE_FILTER_BICUBIC (a = -0.75: cv2.INTER_CUBIC, F.interpolate(mode="bicubic", align_corners=False) on floats).
 * Per axis, S samples resized to D, resized index o (top + r for rows, left + q for columns):
 *     num = (2 o + 1) S - D        (not clamped at 0: it may be negative)
 *     i = floor(num / 2 D) (>= -1);  rem = num - 2 D i;  t = fdiv_rn((float)rem, (float)(2 D));  s = fsub_rn(1, t)
 *     taps k = 0..3 read sample clamp(i - 1 + k, 0, S - 1)          (the border is replicated)
 *     p1(z) = ((1.25 z - 2.25) z) z + 1       p2(z) = ((-0.75 z + 3.75) z - 6) z + 3     (left to right as written)
 *     w0 = p2(fadd_rn(t, 1));  w1 = p1(t);  w2 = p1(s);  w3 = p2(fadd_rn(s, 1))
 * Per output element of source channel cs, wx / wy the column / row weights:
 *     per tap row k in order:  g_k = fmul_rn(wx0, x0);  g_k = fadd_rn(g_k, fmul_rn(wxj, xj)) for j = 1..3
 *     v = fmul_rn(wy0, g_0);  v = fadd_rn(v, fmul_rn(wyk, g_k)) for k = 1..3
 *     y = fadd_rn(fmul_rn(v, scale[ch]), shift[ch])
 * There is no division by a weight sum and NO clamp to [0, 255]: the kernel's negative lobes overshoot at edges and
 * the overshoot is kept, as F.interpolate keeps it on float tensors (PIL and cv2 clamp because they store bytes).
 * There is no ratio rule: 16384 -> 1 is accepted, as under ORE_FILTER_BILINEAR.
 *
 * ORE_FILTER_BICUBIC_AA (a = -0.5: PIL's BICUBIC up to its rounding to bytes, F.interpolate(mode="bicubic",
 * antialias=True), torchvision's Resize(interpolation=BICUBIC, antialias=True) on tensors).  Per axis, shrinking
 * or not, with F = max(S, D), G = 2 F, c = (2 o + 1) S:
 *     a_j = |(2 j + 1) D - c|;   taps: every j of [0, S - 1] with a_j < 2 G   (a contiguous, never empty run)
 *     z_j = fdiv_rn((float)a_j, (float)G);   w_j = a_j < G ? q1(z_j) : q2(z_j)
 *     q1(z) = ((1.5 z - 2.5) z) z + 1         q2(z) = ((-0.5 z + 2.5) z - 4) z + 2
 *     W = +0; for j ascending: W = fadd_rn(W, w_j)                  (over the clipped run: the edges renormalise)
 * S <= 16 D is required of every axis (ORE_CUBIC_AA_MAX_RATIO; ORE_ERR_INVALID naming the axis otherwise, in the
 * position of the 32-times rule): a run is then at most 64 taps (ORE_AA_MAX_TAPS); an axis that does not shrink
 * has at most 4.  Per output element, u_j, U the column weights and sum, v_r, V the row ones:
 *     acc = +0;  per tap row r ascending:  g = +0; for j ascending: g = fadd_rn(g, fmul_rn(u_j, x[r,j,cs]));
 *                                          acc = fadd_rn(acc, fmul_rn(v_r, g))
 *     w = fdiv_rn(fdiv_rn(acc, V), U);   y = fadd_rn(fmul_rn(w, scale[ch]), shift[ch])
 * Overshoot is kept here too.  With S == D on both axes either filter returns the source bytes exactly (weights
 * 0, 1, 0, 0; a run whose weights are a single 1 and zeros, W = 1).
 *  ore_resize_cubic_taps: one axis's table into HOST arrays (host only, as ore_resize_taps), for filter 256 or 257:
 *    tap k of resized index origin + i reads source sample clamp(first[i] + k, 0, src - 1), k < ntaps[i].  Plain:
 *    ntaps is 4, first may be negative (>= -2), sum is 1.0f.  Antialiased: the run lies inside the image and sum
 *    is W.  weights, when non-null, is [count][ORE_AA_MAX_TAPS], zero padded.  ORE_ERR_INVALID: a null first,
 *    ntaps or sum; then a filter other than 256 / 257; then a bad axis (as ore_resize_taps); then, under 257,
 *    src > 16 resized. */
#define ORE_FILTER_CUBIC_BIT 256
#define ORE_FILTER_BICUBIC 256
#define ORE_FILTER_BICUBIC_AA 257
#define ORE_CUBIC_AA_MAX_RATIO 16
ore_status ore_resize_cubic_taps(int64_t src, int64_t resized, int64_t origin, int64_t count, int32_t filter,
                                 int32_t* first, int32_t* ntaps, float* weights, float* sum);
/* NV12 image lists (extension, the *_nv12_list kernels in ore_resize.hip): frames as a video decoder leaves
 * them -- a full-resolution Y plane and a half-resolution plane of interleaved (U, V) pairs, each with its own
 * pitch -- straight into an image list, without a colour-conversion pass in between.  Chroma is taken nearest:
 * source pixel (r, j) is Y at (r, j) and the UV pair at (r >> 1, j >> 1) (cv2.COLOR_YUV2RGB_NV12, libyuv).  The
 * conversion is fixed in integers (csrc/ore_yuv.h): with U' = U - 128, V' = V - 128, a matrix {yoff, cy, cvr,
 * cug, cvg, cub} and >> an arithmetic shift (floor),
 *     y = max(Y - yoff, 0) * cy + 2^19
 *     R = clamp((y + cvr V') >> 20, 0, 255)
 *     G = clamp((y - cug U' - cvg V') >> 20, 0, 255)
 *     B = clamp((y + cub U') >> 20, 0, 255)
 * with each coefficient round(k * 2^20) of the usual three-decimal constants:
 *     ORE_YUV_BT601      (limited range, OpenCV's)  {16, 1220542, 1673527, 409993, 852492, 2116026}
 *     ORE_YUV_BT709      (limited range)            {16, 1220542, 1880097, 223347, 558891, 2214593}
 *     ORE_YUV_BT601_FULL (JPEG / JFIF)              { 0, 1048576, 1470104, 360853, 748826, 1858077}
 * Over all 2^24 triples every accumulator fits int32 and every channel is within 1 of the float64 formula
 * rounded half up.  Image i of an NV12 list is, bit for bit, what an interleaved list (c = 3) of the same
 * filter gives for the [hs,ws,3] R, G, B bytes of that frame converted by this formula, for the same geometry,
 * scale / shift and ORE_PRE_REVERSE_CHANNELS (which then yields B, G, R planes).
 *  ore_yuv_to_rgb: the conversion of n triples from three HOST arrays into rgb[3 n] (host only, it touches no
 *    device, as ore_resize_taps); it is the map the kernels use.  An unknown matrix is ORE_ERR_INVALID.
 *  ore_image_nv12: y and uv are DEVICE pointers of any alignment; the UV plane has ceil(hs/2) rows of ceil(ws/2)
 *    pairs, so odd sizes are legal (the last row / column has a chroma pair of its own).  Strides are in bytes;
 *    0 means dense: ws for Y, 2 * ceil(ws/2) for UV.  A region of interest of a larger frame is a descriptor
 *    whose pointers are offset to an EVEN origin (y0, x0): y + y0 * y_pitch + x0 and uv + (y0/2) * uv_pitch + x0.
 *    At an odd origin the pixels would pair up with the wrong chroma samples: rounding an odd origin to an even
 *    one is the caller's to do, the library sees only the pointers.
 *  ore_image_check_nv12: host only, the rules and messages of ore_image_check_ex with c = 3: both pointers
 *    non-null; sizes, geometry and (under ORE_FILTER_BILINEAR_AA) the ratio rule as there; y_stride 0 or >= ws;
 *    uv_stride 0 or >= 2 * ceil(ws/2); (hs-1) * y_stride + ws < 2^31 and (ceil(hs/2)-1) * uv_stride +
 *    2 * ceil(ws/2) < 2^31.
 *  ore_image_list_create_nv12: an ore_image_list with c = 3 whose format (ore_image_list_format: ORE_IMAGE_NV12)
 *    and matrix (ore_image_list_matrix) are fixed at creation, as the filter is.  Every entry that takes a list
 *    -- ore_preprocess_list_u8, the model's _u8_list runs, classifications and captures -- takes it as is.
 *  ore_image_list_set_nv12: ore_image_list_set for an NV12 list, with the same semantics (check first, the old
 *    content kept on failure, stream-ordered upload, ORE_ERR_INVALID inside a capture, n == 0 empties).
 *    ore_image_list_set on an NV12 list and ore_image_list_set_nv12 on an interleaved one are ORE_ERR_INVALID
 *    and leave the list unchanged. */
typedef enum { ORE_YUV_BT601 = 0, ORE_YUV_BT709 = 1, ORE_YUV_BT601_FULL = 2 } ore_yuv_matrix;
typedef enum { ORE_IMAGE_INTERLEAVED = 0, ORE_IMAGE_NV12 = 1, ORE_IMAGE_YUV = 2 } ore_image_format;
typedef struct ore_image_nv12 {
  const uint8_t* y;          /* DEVICE pointer to row 0, column 0 of the Y plane; any alignment */
  const uint8_t* uv;         /* DEVICE pointer to row 0, pair 0 of the UV plane; any alignment */
  int64_t hs, ws;            /* frame size, each 1..16384; odd sizes are legal */
  int64_t y_stride;          /* bytes from a Y row to the next, >= ws; 0 means dense */
  int64_t uv_stride;         /* bytes from a UV row to the next, >= 2 * ceil(ws/2); 0 means dense */
  ore_resize g;              /* this frame's own {rh, rw, top, left} */
} ore_image_nv12;            /* 80 bytes */
ore_status ore_yuv_to_rgb(int32_t matrix, const uint8_t* y, const uint8_t* u, const uint8_t* v, int64_t n, uint8_t* rgb);
ore_status ore_image_check_nv12(const ore_image_nv12* imgs, int64_t n, int64_t h, int64_t w, int32_t filter,
                                int64_t* bad_index);
ore_status ore_image_list_create_nv12(ore_ctx* ctx, int64_t capacity, int64_t h, int64_t w, int32_t filter,
                                      int32_t matrix, ore_image_list** out);
ore_status ore_image_list_set_nv12(ore_image_list* l, const ore_image_nv12* imgs, int64_t n);
int32_t ore_image_list_format(ore_image_list* l);
int32_t ore_image_list_matrix(ore_image_list* l);
/* YUV image lists (extension, the *_yuv_list kernels in ore_resize.hip): frames as a JPEG decoder leaves them.  A
 * hardware JPEG decoder writes what the file's chroma subsampling dictates -- three planes for 4:4:4 and 4:4:0,
 * one packed YUYV plane for 4:2:2, NV12 for 4:2:0, a single Y plane for 4:0:0, or three planes for every
 * subsampling (4:1:1 included) in its planar mode -- and one batch of files mixes them.  So every descriptor of
 * such a list carries its own plane layout (ore_yuv_format), and one launch takes the batch as it was decoded.
 * With (sx, sy) the format's chroma shifts, source pixel (r, j) is Y at (r, j) and the chroma sample at
 * (r >> sy, j >> sx): chroma is taken nearest, as for NV12 lists.  A chroma plane has ceil(hs / 2^sy) rows of
 * ceil(ws / 2^sx) samples, so the last row / column of an odd-sized frame has a sample of its own.  The conversion
 * is the one above under the list's matrix (a property of the list, as for NV12 lists; a JPEG caller passes
 * ORE_YUV_BT601_FULL); a grey frame has U = V = 128, hence R = G = B.
 * Image i of a YUV list is, bit for bit, what an interleaved list (c = 3) of the same filter gives for the
 * [hs,ws,3] R, G, B bytes of that frame converted by this rule, for the same geometry, scale / shift,
 * ORE_PRE_REVERSE_CHANNELS and ORE_IMAGE_FLIP_H.  Hence an ORE_YUV_FMT_NV12 descriptor gives what the same frame
 * gives in an NV12 list.
 *  ore_image_yuv: plane[] are DEVICE pointers of any alignment; a plane the format does not use must be NULL.
 *    stride[] are bytes between rows, 0 meaning dense; the bytes of a row ("row bytes") are, with wc = ceil(ws/2^sx):
 *        plane[0]: ws (4 * ceil(ws/2) for YUYV);  plane[1]: wc (2 * ceil(ws/2) for NV12's UV);  plane[2]: wc.
 *    plane[0] has hs rows, the others ceil(hs / 2^sy).  reserved must be 0.  A region of interest of a larger frame
 *    is a descriptor whose pointers are offset to an origin (y0, x0) that is a multiple of (2^sy, 2^sx) -- for YUYV
 *    an even column: plane[0] + y0 * stride[0] + x0 (2 * x0 for YUYV) and plane[k] + (y0 >> sy) * stride[k] +
 *    (x0 >> sx) (times 2 for NV12's UV).  At any other origin the pixels would pair up with the wrong chroma
 *    samples: rounding the origin is the caller's to do, the library sees only the pointers.
 *  ore_image_check_yuv: host only.  Per descriptor, in this order: the format is one of ore_yuv_format; reserved
 *    is 0; every plane the format uses is non-null and every other is NULL; sizes, geometry as in
 *    ore_image_check_ex with c = 3; each used plane's stride is 0 or >= its row bytes; (rows - 1) * stride + row
 *    bytes < 2^31 for each used plane (a plane of one row never steps a row); under ORE_FILTER_BILINEAR_AA the
 *    ratio rule.  The first failing descriptor gives ORE_ERR_INVALID, a message with its index, the plane where
 *    one is at fault and the reason, and *bad_index (when non-null).  n == 0 is ORE_OK.
 *  ore_image_list_create_yuv: an ore_image_list with c = 3 whose format (ore_image_list_format: ORE_IMAGE_YUV) and
 *    matrix are fixed at creation.  Every entry that takes a list -- ore_preprocess_list_u8, the model's _u8_list
 *    runs, classifications and captures, chunked runs and views -- takes it as is.
 *  ore_image_list_set_yuv / _set_yuv_ex: ore_image_list_set / _set_ex for a YUV list, with the same semantics
 *    (check first, the old content kept on failure, stream-ordered upload from the pinned mirror,
 *    ORE_ERR_INVALID inside a capture, n == 0 empties, flags as for ore_image_list_set_ex).  A set of another kind
 *    on a YUV list, and these on a list of another kind (an NV12 list included), are ORE_ERR_INVALID and leave
 *    the list unchanged. */
typedef enum {
  ORE_YUV_FMT_NV12 = 0,  /* plane[0] Y, plane[1] interleaved (U,V) pairs; chroma halved both ways */
  ORE_YUV_FMT_YUYV = 1,  /* plane[0] packed Y0 U Y1 V groups of 4 bytes, ceil(ws/2) per row; chroma halved horizontally */
  ORE_YUV_FMT_I444 = 2,  /* plane[0] Y, plane[1] U, plane[2] V; chroma (sx, sy) = (0, 0) */
  ORE_YUV_FMT_I440 = 3,  /* (0, 1) */
  ORE_YUV_FMT_I422 = 4,  /* (1, 0) */
  ORE_YUV_FMT_I420 = 5,  /* (1, 1) */
  ORE_YUV_FMT_I411 = 6,  /* (2, 0) */
  ORE_YUV_FMT_GRAY = 7   /* plane[0] Y only; U = V = 128, so R = G = B */
} ore_yuv_format;
typedef struct ore_image_yuv {
  const uint8_t* plane[3];  /* DEVICE pointers, any alignment; planes the format does not use must be NULL */
  int64_t stride[3];        /* bytes between rows of each plane; 0 = dense */
  int64_t hs, ws;           /* 1..16384, any parity */
  int32_t format;           /* ore_yuv_format */
  int32_t reserved;         /* must be 0 */
  ore_resize g;             /* this frame's own {rh, rw, top, left} */
} ore_image_yuv;            /* 104 bytes */
ore_status ore_image_check_yuv(const ore_image_yuv* imgs, int64_t n, int64_t h, int64_t w, int32_t filter,
                               int64_t* bad_index);
ore_status ore_image_list_create_yuv(ore_ctx* ctx, int64_t capacity, int64_t h, int64_t w, int32_t filter,
                                     int32_t matrix, ore_image_list** out);
ore_status ore_image_list_set_yuv(ore_image_list* l, const ore_image_yuv* imgs, int64_t n);
ore_status ore_image_list_set_yuv_ex(ore_image_list* l, const ore_image_yuv* imgs, const uint32_t* flags, int64_t n);
/* Row-wise top-k (extension; no reference counterpart -- the reference prints the full output tensor): the
 * k best elements of every row of x, in one launch (ore_topk.hip).  Rows are x->dims[0], the row length D
 * the product of the remaining dims (as for ore_softmax_f32); x->nstride >= D is honoured.  values and
 * indices are contiguous DEVICE arrays [rows, k], 1 <= k <= min(D, 64).  Output j of a row is the element
 * ranked j in the order "larger value first; among equal values the lower index first", where -0.0 and
 * +0.0 are equal and every NaN ranks after every number (-inf included), NaNs among themselves by index:
 * exactly np.argsort(-x, axis=1, kind="stable")[:, :k].  values[r,j] is a bit copy of x[r, indices[r,j]]
 * (a zero keeps its sign, a NaN its payload).  rows == 0 is ORE_OK and launches nothing; a null argument
 * or a k out of range is ORE_ERR_INVALID, checked before any device call. */
ore_status ore_topk_f32(ore_ctx* ctx, const ore_tensor* x, int32_t k, float* values, int32_t* indices);
/* Several views of one subject (extension): mirrored images in image lists, and the top-k of
 * the mean of every `views` consecutive rows -- the five / ten-crop evaluation protocol, or the frames of a clip.
 *  ore_image_list_set_ex / _set_nv12_ex: ore_image_list_set / _set_nv12 with one flag word per descriptor.
 *    flags is a HOST array of n words, read before the call returns; NULL means all zero, and the call is then
 *    ore_image_list_set / _set_nv12 exactly.  A bit other than ORE_IMAGE_FLIP_H is ORE_ERR_INVALID with the
 *    descriptor's index in the message, and the list keeps its previous content, as for every rejected set.
 *    Everything else is ore_image_list_set's: the descriptors are checked first, the upload is stream-ordered
 *    from the pinned mirror, a set inside a capture or on a list of the other format is ORE_ERR_INVALID, and
 *    n == 0 empties the list.  ore_image_u8 and ore_image_nv12 are unchanged.
 *  ORE_IMAGE_FLIP_H: a horizontal mirror, defined by the unflipped result: output element (ch, r, q) of a
 *    flipped descriptor is, bit for bit, output element (ch, r, W-1-q) of the same descriptor without the flag.
 *    It is the mirror of the window at (top, left) of the resized image, NOT a resize of the mirrored source: the
 *    two differ in the last bits, because a tap weight t and its mirror image 1 - t do not round alike.  (The
 *    window of the mirrored image at column `left` is this flag with left' = rw - W - left.)  It holds for both
 *    filters, interleaved c = 1..4 and NV12 under every matrix, ORE_PRE_REVERSE_CHANNELS and y given as a
 *    slice; flipped image i of an NV12 list equals what a flipped interleaved list gives for the converted bytes.
 *    The dense entries (ore_preprocess_resize_u8*, ore_model_set_input_resize*) have no flip.
 *  ore_topk_mean_f32: ore_topk_f32 over the mean rows of groups of `views` consecutive rows.  x is [rows, D] as
 *    there (nstride >= D honoured), 1 <= views <= ORE_MAX_VIEWS, rows % views == 0; values and indices are
 *    contiguous DEVICE arrays [rows / views, k], 1 <= k <= min(D, 64).  All of this is checked from the arguments
 *    alone, before the context and any device call (ORE_ERR_INVALID, the message names views or k); rows == 0 is
 *    ORE_OK and launches nothing.  Element i of group g's mean:
 *        acc = x[gV, i];  for v = 1 .. V-1: acc = fadd_rn(acc, x[gV+v, i]);  m_i = fdiv_rn(acc, (float)V)
 *    in ascending view order, every operation rounded on its own, IEEE division, subnormals kept: numpy float32
 *    arrays reproduce m bit for bit.  The selection is ore_topk_f32's order applied to m; values[g,j] is a bit
 *    copy of m at indices[g,j] (a zero keeps its sign).  A NaN mean ranks as a NaN, after every number, by
 *    index; its payload is unspecified.  views == 1 is ore_topk_f32 itself (NaN payloads kept).  One launch, one
 *    wavefront per group. */
#define ORE_IMAGE_FLIP_H 1u
#define ORE_MAX_VIEWS 64
ore_status ore_image_list_set_ex(ore_image_list* l, const ore_image_u8* imgs, const uint32_t* flags, int64_t n);
ore_status ore_image_list_set_nv12_ex(ore_image_list* l, const ore_image_nv12* imgs, const uint32_t* flags, int64_t n);
ore_status ore_topk_mean_f32(ore_ctx* ctx, const ore_tensor* x, int32_t views, int32_t k, float* values, int32_t* indices);
/* Oriented list images (extension): what a hardware decoder leaves undone -- a JPEG's EXIF
 * orientation tag, a video container's display rotation -- applied inside the list's one launch.  An orientation is
 * an EXIF code 1..8 per descriptor.  hs, ws and the plane pointers still describe the STORED image; the geometry
 * g = {rh, rw, top, left} and the list's h x w describe the DISPLAYED image, which for codes 5..8 is ws x hs.  With
 * D the displayed and S the stored image (hs x ws), as PIL's ImageOps.exif_transpose shows it:
 *     1  D[r,c] = S[r, c]            5  D[r,c] = S[c, r]
 *     2  D[r,c] = S[r, ws-1-c]       6  D[r,c] = S[hs-1-c, r]        (rotate 90 degrees clockwise to display)
 *     3  D[r,c] = S[hs-1-r, ws-1-c]  7  D[r,c] = S[hs-1-c, ws-1-r]
 *     4  D[r,c] = S[hs-1-r, c]       8  D[r,c] = S[c, ws-1-r]        (rotate 270 degrees clockwise to display)
 * The resized image obeys the same table: the stored image is resized to rh_s x rw_s = (rh, rw) for codes 1..4 and
 * (rw, rh) for codes 5..8, and output element (ch, i, j) of the descriptor, with r = top + i and c = left + j, is the
 * filter's value at resized row a and resized column b of the STORED image, (a, b) the table's index pair for (r, c)
 * with rh_s, rw_s in place of hs, ws.  Row taps come from a, column taps from b, every float operation in the order
 * given above for the list's filter (columns inside, rows outside, in stored coordinates).  A tap depends only on
 * the absolute resized index, so the result is, bit for bit: the output of the unoriented descriptor of a list of
 * output shape (hz, wz) = (h, w) for codes 1..4 and (w, h) for codes 5..8 with the stored-space window
 * ore_orient_geometry gives, its rows reversed (codes 3 4 6 7) and / or its columns reversed (codes 2 3 7 8) and then
 * transposed (codes 5..8).  It is a permutation of the resized stored image, NOT a resize of the rotated bytes: the
 * two differ in the last bits for the reason given under ORE_IMAGE_FLIP_H, and because the separable passes run in
 * the other order.  An image that is not resized comes out as the oriented bytes exactly.  ORE_IMAGE_FLIP_H composes
 * on top: a flagged oriented descriptor is the oriented output with its columns reversed.  Of an NV12 or YUV frame the
 * chroma pairing stays in stored coordinates, so oriented image i of such a list equals, bit for bit, what an
 * interleaved list gives for the converted stored bytes with the same orientation, flag, geometry and filter.  The
 * ratio rules (ORE_AA_MAX_RATIO, ORE_CUBIC_AA_MAX_RATIO) apply to the stored axes: hs against rh_s, ws against rw_s.
 *  ore_orient_geometry: host only; the map above, the one the kernels use.  For a code 1..8, a displayed geometry g
 *    and the list's h x w: *stored_g = {rh_s, rw_s, top_s, left_s} with top_s = rev_rows ? rh_s - hz - a0 : a0, a0 =
 *    top for codes 1..4 and left for 5..8, and the analogous column rule; *hz, *wz; and the three permutation bits.
 *    Any output pointer may be NULL.  A code outside 1..8 or a NULL g is ORE_ERR_INVALID; nothing else is checked.
 *  ore_image_check_oriented / _check_nv12_oriented / _check_yuv_oriented: the _ex checks with a HOST array of n codes
 *    (NULL: all 1, the _ex check exactly).  A code outside 1..8 is ORE_ERR_INVALID with the descriptor's index and
 *    the word `orientation` in the message, checked before that descriptor's geometry.  The crop is checked in
 *    displayed space (top + h <= rh, left + w <= rw), which is the stored-space window's check; the ratio rules in
 *    stored space.  Messages about a descriptor's geometry quote its stored-space numbers.
 *  ore_image_list_set_oriented / _set_nv12_oriented / _set_yuv_oriented: _set_ex with the codes array, read before
 *    return; NULL means all 1.  Everything else is _set_ex's: the check first, the previous content, count and
 *    orientations kept on any failure, the upload stream-ordered from the pinned mirror, ORE_ERR_INVALID inside a
 *    capture or on a list of another kind, n == 0 empties the list.  The _ex sets still reject every flag bit other
 *    than ORE_IMAGE_FLIP_H; ore_image_u8, ore_image_nv12 and ore_image_yuv keep their layouts.
 *  ore_image_list_oriented: 1 once an oriented set has succeeded on the list (n == 0 and all-1 codes included), for
 *    good; 0 before.  The mark decides which kernels a CAPTURE of the list records: a marked list records the
 *    orientation-reading instances, which serve whatever a later set uploads; an unmarked list records the instances
 *    it records today, and ore_model_graph_launch of such a graph is ORE_ERR_INVALID ("re-capture") once the list
 *    holds a code other than 1.  A caller that captures ore_preprocess_list_u8 into a graph of its own and means to
 *    set orientations later MUST mark the list first (one ore_image_list_set_oriented call, n == 0 will do): the
 *    library cannot check a graph it does not own, and an unmarked capture ignores the orientation bits.  Outside a
 *    capture the kernels follow the list's last set: all codes 1 launches exactly what a list without orientations
 *    launches, flags included.  The dense entries (ore_preprocess_resize_u8*, ore_model_set_input_resize*) take no
 *    orientation, as they take no flip. */
ore_status ore_orient_geometry(int32_t orientation, const ore_resize* g, int64_t h, int64_t w, ore_resize* stored_g,
                               int64_t* hz, int64_t* wz, int32_t* rev_rows, int32_t* rev_cols, int32_t* transpose);
ore_status ore_image_check_oriented(const ore_image_u8* imgs, int64_t n, int64_t c, int64_t h, int64_t w, int32_t filter,
                                    const uint8_t* orientations, int64_t* bad_index);
ore_status ore_image_check_nv12_oriented(const ore_image_nv12* imgs, int64_t n, int64_t h, int64_t w, int32_t filter,
                                         const uint8_t* orientations, int64_t* bad_index);
ore_status ore_image_check_yuv_oriented(const ore_image_yuv* imgs, int64_t n, int64_t h, int64_t w, int32_t filter,
                                        const uint8_t* orientations, int64_t* bad_index);
ore_status ore_image_list_set_oriented(ore_image_list* l, const ore_image_u8* imgs, const uint32_t* flags,
                                       const uint8_t* orientations, int64_t n);
ore_status ore_image_list_set_nv12_oriented(ore_image_list* l, const ore_image_nv12* imgs, const uint32_t* flags,
                                            const uint8_t* orientations, int64_t n);
ore_status ore_image_list_set_yuv_oriented(ore_image_list* l, const ore_image_yuv* imgs, const uint32_t* flags,
                                           const uint8_t* orientations, int64_t n);
int32_t ore_image_list_oriented(ore_image_list* l);

/* ------------------------------------------------------------------ graph walker (inference()) */
/* Parse an ONNX ModelProto (bytes), upload every initializer to HBM once, plan the value
 * buffers for up to max_batch images, and prepare the node list in file order.  Any max_batch is
 * accepted: the arena holds run_batch = min(max_batch, the largest batch whose every activation fits
 * the kernels' 32-bit byte offsets) images (ore_model_run_batch), and larger runs go in image chunks.
 * Unsupported ops/attributes fail here (the reference panics when it reaches them). */
ore_status ore_model_load(ore_ctx* ctx, const void* onnx_bytes, size_t len, int64_t max_batch,
                          ore_model** out);
/* Host-only wire-format check of an ONNX ModelProto, the reference's
 * `ModelProto::parse_from_bytes` (main.rs:30) before any inference: ORE_OK, or ORE_ERR_PARSE for
 * malformed protobuf (truncated payloads, a field sent with the wrong wire type, ...) with the
 * reason in ore_last_error(NULL).  Touches no device; ore_model_load runs the same parser. */
ore_status ore_model_parse(const void* onnx_bytes, size_t len);
/* Load flags.  ORE_LOAD_F16: the fp16 variant (no reference
 * counterpart -- the reference is f32 only): Conv weights and the activations of Conv / MaxPool /
 * Relu / Concat / Dropout are f16, Conv accumulates in f32 on the f16 matrix cores (bias and Relu
 * in f32, rounded once), GlobalAveragePool sums f16 inputs in f32, and Softmax, Add and MatMul
 * stay f32 (Add / MatMul / Softmax on an f16 value is rejected).  The model input and
 * graph.output[0] stay f32 (an f16 graph output is rejected).
 * One conv layer is y = RNE_f16(relu?(sum_k f16(x_k) f16(w_k) [f32 accumulate] + b_f32)): the operands are
 * rounded to nearest even, their products are exact in f32, and tests/test_f16_parity_gpu.py holds every
 * output to the correctly rounded f16 of a value within 2e-6 * (sum |w x| + |b|) of the float64 sum
 * (measured accumulation error: at most 5.4e-8 of that magnitude).  Outputs past 65504 in magnitude
 * are +-inf: the kernels do a plain (_Float16) cast and no clamp.  f16 subnormals are kept -- as
 * weights, as activations read by the matrix cores and as outputs (gradual underflow, nothing is
 * flushed; measured on gfx950). */
#define ORE_LOAD_F16 1
/* ORE_LOAD_NO_WINOGRAD: an f32 model runs its 3x3 / stride-1 / pad-1 convs (SqueezeNet's
 * expand3x3) on the direct kernels only, every output in the reference's k order.  By default (f32
 * models) every such conv with C % 16 == 0 that no direct-kernel fusion takes runs Winograd
 * F(2x2, 3x3) in f32 (ore_conv_wino.hip; see ORE_CONV_ALGO_WINOGRAD above).  NOTE: this makes the
 * default f32 results differ from the direct path by rounding (synthetic SqueezeNet @224: 6e-6
 * max-abs against the oracle vs 2e-7 direct, within the 1e-5 parity bound); load with this flag for
 * the reference's summation order.  The choice is made at load time, never by timing. */
#define ORE_LOAD_NO_WINOGRAD 4
/* ABI 1's ORE_LOAD_X3 (2) and ORE_LOAD_X3_ALL (8): retired, rejected with ORE_ERR_UNSUPPORTED. */
#define ORE_LOAD_RETIRED_MASK 10
ore_status ore_model_load_ex(ore_ctx* ctx, const void* onnx_bytes, size_t len, int64_t max_batch, int32_t flags,
                             ore_model** out);
ore_status ore_model_destroy(ore_model* m);
/* Fusion flags (ore_model_set_fusion; ORE_FUSE_ALL is the default, 0 runs every node as its own kernel
 * for op-by-op parity).  Every fusion is exact: the fused kernels compute each output by the same
 * arithmetic as the separate ones, so results do not depend on the flags (tested bit for bit).
 * bit 0 = fuse Conv->Relu, bit 1 = Concat in place (and padded channel planes), bit 2 = alias
 * Dropout / Reshape; bits 5-10 and 12 below.  Bit 4 (ABI 1's ORE_FUSE_POOL_CONV, a MaxPool inside a
 * 1x1 conv's operand gather, measured slower) is retired: ORE_ERR_UNSUPPORTED.
 * Non-finite activations (an f16 model makes them itself: outputs past 65504 are +-inf, and the next layer
 * sees inf x 0 or inf - inf): every plan of a model still returns the same result, and it is the
 * reference's.  Relu(NaN) = +0 (Relu is f32::max, relu_op.rs); MaxPool ignores NaN and pads with zero (it
 * folds f32::max from f32::MIN over the zero-padded window, so a window of NaN alone gives f32::MIN, which an
 * f16 model stores as -inf); Conv, GlobalAveragePool and Softmax propagate NaN, and inf x 0 is NaN under a
 * zero weight as under any other -- but only under a weight of the graph: the zero weights and zero operands
 * the kernels pad their tiles with never meet an activation's inf or NaN (tests/test_nonfinite_gpu.py).
 * Winograd is exempt: its input transform adds and subtracts neighbouring pixels before the multiply, so inf -
 * inf and the footprint of a NaN differ from the direct sum; load with ORE_LOAD_NO_WINOGRAD where that matters. */
#define ORE_FUSE_CONV_RELU 1
#define ORE_FUSE_CONCAT 2
#define ORE_FUSE_ALIAS 4
#define ORE_FUSE_ALL 14311
/* bit 5 (in ORE_FUSE_ALL): Conv (-> Relu) -> 3x3 / stride-2 MaxPool as ONE launch when the conv
 * output has no other consumer: each block computes a 13 x 19 patch of conv outputs covering a
 * 6 x 9 tile of pooled outputs (the overlapping window row / column is recomputed by the
 * neighbouring tile) and stores only the pooled values; the pre-pool tensor never reaches HBM.
 * Bit-identical (same per-output MFMA chain; max is exact).  Applied when the computed columns are
 * <= 1.25 x the conv's own (SqueezeNet @224: conv1 + pool1 only, 1.16x).  f32 models: ore_model_autotune also times the row-walking kernels
 * (ore_conv_pool.hip: a block walks the conv plane row-major and max-reduces into an LDS ring of
 * pooled rows, nothing recomputed) and keeps the fastest -- conv1 + pool1: 96 channels x 128
 * quads per block, 1016 -> ~900 us at batch 256. */
#define ORE_FUSE_CONV_POOL 32
/* bit 6: a fire module (Concat of a 1x1 and a 3x3 'same' Conv + Relu of one value, 64-multiple
 * channel counts) and the 1x1 Conv + Relu (<= 64 channels) that is the Concat's only reader -- the
 * next fire's squeeze -- as ONE launch: the expand outputs and the Concat never reach HBM.
 * Bit-identical (every output keeps its k-ordered MFMA chain; the squeeze still sums the concat
 * channels in ascending order).  f32 (fire_kernel) and f16 (fire_f16_kernel) models; f32: applied when
 * max_batch * H * W >= 65536 (one 64-pixel wave per SIMD), below which the fused launch has too few
 * waves (batch 1 keeps the separate kernels).  f16 models also take a fire module whose Concat is
 * read by something other than a squeeze (SqueezeNet's fire9, read by conv10): its expands and the
 * Concat run as one fire_f16_kernel launch that stores the Concat. */
#define ORE_FUSE_FIRE 64
/* bit 7 (in ORE_FUSE_ALL): Concat(e1, e3) -> 3x3 / stride-2 MaxPool with e1 / e3 Convs
 * (+ Relu) read only by the Concat (SqueezeNet's fire4 -> pool3, fire8 -> pool5): each conv's pooled
 * epilogue (the row-walking kernel, ore_conv_pool.hip) writes its channel slice of the pool output,
 * so neither the expand outputs nor the Concat reach HBM.  Bit-identical (the pool is per channel;
 * every pooled value is the max of the same nine values).  f32 models, conv planes of at least 1024
 * pixels: at batch 256 fire4 -> pool3 (54 x 54) saves 40 us per step, fire8 -> pool5 (27 x 27)
 * would cost 21 us (the walker's expand3x3 runs at 88-92 % of the streaming kernel's rate). */
#define ORE_FUSE_CONCAT_POOL 128
/* bit 8: a fire module, the 3x3 / stride-2 MaxPool of its Concat and the next squeeze as ONE launch
 * (f32 fire_pool_kernel on expand planes of >= 1024 pixels at max_batch * H * W >= 65536: fire4 +
 * pool3 + fire5/squeeze; f16 fire_pool_f16_kernel: also fire8 + pool5 + fire9/squeeze). */
#define ORE_FUSE_FIRE_POOL 256
/* bit 9: the first conv + its pooled epilogue also runs the pooled map's only reader, a 1x1 conv
 * (+ Relu) with <= 16 (f32) / 32 (f16) channels (conv1 + pool1 + fire2/squeeze). */
#define ORE_FUSE_FIRST_SQUEEZE 512
/* bit 10: a 3x3 / stride-2 MaxPool read only by a 1x1 conv (+ Relu, <= 64 channels) runs inside that
 * conv (f32 pool_conv1x1_f32_kernel: pool5 + fire9/squeeze). */
#define ORE_FUSE_POOL_SQUEEZE 1024
/* bit 12: a 1x1 conv (+ Relu) whose only reader is GlobalAveragePool runs with the GAP in its
 * epilogue: conv10 + relu10 + pool10 in one launch, the conv map never stored (f16 models:
 * conv1x1_gap_f16_kernel; f32 models since round 4: conv1x1_gap_f32_kernel, input channels a multiple
 * of 32, <= 256 pixels).  Bit-identical to the separate launches; not under ORE_KEEP_VALUES. */
#define ORE_FUSE_CONV_GAP 4096
/* bit 13 (round 5): with ORE_FUSE_POOL_SQUEEZE, a pool whose input is Concat(e1, e3) with e1 a 1x1
 * conv (+ Relu) of 32 / 64 channels read only by the Concat: e1 is recomputed inside the pooled
 * squeeze from its own input, so its map is never stored (SqueezeNet fire4 -> pool3 -> fire5 and
 * fire8 -> pool5 -> fire9 when their expand3x3 runs Winograd).  Bit-identical; f32 models; not
 * under ORE_KEEP_VALUES. */
#define ORE_FUSE_POOL_EXPAND 8192
/* bit 11 (tests, not in ORE_FUSE_ALL): apply every eligible fusion regardless of the size
 * heuristics above (batch / plane thresholds, the 1.25 patch-work bound). */
#define ORE_FUSE_EAGER 2048
/* debug: give every value its own storage (no liveness reuse) so any value can be read back */
#define ORE_KEEP_VALUES 8
ore_status ore_model_set_fusion(ore_model* m, int32_t flags);
/* Scratch poisoning (debug extension, off by default; nothing on a run's path reads these settings).  The
 * library never initialises the device memory it allocates for itself, and kernels read parts of it by
 * design: padded channel planes, the slots' 256-B rounding tails, the 4 KiB lead in front of the arena, the
 * slots of images n .. run_batch-1 of a smaller run, what an earlier value left in a reused slot.  None of
 * that may reach a result, whatever bits it holds (tests/test_scratch_poison_gpu.py, with NaN and +inf).
 *  ore_ctx_set_alloc_fill: while on, every device allocation the library makes for itself on this context
 *    -- a model's arena block with its lead, its f16 input conversion buffer (xcvt), uint8 staging buffer
 *    (stage) and top-k rows buffer (rows), its initializer block, its packed weights and the fused kernels'
 *    weight packs, and the context's per-op weight scratch -- is filled with the 32-bit pattern on the
 *    context's stream before anything else touches it.  ore_malloc is the caller's memory and is not filled;
 *    the image lists' descriptor tables hold device addresses and are not filled either.
 *  ore_model_fill_scratch: the same fill, now, of the model's activation memory (arena block with lead, xcvt,
 *    stage, rows; never weights), stream-ordered: between ore_model_set_fusion (which plans into the arena
 *    it has) and a run, or between two runs.  ORE_ERR_INVALID while the context's stream is capturing.
 *  ore_model_scratch_info: buffer i of that activation memory (those that exist, in the order above): its
 *    name, device pointer and size, for ore_download; ORE_ERR_INVALID past the last one.  Host only.
 * A null context / model is ORE_ERR_INVALID before any device call. */
ore_status ore_ctx_set_alloc_fill(ore_ctx* ctx, int32_t on, uint32_t pattern);
ore_status ore_model_fill_scratch(ore_model* m, uint32_t pattern);
ore_status ore_model_scratch_info(ore_model* m, int32_t i, const char** name, void** dptr, size_t* bytes);
/* The seeded model input (graph.input entries that are not initializers, utils.rs:29-45):
 * per-image dims; dims[0] is the batch. */
ore_status ore_model_input_dims(ore_model* m, int64_t dims[4]);
/* Elements per image of graph.output[0] (the reference only prints it; we keep it). */
ore_status ore_model_output_elems(ore_model* m, int64_t* elems);
/* Run all nodes on n <= max_batch images.  d_input/d_output are device pointers
 * (n * input elems / n * output elems).  Asynchronous on the context stream.  n > run_batch runs the
 * graph once per chunk of at most run_batch consecutive images (each image's arithmetic is the same
 * in any chunk). */
ore_status ore_model_run(ore_model* m, const float* d_input, int64_t n, float* d_output);
/* Images one pass of the graph covers (see ore_model_load). */
int64_t ore_model_run_batch(ore_model* m);
/* Copy a named value of the last run to host memory (for node-level parity checks; values
 * elided by fusion, and values of a run chunked over run_batch, are unavailable -> ORE_ERR_INVALID).
 * Synchronises. */
ore_status ore_model_read_value(ore_model* m, const char* name, float* host_dst, size_t cap_elems,
                                int64_t dims[4], int32_t* ndim);
/* Per-node timing with HIP events on the context stream (enable, run, then query).
 * ore_model_node_count/ore_model_node_info describe the executed kernel steps. */
/* Measure every Conv step's candidate block tiles (128x128, 96x128, 64x128, 32x256) on a real
 * run of n images (d_input / d_output as for ore_model_run) and keep the fastest per layer (like
 * a benchmark-mode convolution search).  Results do not depend on the tile.  Synchronous.
 * reps: timed launches per candidate (<= 0: 3).  The choice survives ore_model_set_fusion.  A batch
 * above run_batch is tuned on its first chunk, then run whole once, so on return d_output holds the
 * output of all n images either way. */
ore_status ore_model_autotune(ore_model* m, const float* d_input, int64_t n, float* d_output, int32_t reps);
/* Block tile chosen for exec step i (-1 for non-conv steps); steps with one fixed kernel report its
 * id (e.g. 49 / 50: conv + GlobalAveragePool, f16 / f32).  The f32 first conv + pool + squeeze step
 * has two: 44 (13 x 19 patches) and 51 (the band walker, round 5); the f16 one 43 (patches) and 52 (the
 * f16 band walker, round 6).  The autotune keeps the faster. */
int32_t ore_model_step_tile(ore_model* m, int32_t i);
/* Set exec step i's tile (one of the ids ore_model_autotune chooses among for that step; e.g. to
 * restore a saved autotune result).  ORE_ERR_INVALID for an id outside the step's kernel family.
 * Survives ore_model_set_fusion like the autotuned choice. */
ore_status ore_model_set_step_tile(ore_model* m, int32_t i, int32_t tile);
/* MFMA FLOPs exec step i issued in the last run: its algorithmic FLOPs (ore_model_step_info), except
 * Winograd steps, which issue 16 C M per 2x2 output tile against the direct 36 C M. */
ore_status ore_model_step_mfma_flops(ore_model* m, int32_t i, double* flops);
/* Branch concurrency (the reference runs the two expand branches of a fire
 * module on threads, multithreading.rs:20-62): with 2 streams, adjacent independent steps (no
 * data dependence, no overlapping storage) run on a side stream beside the main one, joined by
 * events.  Pays off at small batch, where one conv does not fill the GPU.  Default 1. */
ore_status ore_model_set_streams(ore_model* m, int32_t streams);
/* Capture one ore_model_run(d_input, n, d_output) into a HIP graph (launch-bound small batches:
 * one graph launch replaces ~30 kernel launches); replay it with ore_model_graph_launch on the
 * context stream.  The graph keeps the buffers and batch it was captured with; re-capture after
 * ore_model_set_fusion / set_streams.  Needs a non-null context stream. */
ore_status ore_model_graph_capture(ore_model* m, const float* d_input, int64_t n, float* d_output);
ore_status ore_model_graph_launch(ore_model* m);
/* uint8 input (extension, see ore_preprocess_u8): the _u8 entries take n images as device uint8
 * [n,H,W,C] (C, H, W = ore_model_input_dims), convert them into a model-owned float32 NCHW staging buffer
 * and run the graph on it, for f32 and f16 models alike (the staging tensor is the float32 model input
 * both consume).
 *  ore_model_set_input_norm: the scale / shift (HOST arrays of c floats, NULL = 1 / 0, copied) and flags
 *    (ORE_PRE_REVERSE_CHANNELS) of the conversion; c must equal the model input's channel count.
 *    Defaults: scale 1, shift 0, no reversal.  Also allocates the staging buffer.
 *  The staging buffer holds run_batch images (154 MB at 256 x 3 x 224 x 224) and lives until
 *    ore_model_destroy.  It is allocated by ore_model_set_input_norm, ore_model_graph_capture_u8 or the
 *    first ore_model_run_u8 -- never inside a stream capture: a caller capturing ore_model_run_u8 into a
 *    graph of its own calls ore_model_set_input_norm first (ORE_ERR_INVALID otherwise).
 *  ore_model_run_u8: as ore_model_run, chunks included (the same chunks: convert a chunk, run it).
 *    ore_model_read_value afterwards behaves as after ore_model_run; the input value reads back as the
 *    converted float32 tensor.  The conversion is not an exec step: ore_model_step_count / _step_info /
 *    _step_tile / _step_times do not see it, and ore_model_autotune stays float32-only (tune on a batch
 *    converted with ore_preprocess_u8).
 *  ore_model_graph_capture_u8: as ore_model_graph_capture, with the conversion inside the graph:
 *    ore_model_graph_launch converts and runs whatever d_input holds at that moment.
 *  ore_model_set_input_resize: from then on every _u8 entry (run_u8, classify_u8 and their captures) takes
 *    [n,hs,ws,C] images and resizes and crops them to the model's H x W with geometry g (see
 *    ore_preprocess_resize_u8; checked here, ORE_ERR_INVALID) in the launch that converts; g == NULL
 *    restores the direct conversion of [n,H,W,C].  scale, shift and flags stay those of
 *    ore_model_set_input_norm; the staging buffer, the chunks (chunk i0 reads from image i0 of d_input) and
 *    the step list are unchanged, and a captured graph keeps the geometry it was captured with.
 *  ore_model_set_input_resize_ex: the same with an ore_resize_filter (ORE_FILTER_BILINEAR_AA: the antialiased
 *    resize of ore_preprocess_resize_u8_ex, its ratio rule checked here); ore_model_set_input_resize means
 *    ORE_FILTER_BILINEAR.  A captured graph keeps the filter it was captured with. */
ore_status ore_model_set_input_norm(ore_model* m, const float* scale, const float* shift, int32_t c, int32_t flags);
ore_status ore_model_set_input_resize(ore_model* m, int64_t hs, int64_t ws, const ore_resize* g);
ore_status ore_model_set_input_resize_ex(ore_model* m, int64_t hs, int64_t ws, const ore_resize* g, int32_t filter);
ore_status ore_model_run_u8(ore_model* m, const uint8_t* d_input, int64_t n, float* d_output);
ore_status ore_model_graph_capture_u8(ore_model* m, const uint8_t* d_input, int64_t n, float* d_output);
/* Top-k output (extension, see ore_topk_f32): the classify entries run the graph as ore_model_run /
 * ore_model_run_u8 do, chunks included, but keep the [n, output elems] rows in a model-owned buffer and
 * write only the k best per image: d_scores float32 [n,k] and d_classes int32 [n,k], both contiguous
 * DEVICE arrays, in ore_topk_f32's order.
 *  ore_model_set_topk: k for the entries below, 1 <= k <= min(output elems, 64); default 1.  Also
 *    allocates the rows buffer.
 *  The rows buffer holds run_batch images' outputs (1 MB at 256 x 1000) and lives until
 *    ore_model_destroy.  It is allocated by ore_model_set_topk, a _capture_classify entry or the first
 *    classify call -- never inside a stream capture: a caller capturing ore_model_classify into a graph
 *    of its own calls ore_model_set_topk first (ORE_ERR_INVALID otherwise).
 *  ore_model_classify / _classify_u8: per chunk, one pass of the graph, then one top-k launch over the
 *    chunk's rows.  The selection comes after the pass's last timing event and is not an exec step:
 *    ore_model_step_count / _step_info / _step_tile / _step_times and ore_model_autotune do not see it.
 *    ore_model_read_value afterwards behaves as after ore_model_run.  n == 0 is ORE_OK.
 *  ore_model_graph_capture_classify / _classify_u8: as ore_model_graph_capture / _capture_u8 with the
 *    selection inside the graph: ore_model_graph_launch converts (u8), runs and selects. */
ore_status ore_model_set_topk(ore_model* m, int32_t k);
ore_status ore_model_classify(ore_model* m, const float* d_input, int64_t n, float* d_scores, int32_t* d_classes);
ore_status ore_model_classify_u8(ore_model* m, const uint8_t* d_input, int64_t n, float* d_scores, int32_t* d_classes);
ore_status ore_model_graph_capture_classify(ore_model* m, const float* d_input, int64_t n, float* d_scores,
                                            int32_t* d_classes);
ore_status ore_model_graph_capture_classify_u8(ore_model* m, const uint8_t* d_input, int64_t n, float* d_scores,
                                               int32_t* d_classes);
/* Image-list input (extension, see ore_image_list_create): the _u8_list entries are the _u8 entries with an
 * image list as the input; n is the list's count at the call (<= max_batch).  The list's (c, h, w) must equal
 * the model's input dims and its context the model's (ORE_ERR_INVALID).  Scale, shift and flags are those of
 * ore_model_set_input_norm; ore_model_set_input_resize is ignored by these entries and not changed by them
 * (it governs the pointer entries only).  Chunks as ore_model_run_u8: chunk i0 converts descriptors
 * [i0, i0 + nc) into the staging buffer, in front of the pass's first timing event; the conversion is not an
 * exec step.  The staging and rows buffers are allocated where the _u8 entries allocate them, never inside
 * a stream capture.
 *  ore_model_graph_capture_u8_list / _classify_u8_list: the graph keeps the list and the count it was
 *    captured with, and ore_model_graph_launch converts whatever the table holds at replay time:
 *    ore_image_list_set with the same count followed by a launch runs new images of new sizes.  With another
 *    count ore_model_graph_launch answers ORE_ERR_INVALID.  The list must outlive the graph. */
ore_status ore_model_run_u8_list(ore_model* m, ore_image_list* l, float* d_output);
ore_status ore_model_classify_u8_list(ore_model* m, ore_image_list* l, float* d_scores, int32_t* d_classes);
ore_status ore_model_graph_capture_u8_list(ore_model* m, ore_image_list* l, float* d_output);
ore_status ore_model_graph_capture_classify_u8_list(ore_model* m, ore_image_list* l, float* d_scores, int32_t* d_classes);
/* Views (extension, see ore_topk_mean_f32): after ore_model_set_views(m, V) every classify entry --
 * ore_model_classify, _classify_u8, _classify_u8_list and the three _graph_capture_classify* -- treats
 * consecutive runs of V images as one subject: the selection is ore_topk_mean_f32 over the rows, and d_scores /
 * d_classes are [n / V, k].  1 <= V <= min(ORE_MAX_VIEWS, run_batch), default 1; n (or the list's count) must be
 * a multiple of V (ORE_ERR_INVALID otherwise).  ore_model_run* and the full-row outputs ignore the setting; a
 * captured graph keeps the V it was captured with.  Chunks hold whole groups: with G = n / V and gb = run_batch
 * / V there are ceil(G / gb) chunks of ceil(G / nchunks) groups each, chunk c writing rows [g0, g0 + gc) -- at
 * V == 1 the arithmetic of ore_model_run.  Buffers, timing events and the step list are unchanged. */
ore_status ore_model_set_views(ore_model* m, int32_t views);
/* Class activation maps of the selected classes (extension; ore_cam.hip).  A model "has a map
 * conv" when, walking back from graph.output[0] through an optional Softmax and any Dropout / Reshape, it meets a
 * GlobalAveragePool fed by an optional Relu and then a Conv with a 1x1 kernel, stride 1, zero pads and M = the
 * model's output elems.  The pool's input T [n, M, Hm, Wm] is, class by class, the class activation map (Zhou et
 * al. 2016).  With classes c[g, j] as the classify entries return them (group g = image i / views):
 *     maps[i, j, r, q] = T[i, c[i / views, j], r, q]      float32, contiguous [n, k, Hm, Wm]
 * with the bits of T as the model's unfused plan stores it: f32 models the conv kernels' k-ordered f32 fma
 * chain, + bias, Relu; f16 models RNE_f16(relu?(sum_k f16(x_k) f16(w_k) [f32 accumulate] + b)) widened exactly.
 * Non-finite values follow the Conv and Relu rules above.  The maps do not depend on the fusion flags, the streams
 * setting or the tiles: one launch per chunk gathers the k weight rows and recomputes them from the conv's input.
 *  ore_class_maps_f32: the kernel alone, on f32 NCHW x [n, C, H, W] (x->nstride honoured, any 4-byte aligned
 *    base), DEVICE weights w [M, C] row-major, DEVICE bias [M] or NULL, DEVICE classes [n / views, k] int32, into
 *    DEVICE maps [n, k, H, W].  Checked from the arguments alone, before the context and any device call
 *    (ORE_ERR_INVALID): null pointers, x not 4-D, k outside 1..min(M, 64), views outside 1..ORE_MAX_VIEWS, n not a
 *    multiple of views, the nstride rule at the top of this file.  n == 0 is ORE_OK and launches nothing.  A class
 *    id outside 0..M-1 cannot be checked on the host: the kernel clamps the row index, so it never reads outside w,
 *    and that slot's content is unspecified.  Nothing outside [n, k, H, W] is written.
 *  ore_model_cam_dims: Hm, Wm; ORE_ERR_UNSUPPORTED with a message naming what was found when the model has no
 *    map conv (MNIST-8).
 *  ore_model_set_cam: while d_maps (DEVICE, cap_elems floats) is set, every classify entry -- ore_model_classify,
 *    _classify_u8, _classify_u8_list and the three _graph_capture_classify* -- launches the map kernel behind each
 *    chunk's top-k launch, images [i0, i0 + nc) with the class rows from i0 / views, after the pass's last timing
 *    event (it is not an exec step); ore_model_run* ignore the setting.  A call with n * topk * Hm * Wm > cap_elems
 *    is ORE_ERR_INVALID before any device call.  NULL turns it off (the default).  Turning it on or off replans
 *    (the conv's input stays live to the end of the pass, as the output value does): ORE_ERR_INVALID while the
 *    stream is capturing; re-capture afterwards, as after ore_model_set_fusion; autotuned tiles survive.  Changing
 *    only the pointer or the capacity does not replan.  Off, the plan, the arena and the launches are those of a
 *    model that never had it on.  A captured graph keeps the buffer and setting it was captured with.
 *    ore_model_read_value of the conv's input works after a run with the maps on. */
ore_status ore_class_maps_f32(ore_ctx* ctx, const ore_tensor* x, const float* w, const float* bias, int64_t M, int32_t relu,
                              const int32_t* classes, int32_t k, int32_t views, float* maps);
ore_status ore_model_cam_dims(ore_model* m, int64_t hw[2]);
ore_status ore_model_set_cam(ore_model* m, float* d_maps, int64_t cap_elems);
/* Localisation from class activation maps (extension; ore_cam_box.hip): the maps at image
 * resolution, and one box per map (Zhou et al. 2016: resize the map to the image, keep what is above a fraction
 * of its range, box the largest connected component).  Given the bits of a map, both answers are exact.
 *  Upsampled value.  A plane m [Hm, Wm] resized to H x W, H >= Hm and W >= Wm: with (y0, y1, ty) row r's entry of
 *    ore_resize_taps(Hm, H, 0, H), (x0, x1, tx) column q's of ore_resize_taps(Wm, W, 0, W), and a, b, c, d =
 *    m[y0, x0], m[y0, x1], m[y1, x0], m[y1, x1]:
 *        top = a + (b - a) tx;  bot = c + (d - c) tx;  u[r, q] = top + (bot - top) ty
 *    where every -, * and + rounds on its own (never an FMA), as in the resize above.  With H = Hm and W = Wm it is
 *    m exactly.  NaN and +-inf follow the arithmetic as written.
 *  Box.  For one plane, u its upsampled values and a fraction 0 <= frac <= 1: lo, hi = the minimum and maximum of
 *    the non-NaN elements of u (np.fmin / np.fmax reductions; NaN when there is none);
 *        thr = fadd_rn(lo, fmul_rn(frac, fsub_rn(hi, lo)));   mask = u >= thr
 *    (a NaN u or a NaN thr is false).  Components of the mask are 8-connected; the chosen one has the most pixels,
 *    and among equal counts the one whose first pixel in raster order comes first.  box = (top, left, bottom, right),
 *    half-open, in the H x W grid, and area = the component's pixel count; an empty mask gives (0, 0, 0, 0) and 0.
 *  Caps of the box: Hm Wm <= ORE_CAM_BOX_MAX_MAP, Hm <= H <= ORE_CAM_BOX_MAX_SIDE, Wm <= W <= ORE_CAM_BOX_MAX_SIDE.
 *  ore_upsample_maps_f32: DEVICE contiguous maps [planes, hm, wm] -> DEVICE out [planes, h, w]; nothing else is written.
 *    Checked in this order, the context last, all before any device call (ORE_ERR_INVALID, the message names the
 *    quantity): null pointers; planes < 0; hm, wm, h, w outside 1..16384; h < hm or w < wm; planes h w >= 2^31.
 *  ore_cam_boxes_f32: DEVICE contiguous maps [planes, hm, wm] -> DEVICE boxes [planes, 4] and areas [planes] (or
 *    NULL), one workgroup per plane, no global scratch; the H x W planes are never stored.  Checked in this order,
 *    the context last (ORE_ERR_INVALID): null maps or boxes; planes < 0 (or >= 2^31); the caps (hm wm, then h, then
 *    w); h < hm or w < wm; frac outside [0, 1] or NaN.
 *  Both: planes == 0 is ORE_OK and launches nothing.
 *  ore_cam_box_host: host only, one plane in HOST memory, as ore_resize_taps is: the plain C++ restatement (the
 *    shared tap header, a queue flood fill) for integrators to test against.  The checks of ore_cam_boxes_f32;
 *    area may be NULL.
 *  ore_model_set_cam_boxes: while d_boxes (DEVICE, cap_planes x 4 int32; d_areas cap_planes int32 or NULL) is set,
 *    every classify entry that ore_model_set_cam governs launches the box kernel behind each chunk's map launch
 *    (after the pass's last timing event; not an exec step) over planes [i0 topk, (i0 + nc) topk) of the maps buffer,
 *    H x W the model's input size: boxes[i, j] belongs to maps[i, j] (per image under views, as the maps are).
 *    ORE_ERR_INVALID when the maps are off, when frac is outside [0, 1], when cap_planes < 0, and inside a stream
 *    capture; ORE_ERR_UNSUPPORTED naming it when the model's map or input size is outside the caps.  A classify
 *    call with n topk > cap_planes is ORE_ERR_INVALID before any device call.  d_boxes == NULL turns the boxes off
 *    (the default), and so does ore_model_set_cam(m, NULL, 0).  It never replans and allocates nothing; a captured
 *    graph keeps the setting it was captured with.  Off, every entry launches what it launched without it. */
#define ORE_CAM_BOX_MAX_MAP 4096
#define ORE_CAM_BOX_MAX_SIDE 512
ore_status ore_upsample_maps_f32(ore_ctx* ctx, const float* maps, int64_t planes, int64_t hm, int64_t wm, int64_t h, int64_t w,
                                 float* out);
ore_status ore_cam_boxes_f32(ore_ctx* ctx, const float* maps, int64_t planes, int64_t hm, int64_t wm, int64_t h, int64_t w,
                             float frac, int32_t* boxes, int32_t* areas);
ore_status ore_cam_box_host(const float* map, int64_t hm, int64_t wm, int64_t h, int64_t w, float frac, int32_t box[4],
                            int32_t* area);
ore_status ore_model_set_cam_boxes(ore_model* m, int32_t* d_boxes, int32_t* d_areas, int64_t cap_planes, float frac);
ore_status ore_model_enable_timing(ore_model* m, int32_t on);
int32_t ore_model_step_count(ore_model* m);
ore_status ore_model_step_info(ore_model* m, int32_t i, const char** op, const char** name, double* flops,
                               double* bytes);
ore_status ore_model_step_times(ore_model* m, float* ms, int32_t cap);

#ifdef __cplusplus
}
#endif
#endif /* ORE_H */
