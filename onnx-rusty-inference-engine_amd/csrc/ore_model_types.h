// The walker's private types, shared by the graph builder / launch side (ore_model.cpp) and the
// planner (ore_plan.cpp): values, steps, the model, and the few helpers both sides use.
#pragma once
#include <utility>

#include "ore_internal.h"

namespace ore {

enum StepKind { S_CONV, S_MAXPOOL, S_RELU, S_ADD, S_SOFTMAX, S_MATMUL, S_GAP, S_CONCAT, S_COPY, S_NOP, S_FIRE };

struct Value {
  std::string name;
  bool is_const = false;
  bool is_input = false;
  bool is_output = false;
  int ndim = 0;
  int64_t dims[4] = {0, 0, 0, 0};  // activations: dims[0] = 1 (per image)
  float* cptr = nullptr;           // const f32 device data
  std::vector<int64_t> i64;        // const int64 host data
  bool has_i64 = false;
  int alias_of = -1;               // view into another value's storage
  int64_t alias_ch = 0;            // concat slice: first channel inside the base
  bool slice = false;              // alias is a channel slice of its base (Concat in place)
  int64_t ps = 0;                  // 4-D activations: channel-plane stride (>= H*W; padded planes),
                                   // or for nhwc values the pixel stride (the root's channel count)
  int es = 4;                      // element bytes: 4 f32, 2 f16 (f16 models, ORE_LOAD_F16)
  bool nhwc = false;               // channels-last storage (every 4-D f16 activation)
  bool elided = false;             // produced and consumed inside one fused kernel
  int64_t arena_off = -1;          // byte offset in the arena (root values)
  int first = -1, last = -1;       // live interval in step indices
  int uses = 0;                    // consumer count (node inputs)

  // elements between images in this value's own storage (roots)
  int64_t image_stride() const {
    if (ndim != 4 || !ps) return per_image();
    return nhwc ? dims[2] * dims[3] * ps : dims[1] * ps;
  }
  int64_t per_image() const {
    int64_t s = 1;
    for (int i = 1; i < ndim; ++i) s *= dims[i];
    return s;
  }
  int64_t numel_const() const {
    int64_t s = 1;
    for (int i = 0; i < ndim; ++i) s *= dims[i];
    return s;
  }
};

struct Step {
  StepKind kind = S_NOP;
  std::string op, name;
  int in0 = -1, in1 = -1, in2 = -1, out = -1;
  int in3 = -1;  // a fourth activation input: the recomputed expand1x1's input S (pin.e1)
  // conv / pool geometry (per image)
  int64_t C = 0, H = 0, W = 0, M = 0, kh = 0, kw = 0, sh = 1, sw = 1;
  Window win;
  bool relu = false;
  bool w_kmajor = false;  // MatMul: the constant operand is [K][M]
  // The fusions' payloads, each owned by the pass that switches it `on`.
  // A preceding 3x3 / stride-2 MaxPool inside this 1x1 conv (pass pool_squeeze, pool_conv1x1_f32_kernel): in0
  // is the pool's input, of H x W planes
  struct PoolIn {
    bool on = false;
    int64_t H = 0, W = 0, sh = 1, sw = 1;
    Window win;
    // ... whose input is Concat(e1, e3) with e1 (a 1x1 conv + Relu of in3) recomputed inside the kernel
    // (pass pool_expand, ORE_FUSE_POOL_EXPAND): e1's K-major packing, its bias and shape
    struct E1 {
      bool on = false;
      const float *w = nullptr, *b = nullptr;
      int64_t C = 0, E = 0;
      int Mp = 0;
    } e1;
  } pin;
  // A following MaxPool in this conv's epilogue (ORE_FUSE_CONV_POOL): out is the pool's output
  struct Epool {
    bool on = false;
    int64_t kh = 0, kw = 0, sh = 1, sw = 1;
    Window win;
  } ep;
  int ran_tile = -1;  // S_CONV / S_MATMUL: the tile id its last launch ran (launch_step; -1: none, or a kernel without one)
  // S_FIRE (ORE_FUSE_FIRE): this squeeze conv also computes the fire module feeding it; in0 is the fire's
  // input S of C channels, the squeeze's K = E1 + E3.  M = 0: no squeeze, the Concat is the output.
  struct Fire {
    bool on = false;
    int64_t C = 0, E1 = 0, E3 = 0;
    const float *w1 = nullptr, *w3 = nullptr;  // the expand weights in launch_fire_pack layout
    const float *b1 = nullptr, *b3 = nullptr;
    bool f16 = false;            // f16 model: fire_f16_kernel, w1 / w3 / ws16 in launch_fire_pack_f16 layout
    const void* ws16 = nullptr;
    bool pool = false;           // a 3x3 / stride-2 MaxPool between the Concat and this squeeze
    int64_t H = 0, W = 0;        //   (fire_pool_kernel / fire_pool_f16_kernel): the expands' plane and the pool window
    Window pwin;
  } fire;
  // The pooled first conv with the next 1x1 conv (+ Relu) fused in (pass first_squeeze): out is that conv's
  // output; w in launch_fire_pack_f16 layout (f16) or the ONNX [M][K] (f32)
  struct FirstSqueeze {
    bool on = false;
    const void* w = nullptr;
    const float* b = nullptr;
    int64_t M = 0;
  } sq;
  // a 1x1 conv (+ Relu) whose only reader was GlobalAveragePool (ORE_FUSE_CONV_GAP, conv1x1_gap_f16_kernel /
  // conv1x1_gap_f32_kernel): out is the GAP's f32 [N][M] output
  bool gap = false;
  ConvPlan plan{};        // kernel choice and weight layout for S_CONV / S_MATMUL
  float* wp = nullptr;    // packed weights (layout per plan) for S_CONV / S_MATMUL
  const int2* ktab = nullptr;  // gather table (follows wp in the packed allocation; gather kernel only)
  // f32 models (not x3, not ORE_LOAD_NO_WINOGRAD): the Winograd F(2x2, 3x3) plan of a 3x3 / stride-1 /
  // pad-1 conv (ore_conv_wino.hip), packed next to the direct one; plan() switches a conv that no
  // direct-kernel fusion takes to it
  bool has_wino = false;
  ConvPlan plan_wino{};
  float* wp_wino = nullptr;
  const float* wc1 = nullptr;  // f32: the pooled first conv's weights for variant 7 (launch_pack_c1_f32), or the
                               // conv + GAP kernel's (launch_pack_cg_f32)
  int64_t axis = 1;
  double flops_per_img = 0, bytes_per_img = 0, bytes_fixed = 0;
  double mfma_flops_per_img = -1;  // MFMA FLOPs the kernel issues when they differ from flops (Winograd)
};

// the weight layouts of the fused kernels, packed on demand by the passes that plan them (ore_model::packs)
enum PackKind {
  PACK_FIRE_F32,   // launch_fire_pack: an expand conv of the f32 fire kernels
  PACK_FIRE_F16,   // launch_fire_pack_f16: an expand conv of the f16 fire kernels
  PACK_SQ_F16,     // launch_fire_pack_f16: their squeeze
  PACK_C1_F32,     // launch_pack_c1_f32: the pooled first conv's window kernel
  PACK_CG_F32,     // launch_pack_cg_f32: the conv + GAP kernel
  PACK_C1SQ_F16,   // launch_fire_pack_f16: the squeeze inside the f16 first conv + pool
};

}  // namespace ore

struct ore_model {
  ore_ctx* ctx = nullptr;
  int64_t max_batch = 0;
  int64_t run_batch = 0;         // images per pass of the graph (the arena's size; ore_model_run chunks above it)
  void* xcvt = nullptr;          // f16 F16_X_NHWC_PAIR: the f32 NCHW input converted to NHWC4 f16 (run_batch)
  size_t xcvt_bytes = 0;
  int32_t fusion = ORE_FUSE_ALL;
  bool f16 = false;              // ORE_LOAD_F16: f16 conv/pool activations, f32 accumulation
  bool wino = false;             // f32 model without ORE_LOAD_NO_WINOGRAD: Winograd plans for 3x3 s1 p1 convs
  int conv_tile = -1;            // the context's forced conv tile at load (ore_ctx_set_conv_tile)
  std::vector<ore::Value> values;
  size_t n_base_values = 0;      // values of the graph; plan() appends views after them (pooled slices)
  std::map<std::string, int> by_name;
  std::vector<ore::Step> base_steps;  // unfused, one per node
  std::vector<ore::Step> steps;  // after fusion
  int input_value = -1;
  int output_value = -1;
  float* consts = nullptr;       // one device allocation for all f32 initializers
  float* packed = nullptr;       // packed conv / matmul weights (one allocation)
  std::map<std::pair<ore::PackKind, int>, float*> packs;  // (layout, base step index) -> that conv's weights, packed once
  char* arena = nullptr;        // arena_alloc + ARENA_LEAD
  char* arena_alloc = nullptr;  // the hipMalloc'd block (the lead, then the arena proper)
  size_t arena_bytes = 0;
  // timing
  bool timing = false;
  std::vector<hipEvent_t> events;
  // branch concurrency (ore_model_set_streams): exec_steps[k] with pair_next[k] runs on the side
  // stream beside exec_steps[k + 1] (the two expand convs of a fire module: the reference's
  // branch threads, multithreading.rs:20-62)
  int streams = 1;
  std::vector<char> pair_next;
  hipStream_t side = nullptr;
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  // captured run (ore_model_graph_capture)
  hipGraph_t graph = nullptr;
  hipGraphExec_t graph_exec = nullptr;
  ore_image_list* graph_list = nullptr;  // a _u8_list capture: the list whose table the graph reads at replay,
  int64_t graph_list_count = 0;          // and the count it was captured with (ore_model_graph_launch checks it)
  bool graph_list_oriented = false;      // the list was marked (ore_image_list_oriented) at the capture: the graph reads orientations
  int timed_chunks = 0;          // image chunks of the last timed run (events: chunk x (exec_steps + 1))
  std::vector<int> exec_steps;   // indices into steps of launched (non-NOP) steps
  // run-time binding
  const float* cur_in = nullptr;
  float* cur_out = nullptr;
  bool out_bound = false;
  int64_t last_n = 0;
  bool last_chunked = false;     // the last run went in image chunks (arena values hold only the last one)
  // uint8 input (ore_model_run_u8): the f32 NCHW staging buffer of run_batch images the conversion writes
  // and the graph reads, and the normalisation of ore_model_set_input_norm (per output channel)
  float* stage = nullptr;
  size_t stage_bytes = 0;
  float in_scale[4] = {1.f, 1.f, 1.f, 1.f}, in_shift[4] = {0.f, 0.f, 0.f, 0.f};
  int32_t in_flags = 0;
  // ore_model_set_input_resize: the _u8 entries take [n, in_hs, in_ws, C] and resize into the staging buffer
  bool in_resized = false;
  int64_t in_hs = 0, in_ws = 0;
  ore_resize in_resize = {0, 0, 0, 0};
  int32_t in_filter = 0;  // ore_resize_filter of ore_model_set_input_resize_ex
  // top-k output (ore_model_classify): the f32 rows buffer of run_batch images' outputs the graph writes
  // and the selection reads, and the k of ore_model_set_topk
  float* rows = nullptr;
  size_t rows_bytes = 0;
  int32_t topk = 1;
  int32_t views = 1;  // ore_model_set_views: the classify entries select over the mean of this many consecutive rows
  // class activation maps (ore_model_set_cam): the map conv found at load (find_map_conv; cam_conv < 0: none, cam_why
  // says what was found instead), and the caller's buffer the classify entries fill behind each chunk's top-k launch
  int cam_conv = -1;             // base step index of the 1x1 conv in front of [Relu ->] GlobalAveragePool
  int cam_in = -1;               // its input value: with the maps on, never elided and live to the end of the pass
  int cam_map = -1;              // the pool's input value T (its dims are the map's)
  bool cam_relu = false;         // a Relu between the conv and the pool
  std::string cam_why;
  float* cam_buf = nullptr;      // DEVICE [n, topk, Hm, Wm]; null: off
  int64_t cam_cap = 0;           // its capacity in floats
  // boxes of the class activation maps (ore_model_set_cam_boxes): one launch behind each chunk's map launch
  int32_t* box_buf = nullptr;    // DEVICE [n, topk, 4]; null: off
  int32_t* box_areas = nullptr;  // DEVICE [n, topk] or null
  int64_t box_cap = 0;           // planes both hold
  float box_frac = 0.0f;         // the threshold's share of the map's range
};

namespace ore {

constexpr size_t ARENA_LEAD = 4096;  // mapped bytes before the arena proper (ore_ctx::mapped_lo)

inline ore_status err(ore_model* m, ore_status st, const std::string& msg) {
  return set_error(m->ctx, st, "%s", msg.c_str());
}

inline int value_id(ore_model* m, const std::string& name) {
  auto it = m->by_name.find(name);
  return it == m->by_name.end() ? -1 : it->second;
}

// the storage a view resolves to
inline int root(const ore_model* m, int id) {
  while (m->values[id].alias_of >= 0) id = m->values[id].alias_of;
  return id;
}

// bytes of a root value's arena slot: run_batch images, rounded to 256
inline int64_t slot_extent(const ore_model* m, const Value& v) {
  return ((v.image_stride() * m->run_batch * v.es) + 255) / 256 * 256;
}

// storage of a value for the current run
inline Ref ref_of(ore_model* m, int id) {
  const Value& v = m->values[id];
  if (v.is_const) return {v.cptr, 0, 0, 4};
  if (v.alias_of >= 0) {
    Ref base = ref_of(m, v.alias_of);
    if (v.slice)  // NCHW: the slice's first plane; NHWC: its first channel inside each pixel
      return {reinterpret_cast<float*>(reinterpret_cast<char*>(base.p) + v.alias_ch * (v.nhwc ? 1 : base.ps) * base.es),
              base.nstride, base.ps, base.es};
    return base;
  }
  if (v.is_input) return {const_cast<float*>(m->cur_in), v.image_stride(), v.ps, v.es};
  if (v.is_output && m->out_bound) return {m->cur_out, v.image_stride(), v.ps, v.es};
  return {reinterpret_cast<float*>(m->arena + v.arena_off), v.image_stride(), v.ps, v.es};
}

// fusion + planning (ore_plan.cpp): base_steps -> steps, the layout, the arena
ore_status plan(ore_model* m);
// the band walkers' geometry of a fused first conv + pool + squeeze step (ore_model.cpp, beside step_tile_family)
bool band_step(const Step& s);
bool band_f16_step(const Step& s);

}  // namespace ore
