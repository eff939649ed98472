// Graph walker: the device-resident replacement of `inference()` / `node_inference()`
// (model_inference.rs:29-162) and of the value map they share
// (`Arc<Mutex<HashMap<String, (Option<Array2>, Option<Array4>)>>>`, :30-32).
//
//  * Load: parse the ModelProto, upload every f32 initializer to HBM once (the reference
//    re-decodes them on every op call, utils.rs:113-185), run the reference's per-op shape and
//    attribute rules over the nodes in file order (the order the reference executes them in,
//    :84-115; its branch threads only reorder independent siblings), and turn each node into
//    a kernel step.  Anything the reference would panic on is reported here.
//  * Fuse (ORE_FUSE_*): Conv -> Relu into the conv epilogue; Concat(axis 1) of two
//    conv/pool outputs by writing both producers into channel slices of the concat buffer;
//    Dropout and activation Reshape as aliases.
//  * Plan: every materialised activation gets a slot in one device arena sized for max_batch,
//    slots reused by liveness (first-fit over [first write, last read] intervals).
//  * Run: launch the steps in order on the context stream; the model input and output are the
//    caller's device buffers.
//
// Batch: every activation carries a leading batch dim n (the reference is batch-1: it writes
// only image 0, e.g. convolution_op.rs:480).  Constants (initializers, Reshape of an
// initializer) carry none.
#include <algorithm>
#include <cstring>

#include "ore_chunk.h"
#include "ore_model_types.h"

using namespace ore;

namespace {

// IEEE binary16 -> binary32 (exact)
float half_bits_to_float(uint16_t h) {
  const uint32_t sign = uint32_t(h & 0x8000) << 16;
  uint32_t exp = (h >> 10) & 0x1f, man = h & 0x3ff, bits;
  if (exp == 0x1f) {
    bits = sign | 0x7f800000u | (man << 13);
  } else if (exp != 0) {
    bits = sign | ((exp + 112) << 23) | (man << 13);
  } else if (man == 0) {
    bits = sign;
  } else {  // subnormal: renormalise
    int e = -1;
    do { man <<= 1; ++e; } while (!(man & 0x400));
    bits = sign | (uint32_t(112 - e) << 23) | ((man & 0x3ff) << 13);
  }
  float f;
  std::memcpy(&f, &bits, 4);
  return f;
}

int new_value(ore_model* m, const std::string& name) {
  Value v;
  v.name = name;
  m->values.push_back(v);
  int id = int(m->values.size()) - 1;
  m->by_name[name] = id;  // re-definition shadows, as HashMap::insert does
  return id;
}

bool is_act(const Value& v, int rank) { return !v.is_const && v.ndim == rank; }

// ------------------------------------------------------------------ per-node shape/attr rules
ore_status build_conv(ore_model* m, const Node& n, Step* s) {
  if (n.inputs.size() < 2) return err(m, ORE_ERR_INVALID, "Conv '" + n.name + "' needs 2 inputs");
  int x = value_id(m, n.inputs[0]), w = value_id(m, n.inputs[1]);
  if (x < 0 || w < 0) return err(m, ORE_ERR_INVALID, "Conv '" + n.name + "': input not available");
  const Value &X = m->values[x], &Wt = m->values[w];
  if (!is_act(X, 4)) return err(m, ORE_ERR_UNSUPPORTED, "Conv '" + n.name + "': input must be a 4-D activation");
  if (!Wt.is_const || Wt.ndim != 4 || !Wt.cptr)
    return err(m, ORE_ERR_UNSUPPORTED, "Conv '" + n.name + "': weights must be a 4-D f32 initializer");
  int b = -1;
  if (n.inputs.size() > 2) {  // get_stored_tensor(2) (:124-130)
    b = value_id(m, n.inputs[2]);
    if (b < 0 || !m->values[b].is_const || m->values[b].ndim != 1 || !m->values[b].cptr)
      return err(m, ORE_ERR_UNSUPPORTED, "Conv '" + n.name + "': bias must be a 1-D f32 initializer");
    if (m->values[b].dims[0] != Wt.dims[0]) return err(m, ORE_ERR_INVALID, "Bias array has the wrong shape");
  }
  ore_conv_attrs a{};
  a.auto_pad = ORE_PAD_VALID;  // default (:134)
  a.group = 1;
  a.dilations[0] = a.dilations[1] = 1;
  bool have_strides = false;
  for (auto& at : n.attrs) {  // :137-163
    if (at.name == "auto_pad") {
      if (at.s == "SAME_UPPER") a.auto_pad = ORE_PAD_SAME_UPPER;
      else if (at.s == "SAME_LOWER") a.auto_pad = ORE_PAD_SAME_LOWER;
      else if (at.s == "VALID") a.auto_pad = ORE_PAD_VALID;
      else if (at.s == "NOT_SET") a.auto_pad = ORE_PAD_NOTSET;
      else return err(m, ORE_ERR_UNSUPPORTED, "Convolution Auto Pad specified not found: " + at.s);
    } else if (at.name == "dilations") {
      if (at.ints.size() < 2) return err(m, ORE_ERR_INVALID, "Conv dilations need 2 values");
      a.dilations[0] = at.ints[0]; a.dilations[1] = at.ints[1];
    } else if (at.name == "group") {
      a.group = at.i;
    } else if (at.name == "kernel_shape") {
    } else if (at.name == "pads") {
      a.n_pads = int32_t(std::min<size_t>(at.ints.size(), 4));
      for (int i = 0; i < a.n_pads; ++i) a.pads[i] = at.ints[i];
    } else if (at.name == "strides") {
      if (at.ints.size() < 2) return err(m, ORE_ERR_INVALID, "Conv strides need 2 values");
      a.strides[0] = at.ints[0]; a.strides[1] = at.ints[1];
      have_strides = true;
    } else {
      return err(m, ORE_ERR_UNSUPPORTED, "ATTRIBUTE NAME FOR CONVOLUTION NOT FOUND, " + at.name);
    }
  }
  if (!have_strides) return err(m, ORE_ERR_UNSUPPORTED, "Conv '" + n.name + "': strides attribute required");
  int64_t yd[4], p[4];
  if (ore_status st = ore_conv_out_shape(X.dims, Wt.dims, &a, yd, p)) {
    return err(m, st, "Conv '" + n.name + "': " + ore_last_error(nullptr));
  }
  s->kind = S_CONV;
  s->in0 = x; s->in1 = w; s->in2 = b;
  s->C = X.dims[1]; s->H = X.dims[2]; s->W = X.dims[3];
  s->M = Wt.dims[0]; s->kh = Wt.dims[2]; s->kw = Wt.dims[3];
  s->sh = a.strides[0]; s->sw = a.strides[1];
  s->win.pt = p[0]; s->win.pl = p[1]; s->win.pb = p[2]; s->win.pr = p[3];
  s->win.Ho = yd[2]; s->win.Wo = yd[3];
  const double P = double(yd[2] * yd[3]);
  s->flops_per_img = 2.0 * double(s->M) * P * double(s->C * s->kh * s->kw);
  const int yes = m->f16 ? 2 : 4;
  s->bytes_per_img = double(X.es) * double(s->C * s->H * s->W) + double(yes) * double(s->M) * P;
  s->bytes_fixed = double(yes) * double(Wt.numel_const()) + 4.0 * double(b >= 0 ? s->M : 0);
  int y = new_value(m, n.outputs[0]);
  Value& Y = m->values[y];
  Y.ndim = 4; Y.dims[0] = 1; Y.dims[1] = yd[1]; Y.dims[2] = yd[2]; Y.dims[3] = yd[3];
  Y.es = yes;
  s->out = y;
  return ORE_OK;
}

ore_status build_maxpool(ore_model* m, const Node& n, Step* s) {
  int x = value_id(m, n.inputs.empty() ? "" : n.inputs[0]);
  if (x < 0) return err(m, ORE_ERR_INVALID, "MaxPool '" + n.name + "': input not available");
  const Value& X = m->values[x];
  if (!is_act(X, 4)) return err(m, ORE_ERR_UNSUPPORTED, "MaxPool '" + n.name + "': input must be a 4-D activation");
  ore_pool_attrs a{};
  a.auto_pad = ORE_PAD_VALID;  // default (max_pool_op.rs:88); pads do NOT force NOTSET here
  bool have_k = false, have_s = false;
  for (auto& at : n.attrs) {  // :90-114
    if (at.name == "auto_pad") {
      if (at.s == "SAME_UPPER") a.auto_pad = ORE_PAD_SAME_UPPER;
      else if (at.s == "SAME_LOWER") a.auto_pad = ORE_PAD_SAME_LOWER;
      else if (at.s == "VALID") a.auto_pad = ORE_PAD_VALID;
      else if (at.s == "NOTSET") a.auto_pad = ORE_PAD_NOTSET;
      else return err(m, ORE_ERR_UNSUPPORTED, "MaxPool Auto Pad specified not found: " + at.s);
    } else if (at.name == "kernel_shape") {
      if (at.ints.size() < 2) return err(m, ORE_ERR_INVALID, "MaxPool kernel_shape needs 2 values");
      a.kernel[0] = at.ints[0]; a.kernel[1] = at.ints[1]; have_k = true;
    } else if (at.name == "pads") {
      a.n_pads = int32_t(std::min<size_t>(at.ints.size(), 4));
      for (int i = 0; i < a.n_pads; ++i) a.pads[i] = at.ints[i];
    } else if (at.name == "storage_order") {
    } else if (at.name == "strides") {
      if (at.ints.size() < 2) return err(m, ORE_ERR_INVALID, "MaxPool strides need 2 values");
      a.strides[0] = at.ints[0]; a.strides[1] = at.ints[1]; have_s = true;
    } else {
      return err(m, ORE_ERR_UNSUPPORTED, "ATTRIBUTE NAME FOR MAX POOL NOT FOUND, " + at.name);
    }
  }
  if (!have_k || !have_s) return err(m, ORE_ERR_UNSUPPORTED, "MaxPool '" + n.name + "': kernel_shape and strides required");
  int64_t yd[4], p[4];
  if (ore_status st = ore_pool_out_shape(X.dims, &a, yd, p))
    return err(m, st, "MaxPool '" + n.name + "': " + ore_last_error(nullptr));
  s->kind = S_MAXPOOL;
  s->in0 = x;
  s->C = X.dims[1]; s->H = X.dims[2]; s->W = X.dims[3];
  s->kh = a.kernel[0]; s->kw = a.kernel[1]; s->sh = a.strides[0]; s->sw = a.strides[1];
  s->win.pt = p[0]; s->win.pl = p[1]; s->win.pb = p[2]; s->win.pr = p[3];
  s->win.Ho = yd[2]; s->win.Wo = yd[3];
  s->bytes_per_img = double(X.es) * double(X.per_image() + s->C * yd[2] * yd[3]);
  const int xes = X.es;
  int y = new_value(m, n.outputs[0]);
  Value& Y = m->values[y];
  Y.ndim = 4; Y.dims[0] = 1; Y.dims[1] = yd[1]; Y.dims[2] = yd[2]; Y.dims[3] = yd[3];
  Y.es = xes;
  s->out = y;
  return ORE_OK;
}

ore_status build_unary4(ore_model* m, const Node& n, Step* s, StepKind kind) {
  int x = value_id(m, n.inputs.empty() ? "" : n.inputs[0]);
  if (x < 0 || !is_act(m->values[x], 4))  // `.1.clone().unwrap()` on a map entry
    return err(m, ORE_ERR_UNSUPPORTED, n.op_type + " '" + n.name + "': input must be a 4-D activation");
  s->kind = kind;
  s->in0 = x;
  const Value X = m->values[x];
  int y = new_value(m, n.outputs[0]);
  Value& Y = m->values[y];
  Y.ndim = X.ndim;
  for (int i = 0; i < 4; ++i) Y.dims[i] = X.dims[i];
  Y.es = X.es;
  s->out = y;
  s->bytes_per_img = 2.0 * X.es * double(X.per_image());
  return ORE_OK;
}

ore_status build_node(ore_model* m, const Node& n, Step* s) {
  s->op = n.op_type;
  s->name = n.name.empty() ? (n.outputs.empty() ? n.op_type : n.outputs[0]) : n.name;
  if (n.outputs.empty()) return err(m, ORE_ERR_INVALID, "node '" + n.name + "' has no outputs");
  const std::string& op = n.op_type;
  if (op == "Conv") return build_conv(m, n, s);
  if (op == "MaxPool") return build_maxpool(m, n, s);
  if (op == "Relu") return build_unary4(m, n, s, S_RELU);
  if (op == "Dropout") {  // dropout_op.rs:22-28: only `ratio`
    for (auto& at : n.attrs)
      if (at.name != "ratio") return err(m, ORE_ERR_UNSUPPORTED, "ATTRIBUTE NAME FOR DROP OUT NOT FOUND, " + at.name);
    return build_unary4(m, n, s, S_COPY);
  }
  if (op == "GlobalAveragePool") {
    ore_status st = build_unary4(m, n, s, S_GAP);
    if (st) return st;
    Value& Y = m->values[s->out];
    const Value& X = m->values[s->in0];
    Y.dims[2] = 1; Y.dims[3] = 1;
    Y.es = 4;  // f32 sums and output either way
    s->bytes_per_img = double(X.es) * double(X.per_image()) + 4.0 * double(X.dims[1]);
    return ORE_OK;
  }
  if (op == "Softmax") {  // softmax_wrapper flattens to (N, C*H*W), axis 1 (:46-51)
    ore_status st = build_unary4(m, n, s, S_SOFTMAX);
    if (st) return st;
    Value& Y = m->values[s->out];
    const Value& X = m->values[s->in0];
    Y.ndim = 2; Y.dims[0] = 1; Y.dims[1] = X.per_image(); Y.dims[2] = Y.dims[3] = 0;
    if (X.es != 4) return err(m, ORE_ERR_UNSUPPORTED, "Softmax '" + n.name + "': f16 input (f16 models end in f32 after GlobalAveragePool)");
    return ORE_OK;
  }
  if (op == "Concat") {  // concatenate_op.rs:22-32
    int64_t axis = 1;
    for (auto& at : n.attrs) {
      if (at.name != "axis") return err(m, ORE_ERR_UNSUPPORTED, "ATTRIBUTE NAME FOR CONCATENATE NOT FOUND, " + at.name);
      axis = at.i;
    }
    if (n.inputs.size() != 2) return err(m, ORE_ERR_UNSUPPORTED, "Concat '" + n.name + "': exactly 2 inputs supported");
    int a = value_id(m, n.inputs[0]), b = value_id(m, n.inputs[1]);
    if (a < 0 || b < 0 || !is_act(m->values[a], 4) || !is_act(m->values[b], 4))
      return err(m, ORE_ERR_UNSUPPORTED, "Concat '" + n.name + "': inputs must be 4-D activations");
    if (axis < 1 || axis > 3)
      return err(m, ORE_ERR_UNSUPPORTED, "Concat '" + n.name + "': axis must be 1..3 (axis 0 is the batch)");
    const Value A = m->values[a], B = m->values[b];
    for (int i = 1; i < 4; ++i)
      if (i != axis && A.dims[i] != B.dims[i]) return err(m, ORE_ERR_INVALID, "Concat '" + n.name + "': shape mismatch");
    if (A.es != B.es) return err(m, ORE_ERR_UNSUPPORTED, "Concat '" + n.name + "': inputs of different precision");
    if (A.es == 2 && axis != 1)
      return err(m, ORE_ERR_UNSUPPORTED, "Concat '" + n.name + "': f16 (channels-last) activations concatenate along axis 1 only");
    s->kind = S_CONCAT; s->in0 = a; s->in1 = b; s->axis = axis;
    int y = new_value(m, n.outputs[0]);
    Value& Y = m->values[y];
    Y.ndim = 4;
    for (int i = 0; i < 4; ++i) Y.dims[i] = A.dims[i];
    Y.dims[axis] = A.dims[axis] + B.dims[axis];
    Y.es = A.es;
    s->out = y;
    s->bytes_per_img = 2.0 * A.es * double(Y.per_image());
    return ORE_OK;
  }
  if (op == "Add") {  // add_op.rs:16-107
    if (n.inputs.size() < 2) return err(m, ORE_ERR_INVALID, "Add '" + n.name + "' needs 2 inputs");
    int a = value_id(m, n.inputs[0]), b = value_id(m, n.inputs[1]);
    if (a < 0) return err(m, ORE_ERR_INVALID, "Cannot retrieve input 1 for Add operation from hashmap input/output");
    if (b < 0 || !m->values[b].is_const || !m->values[b].cptr)
      return err(m, ORE_ERR_UNSUPPORTED, "Cannot retrieve input 2 for Add operation");
    const Value A = m->values[a], B = m->values[b];
    if (A.is_const) return err(m, ORE_ERR_UNSUPPORTED, "Add '" + n.name + "': constant first input not supported");
    if (A.es != 4) return err(m, ORE_ERR_UNSUPPORTED, "Add '" + n.name + "': f16 input is not supported (f32 op)");
    if (!((A.ndim == 4 && B.ndim == 3) || (A.ndim == 2 && B.ndim == 2)))
      return err(m, ORE_ERR_UNSUPPORTED, "Add '" + n.name + "': supports 4-D + 3-D or 2-D + 2-D");
    for (int i = 0; i < B.ndim; ++i) {  // right-aligned broadcast; the batch axis of A is 1 here
      const int ai = A.ndim - B.ndim + i;
      const int64_t ad = A.dims[ai];
      if (B.dims[i] != 1 && B.dims[i] != ad && !(ai == 0 && B.dims[i] == 1))
        return err(m, ORE_ERR_INVALID, "Add '" + n.name + "': shapes not broadcastable");
      if (ai == 0 && B.dims[i] != 1)
        return err(m, ORE_ERR_UNSUPPORTED, "Add '" + n.name + "': constant may not span the batch axis");
    }
    s->kind = S_ADD; s->in0 = a; s->in1 = b;
    int y = new_value(m, n.outputs[0]);
    Value& Y = m->values[y];
    Y.ndim = A.ndim;
    for (int i = 0; i < 4; ++i) Y.dims[i] = A.dims[i];
    s->out = y;
    s->bytes_per_img = 8.0 * double(A.per_image());
    return ORE_OK;
  }
  if (op == "Reshape") {  // reshape_op.rs:16-92
    if (n.inputs.size() < 2) return err(m, ORE_ERR_INVALID, "Reshape '" + n.name + "' needs 2 inputs");
    int x = value_id(m, n.inputs[0]), sh = value_id(m, n.inputs[1]);
    if (x < 0) return err(m, ORE_ERR_INVALID, "Reshape '" + n.name + "': input not available");
    if (sh < 0 || !m->values[sh].is_const || !m->values[sh].has_i64)
      return err(m, ORE_ERR_UNSUPPORTED, "Unable to retrieve Shape for Reshape operation");
    const Value X = m->values[x];
    const std::vector<int64_t> shape = m->values[sh].i64;
    if (X.ndim != 4) return err(m, ORE_ERR_UNSUPPORTED, "Reshape '" + n.name + "': data must be 4-D");
    if (shape.size() < 2) return err(m, ORE_ERR_UNSUPPORTED, "Reshape '" + n.name + "': shape must have 2 values");
    int64_t ns[2] = {shape[0], shape[1]};
    for (int i = 0; i < 2; ++i)
      if (ns[i] == 0) ns[i] = X.dims[i];
    if (ns[0] < 0 || ns[1] < 0) return err(m, ORE_ERR_UNSUPPORTED, "Reshape '" + n.name + "': negative dims");
    if (X.is_const) {  // fold: a reinterpretation of the uploaded initializer
      if (ns[0] * ns[1] != X.numel_const()) return err(m, ORE_ERR_INVALID, "Reshape: element count mismatch");
      int y = new_value(m, n.outputs[0]);
      Value& Y = m->values[y];
      Y.is_const = true; Y.ndim = 2; Y.dims[0] = ns[0]; Y.dims[1] = ns[1]; Y.cptr = m->values[x].cptr;
      s->kind = S_NOP;
      s->out = y;
      return ORE_OK;
    }
    if (ns[0] != 1 || ns[1] != X.per_image())
      return err(m, ORE_ERR_UNSUPPORTED, "Reshape '" + n.name + "': activation reshape must be [1 or 0, C*H*W] per image");
    if (X.es == 2 && X.dims[2] * X.dims[3] != 1)
      return err(m, ORE_ERR_UNSUPPORTED, "Reshape '" + n.name + "': f16 activations are channels-last; flattening one is not supported");
    s->kind = S_COPY; s->in0 = x;
    int y = new_value(m, n.outputs[0]);
    Value& Y = m->values[y];
    Y.ndim = 2; Y.dims[0] = 1; Y.dims[1] = ns[1];
    Y.es = X.es;
    s->out = y;
    s->bytes_per_img = 8.0 * double(X.per_image());
    return ORE_OK;
  }
  if (op == "MatMul") {  // mul_op.rs:11-32: both operands Array2 from the map
    if (n.inputs.size() < 2) return err(m, ORE_ERR_INVALID, "MatMul '" + n.name + "' needs 2 inputs");
    int a = value_id(m, n.inputs[0]), b = value_id(m, n.inputs[1]);
    if (a < 0 || b < 0) return err(m, ORE_ERR_INVALID, "MatMul '" + n.name + "': input not available");
    const Value A = m->values[a], B = m->values[b];
    if (A.ndim != 2 || B.ndim != 2) return err(m, ORE_ERR_UNSUPPORTED, "MatMul '" + n.name + "': operands must be 2-D");
    if (A.is_const || !B.is_const || !B.cptr)
      return err(m, ORE_ERR_UNSUPPORTED, "MatMul '" + n.name + "': expects activation . constant");
    if (A.dims[1] != B.dims[0]) return err(m, ORE_ERR_INVALID, "MatMul '" + n.name + "': inner dims differ");
    if (A.es != 4) return err(m, ORE_ERR_UNSUPPORTED, "MatMul '" + n.name + "': f16 input is not supported (f32 op)");
    s->kind = S_MATMUL; s->in0 = a; s->in1 = b;
    s->C = A.dims[1]; s->M = B.dims[1]; s->w_kmajor = true;
    s->win.Ho = 1; s->win.Wo = 1; s->H = 1; s->W = 1; s->kh = 1; s->kw = 1;
    s->flops_per_img = 2.0 * double(A.dims[1] * B.dims[1]);
    s->bytes_per_img = 4.0 * double(A.dims[1] + B.dims[1]);
    s->bytes_fixed = 4.0 * double(B.numel_const());
    int y = new_value(m, n.outputs[0]);
    Value& Y = m->values[y];
    Y.ndim = 2; Y.dims[0] = 1; Y.dims[1] = B.dims[1];
    s->out = y;
    return ORE_OK;
  }
  return err(m, ORE_ERR_UNSUPPORTED, "INFERENCE OPERATION '" + op + "' NOT FOUND FOR NODE " + n.name);
}

// steps on NHWC f16 values (f16 models): Relu, GAP (f32 out), Concat (channels), Dropout copies
ore_status launch_step_f16(ore_model* m, const Step& s, int64_t n) {
  ore_ctx* ctx = m->ctx;
  const Value& X = m->values[s.in0];
  const Ref x = ref_of(m, s.in0), y = ref_of(m, s.out);
  const int64_t count = n * X.per_image();
  if (count == 0) return ORE_OK;
  if (s.kind == S_GAP) {
    launch_gap_nhwc(x.p, reinterpret_cast<float*>(y.p), int(n), int(X.dims[1]), int(X.dims[2] * X.dims[3]), int(x.ps),
                    x.nstride, ctx->stream);
    ORE_HIP_CHECK(ctx, hipGetLastError());
    return ORE_OK;
  }
  if (x.nstride != X.per_image() || y.nstride != m->values[s.out].per_image())
    return err(m, ORE_ERR_INVALID, "internal: f16 step on a strided view");
  switch (s.kind) {
    case S_RELU: launch_relu_f16(x.p, y.p, count, ctx->stream); break;
    case S_COPY:
      if (x.p != y.p)
        ORE_HIP_CHECK(ctx, hipMemcpyAsync(y.p, x.p, size_t(count) * 2, hipMemcpyDeviceToDevice, ctx->stream));
      break;
    case S_CONCAT: {  // axis 1 (build_node): per pixel, a's channels then b's
      const Value& B = m->values[s.in1];
      const Ref b = ref_of(m, s.in1);
      if (b.nstride != B.per_image() || s.axis != 1)
        return err(m, ORE_ERR_INVALID, "internal: f16 concat of a strided view");
      launch_concat_nhwc(x.p, b.p, y.p, n * X.dims[2] * X.dims[3], int(X.dims[1]), int(B.dims[1]), ctx->stream);
      break;
    }
    default: return err(m, ORE_ERR_UNSUPPORTED, "internal: step '" + s.name + "' has no f16 kernel");
  }
  ORE_HIP_CHECK(ctx, hipGetLastError());
  return ORE_OK;
}

// For its lifetime the context knows the arena and its lead as mapped memory: the f32 conv and fire launches
// run under one (the streaming conv may read a few bytes before an input inside the arena).
struct MappedArena {
  ore_ctx* ctx;
  explicit MappedArena(const ore_model* m) : ctx(m->ctx) { set(m->arena_alloc, m->arena ? m->arena + m->arena_bytes : nullptr); }
  ~MappedArena() { set(nullptr, nullptr); }
  void set(const char* lo, const char* hi) {
    ctx->mapped_lo = lo;
    ctx->mapped_hi = hi;
  }
};

ConvGeom conv_geom(const Step& s) { return {s.C, s.H, s.W, s.M, s.kh, s.kw, s.sh, s.sw, s.win, s.relu}; }

// an S_CONV step on the kernel its plan and fusions name
ConvRun launch_conv_step(ore_model* m, const Step& s, int64_t n) {
  ore_ctx* ctx = m->ctx;
  const Ref x = ref_of(m, s.in0), y = ref_of(m, s.out);
  const ConvGeom g = conv_geom(s);
  ConvOperands w{s.wp, s.ktab, s.in2 >= 0 ? m->values[s.in2].cptr : nullptr, s.wc1};
  const PoolGeom ep{s.ep.kh, s.ep.kw, s.ep.sh, s.ep.sw, s.ep.win};
  // with the next 1x1 conv fused in (s.sq), out is that conv's output and the pooled conv's own is never stored
  const Ref yc = s.sq.on ? Ref{nullptr, y.nstride, 0, y.es} : y;
  // the one-launch f16 first conv + pool from the f32 input (plan.epv 1: the two-launch patch path)
  if (s.plan.f16 && s.plan.xmode == F16_X_NHWC_PAIR && s.ep.on && (s.sq.on || s.plan.epv != 1)) {
    const C1Squeeze sq{s.sq.w, s.sq.b, int(s.sq.M), y.p, y.nstride, int(pixel_stride(y, s.sq.M))};
    if (s.sq.on) w.sq16 = &sq;
    const ConvRun r = run_conv_pair_pool_f16(ctx, s.plan, x, yc, n, g, w, ep);
    if (r.st != ORE_OK || r.tile >= 0) return r;  // ran: C1_POOL_F16_TILE or C1_BAND_F16_TILE
    if (s.sq.on) return err(m, ORE_ERR_INVALID, "internal: the fused first conv + squeeze declined its launch");
  }
  if (s.plan.f16 && s.plan.xmode == F16_X_NHWC_PAIR) {
    // convert the f32 NCHW input to NHWC f16 (4 channels per pixel), then gather
    const int cs = 4;
    launch_nchw_to_nhwc(x.p, m->xcvt, int(n), int(s.C), int(s.H * s.W), x.nstride, int(plane_stride(x, s.H * s.W)), cs,
                        ctx->stream);
    ORE_HIP_CHECK(ctx, hipGetLastError());
    const Ref xc{static_cast<float*>(m->xcvt), s.H * s.W * cs, cs, 2};
    ConvRun r = run_conv_f16(ctx, s.plan, xc, y, n, g, w, s.ep.on ? &ep : nullptr);
    if (s.ep.on) r.tile = EPOOL_TILE_BASE + 1;  // "epool patch": conv_f16's pooled epilogue
    return r;
  }
  if (s.plan.f16 && s.gap) {
    const Conv1x1GapF16 q{x.p, s.wp, w.bias, y.p, int(n), int(s.C), int(s.H * s.W), int(s.M), s.plan.Mp,
                          int((s.C + 31) / 32 * 32), int(pixel_stride(x, s.C)), s.relu ? 1 : 0, x.nstride, y.nstride};
    if (!conv1x1_gap_f16_eligible(q)) return err(m, ORE_ERR_INVALID, "internal: conv + GAP on an unsupported layout");
    launch_conv1x1_gap_f16(q, ctx->stream);
    ORE_HIP_CHECK(ctx, hipGetLastError());
    return {ORE_OK, CONV_GAP_F16_TILE};
  }
  if (s.gap) {  // f32: conv1x1_gap_f32_kernel
    const Conv1x1GapF32 q{x.p, s.wc1, w.bias, y.p, int(n), int(s.C), int(s.H * s.W), int(s.M),
                          int(plane_stride(x, s.H * s.W)), s.relu ? 1 : 0, x.nstride, y.nstride};
    if (!conv1x1_gap_f32_eligible(q)) return err(m, ORE_ERR_INVALID, "internal: conv + GAP on an unsupported layout");
    if (n > 0) launch_conv1x1_gap_f32(q, ctx->stream);
    ORE_HIP_CHECK(ctx, hipGetLastError());
    return {ORE_OK, CONV_GAP_F32_TILE};
  }
  if (s.plan.f16) return run_conv_f16(ctx, s.plan, x, y, n, g, w, s.ep.on ? &ep : nullptr);
  if (s.ep.on) {
    const MappedArena mapped(m);
    const C1SqueezeF32 sq1{static_cast<const float*>(s.sq.w), s.sq.b, int(s.sq.M), y.p, y.nstride,
                           int(plane_stride(y, s.ep.win.Ho * s.ep.win.Wo))};
    if (s.sq.on) w.sq1 = &sq1;
    return run_conv_epool(ctx, s.plan, x, yc, n, g, w, ep);
  }
  if (s.pin.on) {
    const Step::PoolIn& pin = s.pin;
    PoolExpand pe{};
    if (pin.e1.on) {
      const Ref sv = ref_of(m, s.in3);
      pe = {sv.p, pin.e1.w, pin.e1.b, int(pin.e1.C), int(pin.e1.E), pin.e1.Mp, plane_stride(sv, pin.H * pin.W), sv.nstride};
      w.pe = &pe;
    }
    const ConvGeom gp{s.C, pin.H, pin.W, s.M, 1, 1, 1, 1, s.win, s.relu};  // the 1x1 conv over x, the pool's input
    return run_conv_pool(ctx, s.plan, x, y, n, gp, w, PoolGeom{3, 3, pin.sh, pin.sw, pin.win});
  }
  const MappedArena mapped(m);
  return run_conv(ctx, s.plan, x, y, n, g, w);
}

// records the tile a conv or MatMul step ran
ore_status ran(Step& s, const ConvRun& r) {
  s.ran_tile = r.tile;
  return r.st;
}

ore_status launch_step(ore_model* m, Step& s, int64_t n) {
  ore_ctx* ctx = m->ctx;
  const Ref y = ref_of(m, s.out);
  switch (s.kind) {
    case S_CONV: return ran(s, launch_conv_step(m, s, n));
    case S_FIRE: {
      const Ref x = ref_of(m, s.in0);
      const Step::Fire& f = s.fire;
      const FireOperands fo{f.C, f.E1, f.E3, s.M, s.plan.Mp, f.w1, f.w3, f.f16 ? f.ws16 : s.wp,
                            f.b1, f.b3, s.in2 >= 0 ? m->values[s.in2].cptr : nullptr};
      const Window* pool = f.pool ? &f.pwin : nullptr;
      if (f.f16) return run_fire_f16(ctx, x, y, n, f.H, f.W, fo, pool);
      const MappedArena mapped(m);
      return run_fire(ctx, x, y, n, f.H, f.W, fo, pool);
    }
    case S_MATMUL: {  // a 1x1 conv over rows: 2-D operands, whatever planes the storage they alias has
      const Ref x = ref_of(m, s.in0);
      return ran(s, run_conv(ctx, s.plan, Ref{x.p, x.nstride, 0, x.es}, Ref{y.p, y.nstride, 0, y.es}, n, conv_geom(s),
                             ConvOperands{s.wp, s.ktab, nullptr}));
    }
    case S_MAXPOOL: {
      const Ref x = ref_of(m, s.in0);
      return run_maxpool(ctx, x, y, n, s.C, s.H, s.W, PoolGeom{s.kh, s.kw, s.sh, s.sw, s.win});
    }
    default: break;
  }
  if (s.kind == S_GAP && m->values[s.in0].es == 4) {  // f32 NCHW rows, possibly padded planes
    const Value& X = m->values[s.in0];
    const Ref x = ref_of(m, s.in0);
    const int64_t HW = X.dims[2] * X.dims[3], ps = x.ps ? x.ps : HW;
    if (x.nstride != X.dims[1] * ps || y.nstride != X.dims[1])
      return err(m, ORE_ERR_INVALID, "internal: GlobalAveragePool on a strided view");
    launch_gap(x.p, 4, y.p, n * X.dims[1], int(HW), int(ps), ctx->stream);
    ORE_HIP_CHECK(ctx, hipGetLastError());
    return ORE_OK;
  }
  if (m->values[s.in0].es == 2) return launch_step_f16(m, s, n);
  // contiguous ops through the public entry points
  auto as_tensor = [&](int id, int64_t batch) {
    const Value& v = m->values[id];
    const Ref r = ref_of(m, id);
    ore_tensor t{};
    t.data = r.p;
    t.ndim = v.ndim;
    for (int i = 0; i < v.ndim; ++i) t.dims[i] = v.dims[i];
    if (!v.is_const) t.dims[0] = batch;
    t.nstride = v.is_const ? 0 : r.nstride;
    return t;
  };
  ore_tensor X = as_tensor(s.in0, n), Y = as_tensor(s.out, n);
  switch (s.kind) {
    case S_RELU: return ore_relu_f32(ctx, &X, &Y);
    case S_SOFTMAX: return ore_softmax_f32(ctx, &X, &Y);
    case S_GAP: return ore_gap_f32(ctx, &X, &Y);
    case S_COPY: return ore_dropout_f32(ctx, &X, &Y);
    case S_ADD: {
      ore_tensor B = as_tensor(s.in1, n);
      return ore_add_f32(ctx, &X, &B, &Y);
    }
    case S_CONCAT: {
      ore_tensor B = as_tensor(s.in1, n);
      return ore_concat_f32(ctx, &X, &B, s.axis, &Y);
    }
    default: return err(m, ORE_ERR_INVALID, "internal: unexpected step kind");
  }
}

// the tile ids a step may run (its kernel family): autotune candidates and ore_model_set_step_tile's
// accepted values; empty for steps with one fixed kernel
std::vector<int> step_tile_family(const Step& s) {
  std::vector<int> c;
  if (s.kind != S_CONV && s.kind != S_MATMUL) return c;
  if (s.kind == S_CONV && s.ep.on && !s.plan.f16) {  // f32 pooled conv: patch / row-walk variants, the window kernel
    if (s.sq.on) {  // the fused squeeze: window kernel, band walker (where its geometry allows it)
      if (band_step(s)) return {EPOOL_WIN_TILE, EPOOL_BAND_TILE};
      return {EPOOL_WIN_TILE};
    }
    for (int v = 1; v <= 5; ++v) c.push_back(EPOOL_TILE_BASE + v);
    if (s.wc1) c.push_back(EPOOL_WIN_TILE);
    return c;
  }
  if (s.kind == S_CONV && s.ep.on && s.plan.f16 && s.plan.xmode == F16_X_NHWC_PAIR) {  // f16 first conv + pool
    if (s.sq.on) {  // the fused squeeze: the patch kernel, the band walker (where its geometry allows it)
      if (band_f16_step(s)) return {C1_POOL_F16_TILE, C1_BAND_F16_TILE};
      return {C1_POOL_F16_TILE};
    }
    return {EPOOL_TILE_BASE + 1, C1_POOL_F16_TILE};  // two launches (conversion + patch kernel) / one launch
  }
  if (s.ep.on || s.pin.on || s.gap) return c;  // other f16 pooled epilogues / the pooled 1x1 / conv + GAP: one kernel
  if (s.plan.wino) {
    for (int t = 0; t < WINO_TILES_N; ++t) c.push_back(WINO_TILE_BASE + t);
    return c;
  }
  for (int t = 0; t < 4; ++t) c.push_back(t);  // the LDS-staged conv_gemm tiles
  // the LDS-free streaming kernel (f32 convs; launch_conv falls back to tile 0 where the geometry does
  // not allow it)
  if (!s.plan.f16 && s.kind == S_CONV)
    for (int t = CONV_TILE_STREAM; t < CONV_TILES_F32; ++t) c.push_back(t);
  if (!s.plan.f16 && s.kind == S_CONV && s.kh == 1 && s.kw == 1)  // the persistent 1x1 tiles
    for (int t = CONV_TILE_SP; t < CONV_TILE_SP + CONV_TILES_SP; ++t) c.push_back(t);
  return c;
}

// writes tile t into the step's plan (and the base step the next plan() copies from)
void set_tile(ore_model* m, int k, int t) {
  Step& s = m->steps[m->exec_steps[k]];
  Step& b = m->base_steps[m->exec_steps[k]];
  if (s.kind == S_CONV && s.ep.on) {
    const int v = t == EPOOL_WIN_TILE    ? EPOOL_WIN_VARIANT
                  : t == EPOOL_BAND_TILE ? EPOOL_BAND_VARIANT
                  : t == C1_POOL_F16_TILE ? (s.sq.on ? C1_PATCH_F16_VARIANT : 0)
                  : t == C1_BAND_F16_TILE ? C1_BAND_F16_VARIANT
                                          : t - EPOOL_TILE_BASE;
    s.plan.epv = b.plan.epv = v;
    return;
  }
  s.plan.cfg = t;
  if (s.plan.wino) b.plan_wino.cfg = t;
  else b.plan.cfg = t;
}

// The map conv of ore_model_set_cam (include/ore.h), over the unfused node steps: back from the graph output
// through an optional Softmax and any Dropout / Reshape to a GlobalAveragePool, whose input T comes through an
// optional Relu from a 1x1 / stride-1 / unpadded Conv of M = the output's elems.  Sets cam_conv, cam_in, cam_map and
// cam_relu, or leaves cam_conv < 0 and says in cam_why what it met instead.
void find_map_conv(ore_model* m) {
  std::vector<int> producer(m->values.size(), -1);
  for (size_t i = 0; i < m->base_steps.size(); ++i)
    if (m->base_steps[i].out >= 0) producer[m->base_steps[i].out] = int(i);
  auto found = [&](int v, const char* want) {
    const int p = v >= 0 ? producer[v] : -1;
    m->cam_why = std::string("no map conv: expected ") + want + ", found " +
                 (p < 0 ? "the value '" + m->values[v].name + "' that no node produces"
                        : m->base_steps[p].op + " '" + m->base_steps[p].name + "'");
  };
  int v = m->output_value, p = producer[v];
  bool softmax = false;
  while (p >= 0 && (m->base_steps[p].kind == S_COPY || (m->base_steps[p].kind == S_SOFTMAX && !softmax))) {
    softmax = softmax || m->base_steps[p].kind == S_SOFTMAX;
    v = m->base_steps[p].in0;
    p = producer[v];
  }
  if (p < 0 || m->base_steps[p].kind != S_GAP) return found(v, "GlobalAveragePool");
  const int T = m->base_steps[p].in0;
  v = T;
  p = producer[v];
  bool relu = false;
  if (p >= 0 && m->base_steps[p].kind == S_RELU) {
    relu = true;
    v = m->base_steps[p].in0;
    p = producer[v];
  }
  if (p < 0 || m->base_steps[p].kind != S_CONV) return found(v, "a 1x1 Conv feeding the GlobalAveragePool");
  const Step& s = m->base_steps[p];
  const int64_t out_elems = m->values[m->output_value].per_image();
  if (s.kh != 1 || s.kw != 1 || s.sh != 1 || s.sw != 1 || s.win.pt || s.win.pl || s.win.pb || s.win.pr || s.M != out_elems) {
    m->cam_why = "no map conv: Conv '" + s.name + "' feeding the GlobalAveragePool has a " + std::to_string(s.kh) + "x" +
                 std::to_string(s.kw) + " kernel, stride " + std::to_string(s.sh) + "x" + std::to_string(s.sw) + ", pads " +
                 std::to_string(s.win.pt + s.win.pl + s.win.pb + s.win.pr) + " and " + std::to_string(s.M) +
                 " channels (expected 1x1, stride 1, zero pads, " + std::to_string(out_elems) + " channels)";
    return;
  }
  if (m->values[s.in0].es != (m->f16 ? 2 : 4) || m->values[s.in0].ndim != 4) {
    m->cam_why = "no map conv: the input of Conv '" + s.name + "' is not stored in the model's precision";
    return;
  }
  m->cam_conv = p;
  m->cam_in = s.in0;
  m->cam_map = T;
  m->cam_relu = relu;
}

}  // namespace

// the band walkers' geometry for a fused first conv + pool + squeeze step (their layout checks are the
// launch's: a layout the f32 one declines runs the window kernel)
bool ore::band_f16_step(const Step& s) {
  return s.plan.f16 && conv_band_pool_f16_geometry(int(s.C), int(s.M), int(s.kh), int(s.kw), int(s.sh), int(s.sw),
                                                   int(s.win.pt), int(s.win.pl), int(s.W), int(s.win.Wo),
                                                   int(s.ep.win.Ho), int(s.ep.win.Wo), int(s.ep.win.pt), int(s.ep.win.pl),
                                                   int(s.sq.M)) &&
         s.relu;
}

bool ore::band_step(const Step& s) {
  return conv_band_pool_f32_geometry(int(s.C), int(s.M), int(s.kh), int(s.kw), int(s.sh), int(s.sw), int(s.win.pt),
                                     int(s.win.pl), int(s.W), int(s.win.Wo), int(s.ep.win.Ho), int(s.ep.win.Wo),
                                     int(s.ep.win.pt), int(s.ep.win.pl), int(s.sq.M), s.relu);
}

extern "C" {

ore_status ore_model_load(ore_ctx* ctx, const void* bytes, size_t len, int64_t max_batch, ore_model** out) {
  return ore_model_load_ex(ctx, bytes, len, max_batch, 0, out);
}

ore_status ore_model_parse(const void* bytes, size_t len) {
  if (!bytes) return set_error(nullptr, ORE_ERR_INVALID, "null argument");
  Graph g;
  std::string perr;
  if (!parse_model(static_cast<const uint8_t*>(bytes), len, &g, &perr)) return set_error(nullptr, ORE_ERR_PARSE, "%s", perr.c_str());
  return ORE_OK;
}

ore_status ore_model_load_ex(ore_ctx* ctx, const void* bytes, size_t len, int64_t max_batch, int32_t flags,
                             ore_model** out) {
  if (!ctx || !bytes || !out || max_batch <= 0) return set_error(ctx, ORE_ERR_INVALID, "invalid argument");
  if (flags & ORE_LOAD_RETIRED_MASK)
    return set_error(ctx, ORE_ERR_UNSUPPORTED, "load flags 0x%x were retired in ABI 2 (the bf16x3 kernels, ORE_LOAD_X3)",
                     unsigned(flags & ORE_LOAD_RETIRED_MASK));
  if (flags & ~(ORE_LOAD_F16 | ORE_LOAD_NO_WINOGRAD))
    return set_error(ctx, ORE_ERR_INVALID, "unknown load flags 0x%x", unsigned(flags));
  ORE_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  Graph g;
  std::string perr;
  if (!parse_model(static_cast<const uint8_t*>(bytes), len, &g, &perr)) return set_error(ctx, ORE_ERR_PARSE, "%s", perr.c_str());
  ore_model* m = new ore_model();
  m->ctx = ctx;
  m->max_batch = max_batch;
  m->f16 = (flags & ORE_LOAD_F16) != 0;
  m->wino = !m->f16 && (flags & ORE_LOAD_NO_WINOGRAD) == 0;
  m->conv_tile = ctx->conv_tile;
  auto fail = [&](ore_status st) {
    ore_model_destroy(m);
    return st;
  };
  // initializers: shapes from graph.input when listed there (get_input_data_shape, utils.rs:53-97),
  // else TensorProto.dims; f32 data uploaded once into one allocation.
  std::map<std::string, const ValueInfo*> gin;
  for (auto& vi : g.inputs) gin[vi.name] = &vi;
  size_t total = 0;
  for (auto& t : g.inits) total += (t.f32.size() * 4 + 255) / 256 * 256;
  std::vector<char> host(total ? total : 1, 0);
  if (total && device_alloc(ctx, reinterpret_cast<void**>(&m->consts), total, true) != hipSuccess)
    return fail(set_error(ctx, ORE_ERR_OOM, "initializer upload allocation failed"));
  // the upload below is not on the context's stream: a fill (ore_ctx_set_alloc_fill) has to land first
  if (total && ctx->alloc_fill && hipStreamSynchronize(ctx->stream) != hipSuccess)
    return fail(set_error(ctx, ORE_ERR_HIP, "initializer buffer fill failed"));
  size_t off = 0;
  for (auto& t : g.inits) {
    int id = new_value(m, t.name);
    Value& v = m->values[id];
    v.is_const = true;
    std::vector<int64_t> shape = t.dims;
    auto it = gin.find(t.name);
    if (it != gin.end() && !it->second->shape.empty()) shape = it->second->shape;
    if (shape.size() > 4) return fail(set_error(ctx, ORE_ERR_UNSUPPORTED, "initializer '%s' rank > 4", t.name.c_str()));
    v.ndim = int(shape.size());
    for (size_t i = 0; i < shape.size(); ++i) v.dims[i] = shape[i];
    if (!t.f32.empty()) {
      if (int64_t(t.f32.size()) != v.numel_const())
        return fail(set_error(ctx, ORE_ERR_INVALID, "initializer '%s' has %zu values for its shape", t.name.c_str(), t.f32.size()));
      std::memcpy(host.data() + off, t.f32.data(), t.f32.size() * 4);
      v.cptr = reinterpret_cast<float*>(reinterpret_cast<char*>(m->consts) + off);
      off += (t.f32.size() * 4 + 255) / 256 * 256;
    }
    if (!t.i64.empty()) { v.i64 = t.i64; v.has_i64 = true; }
  }
  if (total) {
    if (hipMemcpy(m->consts, host.data(), total, hipMemcpyHostToDevice) != hipSuccess)
      return fail(set_error(ctx, ORE_ERR_HIP, "initializer upload failed"));
  }
  // seeded input (manage_input_data, utils.rs:29-45): graph inputs that are not initializers
  for (auto& vi : g.inputs) {
    if (value_id(m, vi.name) >= 0) continue;
    if (m->input_value >= 0) return fail(set_error(ctx, ORE_ERR_UNSUPPORTED, "more than one seeded model input"));
    if (vi.shape.size() != 4) return fail(set_error(ctx, ORE_ERR_UNSUPPORTED, "model input '%s' must be 4-D", vi.name.c_str()));
    int id = new_value(m, vi.name);
    Value& v = m->values[id];
    v.is_input = true;
    v.ndim = 4;
    v.dims[0] = 1;
    for (int i = 1; i < 4; ++i) {
      if (vi.shape[i] <= 0) return fail(set_error(ctx, ORE_ERR_UNSUPPORTED, "symbolic input dims are not supported"));
      v.dims[i] = vi.shape[i];
    }
    m->input_value = id;
  }
  if (m->input_value < 0) return fail(set_error(ctx, ORE_ERR_UNSUPPORTED, "model has no seeded input"));
  for (auto& n : g.nodes) {
    Step s;
    ore_status st = build_node(m, n, &s);
    if (st) { std::string e = ctx->err; ore_model_destroy(m); return set_error(ctx, st, "%s", e.c_str()); }
    m->base_steps.push_back(s);
  }
  // pack every conv / matmul weight once (K-major, zero padded) for the MFMA A tiles
  {
    size_t total_packed = 0;
    for (auto& s : m->base_steps) {
      if (s.kind == S_CONV) {
        // f16 operand mode by the input's layout: an f32 NCHW value (the model input: converted to
        // NHWC4 when C <= 4, else gathered per element), or NHWC f16 (16-B channel groups when C % 8 == 0)
        // (SqueezeNet conv1 at B = 256: NHWC4 pairs 355 us, per-element NCHW 459 us,
        // profiles/r01p_f16_first_conv.txt)
        const int xmode = m->values[s.in0].es == 4 ? (s.C <= 4 ? F16_X_NHWC_PAIR : F16_X_NCHW32)
                          : s.C % 8 == 0           ? F16_X_NHWC_VEC
                                                   : F16_X_NHWC_ELEM;
        s.plan = conv_plan(s.M, s.C, s.H, s.W, s.kh, s.kw, s.sh, s.sw, s.win, m->f16, xmode, false, m->conv_tile);
      }
      else if (s.kind == S_MATMUL)
        s.plan = conv_plan(s.M, s.C, 1, 1, 1, 1, 1, 1, s.win, false, 0, false, m->conv_tile);
      else
        continue;
      total_packed += (packed_bytes(s.plan) + 255) / 256 * 256;
      if (m->wino && s.kind == S_CONV) {
        s.plan_wino = conv_plan(s.M, s.C, s.H, s.W, s.kh, s.kw, s.sh, s.sw, s.win, false, 0, true, m->conv_tile);
        s.has_wino = s.plan_wino.wino != 0;
        if (s.has_wino) total_packed += (conv_packed_bytes(s.plan_wino) + 255) / 256 * 256;
      }
    }
    if (total_packed) {
      if (device_alloc(ctx, reinterpret_cast<void**>(&m->packed), total_packed, true) != hipSuccess)
        return fail(set_error(ctx, ORE_ERR_OOM, "packed weight allocation failed"));
      size_t poff = 0;
      for (auto& s : m->base_steps) {
        if (s.kind != S_CONV && s.kind != S_MATMUL) continue;
        char* base = reinterpret_cast<char*>(m->packed) + poff;
        s.wp = reinterpret_cast<float*>(base);
        launch_pack(m->values[s.in1].cptr, s.w_kmajor, int(s.M), int(s.C), int(s.kh), int(s.kw), s.plan, s.wp,
                    ctx->stream);
        s.ktab = reinterpret_cast<int2*>(base + conv_packed_bytes(s.plan));
        poff += (packed_bytes(s.plan) + 255) / 256 * 256;
        if (s.has_wino) {
          s.wp_wino = reinterpret_cast<float*>(reinterpret_cast<char*>(m->packed) + poff);
          launch_pack(m->values[s.in1].cptr, false, int(s.M), int(s.C), int(s.kh), int(s.kw), s.plan_wino, s.wp_wino,
                      ctx->stream);
          poff += (conv_packed_bytes(s.plan_wino) + 255) / 256 * 256;
        }
      }
      if (hipGetLastError() != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess)
        return fail(set_error(ctx, ORE_ERR_HIP, "weight packing failed"));
    }
  }
  if (g.outputs.empty()) return fail(set_error(ctx, ORE_ERR_INVALID, "model has no outputs"));
  m->output_value = value_id(m, g.outputs[0].name);
  if (m->output_value < 0 || m->values[m->output_value].is_const)
    return fail(set_error(ctx, ORE_ERR_INVALID, "graph output '%s' is not produced", g.outputs[0].name.c_str()));
  m->values[m->output_value].is_output = true;
  if (m->values[m->output_value].es != 4)
    return fail(set_error(ctx, ORE_ERR_UNSUPPORTED, "f16 model: graph output '%s' must be f32 (end with GlobalAveragePool / Softmax)",
                          g.outputs[0].name.c_str()));
  find_map_conv(m);
  if (ore_status st = plan(m)) { std::string e = ctx->err; ore_model_destroy(m); return set_error(ctx, st, "%s", e.c_str()); }
  *out = m;
  return ORE_OK;
}

ore_status ore_model_destroy(ore_model* m) {
  if (!m) return ORE_OK;
  (void)hipSetDevice(m->ctx->device);
  (void)hipStreamSynchronize(m->ctx->stream);
  for (auto e : m->events) (void)hipEventDestroy(e);
  if (m->graph_exec) (void)hipGraphExecDestroy(m->graph_exec);
  if (m->graph) (void)hipGraphDestroy(m->graph);
  if (m->side) (void)hipStreamDestroy(m->side);
  if (m->ev_fork) (void)hipEventDestroy(m->ev_fork);
  if (m->ev_join) (void)hipEventDestroy(m->ev_join);
  if (m->arena_alloc) (void)hipFree(m->arena_alloc);
  if (m->consts) (void)hipFree(m->consts);
  if (m->packed) (void)hipFree(m->packed);
  for (auto& kv : m->packs) (void)hipFree(kv.second);
  if (m->xcvt) (void)hipFree(m->xcvt);
  if (m->stage) (void)hipFree(m->stage);
  if (m->rows) (void)hipFree(m->rows);
  delete m;
  return ORE_OK;
}

ore_status ore_model_set_fusion(ore_model* m, int32_t flags) {
  if (!m) return set_error(nullptr, ORE_ERR_INVALID, "null model");
  const int32_t known = ORE_FUSE_ALL | ORE_FUSE_EAGER | ORE_KEEP_VALUES;
  if (flags & 16) return set_error(m->ctx, ORE_ERR_UNSUPPORTED, "fusion bit 16 (ORE_FUSE_POOL_CONV) was retired (ABI 2)");
  if (flags & ~known) return set_error(m->ctx, ORE_ERR_INVALID, "unknown fusion flags 0x%x", unsigned(flags & ~known));
  m->fusion = flags;
  return plan(m);
}

// the model's activation memory, in the order ore_model_scratch_info enumerates it
namespace {
struct ScratchBuf { const char* name; void* p; size_t bytes; };
int scratch_bufs(ore_model* m, ScratchBuf out[4]) {
  int n = 0;
  if (m->arena_alloc) out[n++] = {"arena", m->arena_alloc, m->arena_bytes + ARENA_LEAD};
  if (m->xcvt) out[n++] = {"xcvt", m->xcvt, m->xcvt_bytes};
  if (m->stage) out[n++] = {"stage", m->stage, m->stage_bytes};
  if (m->rows) out[n++] = {"rows", m->rows, m->rows_bytes};
  return n;
}
}  // namespace

ore_status ore_model_fill_scratch(ore_model* m, uint32_t pattern) {
  if (!m) return set_error(nullptr, ORE_ERR_INVALID, "null model");
  ore_ctx* ctx = m->ctx;
  ORE_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  if (ctx->stream && hipStreamIsCapturing(ctx->stream, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone)
    return set_error(ctx, ORE_ERR_INVALID, "ore_model_fill_scratch inside a stream capture");
  ScratchBuf b[4];
  const int n = scratch_bufs(m, b);
  for (int i = 0; i < n; ++i) ORE_HIP_CHECK(ctx, device_fill(ctx, b[i].p, b[i].bytes, pattern));
  return ORE_OK;
}

ore_status ore_model_scratch_info(ore_model* m, int32_t i, const char** name, void** dptr, size_t* bytes) {
  if (!m) return set_error(nullptr, ORE_ERR_INVALID, "null model");
  ScratchBuf b[4];
  const int n = scratch_bufs(m, b);
  if (i < 0 || i >= n) return set_error(m->ctx, ORE_ERR_INVALID, "scratch buffer %d of %d", int(i), n);
  if (name) *name = b[i].name;
  if (dptr) *dptr = b[i].p;
  if (bytes) *bytes = b[i].bytes;
  return ORE_OK;
}

ore_status ore_model_input_dims(ore_model* m, int64_t dims[4]) {
  if (!m || !dims) return set_error(nullptr, ORE_ERR_INVALID, "null argument");
  for (int i = 0; i < 4; ++i) dims[i] = m->values[m->input_value].dims[i];
  return ORE_OK;
}

ore_status ore_model_output_elems(ore_model* m, int64_t* elems) {
  if (!m || !elems) return set_error(nullptr, ORE_ERR_INVALID, "null argument");
  *elems = m->values[m->output_value].per_image();
  return ORE_OK;
}

// one pass of the graph over n <= run_batch images; ev: this pass's timing events (exec_steps + 1).  With
// copy_out false an output value that lives in the arena stays there (the caller reads it through ref_of).
static ore_status run_pass(ore_model* m, const float* d_input, int64_t n, float* d_output, hipEvent_t* ev,
                           bool copy_out = true) {
  ore_ctx* ctx = m->ctx;
  m->cur_in = d_input;
  m->cur_out = d_output;
  const Value& ov = m->values[m->output_value];
  const bool branches = m->streams > 1 && !m->timing;
  for (size_t k = 0; k < m->exec_steps.size(); ++k) {
    if (m->timing) ORE_HIP_CHECK(ctx, hipEventRecord(ev[k], ctx->stream));
    if (branches && m->pair_next[k]) {
      // fork: step k on the side stream, step k + 1 on the main stream, then join
      ORE_HIP_CHECK(ctx, hipEventRecord(m->ev_fork, ctx->stream));
      ORE_HIP_CHECK(ctx, hipStreamWaitEvent(m->side, m->ev_fork, 0));
      hipStream_t main = ctx->stream;
      ctx->stream = m->side;
      ore_status st = launch_step(m, m->steps[m->exec_steps[k]], n);
      ctx->stream = main;
      if (st) return st;
      ORE_HIP_CHECK(ctx, hipEventRecord(m->ev_join, m->side));
      st = launch_step(m, m->steps[m->exec_steps[k + 1]], n);
      if (st) return st;
      ORE_HIP_CHECK(ctx, hipStreamWaitEvent(ctx->stream, m->ev_join, 0));
      ++k;
      continue;
    }
    ore_status st = launch_step(m, m->steps[m->exec_steps[k]], n);
    if (st) return st;
  }
  if (m->timing) ORE_HIP_CHECK(ctx, hipEventRecord(ev[m->exec_steps.size()], ctx->stream));
  if (!m->out_bound && copy_out) {
    const Ref r = ref_of(m, m->output_value);
    const int64_t pe = ov.per_image();
    if (r.nstride == pe) {
      ORE_HIP_CHECK(ctx, hipMemcpyAsync(d_output, r.p, size_t(n * pe) * 4, hipMemcpyDeviceToDevice, ctx->stream));
    } else {
      ORE_HIP_CHECK(ctx, hipMemcpy2DAsync(d_output, size_t(pe) * 4, r.p, size_t(r.nstride) * 4, size_t(pe) * 4, size_t(n),
                                          hipMemcpyDeviceToDevice, ctx->stream));
    }
  }
  return ORE_OK;
}

// the staging buffer of the _u8 entries, sized for run_batch images (plan() may have changed it); never
// allocated inside a stream capture
static ore_status ensure_stage(ore_model* m) {
  ore_ctx* ctx = m->ctx;
  const size_t need = size_t(m->values[m->input_value].per_image()) * size_t(m->run_batch) * 4;
  if (m->stage && m->stage_bytes >= need) return ORE_OK;
  ORE_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  if (ctx->stream && hipStreamIsCapturing(ctx->stream, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone)
    return set_error(ctx, ORE_ERR_INVALID, "the uint8 staging buffer cannot be allocated inside a stream capture: call "
                                           "ore_model_set_input_norm first");
  ORE_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));  // an earlier run may still read the old buffer
  if (m->stage) (void)hipFree(m->stage);
  m->stage = nullptr;
  m->stage_bytes = 0;
  if (device_alloc(ctx, reinterpret_cast<void**>(&m->stage), need, true) != hipSuccess) {
    (void)hipGetLastError();
    return set_error(ctx, ORE_ERR_OOM, "uint8 input staging buffer (%zu bytes) allocation failed", need);
  }
  m->stage_bytes = need;
  return ORE_OK;
}

// the rows buffer of the classify entries, sized for run_batch images' outputs (plan() may have changed it);
// never allocated inside a stream capture
static ore_status ensure_rows(ore_model* m) {
  ore_ctx* ctx = m->ctx;
  const size_t need = size_t(m->values[m->output_value].per_image()) * size_t(m->run_batch) * 4;
  if (m->rows && m->rows_bytes >= need) return ORE_OK;
  ORE_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  if (ctx->stream && hipStreamIsCapturing(ctx->stream, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone)
    return set_error(ctx, ORE_ERR_INVALID, "the top-k rows buffer cannot be allocated inside a stream capture: call "
                                           "ore_model_set_topk first");
  ORE_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));  // an earlier run may still read the old buffer
  if (m->rows) (void)hipFree(m->rows);
  m->rows = nullptr;
  m->rows_bytes = 0;
  if (device_alloc(ctx, reinterpret_cast<void**>(&m->rows), need, true) != hipSuccess) {
    (void)hipGetLastError();
    return set_error(ctx, ORE_ERR_OOM, "top-k rows buffer (%zu bytes) allocation failed", need);
  }
  m->rows_bytes = need;
  return ORE_OK;
}

// argument checks of the run / capture entries; d_input is the float32 or the uint8 batch
static ore_status check_run_args(ore_model* m, const void* d_input, int64_t n, float* d_output) {
  if (!m || !d_input || !d_output) return set_error(m ? m->ctx : nullptr, ORE_ERR_INVALID, "null argument");
  if (n < 0 || n > m->max_batch)
    return set_error(m->ctx, ORE_ERR_INVALID, "batch %lld exceeds max_batch %lld", (long long)n, (long long)m->max_batch);
  return ORE_OK;
}

// the classify entries' rule for n images under ore_model_set_views: whole groups (plan() may have lowered
// run_batch since the views were set)
static ore_status check_views(ore_model* m, int64_t n) {
  if (m->views > m->run_batch)
    return set_error(m->ctx, ORE_ERR_INVALID, "views = %d exceed the run batch %lld: call ore_model_set_views again", int(m->views),
                     (long long)m->run_batch);
  if (n % m->views != 0)
    return set_error(m->ctx, ORE_ERR_INVALID, "%lld images are not a multiple of views = %d", (long long)n, int(m->views));
  return ORE_OK;
}

// the classify entries' rule under ore_model_set_cam: the maps of n images fit the caller's buffer
static ore_status check_cam(ore_model* m, int64_t n) {
  if (!m->cam_buf) return ORE_OK;
  const Value& T = m->values[m->cam_map];
  const int64_t need = n * m->topk * T.dims[2] * T.dims[3];
  if (need > m->cam_cap)
    return set_error(m->ctx, ORE_ERR_INVALID, "the class maps of %lld images at k = %d (%lld x %lld) need %lld floats, the buffer of "
                     "ore_model_set_cam holds %lld", (long long)n, int(m->topk), (long long)T.dims[2], (long long)T.dims[3],
                     (long long)need, (long long)m->cam_cap);
  if (m->box_buf && n * m->topk > m->box_cap)
    return set_error(m->ctx, ORE_ERR_INVALID, "the boxes of %lld images at k = %d need %lld planes, the buffers of "
                     "ore_model_set_cam_boxes hold %lld", (long long)n, int(m->topk), (long long)(n * m->topk), (long long)m->box_cap);
  return ORE_OK;
}

// the classify entries' checks: check_run_args with two outputs, whole groups of views, and room for the class maps
static ore_status check_classify_args(ore_model* m, const void* d_input, int64_t n, float* d_scores, int32_t* d_classes) {
  if (!d_classes) return set_error(m ? m->ctx : nullptr, ORE_ERR_INVALID, "null argument");
  if (ore_status st = check_run_args(m, d_input, n, d_scores)) return st;
  if (ore_status st = check_views(m, n)) return st;
  return check_cam(m, n);
}

// The class maps of a chunk (ore_model_set_cam): images [i0, i0 + nc) of the run, whose map conv input the pass
// just left in place (pinned by the plan), under the classes the chunk's top-k launch wrote for groups i0 / views ...
static ore_status launch_cam(ore_model* m, int64_t i0, int64_t nc, int64_t views, const int32_t* d_classes) {
  ore_ctx* ctx = m->ctx;
  const Step& cv = m->base_steps[m->cam_conv];
  const Value& T = m->values[m->cam_map];
  const Ref x = ref_of(m, m->cam_in);
  const int64_t P = T.dims[2] * T.dims[3];
  if (!x.p || x.es != (m->f16 ? 2 : 4)) return err(m, ORE_ERR_INVALID, "internal: the map conv's input is not materialised");
  const ClassMaps p{x.p, m->values[cv.in1].cptr, cv.in2 >= 0 ? m->values[cv.in2].cptr : nullptr,
                    d_classes + (i0 / views) * m->topk, m->cam_buf + i0 * m->topk * P, x.nstride, int(nc), int(cv.C), int(P),
                    int(cv.M), int(m->topk), int(views), m->cam_relu ? 1 : 0,
                    int(m->f16 ? pixel_stride(x, cv.C) : plane_stride(x, P))};
  if (!class_maps_eligible(p)) return err(m, ORE_ERR_INVALID, "internal: class maps on an unsupported layout");
  if (m->f16) launch_class_maps_f16(p, ctx->stream);
  else launch_class_maps_f32(p, ctx->stream);
  ORE_HIP_CHECK(ctx, hipGetLastError());
  return ORE_OK;
}

// The boxes of a chunk's maps (ore_model_set_cam_boxes): planes [i0 topk, (i0 + nc) topk) of the maps buffer that
// launch_cam just filled, resized to the model's input size
static ore_status launch_cam_boxes(ore_model* m, int64_t i0, int64_t nc) {
  ore_ctx* ctx = m->ctx;
  const Value& T = m->values[m->cam_map];
  const Value& iv = m->values[m->input_value];
  const int64_t P = T.dims[2] * T.dims[3], p0 = i0 * m->topk;
  launch_cam_boxes_f32(m->cam_buf + p0 * P, nc * m->topk, int(T.dims[2]), int(T.dims[3]), int(iv.dims[2]), int(iv.dims[3]),
                       m->box_frac, m->box_buf + p0 * 4, m->box_areas ? m->box_areas + p0 : nullptr, ctx->stream);
  ORE_HIP_CHECK(ctx, hipGetLastError());
  return ORE_OK;
}

// ore_model_run, ore_model_run_u8 and the classify entries: the graph over n images, in chunks of at most
// run_batch.  With d_u8 the input is the uint8 NHWC batch: each chunk is converted into the staging buffer
// (ensure_stage), then run.  With d_classes each chunk's output stays on the model's side (the rows buffer of
// ensure_rows, or the arena where the output value lives there) and its m->topk best per image go to rows
// [i0, i0 + nc) of d_output (the scores) and d_classes, both [n, topk] -- under ore_model_set_views the best of
// the mean of every `views` consecutive rows, to rows [i0 / views, (i0 + nc) / views) of [n / views, topk], the
// chunks holding whole groups.  With lst the input is an image list
// of n descriptors (check_list_args): chunk i0 converts descriptors [i0, i0 + nc) into the staging buffer.
static ore_status run_chunks(ore_model* m, const float* d_input, const uint8_t* d_u8, int64_t n, float* d_output,
                             int32_t* d_classes = nullptr, ore_image_list* lst = nullptr) {
  ore_ctx* ctx = m->ctx;
  ORE_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  const Value& iv = m->values[m->input_value];
  PreprocParams pre;
  ResizeParams rsz;  // instead of pre after ore_model_set_input_resize
  ResizeListParams lsp;  // an image list: its own geometries, whatever ore_model_set_input_resize holds
  if (lst) {
    if (ore_status st = list_params(ctx, lst, m->in_scale, m->in_shift, m->in_flags, &lsp)) return st;
    lsp.y = m->stage;
    lsp.y_nstride = iv.per_image();
  } else if (d_u8 && m->in_resized) {
    if (ore_status st = resize_params(ctx, m->in_hs, m->in_ws, iv.dims[1], iv.dims[2], iv.dims[3], &m->in_resize, m->in_scale,
                                      m->in_shift, m->in_flags, &rsz, m->in_filter))
      return st;
    rsz.y = m->stage;
    rsz.y_nstride = iv.per_image();
  } else if (d_u8) {
    if (ore_status st = preproc_params(ctx, iv.dims[2], iv.dims[3], iv.dims[1], m->in_scale, m->in_shift, m->in_flags, &pre))
      return st;
    pre.y = m->stage;
    pre.y_nstride = iv.per_image();
  }
  m->last_n = n;
  const Value& ov = m->values[m->output_value];
  // bind the output buffer directly when its producer writes a plain contiguous tensor
  m->out_bound = ov.alias_of < 0 && !ov.elided;
  // n > run_batch: equal chunks of consecutive images, at most run_batch each (every image's
  // arithmetic is independent of the batch it runs in)
  // the classify entries keep the groups of ore_model_set_views whole (group_chunks; the same arithmetic at 1)
  const int64_t views = d_classes ? m->views : 1;
  const GroupChunks gc = group_chunks(n, m->run_batch, views);
  const int64_t nchunks = gc.nchunks, chunk = gc.chunk;
  m->last_chunked = nchunks > 1;
  const size_t nev = m->exec_steps.size() + 1;
  if (m->timing && m->events.size() < nev * size_t(nchunks)) {
    for (auto e : m->events) (void)hipEventDestroy(e);
    m->events.assign(nev * size_t(nchunks), nullptr);
    for (auto& e : m->events) ORE_HIP_CHECK(ctx, hipEventCreate(&e));
  }
  m->timed_chunks = m->timing ? int(nchunks) : 0;
  if (m->streams > 1 && !m->timing && !m->side) {
    ORE_HIP_CHECK(ctx, hipStreamCreateWithFlags(&m->side, hipStreamNonBlocking));
    ORE_HIP_CHECK(ctx, hipEventCreateWithFlags(&m->ev_fork, hipEventDisableTiming));
    ORE_HIP_CHECK(ctx, hipEventCreateWithFlags(&m->ev_join, hipEventDisableTiming));
  }
  const int64_t in_img = iv.per_image(), out_img = ov.per_image();
  for (int64_t c = 0, i0 = 0; c < nchunks; ++c, i0 += chunk) {
    const int64_t nc = std::min(chunk, n - i0);
    const float* x = d_input ? d_input + i0 * in_img : m->stage;
    if (lst) {  // as the uint8 batch below: in front of the pass's first timing event
      lsp.first = i0;
      lsp.N = nc;
      launch_list(ctx, lst, lsp);
      ORE_HIP_CHECK(ctx, hipGetLastError());
    } else if (d_u8) {  // before the pass's first timing event: ore_model_step_times does not include it
      if (m->in_resized) {  // the source images have their own size
        rsz.x = d_u8 + i0 * m->in_hs * m->in_ws * iv.dims[1];
        rsz.N = nc;
        launch_resize_dense(rsz, m->in_filter, ctx->stream);
      } else {
        pre.x = d_u8 + i0 * in_img;
        pre.N = nc;
        launch_preproc_u8(pre, ctx->stream);
      }
      ORE_HIP_CHECK(ctx, hipGetLastError());
    }
    if (ore_status st = run_pass(m, x, nc, d_classes ? m->rows : d_output + i0 * out_img,
                                 m->timing ? m->events.data() + size_t(c) * nev : nullptr, !d_classes))
      return st;
    if (d_classes) {  // after the pass's last timing event: not an exec step
      const Ref r = ref_of(m, m->output_value);
      const int64_t g0 = i0 / views;  // the chunk's nc / views groups go to rows [g0, g0 + nc / views)
      launch_topk_mean(r.p, r.nstride, nc / views, int(views), int(out_img), m->topk, d_output + g0 * m->topk,
                       d_classes + g0 * m->topk, ctx->stream);
      ORE_HIP_CHECK(ctx, hipGetLastError());
      if (m->cam_buf)  // the maps of the classes just selected, from the map conv's input the pass left in place
      {
        if (ore_status st = launch_cam(m, i0, nc, views, d_classes)) return st;
        if (m->box_buf)
          if (ore_status st = launch_cam_boxes(m, i0, nc)) return st;
      }
    }
  }
  return ORE_OK;
}

ore_status ore_model_run(ore_model* m, const float* d_input, int64_t n, float* d_output) {
  if (ore_status st = check_run_args(m, d_input, n, d_output)) return st;
  return run_chunks(m, d_input, nullptr, n, d_output);
}

ore_status ore_model_set_input_norm(ore_model* m, const float* scale, const float* shift, int32_t c, int32_t flags) {
  if (!m) return set_error(nullptr, ORE_ERR_INVALID, "null model");
  ore_ctx* ctx = m->ctx;
  const Value& iv = m->values[m->input_value];
  if (c != iv.dims[1])
    return set_error(ctx, ORE_ERR_INVALID, "input norm for %d channels, the model input has %lld", int(c), (long long)iv.dims[1]);
  PreprocParams pre;
  if (ore_status st = preproc_params(ctx, iv.dims[2], iv.dims[3], c, scale, shift, flags, &pre)) return st;
  if (ore_status st = ensure_stage(m)) return st;
  for (int i = 0; i < c; ++i) {
    m->in_scale[i] = scale ? scale[i] : 1.0f;
    m->in_shift[i] = shift ? shift[i] : 0.0f;
  }
  m->in_flags = flags;
  return ORE_OK;
}

ore_status ore_model_set_input_resize(ore_model* m, int64_t hs, int64_t ws, const ore_resize* g) {
  return ore_model_set_input_resize_ex(m, hs, ws, g, ORE_FILTER_BILINEAR);
}

ore_status ore_model_set_input_resize_ex(ore_model* m, int64_t hs, int64_t ws, const ore_resize* g, int32_t filter) {
  if (!m) return set_error(nullptr, ORE_ERR_INVALID, "null model");
  if (!g) {  // back to the direct conversion of [n,H,W,C]
    m->in_resized = false;
    return ORE_OK;
  }
  const Value& iv = m->values[m->input_value];
  ResizeParams rsz;
  if (ore_status st = resize_params(m->ctx, hs, ws, iv.dims[1], iv.dims[2], iv.dims[3], g, m->in_scale, m->in_shift, m->in_flags, &rsz,
                                    filter))
    return st;
  m->in_hs = hs;
  m->in_ws = ws;
  m->in_resize = *g;
  m->in_filter = filter;
  m->in_resized = true;
  return ORE_OK;
}

ore_status ore_model_run_u8(ore_model* m, const uint8_t* d_input, int64_t n, float* d_output) {
  if (ore_status st = check_run_args(m, d_input, n, d_output)) return st;
  if (n == 0) return ORE_OK;
  if (ore_status st = ensure_stage(m)) return st;
  return run_chunks(m, nullptr, d_input, n, d_output);
}

ore_status ore_model_set_topk(ore_model* m, int32_t k) {
  if (!m) return set_error(nullptr, ORE_ERR_INVALID, "null model");
  const int64_t kmax = std::min<int64_t>(m->values[m->output_value].per_image(), 64);
  if (k < 1 || k > kmax)
    return set_error(m->ctx, ORE_ERR_INVALID, "top-k k = %d outside 1..%lld (min(output elems, 64))", int(k), (long long)kmax);
  if (ore_status st = ensure_rows(m)) return st;
  m->topk = k;
  return ORE_OK;
}

ore_status ore_model_set_views(ore_model* m, int32_t views) {
  if (!m) return set_error(nullptr, ORE_ERR_INVALID, "null model");
  const int64_t vmax = std::min<int64_t>(ORE_MAX_VIEWS, m->run_batch);
  if (views < 1 || views > vmax)
    return set_error(m->ctx, ORE_ERR_INVALID, "views = %d outside 1..%lld (min(ORE_MAX_VIEWS, run batch))", int(views), (long long)vmax);
  m->views = views;
  return ORE_OK;
}

ore_status ore_model_cam_dims(ore_model* m, int64_t hw[2]) {
  if (!m || !hw) return set_error(m ? m->ctx : nullptr, ORE_ERR_INVALID, "null argument");
  if (m->cam_conv < 0) return set_error(m->ctx, ORE_ERR_UNSUPPORTED, "%s", m->cam_why.c_str());
  hw[0] = m->values[m->cam_map].dims[2];
  hw[1] = m->values[m->cam_map].dims[3];
  return ORE_OK;
}

ore_status ore_model_set_cam(ore_model* m, float* d_maps, int64_t cap_elems) {
  if (!m) return set_error(nullptr, ORE_ERR_INVALID, "null model");
  ore_ctx* ctx = m->ctx;
  if (d_maps && m->cam_conv < 0) return set_error(ctx, ORE_ERR_UNSUPPORTED, "%s", m->cam_why.c_str());
  if (d_maps && cap_elems < 0) return set_error(ctx, ORE_ERR_INVALID, "class map buffer of %lld floats", (long long)cap_elems);
  if ((d_maps != nullptr) != (m->cam_buf != nullptr)) {  // on <-> off: the plan pins (or releases) the conv's input
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (ctx->stream && hipStreamIsCapturing(ctx->stream, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone)
      return set_error(ctx, ORE_ERR_INVALID, "ore_model_set_cam inside a stream capture (it replans the model)");
    // the arena is sized anew, so that turning the maps off gives back exactly the arena of a model without them
    // (plan() alone only ever grows it)
    ORE_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    ORE_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    if (m->arena_alloc) (void)hipFree(m->arena_alloc);
    m->arena = m->arena_alloc = nullptr;
    m->arena_bytes = 0;
    float* const old_buf = m->cam_buf;
    m->cam_buf = d_maps;
    if (ore_status st = plan(m)) {  // back to the plan that stood
      const std::string e = ctx->err;
      m->cam_buf = old_buf;
      (void)plan(m);
      return set_error(ctx, st, "%s", e.c_str());
    }
  }
  m->cam_buf = d_maps;
  m->cam_cap = d_maps ? cap_elems : 0;
  if (!d_maps) {  // the boxes are those of the maps
    m->box_buf = m->box_areas = nullptr;
    m->box_cap = 0;
  }
  return ORE_OK;
}

ore_status ore_model_set_cam_boxes(ore_model* m, int32_t* d_boxes, int32_t* d_areas, int64_t cap_planes, float frac) {
  if (!m) return set_error(nullptr, ORE_ERR_INVALID, "null model");
  ore_ctx* ctx = m->ctx;
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  if (ctx->stream && hipStreamIsCapturing(ctx->stream, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone)
    return set_error(ctx, ORE_ERR_INVALID, "ore_model_set_cam_boxes inside a stream capture");
  if (d_boxes) {
    if (m->cam_conv < 0) return set_error(ctx, ORE_ERR_UNSUPPORTED, "%s", m->cam_why.c_str());
    if (!m->cam_buf)
      return set_error(ctx, ORE_ERR_INVALID, "ore_model_set_cam_boxes: the class maps are off (ore_model_set_cam first: the boxes "
                       "are computed from its buffer)");
    if (cap_planes < 0) return set_error(ctx, ORE_ERR_INVALID, "box buffers of %lld planes", (long long)cap_planes);
    if (!(frac >= 0.0f && frac <= 1.0f)) return set_error(ctx, ORE_ERR_INVALID, "cam boxes: frac = %g outside [0, 1]", double(frac));
    const Value& T = m->values[m->cam_map];
    const Value& iv = m->values[m->input_value];
    const int64_t hm = T.dims[2], wm = T.dims[3], h = iv.ndim == 4 ? iv.dims[2] : 0, w = iv.ndim == 4 ? iv.dims[3] : 0;
    if (cam_boxes_unsupported(hm, wm, h, w) || h < hm || w < wm)
      return set_error(ctx, ORE_ERR_UNSUPPORTED, "cam boxes: a %lld x %lld map under a %lld x %lld input is outside the box kernel's "
                       "caps (hm * wm <= %d, hm <= h <= %d, wm <= w <= %d)", (long long)hm, (long long)wm, (long long)h, (long long)w,
                       ORE_CAM_BOX_MAX_MAP, ORE_CAM_BOX_MAX_SIDE, ORE_CAM_BOX_MAX_SIDE);
  }
  m->box_buf = d_boxes;
  m->box_areas = d_boxes ? d_areas : nullptr;
  m->box_cap = d_boxes ? cap_planes : 0;
  m->box_frac = d_boxes ? frac : 0.0f;
  return ORE_OK;
}

ore_status ore_model_classify(ore_model* m, const float* d_input, int64_t n, float* d_scores, int32_t* d_classes) {
  if (ore_status st = check_classify_args(m, d_input, n, d_scores, d_classes)) return st;
  if (n == 0) return ORE_OK;
  if (ore_status st = ensure_rows(m)) return st;
  return run_chunks(m, d_input, nullptr, n, d_scores, d_classes);
}

ore_status ore_model_classify_u8(ore_model* m, const uint8_t* d_input, int64_t n, float* d_scores, int32_t* d_classes) {
  if (ore_status st = check_classify_args(m, d_input, n, d_scores, d_classes)) return st;
  if (n == 0) return ORE_OK;
  if (ore_status st = ensure_stage(m)) return st;
  if (ore_status st = ensure_rows(m)) return st;
  return run_chunks(m, nullptr, d_input, n, d_scores, d_classes);
}

// the _u8_list entries' checks: check_run_args with the list as the input and its count as n
static ore_status check_list_args(ore_model* m, ore_image_list* l, float* d_output) {
  if (ore_status st = check_run_args(m, l, l ? l->count : 0, d_output)) return st;
  const Value& iv = m->values[m->input_value];
  if (l->ctx != m->ctx) return set_error(m->ctx, ORE_ERR_INVALID, "the image list belongs to another context than the model");
  if (l->c != iv.dims[1] || l->h != iv.dims[2] || l->w != iv.dims[3])
    return set_error(m->ctx, ORE_ERR_INVALID, "the image list produces %lld x %lld x %lld, the model input is %lld x %lld x %lld",
                     (long long)l->c, (long long)l->h, (long long)l->w, (long long)iv.dims[1], (long long)iv.dims[2], (long long)iv.dims[3]);
  return ORE_OK;
}

ore_status ore_model_run_u8_list(ore_model* m, ore_image_list* l, float* d_output) {
  if (ore_status st = check_list_args(m, l, d_output)) return st;
  if (l->count == 0) return ORE_OK;
  if (ore_status st = ensure_stage(m)) return st;
  return run_chunks(m, nullptr, nullptr, l->count, d_output, nullptr, l);
}

ore_status ore_model_classify_u8_list(ore_model* m, ore_image_list* l, float* d_scores, int32_t* d_classes) {
  if (!d_classes) return set_error(m ? m->ctx : nullptr, ORE_ERR_INVALID, "null argument");
  if (ore_status st = check_list_args(m, l, d_scores)) return st;
  if (ore_status st = check_views(m, l->count)) return st;
  if (ore_status st = check_cam(m, l->count)) return st;
  if (l->count == 0) return ORE_OK;
  if (ore_status st = ensure_stage(m)) return st;
  if (ore_status st = ensure_rows(m)) return st;
  return run_chunks(m, nullptr, nullptr, l->count, d_scores, d_classes, l);
}

ore_status ore_model_read_value(ore_model* m, const char* name, float* host_dst, size_t cap, int64_t dims[4],
                                int32_t* ndim) {
  if (!m || !name) return set_error(nullptr, ORE_ERR_INVALID, "null argument");
  ore_ctx* ctx = m->ctx;
  int id = value_id(m, name);
  if (id < 0) return set_error(ctx, ORE_ERR_INVALID, "no value named '%s'", name);
  const Value& v = m->values[id];
  if (v.elided) return set_error(ctx, ORE_ERR_INVALID, "value '%s' is fused away", name);
  if (!v.is_const && m->last_chunked)
    return set_error(ctx, ORE_ERR_INVALID, "the last run went in image chunks of %lld: value '%s' holds only the last one",
                     (long long)m->run_batch, name);
  const int64_t n = v.is_const ? 1 : m->last_n;
  if (dims) {
    for (int i = 0; i < 4; ++i) dims[i] = v.dims[i];
    if (!v.is_const) dims[0] = n;
  }
  if (ndim) *ndim = v.ndim;
  const int64_t pe = v.is_const ? v.numel_const() : v.per_image();
  if (!host_dst) return ORE_OK;
  if (size_t(n * pe) > cap) return set_error(ctx, ORE_ERR_INVALID, "destination too small");
  {
    const int rid = root(m, id);
    const Value& rv = m->values[rid];
    if (!rv.is_const && rv.first < 0 && !rv.is_input)
      return set_error(ctx, ORE_ERR_INVALID, "value '%s' not materialised", name);
    // Without ORE_KEEP_VALUES the arena reuses slots by liveness: a value whose bytes a later value
    // (first write after this one's last read) overlaps was overwritten during the run -> refuse
    // rather than return stale data.
    if (!(m->fusion & ORE_KEEP_VALUES) && rv.arena_off >= 0) {
      const int64_t lo = rv.arena_off, hi = rv.arena_off + slot_extent(m, rv);
      for (size_t j = 0; j < m->values.size(); ++j) {
        const Value& o = m->values[j];
        if (int(j) == rid || o.arena_off < 0 || o.alias_of >= 0 || o.is_const || o.is_input || o.elided) continue;
        if (o.first > rv.last && o.arena_off < hi && lo < o.arena_off + slot_extent(m, o))
          return set_error(ctx, ORE_ERR_INVALID,
                           "value '%s' was overwritten by a later value in the arena (load with ORE_KEEP_VALUES "
                           "to read intermediate values)", name);
      }
    }
  }
  ORE_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  ORE_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  const Ref r = ref_of(m, id);
  if (!r.p) return set_error(ctx, ORE_ERR_INVALID, "value '%s' has no f32 storage", name);
  const int64_t ns = v.is_const ? pe : r.nstride;
  if (r.es == 2) {  // f16 storage: download the halves, convert (and, channels-last, transpose) on the host
    std::vector<uint16_t> tmp(size_t(n * pe));
    if (v.nhwc) {  // per image: H*W pixels of C channels at pixel stride ps -> NCHW
      const int64_t C = v.dims[1], HW = v.dims[2] * v.dims[3];
      for (int64_t i = 0; i < n; ++i)
        ORE_HIP_CHECK(ctx, hipMemcpy2D(tmp.data() + i * pe, size_t(C) * 2, reinterpret_cast<const char*>(r.p) + i * ns * 2,
                                       size_t(r.ps) * 2, size_t(C) * 2, size_t(HW), hipMemcpyDeviceToHost));
      for (int64_t i = 0; i < n; ++i)
        for (int64_t q = 0; q < HW; ++q)
          for (int64_t c = 0; c < C; ++c) host_dst[i * pe + c * HW + q] = half_bits_to_float(tmp[size_t(i * pe + q * C + c)]);
      return ORE_OK;
    }
    ORE_HIP_CHECK(ctx, hipMemcpy2D(tmp.data(), size_t(pe) * 2, r.p, size_t(ns) * 2, size_t(pe) * 2, size_t(n),
                                   hipMemcpyDeviceToHost));
    for (size_t i = 0; i < tmp.size(); ++i) host_dst[i] = half_bits_to_float(tmp[i]);
    return ORE_OK;
  }
  if (!v.is_const && v.ndim == 4 && r.ps && r.ps != v.dims[2] * v.dims[3]) {  // padded planes
    const int64_t P = v.dims[2] * v.dims[3];
    for (int64_t i = 0; i < n; ++i)
      ORE_HIP_CHECK(ctx, hipMemcpy2D(host_dst + i * pe, size_t(P) * 4, r.p + i * ns, size_t(r.ps) * 4, size_t(P) * 4,
                                     size_t(v.dims[1]), hipMemcpyDeviceToHost));
    return ORE_OK;
  }
  ORE_HIP_CHECK(ctx, hipMemcpy2D(host_dst, size_t(pe) * 4, r.p, size_t(ns) * 4, size_t(pe) * 4, size_t(n),
                                 hipMemcpyDeviceToHost));
  return ORE_OK;
}

ore_status ore_model_autotune(ore_model* m, const float* d_input, int64_t n, float* d_output, int32_t reps) {
  if (!m || !d_input || !d_output) return set_error(m ? m->ctx : nullptr, ORE_ERR_INVALID, "null argument");
  ore_ctx* ctx = m->ctx;
  if (n < 1 || n > m->max_batch) return set_error(ctx, ORE_ERR_INVALID, "batch out of range");
  if (reps < 1) reps = 3;
  const int64_t n_all = n;
  if (n > m->run_batch) {  // tuned on one chunk of the chunked run (ore_model_run)
    const int64_t nchunks = (n + m->run_batch - 1) / m->run_batch;
    n = (n + nchunks - 1) / nchunks;
  }
  m->last_chunked = false;
  ORE_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  m->cur_in = d_input;
  m->cur_out = d_output;
  m->last_n = n;
  const Value& ov = m->values[m->output_value];
  m->out_bound = ov.alias_of < 0 && !ov.elided;
  hipEvent_t e0, e1;
  ORE_HIP_CHECK(ctx, hipEventCreate(&e0));
  ORE_HIP_CHECK(ctx, hipEventCreate(&e1));
  ore_status st = ORE_OK;
  // steps run in order so every conv sees its real input geometry; each candidate tile is timed on
  // the step's own buffers and the fastest kept (results do not depend on the tile: every output is
  // the same k-ordered MFMA chain, every pooled value the same max)
  for (size_t k = 0; k < m->exec_steps.size() && !st; ++k) {
    Step& s = m->steps[m->exec_steps[k]];
    const std::vector<int> cands = step_tile_family(s);
    if (cands.size() < 2) {
      if (cands.size() == 1) set_tile(m, int(k), cands[0]);
      st = launch_step(m, s, n);
      continue;
    }
    int best = -1;
    float best_ms = 1e30f;
    for (size_t ci = 0; ci < cands.size() && !st; ++ci) {
      const int c = cands[ci];
      set_tile(m, int(k), c);
      st = launch_step(m, s, n);  // warm-up
      if (st) break;
      if (s.ran_tile != c) continue;  // fell back to another kernel: not a distinct candidate here
      if (hipEventRecord(e0, ctx->stream) != hipSuccess) { st = set_error(ctx, ORE_ERR_HIP, "event record"); break; }
      for (int r = 0; r < reps && !st; ++r) st = launch_step(m, s, n);
      if (st) break;
      float ms = 0.f;
      if (hipEventRecord(e1, ctx->stream) != hipSuccess || hipEventSynchronize(e1) != hipSuccess ||
          hipEventElapsedTime(&ms, e0, e1) != hipSuccess) {
        st = set_error(ctx, ORE_ERR_HIP, "autotune timing failed");
        break;
      }
      if (ms < best_ms) { best_ms = ms; best = c; }
    }
    if (best >= 0) set_tile(m, int(k), best);
    if (!st) st = launch_step(m, s, n);  // leave the real output for the next step
  }
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  if (!st && hipStreamSynchronize(ctx->stream) != hipSuccess) st = set_error(ctx, ORE_ERR_HIP, "autotune sync");
  // tuned on the first chunk only: run the whole batch once so d_output holds every image's output
  if (!st && n_all > n) st = ore_model_run(m, d_input, n_all, d_output);
  if (!st && n_all > n && hipStreamSynchronize(ctx->stream) != hipSuccess) st = set_error(ctx, ORE_ERR_HIP, "autotune sync");
  return st;
}

int32_t ore_model_step_tile(ore_model* m, int32_t i) {
  if (!m || i < 0 || size_t(i) >= m->exec_steps.size()) return -1;
  const Step& s = m->steps[m->exec_steps[i]];
  if (s.fire.on) return s.fire.f16 ? FIRE_F16_TILE : s.fire.pool ? FIRE_POOL_TILE : FIRE_TILE;
  if (s.kind == S_CONV && s.ep.on && !s.plan.f16 && s.plan.epv > 0) return epool_tile_id(s.plan.epv);
  if (s.kind == S_CONV && s.ep.on && s.ran_tile >= 0) return s.ran_tile;
  if (s.kind == S_CONV && s.gap) return s.plan.f16 ? CONV_GAP_F16_TILE : CONV_GAP_F32_TILE;
  return (s.kind == S_CONV || s.kind == S_MATMUL) ? s.plan.cfg : -1;
}

ore_status ore_model_set_step_tile(ore_model* m, int32_t i, int32_t tile) {
  if (!m || i < 0 || size_t(i) >= m->exec_steps.size()) return set_error(m ? m->ctx : nullptr, ORE_ERR_INVALID, "bad step index");
  const std::vector<int> fam = step_tile_family(m->steps[m->exec_steps[i]]);
  if (std::find(fam.begin(), fam.end(), int(tile)) == fam.end())
    return set_error(m->ctx, ORE_ERR_INVALID, "tile %d is not a kernel of step %d ('%s')", int(tile), int(i),
                     m->steps[m->exec_steps[i]].name.c_str());
  set_tile(m, i, tile);
  return ORE_OK;
}

ore_status ore_model_step_mfma_flops(ore_model* m, int32_t i, double* flops) {
  if (!m || !flops || i < 0 || size_t(i) >= m->exec_steps.size())
    return set_error(m ? m->ctx : nullptr, ORE_ERR_INVALID, "bad step index");
  const Step& s = m->steps[m->exec_steps[i]];
  *flops = (s.mfma_flops_per_img >= 0 ? s.mfma_flops_per_img : s.flops_per_img) * double(m->last_n);
  return ORE_OK;
}

ore_status ore_model_set_streams(ore_model* m, int32_t streams) {
  if (!m || streams < 1 || streams > 2) return set_error(m ? m->ctx : nullptr, ORE_ERR_INVALID, "streams must be 1 or 2");
  m->streams = streams;
  return ORE_OK;
}

// the graph capture entries: one run_chunks(d_input, d_u8, n, d_output, d_classes) as a HIP graph
static ore_status capture_run(ore_model* m, const float* d_input, const uint8_t* d_u8, int64_t n, float* d_output,
                              int32_t* d_classes = nullptr, ore_image_list* lst = nullptr) {
  ore_ctx* ctx = m->ctx;
  if (m->timing) return set_error(ctx, ORE_ERR_INVALID, "disable step timing before capturing a graph");
  if (!ctx->stream) return set_error(ctx, ORE_ERR_INVALID, "graph capture needs a non-null context stream");
  ORE_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  if (m->graph_exec) { (void)hipGraphExecDestroy(m->graph_exec); m->graph_exec = nullptr; }
  if (m->graph) { (void)hipGraphDestroy(m->graph); m->graph = nullptr; }
  m->graph_list = nullptr;
  if (m->streams > 1 && !m->side) {  // created outside the capture
    ORE_HIP_CHECK(ctx, hipStreamCreateWithFlags(&m->side, hipStreamNonBlocking));
    ORE_HIP_CHECK(ctx, hipEventCreateWithFlags(&m->ev_fork, hipEventDisableTiming));
    ORE_HIP_CHECK(ctx, hipEventCreateWithFlags(&m->ev_join, hipEventDisableTiming));
  }
  if (d_u8 || lst)  // allocated outside the capture
    if (ore_status st = ensure_stage(m)) return st;
  if (d_classes)
    if (ore_status st = ensure_rows(m)) return st;
  ORE_HIP_CHECK(ctx, hipStreamBeginCapture(ctx->stream, hipStreamCaptureModeThreadLocal));
  ore_status st = run_chunks(m, d_input, d_u8, n, d_output, d_classes, lst);
  hipGraph_t g = nullptr;
  const hipError_t e = hipStreamEndCapture(ctx->stream, &g);
  if (st) {
    if (g) (void)hipGraphDestroy(g);
    return st;
  }
  if (e != hipSuccess) return set_error(ctx, ORE_ERR_HIP, "hipStreamEndCapture: %s", hipGetErrorString(e));
  m->graph = g;
  ORE_HIP_CHECK(ctx, hipGraphInstantiate(&m->graph_exec, m->graph, nullptr, nullptr, 0));
  m->graph_list = lst;  // the graph reads lst's table at replay: descriptors [0, n)
  m->graph_list_count = n;
  m->graph_list_oriented = lst && lst->oriented;
  return ORE_OK;
}

ore_status ore_model_graph_capture(ore_model* m, const float* d_input, int64_t n, float* d_output) {
  if (ore_status st = check_run_args(m, d_input, n, d_output)) return st;
  return capture_run(m, d_input, nullptr, n, d_output);
}

ore_status ore_model_graph_capture_u8(ore_model* m, const uint8_t* d_input, int64_t n, float* d_output) {
  if (ore_status st = check_run_args(m, d_input, n, d_output)) return st;
  return capture_run(m, nullptr, d_input, n, d_output);
}

ore_status ore_model_graph_capture_classify(ore_model* m, const float* d_input, int64_t n, float* d_scores,
                                            int32_t* d_classes) {
  if (ore_status st = check_classify_args(m, d_input, n, d_scores, d_classes)) return st;
  return capture_run(m, d_input, nullptr, n, d_scores, d_classes);
}

ore_status ore_model_graph_capture_classify_u8(ore_model* m, const uint8_t* d_input, int64_t n, float* d_scores,
                                               int32_t* d_classes) {
  if (ore_status st = check_classify_args(m, d_input, n, d_scores, d_classes)) return st;
  return capture_run(m, nullptr, d_input, n, d_scores, d_classes);
}

ore_status ore_model_graph_capture_u8_list(ore_model* m, ore_image_list* l, float* d_output) {
  if (ore_status st = check_list_args(m, l, d_output)) return st;
  return capture_run(m, nullptr, nullptr, l->count, d_output, nullptr, l);
}

ore_status ore_model_graph_capture_classify_u8_list(ore_model* m, ore_image_list* l, float* d_scores, int32_t* d_classes) {
  if (!d_classes) return set_error(m ? m->ctx : nullptr, ORE_ERR_INVALID, "null argument");
  if (ore_status st = check_list_args(m, l, d_scores)) return st;
  if (ore_status st = check_views(m, l->count)) return st;
  if (ore_status st = check_cam(m, l->count)) return st;
  return capture_run(m, nullptr, nullptr, l->count, d_scores, d_classes, l);
}

ore_status ore_model_graph_launch(ore_model* m) {
  if (!m) return set_error(nullptr, ORE_ERR_INVALID, "null model");
  if (!m->graph_exec) return set_error(m->ctx, ORE_ERR_INVALID, "no captured graph (ore_model_graph_capture)");
  if (m->graph_list && m->graph_list->count != m->graph_list_count)
    return set_error(m->ctx, ORE_ERR_INVALID, "the graph was captured on a list of %lld images, the list now holds %lld",
                     (long long)m->graph_list_count, (long long)m->graph_list->count);
  if (m->graph_list && !m->graph_list_oriented && m->graph_list->any_orient)
    return set_error(m->ctx, ORE_ERR_INVALID, "the graph was captured before the list's first oriented set and runs kernels that "
                                              "read no orientation, the list now holds one: re-capture");
  ORE_HIP_CHECK(m->ctx, hipGraphLaunch(m->graph_exec, m->ctx->stream));
  return ORE_OK;
}

ore_status ore_model_enable_timing(ore_model* m, int32_t on) {
  if (!m) return set_error(nullptr, ORE_ERR_INVALID, "null model");
  m->timing = on != 0;
  return ORE_OK;
}

int32_t ore_model_step_count(ore_model* m) { return m ? int32_t(m->exec_steps.size()) : 0; }

int64_t ore_model_run_batch(ore_model* m) { return m ? m->run_batch : 0; }

ore_status ore_model_step_info(ore_model* m, int32_t i, const char** op, const char** name, double* flops, double* bytes) {
  if (!m || i < 0 || size_t(i) >= m->exec_steps.size()) return set_error(nullptr, ORE_ERR_INVALID, "bad step index");
  const Step& s = m->steps[m->exec_steps[i]];
  static const char* kinds[] = {"Conv", "MaxPool", "Relu", "Add", "Softmax", "MatMul", "GlobalAveragePool", "Concat", "Copy",
                                "Nop", "Conv"};  // S_FIRE: three convs (expand 1x1 / 3x3 + squeeze) in one launch
  if (op) *op = kinds[s.kind];
  if (name) *name = s.name.c_str();
  const double n = double(m->last_n);
  if (flops) *flops = s.flops_per_img * n;
  if (bytes) {
    double b = s.bytes_per_img * n + s.bytes_fixed;
    // fused epilogues/in-place writes move fewer bytes than the op-by-op accounting
    *bytes = b;
  }
  return ORE_OK;
}

ore_status ore_model_step_times(ore_model* m, float* ms, int32_t cap) {
  if (!m || !ms) return set_error(nullptr, ORE_ERR_INVALID, "null argument");
  const size_t nev = m->exec_steps.size() + 1;
  if (!m->timing || m->timed_chunks < 1 || m->events.size() < nev * size_t(m->timed_chunks))
    return set_error(m->ctx, ORE_ERR_INVALID, "timing not enabled");
  ORE_HIP_CHECK(m->ctx, hipEventSynchronize(m->events[nev * size_t(m->timed_chunks) - 1]));
  for (size_t k = 0; k < m->exec_steps.size() && int32_t(k) < cap; ++k) {
    ms[k] = 0.f;
    for (int c = 0; c < m->timed_chunks; ++c) {  // summed over the run's image chunks
      float t = 0.f;
      ORE_HIP_CHECK(m->ctx, hipEventElapsedTime(&t, m->events[c * nev + k], m->events[c * nev + k + 1]));
      ms[k] += t;
    }
  }
  return ORE_OK;
}

}  // extern "C"
