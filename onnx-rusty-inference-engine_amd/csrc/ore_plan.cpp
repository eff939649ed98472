// The planner: plan() and its passes (1)-(15) over the walker's step list (ore_model_types.h).
#include <algorithm>

#include "ore_model_types.h"

namespace ore {

namespace {

// ------------------------------------------------------------------ fusion + planning
// plan() rewrites the unfused node steps (base_steps) into the launched plan in passes, each a
// pattern over the step list that turns a producer -> consumer chain into one kernel step (the
// consumer steps become S_NOP, the values between them `elided`).  Every fusion is exact: the fused
// kernels keep each output's arithmetic (same operands, same k order, the max of the same values),
// so the result of the graph does not depend on which passes ran (tests/test_model_gpu.py checks each
// against the unfused graph bit for bit).  Pass order matters only where two patterns overlap
// (fire + pool + squeeze before concat + pool).  Then: algorithm selection (Winograd), aliases,
// Concat in place, the plane layout, the arena, branch pairs and the gather tables.
void count_uses(ore_model* m, const std::vector<Step>& steps) {
  for (auto& v : m->values) v.uses = 0;
  for (auto& s : steps)
    for (int id : {s.in0, s.in1, s.in2, s.in3})
      if (id >= 0) m->values[id].uses++;
  // the class-map kernel reads the map conv's input after the pass (ore_model_set_cam): no pass may elide it
  if (m->cam_buf && m->cam_in >= 0) m->values[m->cam_in].uses++;
}

// plane stride of a padded activation: 128-B aligned planes when that costs <= 5 %, else 16-B
// aligned ones when that does (13 x 13 -> 172: the streaming conv's 16-B operand loads and stores
// need 4-float planes), else dense
int64_t padded_plane(int64_t P) {
  int64_t Pp = (P + 31) / 32 * 32;
  if (Pp - P > P / 20) Pp = (P + 3) / 4 * 4;
  return Pp - P <= P / 20 ? Pp : P;
}

bool strided_writer(const Step& s) { return s.kind == S_CONV || s.kind == S_FIRE || s.kind == S_MAXPOOL; }

// step geometry, each spelled once; the passes add their own extras (Relu, precision, channel limits)
bool same_plane(const Step& s) { return s.win.Ho == s.H && s.win.Wo == s.W; }
// a 1x1 / stride-1 conv without pads on any side: the output plane is the input plane.  Every pass that takes a
// 1x1 conv into another kernel needs all of it: with bottom / right pads alone the output is a larger plane
// whose pad rows and columns hold relu(bias), which none of the fused kernels writes
bool conv_1x1_s1(const Step& s) {
  return s.kind == S_CONV && s.kh == 1 && s.kw == 1 && s.sh == 1 && s.sw == 1 && s.win.pt == 0 && s.win.pl == 0 &&
         same_plane(s);
}
bool conv_3x3_same(const Step& s) {
  return s.kind == S_CONV && s.kh == 3 && s.kw == 3 && s.sh == 1 && s.sw == 1 && s.win.pt == 1 && s.win.pl == 1 &&
         same_plane(s);
}
bool pool_3x3_s2(const Step& s) { return s.kind == S_MAXPOOL && s.kh == 3 && s.kw == 3 && s.sh == 2 && s.sw == 2; }
// ... of at most 2 top / left pad rows whose every window touches the image (the fire + pool kernels' limits)
bool pool_windows_touch(const Step& pl) {
  return pl.win.pt <= 2 && pl.win.pl <= 2 && 2 * (pl.win.Ho - 1) - pl.win.pt < pl.H && 2 * (pl.win.Wo - 1) - pl.win.pl < pl.W;
}
// no fusion has taken the step yet
bool unfused(const Step& s) { return !s.pin.on && !s.ep.on && !s.sq.on && !s.gap; }
// a plain f32 1x1 conv (+ Relu) on the direct kernels, output the size of its input
bool plain_1x1(const Step& s) { return conv_1x1_s1(s) && s.relu && unfused(s) && !s.plan.f16; }
// an f32 3x3 / stride-1 'same' conv (+ Relu) on the direct kernels
bool same_3x3(const Step& s) { return conv_3x3_same(s) && s.relu && unfused(s) && !s.plan.f16; }
// an f16 conv (+ Relu) on 16-B NHWC gathers (with conv_1x1_s1 / conv_3x3_same: the f16 fire kernels' convs)
bool vec16(const Step& s) {
  return s.kind == S_CONV && s.relu && unfused(s) && s.plan.f16 && s.plan.xmode == F16_X_NHWC_VEC;
}

// pool_conv1x1_f32_kernel's parameters for conv cv over the 3x3 / stride-2 pool (window pw) of H x W planes,
// dense, one image: what its eligibility check reads
PoolConvParams pool_conv_params(const Step& cv, int64_t H, int64_t W, const Window& pw) {
  PoolConvParams q{};
  q.C = int(cv.C); q.H = int(H); q.W = int(W); q.Hp = int(pw.Ho); q.Wp = int(pw.Wo);
  q.pt = int(pw.pt); q.pl = int(pw.pl); q.M = int(cv.M); q.Mp = cv.plan.Mp; q.Kp = cv.plan.krows;
  q.N = 1; q.x_ps = int(H * W); q.y_ps = int(pw.Ho * pw.Wo);
  q.x_nstride = int64_t(q.C) * q.x_ps; q.y_nstride = int64_t(q.M) * q.y_ps;
  return q;
}

// size heuristics of the fusion passes (measured at batch 256, DESIGN.md sections 3 and 7); ORE_FUSE_EAGER
// (tests) applies every eligible fusion regardless
constexpr int64_t FIRE_MIN_COLS = 65536;      // fire fusions: max_batch x H x W >= one 64-pixel wave per SIMD
constexpr int64_t FIRE_POOL_MIN_HW = 1024;    // fire + pool + squeeze on 54 x 54 planes (at 27 x 27 Winograd wins)
constexpr int64_t CONCAT_POOL_MIN_HW = 1024;  // concat + pool in the producers: fire4 -40 us, fire8 +21 us
constexpr double EPOOL_MAX_WORK = 1.25;       // conv + pool patch kernel: recomputed columns <= 1.25 x the conv's
constexpr int64_t WINO_SPLIT_MIN_C = 48;      // fire + squeeze on planes < FIRE_POOL_MIN_HW with >= 48 squeeze
                                              // channels: expand1x1 + Winograd expand3x3 + squeeze as three launches
                                              // (fire6 / fire7: 328 / 323 us vs 345 / 362 fused; fire5 at C = 32: 192 vs 173)

// a fire module as the fire passes see it (step indices, -1: absent): Concat cc of e1 (a 1x1) and e3 (a 3x3
// 'same' conv) of one value S, then optionally a 3x3 / stride-2 MaxPool, then the squeeze sq
struct FireMatch { int cc, e1, e3, pool, sq; };

struct Planner {
  ore_model* m;
  std::vector<int> producer;  // value -> the step that writes it (-1: input / constant)
  bool eager() const { return (m->fusion & ORE_FUSE_EAGER) != 0; }
  bool has(int32_t flags) const { return (m->fusion & flags) == flags; }
  Step& st(int i) { return m->steps[i]; }
  Value& val(int i) { return m->values[i]; }
  // the first launched step at or after `from` that reads v (in0 or in1)
  int reader(int v, size_t from) const {
    for (size_t j = from; j < m->steps.size(); ++j)
      if (m->steps[j].kind != S_NOP && (m->steps[j].in0 == v || m->steps[j].in1 == v || m->steps[j].in3 == v))
        return int(j);
    return -1;
  }
  // a value read once, not the graph output: free to elide
  bool private_value(int v) const { return m->values[v].uses == 1 && !m->values[v].is_output; }
  void nop(Step& s) {
    s.kind = S_NOP;
    s.in0 = s.in1 = s.in3 = -1;
  }
  void recount() { count_uses(m, m->steps); }
  // a weight packing made once per model (m->packs, freed with it); null on a failure
  template <class F>
  float* pack_once(PackKind kind, int idx, size_t bytes, F launch) {
    const auto key = std::make_pair(kind, idx);
    const auto it = m->packs.find(key);
    if (it != m->packs.end()) return it->second;
    float* buf = nullptr;
    if (device_alloc(m->ctx, reinterpret_cast<void**>(&buf), bytes, true) != hipSuccess) return nullptr;
    launch(buf);
    m->packs[key] = buf;
    return hipGetLastError() == hipSuccess && hipStreamSynchronize(m->ctx->stream) == hipSuccess ? buf : nullptr;
  }
  // the f32 fire kernels' row-permuted packing of expand conv idx (launch_fire_pack)
  float* fire_pack_f32(int idx) {
    const Step& e = st(idx);
    const int64_t K = e.C * e.kh * e.kw, Kp = (K + 31) / 32 * 32;
    const float* w = val(e.in1).cptr;
    return pack_once(PACK_FIRE_F32, idx, size_t(Kp * e.M) * 4,
                     [&](float* buf) { launch_fire_pack(w, int(e.M), int(K), buf, m->ctx->stream); });
  }
  // the f16 fire kernels' packing of conv idx (launch_fire_pack_f16): an expand (PACK_FIRE_F16), the squeeze
  // (PACK_SQ_F16), the squeeze fused into the first conv (PACK_C1SQ_F16)
  float* fire_pack_f16(PackKind kind, int idx) {
    const Step& e = st(idx);
    const int kk = int(e.kh * e.kw), M = int(e.M), C = int(e.C);
    const float* w = val(e.in1).cptr;
    return pack_once(kind, idx, fire_pack_f16_bytes(M, C, kk),
                     [&](float* buf) { launch_fire_pack_f16(w, M, C, kk, buf, m->ctx->stream); });
  }
  // the fire modules: Concat step i of two producers (e1 a 1x1, e3 a 3x3 'same' conv of one value S)
  bool fire_concat(int i, int* pa, int* pb) {
    const Step& cc = st(i);
    if (cc.kind != S_CONCAT || cc.axis != 1 || cc.in0 < 0 || cc.in1 < 0 || cc.in0 == cc.in1) return false;
    *pa = producer[cc.in0];
    *pb = producer[cc.in1];
    return *pa >= 0 && *pb >= 0 && *pa != *pb;
  }
  // The walk and the checks the fire passes share: Concat step i of biased e1 / e3 over one value S and one
  // plane, read by the Concat alone.  fm->sq is the biased step that alone reads the Concat -- with allow_pool,
  // through a 3x3 / stride-2 MaxPool (fm->pool) read once -- or -1.  What kinds of conv e1 / e3 / sq are, and
  // every size limit, are the passes' own checks.
  bool match_fire(int i, bool allow_pool, FireMatch* fm) {
    int pa, pb;
    if (!fire_concat(i, &pa, &pb)) return false;
    const Step &cc = st(i), &e1 = st(pa), &e3 = st(pb);
    if (e1.in0 != e3.in0 || e1.H != e3.H || e1.W != e3.W || e1.in2 < 0 || e3.in2 < 0) return false;
    if (!private_value(cc.in0) || !private_value(cc.in1)) return false;
    *fm = {i, pa, pb, -1, -1};
    int v = cc.out, qi = reader(v, size_t(i) + 1), pi = -1;
    if (qi >= 0 && allow_pool && pool_3x3_s2(st(qi)) && st(qi).in0 == v && private_value(st(qi).out)) {
      pi = qi;
      v = st(pi).out;
      qi = reader(v, size_t(pi) + 1);
    }
    if (qi >= 0 && private_value(cc.out) && st(qi).in0 == v && st(qi).in2 >= 0) {
      fm->pool = pi;
      fm->sq = qi;
    }
    return true;
  }
  // The rewrite of the fire passes: the squeeze fm.sq becomes the S_FIRE step over S that also computes e1,
  // e3, the Concat and the pool between, which leave the plan.  Without a squeeze (fm.sq < 0, pass 6b) the
  // Concat step becomes the S_FIRE and its output stays.
  ore_status take_fire(const FireMatch& fm, bool f16) {
    const bool sq = fm.sq >= 0;
    Step &t = st(sq ? fm.sq : fm.cc), &cc = st(fm.cc), &e1 = st(fm.e1), &e3 = st(fm.e3);
    const float* w1 = f16 ? fire_pack_f16(PACK_FIRE_F16, fm.e1) : fire_pack_f32(fm.e1);
    const float* w3 = f16 ? fire_pack_f16(PACK_FIRE_F16, fm.e3) : fire_pack_f32(fm.e3);
    const float* ws16 = f16 && sq ? fire_pack_f16(PACK_SQ_F16, fm.sq) : nullptr;
    if (!w1 || !w3 || (f16 && sq && !ws16))
      return err(m, ORE_ERR_HIP, f16 ? "f16 fire weight packing failed" : "fire weight packing failed");
    const double es = f16 ? 2.0 : 4.0;
    const std::string module = e1.name.substr(0, e1.name.find('/'));
    if (!sq) {  // the Concat is the output: its plane, no squeeze channels
      t.H = e1.H; t.W = e1.W; t.M = 0;
      t.in1 = t.in2 = -1;
    }
    t.kind = S_FIRE;
    t.fire.on = true;
    t.fire.f16 = f16;
    t.fire.pool = fm.pool >= 0;
    t.fire.H = e1.H;
    t.fire.W = e1.W;
    if (fm.pool >= 0) {
      Step& pl = st(fm.pool);
      t.fire.pwin = pl.win;
      val(pl.out).elided = true;
      nop(pl);
    }
    t.in0 = e1.in0;
    t.fire.C = e1.C;
    t.fire.E1 = e1.M;
    t.fire.E3 = e3.M;
    t.fire.w1 = w1;
    t.fire.w3 = w3;
    t.fire.ws16 = ws16;
    t.fire.b1 = val(e1.in2).cptr;
    t.fire.b3 = val(e3.in2).cptr;
    t.flops_per_img += e1.flops_per_img + e3.flops_per_img;
    t.bytes_per_img = es * double(e1.C * e1.H * e1.W) + es * double((sq ? t.M : e1.M + e3.M) * t.H * t.W);
    t.name = sq ? module + (fm.pool >= 0 ? "+pool+" : "+") + t.name : module + "/expand+concat";
    val(e1.out).elided = val(e3.out).elided = true;
    nop(e1); nop(e3);
    if (sq) {
      val(cc.out).elided = true;
      nop(cc);
    }
    return ORE_OK;
  }

  // MaxPool step pl (3x3 / stride 2, f32 NCHW input) feeding 1x1 conv cv fits pool_conv1x1_f32_kernel
  bool pool_squeeze_fits(const Step& pl, const Step& cv) const {
    if (!pool_3x3_s2(pl) || m->values[pl.in0].es != 4 || m->values[pl.in0].nhwc) return false;
    if (!conv_1x1_s1(cv) || !unfused(cv) || cv.plan.f16 || cv.plan.wino || cv.M > 64 || cv.C % 32 ||
        pl.win.pt > 2 || pl.win.pl > 2)
      return false;
    // pool_conv1x1_f32_kernel's own limits (run_conv_pool has no other kernel)
    return pool_conv1x1_f32_eligible(pool_conv_params(cv, pl.H, pl.W, pl.win));
  }
  // Winograd models: a fire module -> MaxPool -> squeeze runs cheaper as expand1x1 + Winograd
  // expand3x3 + the pooled squeeze (pool_squeeze) than in the direct-kernel fusions (fire4 -> pool3
  // -> fire5: 105 + 344 + pool and squeeze vs 713 us fused, profiles/r03_fusion_split.txt)
  bool wino_pool_split(const Step& e3, const Step& pl, int qi) const {
    return !eager() && m->wino && e3.has_wino && has(ORE_FUSE_POOL_SQUEEZE) && qi >= 0 &&
           private_value(pl.out) && m->steps[qi].in0 == pl.out && pool_squeeze_fits(pl, m->steps[qi]);
  }
  // the MaxPool pl in conv s's epilogue (passes 2 and 4): the pool's geometry, and the algorithmic bytes --
  // the conv's input + its pooled output (the pre-pool tensor never moves)
  void set_epool(Step& s, const Step& pl) {
    s.ep = {true, pl.kh, pl.kw, pl.sh, pl.sw, pl.win};
    s.bytes_per_img = double(val(s.in0).es) * double(s.C * s.H * s.W) +
                      double(val(pl.out).es) * double(s.M * pl.win.Ho * pl.win.Wo);
  }
  // Concat in place (passes 8a and 11): the producers of cc's inputs write channel slices of its output
  void place_concat(const Step& cc) {
    Value &a = val(cc.in0), &b = val(cc.in1);
    a.alias_of = cc.out; a.alias_ch = 0; a.slice = true;
    b.alias_of = cc.out; b.alias_ch = a.dims[1]; b.slice = true;
  }

  // (1) Conv -> Relu: the Relu in the conv epilogue
  void conv_relu() {
    if (!has(ORE_FUSE_CONV_RELU)) return;
    for (size_t i = 0; i < m->steps.size(); ++i) {
      Step& r = st(int(i));
      if (r.kind != S_RELU) continue;
      const int v = r.in0, p = producer[v];
      if (p < 0 || st(p).kind != S_CONV || st(p).relu || !private_value(v)) continue;
      st(p).out = r.out;
      st(p).relu = true;
      val(v).elided = true;
      producer[r.out] = p;
      nop(r);
    }
    recount();
  }

  // (2) Conv (-> Relu) -> MaxPool, the conv output read by the pool only: one launch when the
  // recomputed patch costs <= EPOOL_MAX_WORK x the conv's columns (f32 and f16 models)
  ore_status conv_pool() {
    if (!has(ORE_FUSE_CONV_POOL)) return ORE_OK;
    for (size_t i = 0; i < m->steps.size(); ++i) {
      Step& pl = st(int(i));
      if (pl.kind != S_MAXPOOL) continue;
      const int v = pl.in0, pc = producer[v];
      if (pc < 0 || !private_value(v)) continue;
      Step& cv = st(pc);
      if (cv.kind != S_CONV || !unfused(cv)) continue;
      if (cv.plan.f16 != (val(pl.out).es == 2 ? 1 : 0)) continue;  // f16 conv -> f16 pool only
      int a = 0, b = 0;
      const double work = epool_tile(cv.win.Ho, cv.win.Wo, pl.kh, pl.kw, pl.sh, pl.sw, pl.win, &a, &b);
      if (work == 0.0 || (work > EPOOL_MAX_WORK && !eager())) continue;
      // f32: pack the weights for the window kernel (pooled-conv variant 7) when its geometry fits
      if (!cv.plan.f16 && cv.kh == 7 && cv.kw == 7 && cv.sh == 2 && cv.sw == 2 && cv.in1 >= 0 &&
          (cv.C == 1 || cv.C == 3 || cv.C == 4) && cv.M > 32 && cv.M <= 128) {
        const int K = int(cv.C * cv.kh * cv.kw), M = int(cv.M);
        const float* w = val(cv.in1).cptr;
        cv.wc1 = pack_once(PACK_C1_F32, pc, c1_f32_pack_bytes(M, K),
                           [&](float* buf) { launch_pack_c1_f32(w, M, K, buf, m->ctx->stream); });
        if (!cv.wc1) return err(m, ORE_ERR_HIP, "conv weight packing failed");
      }
      set_epool(cv, pl);
      cv.out = pl.out;
      val(v).elided = true;
      producer[pl.out] = pc;
      nop(pl);
    }
    recount();
    return ORE_OK;
  }

  // (3) f32 fire module -> 3x3 / stride-2 MaxPool -> the next squeeze in one fire_pool_kernel launch
  // (ore_fire.hip): Concat(e1 1x1, e3 3x3 'same') (+ Relu), the pool the Concat's only reader, the
  // squeeze (1x1 + Relu, <= 64 channels) the pool's only reader.  Expand planes of >= FIRE_POOL_MIN_HW
  // pixels (SqueezeNet's fire4 -> pool3 -> fire5; at 27 x 27 fire8's expand3x3 runs Winograd, cheaper
  // than the direct K loop).  Runs before concat_pool, which would otherwise take the pattern.
  ore_status fire_pool_f32() {
    if (!has(ORE_FUSE_FIRE_POOL | ORE_FUSE_CONV_RELU | ORE_FUSE_CONCAT) || m->f16) return ORE_OK;
    for (size_t i = 0; i < m->steps.size(); ++i) {
      FireMatch fm;
      if (!match_fire(int(i), true, &fm) || fm.pool < 0 || fm.sq < 0) continue;
      const Step &e1 = st(fm.e1), &e3 = st(fm.e3), &pl = st(fm.pool), &q = st(fm.sq);
      if (!plain_1x1(e1) || !same_3x3(e3) || !plain_1x1(q)) continue;
      if (e1.M % 64 || e3.M % 64 || q.M > 64 || e1.C % 16 || q.C != e1.M + e3.M || pl.H != e1.H || pl.W != e1.W) continue;
      if (!eager() && (e1.H * e1.W < FIRE_POOL_MIN_HW || m->max_batch * e1.H * e1.W < FIRE_MIN_COLS)) continue;
      if (wino_pool_split(e3, pl, fm.sq)) continue;
      if (padded_plane(e1.H * e1.W) % 4 || val(e1.in0).es != 4) continue;  // 16-B input planes
      FireParams fp{};
      fp.H = int(e1.H); fp.W = int(e1.W);
      fp.Hp = int(pl.win.Ho); fp.Wp = int(pl.win.Wo); fp.ppt = int(pl.win.pt); fp.ppl = int(pl.win.pl);
      if (!fire_pool_plan(&fp) || !pool_windows_touch(pl)) continue;
      if (ore_status r = take_fire(fm, false)) return r;
    }
    recount();
    return ORE_OK;
  }

  // (4) Concat(e1, e3) -> 3x3 / stride-2 MaxPool, e1 / e3 Convs (+ Relu) read only by the Concat (f32):
  // each conv's pooled epilogue writes its channel slice of the pool output (a view appended to the
  // values), so neither the two conv outputs nor the concat reach HBM.  The MaxPool of a Concat is the
  // Concat of the per-slice MaxPools (the pool is per channel).  Conv planes of >= CONCAT_POOL_MIN_HW.
  void concat_pool() {
    if (!has(ORE_FUSE_CONCAT_POOL | ORE_FUSE_CONV_POOL | ORE_FUSE_CONCAT) || m->f16) return;
    for (size_t i = 0; i < m->steps.size(); ++i) {
      Step& pl = st(int(i));
      if (!pool_3x3_s2(pl)) continue;
      const int cv = pl.in0, ci = producer[cv];
      if (ci < 0 || !private_value(cv) || val(pl.out).is_output) continue;
      int pa, pb;
      if (!fire_concat(ci, &pa, &pb)) continue;
      Step& cc = st(ci);
      auto ok = [&](const Step& s, int v) {
        return s.kind == S_CONV && s.relu && unfused(s) && !s.plan.f16 && private_value(v) && val(v).ndim == 4;
      };
      if (!ok(st(pa), cc.in0) || !ok(st(pb), cc.in1)) continue;
      int t1 = 0, t2 = 0;
      const Step& sa = st(pa);
      if (epool_tile(sa.win.Ho, sa.win.Wo, pl.kh, pl.kw, pl.sh, pl.sw, pl.win, &t1, &t2) == 0.0) continue;
      if (sa.win.Ho * sa.win.Wo < CONCAT_POOL_MIN_HW && !eager()) continue;
      if (wino_pool_split(st(pb), pl, reader(pl.out, i + 1))) continue;
      const int pout = pl.out;
      const int64_t Hp = val(pout).dims[2], Wp = val(pout).dims[3];
      const int pes = val(pout).es;
      const std::string pname = val(pout).name;
      int64_t ch0 = 0;
      for (int half = 0; half < 2; ++half) {
        const int si = half ? pb : pa, src = half ? cc.in1 : cc.in0;
        Value v;
        v.name = pname + (half ? "#slice1" : "#slice0");
        v.ndim = 4;
        v.dims[0] = 1; v.dims[1] = val(src).dims[1]; v.dims[2] = Hp; v.dims[3] = Wp;
        v.es = pes;
        v.alias_of = pout; v.alias_ch = ch0; v.slice = true;
        ch0 += v.dims[1];
        m->values.push_back(v);
        producer.push_back(si);
        const int vid = int(m->values.size()) - 1;
        Step& s = st(si);
        val(src).elided = true;
        set_epool(s, pl);
        s.out = vid;
      }
      val(cv).elided = true;
      producer[pout] = pa;
      nop(cc);
      nop(pl);
    }
    recount();
  }

  // (5) fire module + the next squeeze in one launch (f32, fire_kernel): Concat(e1, e3) whose inputs
  // are a 1x1 and a 3x3 'same' Conv (+ Relu) of one value S, read only by a 1x1 Conv (+ Relu) with at
  // most 64 output channels
  ore_status fire_f32() {
    if (!has(ORE_FUSE_FIRE | ORE_FUSE_CONV_RELU | ORE_FUSE_CONCAT) || m->f16) return ORE_OK;
    for (size_t i = 0; i < m->steps.size(); ++i) {
      FireMatch fm;
      if (!match_fire(int(i), false, &fm) || fm.sq < 0) continue;
      const Step &e1 = st(fm.e1), &e3 = st(fm.e3), &q = st(fm.sq);
      if (!plain_1x1(e1) || !same_3x3(e3) || !plain_1x1(q)) continue;
      if (e1.M % 64 || e3.M % 64 || q.M > 64 || e1.C % 16 || q.C != e1.M + e3.M) continue;
      if (!eager() && m->max_batch * e1.H * e1.W < FIRE_MIN_COLS) continue;
      // Winograd expand3x3 (f32 models with Winograd on): the split is cheaper on small planes with wide inputs
      if (!eager() && m->wino && e3.has_wino && e1.H * e1.W < FIRE_POOL_MIN_HW && e1.C >= WINO_SPLIT_MIN_C) continue;
      if (padded_plane(e1.H * e1.W) % 4 || val(e1.in0).es != 4) continue;  // 16-B planes (layout below)
      if (ore_status r = take_fire(fm, false)) return r;
    }
    recount();
    return ORE_OK;
  }

  // (6) f16 models: the same fire module + next squeeze pattern in one fire_f16_kernel launch
  // (ore_fire_f16.hip): expand1x1 / expand3x3 (+ Relu) on 16-B NHWC gathers, C % 16 == 0 and <= 64,
  // expands in 32-channel chunks, the squeeze <= 64 channels; bit-identical to the three
  // conv_f16_kernel launches.  With a 3x3 / stride-2 MaxPool between the Concat and the squeeze
  // (SqueezeNet fire4 -> pool3 -> fire5, fire8 -> pool5 -> fire9) the pooled kernel takes all four
  // steps (ORE_FUSE_FIRE_POOL; bit-identical to the three convs + maxpool_nhwc_kernel)
  ore_status fire_f16() {
    if (!has(ORE_FUSE_FIRE | ORE_FUSE_CONV_RELU) || !m->f16) return ORE_OK;
    const bool pooled = has(ORE_FUSE_FIRE_POOL);
    for (size_t i = 0; i < m->steps.size(); ++i) {
      FireMatch fm;
      if (!match_fire(int(i), pooled, &fm) || fm.sq < 0) continue;
      const Step &e1 = st(fm.e1), &e3 = st(fm.e3), &q = st(fm.sq);
      if (!vec16(e1) || !conv_1x1_s1(e1) || !vec16(e3) || !conv_3x3_same(e3) || !vec16(q) || !conv_1x1_s1(q)) continue;
      if (e1.C % 16 || e1.C > 64 || e1.M % 32 || e3.M % 32 || q.M % 8 || q.M > 64 || q.C != e1.M + e3.M) continue;
      if (fm.pool < 0 && fire_f16_lds_bytes(int(e1.C), int(e1.H), int(e1.W)) > FIRE_F16_LDS_MAX) continue;
      if (fm.pool >= 0) {  // a band shape must fit (fire_pool_f16_plan) and every window touch the image
        const Step& pl = st(fm.pool);
        FireF16Params fp{};
        fp.C = int(e1.C); fp.H = int(e1.H); fp.W = int(e1.W);
        fp.Hp = int(pl.win.Ho); fp.Wp = int(pl.win.Wo); fp.ppt = int(pl.win.pt); fp.ppl = int(pl.win.pl);
        if (pl.H != e1.H || pl.W != e1.W || !fire_pool_f16_plan(&fp) || !pool_windows_touch(pl)) continue;
      }
      if (val(e1.in0).es != 2) continue;
      if (ore_status r = take_fire(fm, true)) return r;
    }
    recount();
    return ORE_OK;
  }

  // (6b) f16 models: a fire module whose Concat no squeeze takes (SqueezeNet fire9, read by conv10):
  // expand1x1 + expand3x3 (+ Relu) + Concat in one fire_f16_kernel<NKC, 0> launch that writes the
  // Concat (NHWC) -- the two conv_f16 launches' arithmetic, bit-identical
  ore_status fire_f16_concat() {
    if (!has(ORE_FUSE_FIRE | ORE_FUSE_CONV_RELU) || !m->f16) return ORE_OK;
    for (size_t i = 0; i < m->steps.size(); ++i) {
      FireMatch fm;
      if (!match_fire(int(i), false, &fm)) continue;
      const Step &e1 = st(fm.e1), &e3 = st(fm.e3);
      if (!vec16(e1) || !conv_1x1_s1(e1) || !vec16(e3) || !conv_3x3_same(e3) || e1.C != e3.C) continue;
      if (e1.C % 16 || e1.C > 64 || e1.M % 32 || e3.M % 32 || e1.M + e3.M > 512) continue;
      if (fire_f16_lds_bytes(int(e1.C), int(e1.H), int(e1.W)) > FIRE_F16_LDS_MAX || val(e1.in0).es != 2) continue;
      fm.pool = fm.sq = -1;  // whatever reads the Concat stays
      if (ore_status r = take_fire(fm, true)) return r;
    }
    recount();
    return ORE_OK;
  }

  // (7) the first conv + pool whose pooled map is read only by a small 1x1 conv (+ Relu) takes that
  // conv into its launch (SqueezeNet's conv1 + pool1 + fire2/squeeze1x1; the pooled map is never
  // stored).  Bit-identical to the separate squeeze (the same k-ordered chain over the same pooled
  // values).  f16: conv_pair_pool_f16_kernel SQ (<= 32 channels); f32: the window kernel (pooled-conv
  // variant 7, <= 16 channels).
  ore_status first_squeeze() {
    if (!has(ORE_FUSE_FIRST_SQUEEZE | ORE_FUSE_CONV_POOL | ORE_FUSE_CONV_RELU)) return ORE_OK;
    for (size_t i = 0; i < m->steps.size(); ++i) {
      Step& cv = st(int(i));
      if (cv.kind != S_CONV || !cv.ep.on || cv.sq.on || !private_value(cv.out)) continue;
      const bool f16 = cv.plan.f16 != 0;
      if (f16 ? (cv.plan.xmode != F16_X_NHWC_PAIR || cv.kh != 7 || cv.kw != 7 || cv.sh != 2 || cv.sw != 2 ||
                 cv.win.pl % 2 || cv.C > 4 || (cv.M != 64 && cv.M != 96))
              : (!cv.wc1 || cv.C != 3 || cv.M != 96))
        continue;
      const int qi = reader(cv.out, i + 1);
      if (qi < 0) continue;
      Step& q = st(qi);
      if (!conv_1x1_s1(q) || !q.relu || !unfused(q) || q.in0 != cv.out || q.C != cv.M || q.in2 < 0 || q.in1 < 0 ||
          !val(q.in1).cptr)
        continue;
      if (f16 ? (!q.plan.f16 || q.plan.xmode != F16_X_NHWC_VEC || q.M > 32 || q.M % 8) : (q.plan.f16 || q.M > 16))
        continue;
      // f16: launch_fire_pack_f16's layout; f32: the ONNX [M][C][1][1] = [M][K] as it is
      const float* w = f16 ? fire_pack_f16(PACK_C1SQ_F16, qi) : val(q.in1).cptr;
      if (!w) return err(m, ORE_ERR_HIP, "squeeze weight packing failed");
      cv.sq = {true, w, val(q.in2).cptr, q.M};
      // f32, untuned: the band walker for batches that give every CU an image, where its geometry allows it
      // (one workgroup per band of an image; it bands smaller batches but the window kernel's patches fill
      // the chip better there), else the window kernel; an autotuned / set choice (epv 7 or 8) is kept
      if (!f16 && cv.plan.epv != EPOOL_BAND_VARIANT && cv.plan.epv != EPOOL_WIN_VARIANT)
        cv.plan.epv = m->max_batch >= 128 && band_step(cv) ? EPOOL_BAND_VARIANT : EPOOL_WIN_VARIANT;
      // f16: the band walker (one workgroup per image) for batches that give every CU an image, else the
      // patch kernel; an autotuned / set choice is kept
      if (f16 && cv.plan.epv != C1_BAND_F16_VARIANT && cv.plan.epv != C1_PATCH_F16_VARIANT)
        cv.plan.epv = m->max_batch >= 128 && band_f16_step(cv) ? C1_BAND_F16_VARIANT : C1_PATCH_F16_VARIANT;
      val(cv.out).elided = true;
      cv.out = q.out;
      cv.flops_per_img += q.flops_per_img;
      cv.bytes_per_img = double(val(cv.in0).es) * double(cv.C * cv.H * cv.W) + (f16 ? 2.0 : 4.0) * double(q.M * q.H * q.W);
      cv.name = cv.name + "+" + q.name;
      nop(q);
    }
    recount();
    return ORE_OK;
  }

  // (8) f32: a 3x3 / stride-2 MaxPool left standing (SqueezeNet pool5) whose only reader is a 1x1 Conv
  // (+ Relu) with <= 64 channels runs inside that conv (pool_conv1x1_f32_kernel, the pooled map never
  // stored).  Bit-identical to the MaxPool kernel + the conv.
  void pool_squeeze() {
    if (!has(ORE_FUSE_POOL_SQUEEZE) || m->f16) return;
    for (size_t i = 0; i < m->steps.size(); ++i) {
      Step& pl = st(int(i));
      if (!pool_3x3_s2(pl)) continue;
      const int v = pl.out;
      if (!private_value(v)) continue;
      const int ci = reader(v, i + 1);
      if (ci < 0) continue;
      Step& cv = st(ci);
      if (cv.in0 != v || !pool_squeeze_fits(pl, cv)) continue;
      cv.pin = {true, pl.H, pl.W, pl.sh, pl.sw, pl.win, {}};
      cv.in0 = pl.in0;
      cv.bytes_per_img = 4.0 * double(pl.C * pl.H * pl.W) + 4.0 * double(cv.M * cv.H * cv.W);
      cv.name = pl.name + "+" + cv.name;
      val(v).elided = true;
      nop(pl);
    }
    recount();
  }

  // (8a) f32: the pooled squeeze of (8) whose pool reads Concat(e1, e3), e1 a 1x1 conv + Relu of 32 / 64
  // channels read only by the Concat (SqueezeNet fire4 -> pool3 -> fire5, fire8 -> pool5 -> fire9 under
  // Winograd, wino_pool_split): e1 is recomputed inside pool_conv1x1_f32_kernel from its own input, so
  // its map (fire4: 128 x 54 x 54 floats per image) is neither written nor read back.  The Concat is
  // placed in memory here (e3 writes its slice; e1's slice is never materialised).  Bit-identical: the
  // same k-ordered MFMA chain, bias and Relu as the streaming 1x1 conv, the max of the same nine values.
  // Not under ORE_KEEP_VALUES (e1's output would not exist to read back).
  void pool_expand() {
    if (!has(ORE_FUSE_POOL_EXPAND | ORE_FUSE_POOL_SQUEEZE | ORE_FUSE_CONV_RELU | ORE_FUSE_CONCAT) ||
        has(ORE_KEEP_VALUES) || m->f16)
      return;
    for (size_t i = 0; i < m->steps.size(); ++i) {
      Step& cv = st(int(i));
      if (cv.kind != S_CONV || !cv.pin.on || cv.pin.e1.on || cv.in0 < 0) continue;
      const int ci = producer[cv.in0];
      int pa, pb;
      if (ci < 0 || !fire_concat(ci, &pa, &pb)) continue;
      Step &cc = st(ci), &e1 = st(pa), &e3 = st(pb);
      // C1 = 64 (fire8 -> pool5) holds 48 B registers per lane and halves the launch's occupancy: 218 us
      // against 74 + 106 for the separate launches (profiles/r05_ab_pool_expand.txt), so 32 only unless eager
      if (!eager() && e1.C != 32) continue;
      if (!plain_1x1(e1) || e1.in2 < 0 || !e1.wp || (e1.C != 32 && e1.C != 64) || e1.M % 16 || e1.H != cv.pin.H ||
          e1.W != cv.pin.W || e3.kind != S_CONV || !unfused(e3))
        continue;
      // the Concat's only reader is this launch: e1's slice of it is never written
      if (!private_value(cc.in0) || !private_value(cc.in1) || !private_value(cc.out) || val(e1.in0).es != 4 ||
          val(e1.in0).nhwc || val(cc.in0).alias_of >= 0 || val(cc.in1).alias_of >= 0)
        continue;
      PoolConvParams q = pool_conv_params(cv, cv.pin.H, cv.pin.W, cv.pin.win);  // the kernel's limits with e1 inside
      q.s = q.w1 = q.b1 = e1.wp; q.C1 = int(e1.C); q.E1 = int(e1.M); q.w1_Mp = e1.plan.Mp; q.s_ps = q.H * q.W;
      if (!pool_conv1x1_f32_eligible(q)) continue;
      cv.pin.e1 = {true, e1.wp, val(e1.in2).cptr, e1.C, e1.M, e1.plan.Mp};
      cv.in3 = e1.in0;
      // work: e1 per band row it stages (2 PR + 1 input rows per PR pooled rows, neighbouring bands share one)
      const int pr = pool_conv1x1_f32_rows(int(cv.pin.win.Wo));
      const double rows = double((cv.pin.win.Ho + pr - 1) / pr * (2 * pr + 1));
      cv.mfma_flops_per_img = (cv.mfma_flops_per_img < 0 ? cv.flops_per_img : cv.mfma_flops_per_img) +
                              e1.flops_per_img * rows / double(e1.H);
      cv.flops_per_img += e1.flops_per_img;
      cv.bytes_per_img = 4.0 * double((cv.C - e1.M + e1.C) * cv.pin.H * cv.pin.W) + 4.0 * double(cv.M * cv.H * cv.W);
      cv.name = e1.name + "+" + cv.name;
      place_concat(cc);
      val(cc.in0).elided = true;  // e1's slice is never written
      nop(cc);
      nop(e1);
    }
    recount();
  }

  // (8b) f16: a 1x1 conv (+ Relu) whose only reader is GlobalAveragePool runs with the GAP in its
  // epilogue (conv1x1_gap_f16_kernel: SqueezeNet conv10 -> relu10 -> pool10; the 87 MB map is never
  // stored).  Bit-identical to conv_f16 + gap_nhwc_kernel.  Not under ORE_KEEP_VALUES (the conv output
  // would not exist to read back).
  ore_status conv_gap() {
    if (!has(ORE_FUSE_CONV_GAP) || has(ORE_KEEP_VALUES)) return ORE_OK;
    for (size_t i = 0; i < m->steps.size(); ++i) {
      Step& g = st(int(i));
      if (g.kind != S_GAP) continue;
      const int v = g.in0;
      if (v < 0 || !private_value(v) || producer[v] < 0) continue;
      Step& cv = st(producer[v]);
      if (!conv_1x1_s1(cv) || cv.out != v || !unfused(cv) || cv.H * cv.W > 256) continue;
      if (m->f16) {
        if (!val(v).nhwc || val(v).es != 2 || !cv.plan.f16 || cv.plan.xmode != F16_X_NHWC_VEC || cv.C % 64 != 0) continue;
      } else {  // f32: conv1x1_gap_f32_kernel (the conv's weights in launch_pack_cg_f32's layout)
        if (val(v).nhwc || val(v).es != 4 || cv.plan.f16 || cv.plan.wino || cv.C % 32 != 0 || val(cv.in0).es != 4) continue;
        const int M = int(cv.M), K = int(cv.C);
        const float* w = val(cv.in1).cptr;
        cv.wc1 = pack_once(PACK_CG_F32, producer[v], cg_f32_pack_bytes(M, K),
                           [&](float* buf) { launch_pack_cg_f32(w, M, K, buf, m->ctx->stream); });
        if (!cv.wc1) return err(m, ORE_ERR_HIP, "conv + GAP weight packing failed");
      }
      cv.gap = true;
      cv.out = g.out;
      cv.bytes_per_img = (m->f16 ? 2.0 : 4.0) * double(cv.C * cv.H * cv.W) + 4.0 * double(cv.M);
      cv.name = cv.name + "+" + g.name;
      val(v).elided = true;
      nop(g);
    }
    recount();
    return ORE_OK;
  }

  // (9) algorithm selection, a load-time rule (never by timing): f32 models with Winograd on run every
  // 3x3 / stride-1 / pad-1 conv not taken by a direct-kernel fusion by Winograd F(2x2, 3x3)
  void select_algorithms() {
    for (auto& s : m->steps) {
      if (m->wino && s.kind == S_CONV && s.has_wino && !s.pin.on && !s.ep.on) {
        s.plan = s.plan_wino;
        s.wp = s.wp_wino;
        s.ktab = nullptr;
        // MFMA work issued: 16 positions x C x M per 2x2 output tile (the direct conv's 36 C M / 4 pixels)
        s.mfma_flops_per_img = 2.0 * 16.0 * double(s.C) * double(s.M) * double((s.win.Ho + 1) / 2) *
                               double((s.win.Wo + 1) / 2);
      }
    }
  }

  // (10) Dropout / activation Reshape as aliases
  void alias_copies() {
    if (!has(ORE_FUSE_ALIAS)) return;
    for (auto& s : m->steps) {
      if (s.kind != S_COPY) continue;
      val(s.out).alias_of = s.in0;  // resolved to the root at run time; requires a contiguous source
      s.kind = S_NOP;
    }
  }

  // (11) Concat in place: producers write channel slices of the concat buffer
  void concat_in_place() {
    if (!has(ORE_FUSE_CONCAT)) return;
    for (auto& s : m->steps) {
      if (s.kind != S_CONCAT || s.axis != 1 || s.in0 == s.in1) continue;
      const Value &a = val(s.in0), &b = val(s.in1);
      const int pa = producer[s.in0], pb = producer[s.in1];
      if (pa < 0 || pb < 0 || !strided_writer(st(pa)) || !strided_writer(st(pb))) continue;
      if (a.uses != 1 || b.uses != 1 || a.is_output || b.is_output || a.alias_of >= 0 || b.alias_of >= 0) continue;
      place_concat(s);
      s.kind = S_NOP;
    }
  }

  int root(int id) const { return ore::root(m, id); }

  // (12) layout: an activation touched only by Conv / MaxPool kernels (and f32 GlobalAveragePool)
  // gets channel planes padded to a multiple of 32 floats (128-B aligned rows for the conv epilogue
  // and the 1x1 gathers) when that costs <= 5 % extra columns; everything else stays dense NCHW.
  ore_status layout_planes() {
    for (auto& v : m->values) {  // aliases of aliases must stay contiguous views (Reshape / Dropout of a slice)
      if (v.alias_of < 0 || v.slice) continue;
      if (val(v.alias_of).slice) return err(m, ORE_ERR_INVALID, "internal: alias of a strided view (" + v.name + ")");
    }
    std::vector<char> dense(m->values.size(), 0);
    for (const Step& s : m->steps) {
      if (s.kind == S_NOP) continue;
      const bool ok = s.kind == S_CONV || s.kind == S_FIRE || s.kind == S_MAXPOOL || (s.kind == S_GAP && !val(s.in0).nhwc);
      for (int id : {s.in0, s.in2, s.in3, s.out})
        if (id >= 0 && !val(id).is_const && !ok) dense[root(id)] = 1;
      if (s.in1 >= 0 && !val(s.in1).is_const) dense[root(s.in1)] = 1;
    }
    // a contiguous view (Dropout / Reshape alias) keeps its root's planes only as a 4-D
    // intermediate; as a graph output or a reshaped 2-D value it needs the dense layout
    for (size_t id = 0; id < m->values.size(); ++id) {
      const Value& v = m->values[id];
      if (v.alias_of >= 0 && !v.slice && (v.is_output || v.ndim != 4)) dense[root(int(id))] = 1;
    }
    for (size_t id = 0; id < m->values.size(); ++id) {
      Value& v = m->values[id];
      if (v.is_const || v.ndim != 4 || v.alias_of >= 0) continue;
      if (v.nhwc) {  // channels-last f16: dense pixels of dims[1] channels
        v.ps = v.dims[1];
        continue;
      }
      const int64_t P = v.dims[2] * v.dims[3];
      const bool pad = has(ORE_FUSE_CONCAT) && !dense[id] && !v.is_input && !v.is_output;
      v.ps = pad ? padded_plane(P) : P;
    }
    for (size_t id = 0; id < m->values.size(); ++id) {  // views inherit the plane stride of their root
      Value& v = m->values[id];
      if (v.alias_of < 0 || v.ndim != 4) continue;
      const Value& r = val(root(int(id)));
      v.ps = r.ps;
      if (v.nhwc != r.nhwc) return err(m, ORE_ERR_INVALID, "internal: view of a different layout (" + v.name + ")");
      if (!v.slice && r.ps != (r.nhwc ? r.dims[1] : r.dims[2] * r.dims[3]) &&
          (v.is_output || v.dims[2] * v.dims[3] != r.dims[2] * r.dims[3]))
        return err(m, ORE_ERR_INVALID, "internal: dense alias of a padded value (" + v.name + ")");
    }
    return ORE_OK;
  }

  // (13) one device arena: every materialised root value gets a slot sized for run_batch, slots reused
  // by liveness (first fit over [first write, last read] intervals)
  ore_status assign_arena() {
    const int nsteps = int(m->steps.size());
    for (int i = 0; i < nsteps; ++i) {
      const Step& s = m->steps[i];
      if (s.kind == S_NOP) continue;
      for (int id : {s.in0, s.in1, s.in2, s.in3}) {
        if (id < 0 || val(id).is_const) continue;
        Value& r = val(root(id));
        if (r.first < 0) r.first = i;
        r.last = std::max(r.last, i);
      }
      if (s.out >= 0) {
        Value& r = val(root(s.out));
        if (r.first < 0 || r.first > i) r.first = i;
        r.last = std::max(r.last, i);
      }
    }
    // the model output stays live to the end (it may be copied out after the last step)
    if (m->output_value >= 0) val(root(m->output_value)).last = nsteps;
    // so does the map conv's input while the class maps are on: the kernel behind the top-k launch reads it
    if (m->cam_buf && m->cam_in >= 0) val(root(m->cam_in)).last = nsteps;

    struct Slot { int64_t off, size; int first, last; };
    std::vector<int> roots;
    for (size_t id = 0; id < m->values.size(); ++id) {
      const Value& v = m->values[id];
      if (v.is_const || v.is_input || v.alias_of >= 0 || v.elided || v.first < 0) continue;
      roots.push_back(int(id));
    }
    // the kernels address a launch's activations through buffer resources and 32-bit offsets: one pass
    // of the graph covers run_batch images, the largest batch whose every value (the caller's input and
    // output included) and the f16 input conversion stay below RUN_LIMIT bytes; ore_model_run runs
    // larger batches in image chunks (config 4's 2048 images per GPU: fire4's concat is 3 MB per image)
    constexpr int64_t RUN_LIMIT = (int64_t(1) << 31) - (int64_t(1) << 21);
    int64_t per_img_max = 0;
    for (size_t id = 0; id < m->values.size(); ++id) {
      const Value& v = m->values[id];
      if (v.is_const || v.alias_of >= 0 || v.elided || (v.first < 0 && !v.is_input)) continue;
      per_img_max = std::max(per_img_max, v.image_stride() * v.es);
    }
    int64_t xcvt_img = 0;
    for (const Step& s : m->steps)
      if (s.kind == S_CONV && s.plan.f16 && s.plan.xmode == F16_X_NHWC_PAIR) xcvt_img = std::max(xcvt_img, s.H * s.W * 4 * 2);
    per_img_max = std::max(per_img_max, xcvt_img);
    if (per_img_max >= RUN_LIMIT) return err(m, ORE_ERR_UNSUPPORTED, "one image's activations exceed 2 GiB");
    m->run_batch = std::min<int64_t>(m->max_batch, per_img_max > 0 ? RUN_LIMIT / per_img_max : m->max_batch);
    if (xcvt_img && size_t(xcvt_img * m->run_batch) > m->xcvt_bytes) {
      if (m->xcvt) (void)hipFree(m->xcvt);
      m->xcvt = nullptr;
      m->xcvt_bytes = 0;
      if (device_alloc(m->ctx, &m->xcvt, size_t(xcvt_img * m->run_batch), true) != hipSuccess)
        return err(m, ORE_ERR_OOM, "input conversion buffer allocation failed");
      m->xcvt_bytes = size_t(xcvt_img * m->run_batch);
    }
    std::sort(roots.begin(), roots.end(), [&](int a, int b) { return val(a).image_stride() > val(b).image_stride(); });
    std::vector<Slot> placed;
    int64_t arena = 0;
    for (int id : roots) {
      Value& v = val(id);
      const int64_t size = slot_extent(m, v);
      std::vector<std::pair<int64_t, int64_t>> busy;  // slots whose lifetimes overlap this one
      for (auto& s : placed)
        if (has(ORE_KEEP_VALUES) || !(s.last < v.first || v.last < s.first)) busy.push_back({s.off, s.off + s.size});
      std::sort(busy.begin(), busy.end());
      int64_t off = 0;
      for (auto& b : busy) {
        if (off + size <= b.first) break;
        off = std::max(off, b.second);
      }
      v.arena_off = off;
      placed.push_back({off, size, v.first, v.last});
      arena = std::max(arena, off + size);
    }
    if (size_t(arena) > m->arena_bytes) {
      if (m->arena_alloc) (void)hipFree(m->arena_alloc);
      m->arena = m->arena_alloc = nullptr;
      m->arena_bytes = 0;
      if (arena > 0 &&
          device_alloc(m->ctx, reinterpret_cast<void**>(&m->arena_alloc), size_t(arena) + ARENA_LEAD, true) != hipSuccess)
        return err(m, ORE_ERR_OOM, "arena allocation of " + std::to_string(arena) + " bytes failed");
      if (m->arena_alloc) m->arena = m->arena_alloc + ARENA_LEAD;
      m->arena_bytes = size_t(arena);
    }
    m->exec_steps.clear();
    for (int i = 0; i < nsteps; ++i)
      if (m->steps[i].kind != S_NOP) m->exec_steps.push_back(i);
    return ORE_OK;
  }

  // (14) independent neighbours for the two-stream issue (ore_model_set_streams): B reads nothing A
  // writes, and no byte range A or B writes overlaps one the other reads or writes (arena slots are
  // shared by liveness, so check the memory)
  void pair_steps() {
    m->pair_next.assign(m->exec_steps.size(), 0);
    auto span = [&](int id, int64_t* lo, int64_t* hi) {  // arena byte range of a value's root
      const Value& v = val(root(id));
      if (v.is_const || v.arena_off < 0) return false;
      *lo = v.arena_off;
      *hi = v.arena_off + v.image_stride() * m->run_batch * v.es;
      return true;
    };
    auto overlap = [&](int a, int b) {
      if (a < 0 || b < 0 || val(a).is_const || val(b).is_const) return false;
      const int ra = root(a), rb = root(b);
      if (val(ra).is_input || val(rb).is_input) return false;  // never written
      if (ra == rb) {  // channel slices of one buffer: disjoint unless the same slice
        const Value &va = val(a), &vb = val(b);
        if (va.slice && vb.slice) return va.alias_ch < vb.alias_ch + vb.dims[1] && vb.alias_ch < va.alias_ch + va.dims[1];
        return true;
      }
      if (val(ra).is_output || val(rb).is_output) return true;  // conservative (may live in the arena)
      int64_t a0, a1, b0, b1;
      if (!span(a, &a0, &a1) || !span(b, &b0, &b1)) return false;
      return a0 < b1 && b0 < a1;
    };
    for (size_t k = 0; k + 1 < m->exec_steps.size(); ++k) {
      if (k > 0 && m->pair_next[k - 1]) continue;  // pairs only
      const Step &A = st(m->exec_steps[k]), &B = st(m->exec_steps[k + 1]);
      bool ok = A.out >= 0 && B.out >= 0;
      for (int bi : {B.in0, B.in1, B.in2, B.in3}) ok = ok && !overlap(bi, A.out);
      for (int ai : {A.in0, A.in1, A.in2, A.in3}) ok = ok && !overlap(ai, B.out);
      ok = ok && !overlap(A.out, B.out);
      m->pair_next[k] = ok ? 1 : 0;
    }
  }

  // (15) gather tables: they depend on the input's plane stride
  ore_status gather_tables() {
    for (const Step& s : m->steps) {
      if (s.kind != S_CONV || !s.ktab) continue;
      const Value& xv = val(s.in0);
      int2* kt = const_cast<int2*>(s.ktab);
      if (s.plan.f16 && s.plan.xmode != F16_X_NCHW32)
        launch_ktab_nhwc(kt, s.plan.xmode, int(s.C), int(s.kh), int(s.kw),
                         s.plan.xmode == F16_X_NHWC_PAIR ? 4 : int(xv.ps), int(s.W), m->ctx->stream);
      else
        launch_ktab(kt, int(s.C * s.kh * s.kw), int(s.kh), int(s.kw), int(xv.ps ? xv.ps : s.H * s.W), int(s.W),
                    m->ctx->stream);
    }
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(m->ctx->stream) != hipSuccess)
      return err(m, ORE_ERR_HIP, "gather table build failed");
    return ORE_OK;
  }
};

}  // namespace

ore_status plan(ore_model* m) {
  m->steps = m->base_steps;
  if (!m->n_base_values) m->n_base_values = m->values.size();
  m->values.resize(m->n_base_values);  // drop the previous plan's views
  for (auto& v : m->values) {
    v.alias_of = -1; v.alias_ch = 0; v.slice = false; v.ps = 0; v.elided = false; v.arena_off = -1;
    v.nhwc = !v.is_const && v.es == 2 && v.ndim == 4;
    v.first = v.last = -1;
  }
  count_uses(m, m->steps);
  Planner p{m, std::vector<int>(m->values.size(), -1)};
  for (size_t i = 0; i < m->steps.size(); ++i)
    if (m->steps[i].out >= 0 && m->steps[i].kind != S_NOP) p.producer[m->steps[i].out] = int(i);
  p.conv_relu();
  if (ore_status st = p.conv_pool()) return st;
  if (ore_status st = p.fire_pool_f32()) return st;
  p.concat_pool();
  if (ore_status st = p.fire_f32()) return st;
  if (ore_status st = p.fire_f16()) return st;
  if (ore_status st = p.fire_f16_concat()) return st;
  if (ore_status st = p.first_squeeze()) return st;
  p.pool_squeeze();
  p.pool_expand();
  if (ore_status st = p.conv_gap()) return st;
  p.select_algorithms();
  p.alias_copies();
  p.concat_in_place();
  if (ore_status st = p.layout_planes()) return st;
  if (ore_status st = p.assign_arena()) return st;
  p.pair_steps();
  return p.gather_tables();
}

}  // namespace ore
