// Candidate search for the rerank, kernel 1: the best gallery row of every bin of B consecutive rows
// per query, under ore_topk_f32's order (ore_topk_key.h) of the format's score -- the partial reduce of Chern et al.,
// "TPU-KNN" (2022).  A template over ore_nearest.h's format types, instantiated by ore_nearest_f16.hip and
// ore_nearest_i8.hip; the c best of the winners are picked by ore_nearest_bins.hip.
//
// Split.  grid = (ceil(n / 64) query tiles, S gallery segments), four waves.  A segment is a whole number of 4 B rows
// and wave w walks the quarter [jbeg + w wr, jbeg + (w + 1) wr) of it on its own, 32 rows per step as two A operands
// of 16 rows against the 64 queries of the tile: the streaming kernel's eight MFMAs per k-group and 32 accumulators,
// but the four waves are a quarter segment apart instead of 32 rows.  wr is a multiple of B, so a bin is R = B / 32
// consecutive steps of one wave and no wave ever needs another wave's scores.  Every wave runs the same number of
// steps -- wave 0's, whose range has the most rows below G, in whole bins -- with the rows from G on masked, so the
// chunked tile's barriers stay uniform.
//
// Data movement.  The K loop is the streaming kernel's: the gallery straight into the A operand through the NS_PF deep
// register ring that runs on across the steps, straight-line turns, masked safe-address loads, the scale loads in
// slot 0 of a turn, the query tile converted once and resident in LDS up to NB_RES d, staged in chunks of F::DC d
// between two barriers per chunk above.  LDS holds the tile and the format's QX bytes per query, nothing else: with
// the tile resident the step loop has no barrier at all.
//
// Running best.  Lane l holds, per query block, the scores of rows 16 rb + 4 (l >> 4) + i of the step.  It visits them
// rb-major, i-minor, step after step: its own rows in ascending order.  So per query block it keeps one (image, row)
// pair and replaces it on a strictly larger image; the first of equal images stays.  The pair starts at (0, the lane's
// first row of the bin): an all-NaN bin (image 0 throughout) keeps its lowest row.  A row from G on has its image made
// 0 and so replaces nothing; a lane whose first row of the bin is not there holds no key (0).
//
// Bin end.  Lanes l, l ^ 16, l ^ 32, l ^ 48 share a query: their four 64-bit keys are combined by wave_max's last two
// steps (v_permlane16_swap, v_permlane32_swap) and lane l stores the key of query block l >> 4: 64 lanes, 64 queries.
//
// Winner buffer: keys [n][NB], query-major, because kernel 2 is one workgroup per query that walks its row several
// times: those reads are contiguous.  The price is here: a store instruction's 64 lanes write 64 different rows,
// 8 bytes each, NB keys apart; the eight bins of a 64-byte sector come from eight consecutive bin ends of the same
// wave and meet in the L2.  One such store per R steps of 64 (f16: 16 R, int8: 8 R) MFMAs per k-group of D.
#pragma once
#include "ore_nearest.h"

namespace ore {

namespace {

struct NearestBinsArgs {
  const float* q;
  const void* g;        // [G][D] in the kernel's format
  const float* scales;  // [G], int8 gallery; null otherwise
  u64* win;             // [n][NB]
  long long q_stride, G, NB, seg_rows;  // seg_rows: gallery rows per segment, a multiple of 4 B
  int n, D, lgR;                        // B = 32 << lgR
};

// the largest resident D: two workgroups' LDS on a compute unit, so that one's epilogue runs under the other's MFMAs
template <class F>
__host__ __device__ constexpr int nb_chunk(int D, int res) {
  return D <= res ? (D + F::KG * NS_PF - 1) / (F::KG * NS_PF) * (F::KG * NS_PF) : F::DC;
}
template <class F>
__host__ __device__ constexpr size_t nb_lds_bytes(int D, int res) {
  return size_t(NN_QT) * (nb_chunk<F>(D, res) + F::PAD) * sizeof(typename F::elem) + size_t(NN_QT) * F::QX;
}

template <class F, int RES, bool VQ, bool VG>  // 16-byte loads of the queries / of the gallery
__global__ __launch_bounds__(256) void nearest_bins_kernel(NearestBinsArgs p) {
  typedef typename F::elem elem;
  typedef typename F::opnd opnd;
  typedef typename F::accum accum;
  constexpr int KG = F::KG, OE = KG / 4;
  static_assert(F::DC % (KG * NS_PF) == 0 && RES % (KG * NS_PF) == 0, "chunks of whole ring turns");
  extern __shared__ __attribute__((aligned(16))) unsigned char nb_lds[];
  const bool resident = p.D <= RES;
  const int clen = nb_chunk<F>(p.D, RES), pitch = clen + F::PAD;
  elem* const sq = reinterpret_cast<elem*>(nb_lds);
  [[maybe_unused]] float* const stq = reinterpret_cast<float*>(nb_lds + size_t(NN_QT) * pitch * sizeof(elem));
  [[maybe_unused]] float* const sinv = stq + NN_QT;

  const int tid = threadIdx.x, lane = tid & 63, lr = lane & 15, kq = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const long long q0 = (long long)blockIdx.x * NN_QT;
  const long long jbeg = (long long)blockIdx.y * p.seg_rows, wr = p.seg_rows >> 2;
  const int R = 1 << p.lgR;
  // the steps of wave 0, in whole bins: no other wave has more rows below G (jbeg < G: no segment is empty)
  const int nsteps = int((min(wr, p.G - jbeg) + NS_WR * R - 1) >> (5 + p.lgR)) << p.lgR;
  const long long jw = jbeg + wr * wave, jlim = min(p.G, jw + (long long)NS_WR * nsteps);  // this wave's rows: [jw, jlim)
  const int nkg = ((p.D + KG - 1) / KG + NS_PF - 1) / NS_PF * NS_PF;

  F::template prologue<VQ>(p.q, p.q_stride, p.n, p.D, q0, wave, lane, stq, sinv);

  auto stage = [&](int c0) __attribute__((always_inline)) {
    for (int r = wave; r < NN_QT; r += 4) {
      const long long qi = q0 + r;
      const float* const row = p.q + qi * p.q_stride;
      float inv = 0.0f;
      if constexpr (F::SCALES) inv = sinv[r];
      for (int g4 = lane; 4 * g4 < clen; g4 += 64)
        F::stage4(sq + r * pitch + 4 * g4, nn_load4<VQ>(qi < p.n, row, c0 + 4 * g4, p.D), inv);
    }
  };

  opnd ring[NS_PF][2];
  const long long jl = jw + lr;  // this lane's A row of step 0, rb 0
  const elem* const g0 = static_cast<const elem*>(p.g);
  const elem* const gl = g0 + jl * p.D;
  auto fetch = [&](int slot, int st, int kg) __attribute__((always_inline)) {
    const long long sj = (long long)st * NS_WR;  // st == nsteps: past jlim, nothing of it is read
#pragma unroll
    for (int rb = 0; rb < 2; ++rb)
      ring[slot][rb] = F::template load<VG>(jl + sj + 16 * rb < jlim, gl + (sj + 16 * rb) * p.D, KG * kg + OE * kq, p.D, g0);
  };

  // the running best of the open bin per query block, and whether this lane has a row in it
  unsigned bimg[4] = {0u, 0u, 0u, 0u};
  int brow[4];
  const int jmine = int(jw) + 4 * kq;  // the first row this lane scores (G < 2^31)
#pragma unroll
  for (int qb = 0; qb < 4; ++qb) brow[qb] = jmine;

  const elem* const bq = sq + lr * pitch + OE * kq;
#pragma unroll
  for (int u = 0; u < NS_PF; ++u) {
    fetch(u, 0, u);
    __builtin_amdgcn_sched_barrier(0);
  }
  for (int st = 0; st < nsteps; ++st) {
    const long long js = (long long)st * NS_WR;
    accum acc[4][2];
    [[maybe_unused]] float tg[2][4];
#pragma unroll
    for (int qb = 0; qb < 4; ++qb) acc[qb][0] = acc[qb][1] = accum{};
    for (int kg0 = 0; kg0 < nkg; kg0 += NS_PF) {
      if (resident ? (st == 0 && kg0 == 0) : kg0 % (F::DC / KG) == 0) {  // uniform over the workgroup
        __syncthreads();  // the previous chunk's operand reads (and, first, the prologue's scales) are done
        stage(KG * kg0);
        __syncthreads();
      }
#pragma unroll
      for (int u = 0; u < NS_PF; ++u) {
        const int kg = kg0 + u;
        const opnd a0 = F::template mask<VG>(ring[u][0], jl + js < jlim, KG * kg + OE * kq, p.D);
        const opnd a1 = F::template mask<VG>(ring[u][1], jl + js + 16 < jlim, KG * kg + OE * kq, p.D);
        const elem* const b = bq + (resident ? KG * kg : KG * (kg % (F::DC / KG)));
#pragma unroll
        for (int qb = 0; qb < 4; ++qb) {
          const opnd bv = *reinterpret_cast<const opnd*>(b + 16 * qb * pitch);
          acc[qb][0] = F::mfma(a0, bv, acc[qb][0]);
          acc[qb][1] = F::mfma(a1, bv, acc[qb][1]);
        }
        if constexpr (F::SCALES) {
          if (u == 0) {  // the scales of this lane's eight rows, at a fixed place among the ring's loads
#pragma unroll
            for (int rb = 0; rb < 2; ++rb)
#pragma unroll
              for (int i = 0; i < 4; ++i) tg[rb][i] = p.scales[min(jw + js + 16 * rb + 4 * kq + i, p.G - 1)];
          }
        }
        const bool wrap = kg + NS_PF >= nkg;
        fetch(u, st + wrap, kg + NS_PF - (wrap ? nkg : 0));
        __builtin_amdgcn_sched_barrier(0);  // the loads stay in the ring's order: the waits count on it
      }
    }
    // the step's scores against the running best: this lane's rows in ascending order
    const int j0 = jmine + NS_WR * st;  // rows j0 + e with e < left are there; the difference in 64 bits: jw may pass 2^31
    const int left = int(max(min(jlim - (jw + js + 4 * kq), (long long)NS_WR), 0LL));
#pragma unroll
    for (int qb = 0; qb < 4; ++qb) {
      float tq = 0.0f;
      if constexpr (F::SCALES) tq = stq[16 * qb + lr];
#pragma unroll
      for (int rb = 0; rb < 2; ++rb)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          float s;
          if constexpr (F::SCALES) s = F::score(acc[qb][rb][i], tq, tg[rb][i]);
          else s = F::score(acc[qb][rb][i]);
          unsigned img = unsigned(topk_key(__float_as_uint(s), 0) >> 32);
          img = 16 * rb + i < left ? img : 0u;
          const bool up = img > bimg[qb];
          bimg[qb] = up ? img : bimg[qb];
          brow[qb] = up ? j0 + 16 * rb + i : brow[qb];
        }
    }
    if (((st + 1) & (R - 1)) == 0) {  // the bin ends: wave-uniform
      const bool have = jw + js - NS_WR * (R - 1) + 4 * kq < jlim;  // this lane's first row of the bin is there
      u64 mine = 0ull;
#pragma unroll
      for (int qb = 0; qb < 4; ++qb) {
        u64 v = have ? (u64(bimg[qb]) << 32) | u64(~unsigned(brow[qb])) : 0ull;
        const unsigned lo = unsigned(v), hi = unsigned(v >> 32);
        auto l16 = __builtin_amdgcn_permlane16_swap(lo, lo, false, false);
        auto h16 = __builtin_amdgcn_permlane16_swap(hi, hi, false, false);
        const u64 a = (u64(h16[0]) << 32) | l16[0], b = (u64(h16[1]) << 32) | l16[1];
        v = a > b ? a : b;
        auto l32 = __builtin_amdgcn_permlane32_swap(unsigned(v), unsigned(v), false, false);
        auto h32 = __builtin_amdgcn_permlane32_swap(unsigned(v >> 32), unsigned(v >> 32), false, false);
        const u64 c = (u64(h32[0]) << 32) | l32[0], d = (u64(h32[1]) << 32) | l32[1];
        v = c > d ? c : d;
        mine = kq == qb ? v : mine;
        bimg[qb] = 0u;
        brow[qb] = jmine + NS_WR * (st + 1);
      }
      const long long bin = (jw >> (5 + p.lgR)) + (st >> p.lgR), qi = q0 + lane;  // lane l: query block l >> 4, row l & 15
      if (qi < p.n && bin < p.NB) p.win[qi * p.NB + bin] = mine;
    }
  }
}

// the launch: the four load-path instances and the one-time LDS raise, as nearest_launch
template <class F, int RES, bool VQ, bool VG>
void nearest_bins_launch_instance(const NearestBinsArgs& a, int S, hipStream_t s) {
  static std::atomic<unsigned long long> raised{0};
  const auto kernel = &nearest_bins_kernel<F, RES, VQ, VG>;
  ore_raise_lds_once(raised, reinterpret_cast<const void*>(kernel), int(nb_lds_bytes<F>(RES, RES)));
  const dim3 grid((unsigned)((a.n + NN_QT - 1) / NN_QT), (unsigned)S);
  hipLaunchKernelGGL(kernel, grid, dim3(256), nb_lds_bytes<F>(a.D, RES), s, a);
}

template <class F, int RES>
void nearest_bins_launch(const float* q, long long q_stride, int n, int D, const void* gallery, const float* scales, long long G,
                         int bin_rows, int S, void* win, hipStream_t s) {
  static_assert(2 * nb_lds_bytes<F>(RES, RES) <= 160 * 1024, "two workgroups' tiles on a compute unit");
  static_assert(2 * (nb_lds_bytes<F>(RES, RES) + size_t(NN_QT) * F::KG * NS_PF * sizeof(typename F::elem)) > 160 * 1024,
                "a resident tile one turn longer does not fit twice");
  static_assert(nb_lds_bytes<F>(RES + 1, RES) <= nb_lds_bytes<F>(RES, RES), "a chunk is no longer than the resident tile");
  if (n <= 0) return;
  const long long unit = 4LL * bin_rows, units = (G + unit - 1) / unit, per = (units + S - 1) / S;
  int lgR = 0;
  while ((32 << lgR) < bin_rows) ++lgR;
  const NearestBinsArgs a{q, gallery, scales, static_cast<u64*>(win), q_stride, G, (G + bin_rows - 1) / bin_rows, per * unit, n, D, lgR};
  const bool vg = D % (16 / int(sizeof(typename F::elem))) == 0 && (reinterpret_cast<uintptr_t>(gallery) & 15) == 0;
  const bool vq = D % 4 == 0 && q_stride % 4 == 0 && (reinterpret_cast<uintptr_t>(q) & 15) == 0;
  if (vq && vg) nearest_bins_launch_instance<F, RES, true, true>(a, S, s);
  else if (vg) nearest_bins_launch_instance<F, RES, false, true>(a, S, s);
  else if (vq) nearest_bins_launch_instance<F, RES, true, false>(a, S, s);
  else nearest_bins_launch_instance<F, RES, false, false>(a, S, s);
}

}  // namespace

}  // namespace ore
