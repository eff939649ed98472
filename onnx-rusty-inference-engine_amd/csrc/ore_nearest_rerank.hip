// Exact re-ranking of an approximate search (extension, ore_nearest_rerank_f32 / _f16): for every
// query row the k best of its C candidate rows of a gallery [G][D], scored against that gallery as its full search
// scores them -- the second stage behind a cheap search (int8, f16) that returned k' > k candidates.  A batch of
// gathered matrix-vector products and a small selection: every query has rows of its own, scattered over the gallery,
// so neither search kernel (contiguous segments that all queries of a tile share) serves it.
//
// Candidate rule.  An entry outside [0, G) is padding: nothing is read for it and its key is 0, the empty slot.  A
// row that occurs more than once counts once: its keys are equal (the score's bits depend on the two rows alone),
// and a round of topk_rounds takes the largest key strictly below the previous round's, so equal keys collapse by
// themselves -- there is no de-duplication pass.  Past the distinct valid rows a round finds nothing: its key stays
// 0, which decodes to index -1 and the quiet NaN 0x7fc00000.
//
// Bit contract.  The value of (query i, row j) is, to the bit, what the search of the same gallery returns: the same
// instruction, the same d -> k-slot assignment, the same operand roles (gallery row = A, query = B), one accumulator's
// chain over the k-groups in ascending order from +0.
//   f32 (ore_nearest.hip): v_mfma_f32_16x16x4_f32; a k-group is 16 d, four MFMAs of which MFMA s takes d = 16 kg +
//     4 (l >> 4) + s from lane l.  The search walks chunks of 32 d as two such groups and skips a group that is all
//     padding; here a padded group multiplies +0 by +0 and leaves the accumulator (never -0) unchanged: the same bits.
//   f16 (FmtF16): the query rounded to nearest even to f16, v_mfma_f32_16x16x32_f16, lane l supplies d = 32 kg +
//     8 (l >> 4) + e.
// An element that is not there (d >= D, a padding candidate) is +0 on its bits on the gallery's side and +0 in LDS on
// the query's.
//
// Split.  One workgroup of four waves per query; wave w owns the candidate blocks w, w + 4, ... of 16 rows.  A block
// is the 16 rows of an A operand: lane l carries candidate l & 15 and k-quarter l >> 4.  The query is the B operand
// with the same row in all 16 columns, so every column of the accumulator holds the block's 16 scores and lane l has
// those of candidates 4 (l >> 4) + i in acc[i].  Fifteen of the sixteen columns are redundant: at n = 256, C = 64,
// D = 512 that is 0.27 GFLOP, a few microseconds at the f32 MFMA rate -- the price of the bit contract: the score
// keeps the search's instruction and k-slots, and the diagonals of 16 queries are not packed into one MFMA (they
// would use one column each as well: 16 queries against 16 rows of their own is no matrix product).  Every wave runs
// ceil(blocks / 4) block turns, a block past the last one as 16 padding rows, so the barriers of the chunked query
// below are uniform over the workgroup.
//
// Data movement.  Gallery rows go from global memory straight into the A operand registers, every lane behind its own
// row pointer at the 64-bit offset j * D: 16-byte loads where D and the base allow, element loads otherwise (the VG of
// nearest_launch), RR_PF k-groups ahead of their MFMAs through a ring of registers that runs on across the wave's
// blocks.  A turn of the ring is straight-line code: a load that must not happen reads
// the gallery's first bytes instead and is zeroed on its bits before the MFMA.  The candidate indices are checked once
// and kept in LDS (-1 for padding), so the next block's row pointer comes from LDS and not through the ring's counter.
// The query row is staged once per workgroup in LDS in the format (rounded once for f16) and read as a broadcast -- 16
// lanes, one address; above RR_DC d it is staged in chunks of RR_DC d between two barriers, for every block, and the
// accumulator carries across the chunks.  From global per k-group it would put a ninth load into every ring slot.
//
// Selection.  The lanes l & 15 < 4 write their block's keys, topk_key(score bits, row) or 0, to the C slots in LDS;
// after one barrier wave 0 runs topk_rounds<4> over the 256 slots and writes rank = lane.  No partial buffer, no merge
// launch, no context-owned memory: one launch, legal inside a stream capture.
#include "ore_nearest.h"

namespace ore {

namespace {

typedef _Float16 halfx4 __attribute__((ext_vector_type(4)));
typedef _Float16 halfx8 __attribute__((ext_vector_type(8)));
typedef unsigned uintx4 __attribute__((ext_vector_type(4)));

constexpr int RR_CMAX = 256;  // candidates per query at most: four keys per lane of the selecting wave
constexpr int RR_PF = 8;      // k-groups the gallery loads run ahead of the MFMAs
constexpr int RR_DC = 512;    // the largest resident D, and d per staged chunk above it

struct RerankArgs {
  const float* q;
  const void* g;  // [G][D] in the format
  const int* cand;
  float* values;  // [n][k]
  int* indices;
  long long q_stride, G, cand_stride;
  int D, C, k;
};

// A format supplies: elem, opnd (a lane's 16 bytes of a k-group), KG (d per k-group), load / mask (one gallery operand,
// read without a branch, and its zeroing when it is consumed), stage4 (four staged d of the query) and mfma.
struct RerankF32 {
  typedef float elem;
  typedef floatx4 opnd;
  static constexpr int KG = 16;

  template <bool VEC>
  static __device__ __forceinline__ floatx4 load(bool ok, const float* __restrict__ row, int d, int D, const float* __restrict__ safe) {
    floatx4 v;
    if (VEC) {  // D % 4 == 0: the group is inside the row or outside it
      v = *reinterpret_cast<const floatx4*>(ok && d < D ? row + d : safe);
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = *(ok && d + e < D ? row + d + e : safe);
    }
    return v;
  }

  template <bool VEC>
  static __device__ __forceinline__ floatx4 mask(floatx4 v, bool ok, int d, int D) {
    uintx4 m;
    if (VEC) {
      const unsigned a = ok && d < D ? ~0u : 0u;
      m = uintx4{a, a, a, a};
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) m[e] = ok && d + e < D ? ~0u : 0u;
    }
    return __builtin_bit_cast(floatx4, __builtin_bit_cast(uintx4, v) & m);  // a masked NaN or inf becomes +0 too
  }

  static __device__ __forceinline__ void stage4(float* dst, floatx4 v) { *reinterpret_cast<floatx4*>(dst) = v; }

  static __device__ __forceinline__ floatx4 mfma(floatx4 a, floatx4 b, floatx4 c) {
#pragma unroll
    for (int s = 0; s < 4; ++s) c = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s], b[s], c, 0, 0, 0);
    return c;
  }
};

struct RerankF16 {
  typedef _Float16 elem;
  typedef halfx8 opnd;
  static constexpr int KG = 32;

  template <bool VEC>
  static __device__ __forceinline__ halfx8 load(bool ok, const _Float16* __restrict__ row, int d, int D,
                                                const _Float16* __restrict__ safe) {
    halfx8 v;
    if (VEC) {  // D % 8 == 0
      v = *reinterpret_cast<const halfx8*>(ok && d < D ? row + d : safe);
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = *(ok && d + e < D ? row + d + e : safe);
    }
    return v;
  }

  template <bool VEC>
  static __device__ __forceinline__ halfx8 mask(halfx8 v, bool ok, int d, int D) {
    if (VEC) {
      const unsigned m = ok && d < D ? ~0u : 0u;
      return __builtin_bit_cast(halfx8, __builtin_bit_cast(uintx4, v) & uintx4{m, m, m, m});
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = ok && d + e < D ? v[e] : (_Float16)0.0f;
    return v;
  }

  static __device__ __forceinline__ void stage4(_Float16* dst, floatx4 v) {  // round to nearest even, as FmtF16::stage4
    *reinterpret_cast<halfx4*>(dst) = halfx4{(_Float16)v[0], (_Float16)v[1], (_Float16)v[2], (_Float16)v[3]};
  }

  static __device__ __forceinline__ floatx4 mfma(halfx8 a, halfx8 b, floatx4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
  }
};

template <class F, bool VQ, bool VG>  // 16-byte loads of the query / of the gallery
__global__ __launch_bounds__(256) void nearest_rerank_kernel(RerankArgs p) {
  typedef typename F::elem elem;
  typedef typename F::opnd opnd;
  constexpr int KG = F::KG, OE = KG / 4, CKG = RR_DC / KG;  // d per k-group and per lane of it; k-groups per chunk
  static_assert(RR_DC % (KG * RR_PF) == 0, "chunks of whole ring turns");
  __shared__ __attribute__((aligned(16))) elem sq[RR_DC];
  __shared__ u64 skey[RR_CMAX];
  __shared__ int scand[RR_CMAX + 64];  // -1: padding; the 64 past RR_CMAX are what the last block's turn looks ahead to

  const int tid = threadIdx.x, lane = tid & 63, lr = lane & 15, kq = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const long long qi = blockIdx.x;
  const int nit = ((p.C + 15) / 16 + 3) / 4;                             // block turns of every wave
  const int nkg = ((p.D + KG - 1) / KG + RR_PF - 1) / RR_PF * RR_PF;  // whole turns of the ring
  const bool resident = p.D <= RR_DC;
  const int clen = resident ? nkg * KG : RR_DC;
  const float* const qrow = p.q + qi * p.q_stride;
  const elem* const g0 = static_cast<const elem*>(p.g);

  for (int i = tid; i < RR_CMAX + 64; i += 256) {
    int j = -1;
    if (i < p.C) {
      j = p.cand[qi * p.cand_stride + i];
      if (j < 0 || j >= p.G) j = -1;
    }
    scand[i] = j;
  }
  skey[tid] = 0ull;
  __syncthreads();

  auto stage = [&](int c0) __attribute__((always_inline)) {
    for (int g4 = tid; 4 * g4 < clen; g4 += 256) F::stage4(sq + 4 * g4, nn_load4<VQ>(true, qrow, c0 + 4 * g4, p.D));
  };

  opnd ring[RR_PF];
  auto fetch = [&](int slot, int j, int kg) __attribute__((always_inline)) {
    ring[slot] = F::template load<VG>(j >= 0, g0 + (long long)max(j, 0) * p.D, KG * kg + OE * kq, p.D, g0);
  };

  int jc = scand[16 * wave + lr];
#pragma unroll
  for (int u = 0; u < RR_PF; ++u) {
    fetch(u, jc, u);
    __builtin_amdgcn_sched_barrier(0);
  }
  for (int it = 0; it < nit; ++it) {
    const int blk = wave + 4 * it;
    const int jn = scand[16 * (blk + 4) + lr];
    floatx4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int kg0 = 0; kg0 < nkg; kg0 += RR_PF) {
      if (resident ? (it == 0 && kg0 == 0) : kg0 % CKG == 0) {  // uniform over the workgroup
        __syncthreads();  // the previous chunk's operand reads are done
        stage(KG * kg0);
        __syncthreads();
      }
      // one turn of the ring, without a branch: k-group kg0 + u is consumed from slot u, which then takes the k-group
      // RR_PF further on (of the wave's next block at the end of this one)
#pragma unroll
      for (int u = 0; u < RR_PF; ++u) {
        const int kg = kg0 + u;
        const opnd a = F::template mask<VG>(ring[u], jc >= 0, KG * kg + OE * kq, p.D);
        const opnd b = *reinterpret_cast<const opnd*>(sq + KG * (resident ? kg : kg % CKG) + OE * kq);
        acc = F::mfma(a, b, acc);
        const bool wrap = kg + RR_PF >= nkg;
        fetch(u, wrap ? jn : jc, kg + RR_PF - (wrap ? nkg : 0));
        __builtin_amdgcn_sched_barrier(0);  // the loads stay in the ring's order: the waits count on it
      }
    }
    // acc[i] is candidate 16 blk + 4 kq + i, in every column: column lr < 4 writes i = lr
    if (lr < 4) {
      const int c = 16 * blk + 4 * kq + lr, j = scand[c];
      const float s = lr == 0 ? acc[0] : lr == 1 ? acc[1] : lr == 2 ? acc[2] : acc[3];
      skey[c] = j >= 0 ? topk_key(__float_as_uint(s), j) : 0ull;
    }
    jc = jn;
  }
  __syncthreads();
  if (wave == 0) {
    u64 key[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) key[t] = skey[lane + 64 * t];
    const u64 mine = topk_rounds<4>(key, p.k, lane);
    if (lane < p.k) {  // 0 past the distinct valid rows: the quiet NaN and index -1
      reinterpret_cast<unsigned*>(p.values)[qi * p.k + lane] = topk_key_bits(mine);
      p.indices[qi * p.k + lane] = topk_key_index(mine);
    }
  }
}

template <class F>
void rerank_launch(const RerankArgs& a, int n, hipStream_t s) {
  constexpr int VGE = 16 / int(sizeof(typename F::elem));
  const bool vg = a.D % VGE == 0 && (reinterpret_cast<uintptr_t>(a.g) & 15) == 0;
  const bool vq = a.D % 4 == 0 && a.q_stride % 4 == 0 && (reinterpret_cast<uintptr_t>(a.q) & 15) == 0;
  const dim3 grid((unsigned)n), block(256);
  if (vq && vg) hipLaunchKernelGGL((nearest_rerank_kernel<F, true, true>), grid, block, 0, s, a);
  else if (vg) hipLaunchKernelGGL((nearest_rerank_kernel<F, false, true>), grid, block, 0, s, a);
  else if (vq) hipLaunchKernelGGL((nearest_rerank_kernel<F, true, false>), grid, block, 0, s, a);
  else hipLaunchKernelGGL((nearest_rerank_kernel<F, false, false>), grid, block, 0, s, a);
}

}  // namespace

void launch_nearest_rerank(NearestFmt fmt, const float* q, long long q_stride, int n, int D, const void* gallery, long long G,
                           const int* candidates, long long cand_stride, int C, int k, float* values, int* indices, hipStream_t s) {
  if (n <= 0) return;
  const RerankArgs a{q, gallery, candidates, values, indices, q_stride, G, cand_stride, D, C, k};
  if (fmt == NearestFmt::F16) rerank_launch<RerankF16>(a, n, s);
  else rerank_launch<RerankF32>(a, n, s);
}

}  // namespace ore
