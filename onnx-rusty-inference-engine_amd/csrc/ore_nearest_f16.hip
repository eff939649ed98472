// Nearest neighbours on an f16 gallery (extension, ore_nearest_f16 and ore_gallery_f16): the k best
// of s[i, j] = sum_d RNE_f16(q[i, d]) g[j, d] per query row, products exact in f32, accumulated in f32 by
// v_mfma_f32_16x16x32_f16, under ore_topk_f32's order (ore_topk_key.h) -- and the packer that makes the gallery.
//
// Split.  grid = (ceil(n / 64) query tiles, S gallery segments), four waves.  A step is NF_GT = 128 gallery rows:
// wave w takes rows 32 w .. 32 w + 31 of it, as two A operands of 16 rows, against all 64 queries of the tile, the
// B operands of four query blocks -- eight MFMAs per k-group of 32 d, 32 accumulators over the whole of D.  Lane l
// holds query 16 qb + (l & 15) against rows 32 w + 16 rb + 4 (l >> 4) + i.  A gallery element is used by one wave.
//
// Data movement.  The query tile is rounded to f16 once per workgroup and stays in LDS for the whole segment
// (64 rows of D halves, D rounded up to a whole turn of the ring below, at a pitch of 8 halves more: a row starts
// 16 m + 4 dwords after the one before, an odd multiple of 4 banks, so the 16 rows of a 16-byte operand read fall
// on 16 different bank quads).  The gallery never passes through LDS: a lane loads the 16 bytes of its row and
// k-group straight into the A operand (eight 2-byte loads when D % 8 != 0 or the base is not 16-byte aligned),
// NF_PF k-groups ahead of the MFMAs that consume them, through a ring of registers that runs on across the steps.
// The K loop has no barrier and no branch: a turn of the ring is straight-line code, so the waits count the loads
// in flight (vmcnt 15 and 14 before a k-group's MFMAs) -- with a branch around a load or around a k-group's MFMAs
// the compiler drained the ring once per turn.  So a gallery element that is not there (a row past the segment,
// d past D) is read from the gallery's first elements instead and made +0 on its bits before the MFMA, and the
// k-groups past D that fill the last turn multiply the +0 of that mask by the +0 the tile holds there.  Above
// NF_DRES the tile no longer fits beside the selection state: it is then staged in chunks of NF_DC d, every step,
// between two barriers per chunk, and the accumulators carry across the chunks.  Query rows past n and d past D
// are masked at the load and enter LDS as +0.  Nothing outside q's rows and the gallery's G D elements is read.
//
// Position independence.  K is never split across waves or workgroups.  A score is one accumulator's chain over
// the k-groups in ascending order, the MFMA taking d = 32 kg + 8 (l >> 4) + e from lane l: an order that depends
// on D alone (so does resident or chunked, and the number of turns).  Padded products are +0 and leave the
// accumulator unchanged: it starts at +0 and is never -0.
//
// Selection.  Per query, in LDS: the threshold, the k best keys so far, NF_GT candidate slots and a flag.  Several
// waves score the same query, so a candidate is not appended through a counter: slot r of a query belongs to row r
// of the step and holds the 32-bit score image of the key (the index is j0 + r), or NF_ABSENT, which no image
// equals (an image is at most +inf's 0xff800000).  A buffer cannot overflow: the slots are the rows.  A key above
// its query's threshold is stored and the flag set; behind the step's barrier the flagged queries are dealt out
// over the waves, 16 each, and compacted by topk_rounds over (k held, two slots per lane), which also empties the
// slots.  8-byte slots behind the f32 kernel's atomic counter would need 128 of them per query: with k = 64 that
// is 97 KB of state beside the 65 KB tile of D = 512, past the 160 KB.
//
// Merge.  S == 1: the workgroup writes values and indices.  S > 1: part[n][S][k] and ore_nearest.hip's merge.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>

#include "ore_kernels.h"
#include "ore_topk_key.h"

namespace ore {

namespace {

typedef float floatx4 __attribute__((ext_vector_type(4)));
typedef _Float16 halfx4 __attribute__((ext_vector_type(4)));
typedef _Float16 halfx8 __attribute__((ext_vector_type(8)));

constexpr int NF_QT = 64;               // queries per workgroup
constexpr int NF_WR = 32;               // gallery rows per wave and step
constexpr int NF_GT = 4 * NF_WR;        // gallery rows per step
constexpr int NF_KG = 32;               // d per MFMA
constexpr int NF_PF = 8;                // k-groups the gallery loads run ahead of the MFMAs
constexpr int NF_DRES = 512;            // the largest D whose query tile is resident
constexpr int NF_DC = 512;              // d per staged chunk above it
constexpr int NF_PAD = 8;               // halves added to the LDS row pitch
constexpr int NF_SMAX = 512;            // segments at most: the merge kernel's lists
constexpr unsigned NF_ABSENT = 0xffffffffu;
static_assert(NF_DC % (NF_KG * NF_PF) == 0 && NF_DRES % (NF_KG * NF_PF) == 0 && NF_GT == 128, "chunks of whole ring turns; two slots per lane");

// the d of the tile that are staged at once: D in whole turns of the ring, or a chunk
constexpr int NF_TURN = NF_KG * NF_PF;
__host__ __device__ constexpr int nf_chunk(int D) { return D <= NF_DRES ? (D + NF_TURN - 1) / NF_TURN * NF_TURN : NF_DC; }
// dynamic LDS: the query tile, then per query the threshold, k keys, NF_GT slots and the flag
__host__ __device__ constexpr size_t nf_lds_bytes(int D, int k) {
  return size_t(NF_QT) * (nf_chunk(D) + NF_PAD) * 2 + size_t(NF_QT) * (8 + 8 * size_t(k) + 4 * NF_GT + 4);
}
static_assert(nf_lds_bytes(NF_DRES, 64) <= 160 * 1024 && nf_lds_bytes(NF_DRES + 1, 64) <= nf_lds_bytes(NF_DRES, 64), "LDS");

struct NearestF16Args {
  const float* q;
  const _Float16* g;
  u64* part;       // [n][S][k], S > 1
  float* values;   // [n][k]
  int* indices;
  long long q_stride, G, seg_rows;  // seg_rows: gallery rows per segment, a multiple of NF_GT
  int n, D, k, S;
};

// four consecutive d of a query row / eight of a gallery row, masked: nothing past D or of a row that is not there
template <bool VEC>
__device__ __forceinline__ floatx4 nf_load4(bool row_ok, const float* __restrict__ row, int d, int D) {
  floatx4 v = {0.0f, 0.0f, 0.0f, 0.0f};
  if (VEC) {  // D % 4 == 0: the group is inside the row or outside it
    if (row_ok && d < D) v = *reinterpret_cast<const floatx4*>(row + d);
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (row_ok && d + e < D) v[e] = row[d + e];
  }
  return v;
}

// The gallery loads sit in the K loop, far ahead of their use, so they are masked without a branch: an element that
// is not there is read from `safe` instead (the gallery's first element, or its first eight: always there), and
// nf_mask8 makes it +0 when the operand is consumed.
template <bool VEC>
__device__ __forceinline__ halfx8 nf_load8(bool row_ok, const _Float16* __restrict__ row, int d, int D,
                                           const _Float16* __restrict__ safe) {
  halfx8 v;
  if (VEC) {  // D % 8 == 0: the group is inside the row or outside it
    v = *reinterpret_cast<const halfx8*>(row_ok && d < D ? row + d : safe);
  } else {
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = *(row_ok && d + e < D ? row + d + e : safe);
  }
  return v;
}

template <bool VEC>
__device__ __forceinline__ halfx8 nf_mask8(halfx8 v, bool row_ok, int d, int D) {
  typedef unsigned uintx4 __attribute__((ext_vector_type(4)));
  if (VEC) {
    const unsigned m = row_ok && d < D ? ~0u : 0u;  // on the bits: a NaN or an inf that is masked becomes +0 too
    return __builtin_bit_cast(halfx8, __builtin_bit_cast(uintx4, v) & uintx4{m, m, m, m});
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) v[e] = row_ok && d + e < D ? v[e] : (_Float16)0.0f;
  return v;
}

template <bool VQ, bool VG>  // 16-byte loads of the queries / of the gallery
__global__ __launch_bounds__(256) void nearest_f16_kernel(NearestF16Args p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char nf_lds[];
  const bool resident = p.D <= NF_DRES;
  const int clen = nf_chunk(p.D), pitch = clen + NF_PAD;
  _Float16* const sq = reinterpret_cast<_Float16*>(nf_lds);
  u64* const sthr = reinterpret_cast<u64*>(nf_lds + size_t(NF_QT) * pitch * 2);
  u64* const stop = sthr + NF_QT;                                           // [NF_QT][k]
  unsigned* const scand = reinterpret_cast<unsigned*>(stop + NF_QT * p.k);  // [NF_QT][NF_GT]
  int* const sflag = reinterpret_cast<int*>(scand + NF_QT * NF_GT);

  const int tid = threadIdx.x, lane = tid & 63, lr = lane & 15, kq = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const long long q0 = (long long)blockIdx.x * NF_QT;
  const int seg = blockIdx.y;
  const long long jbeg = (long long)seg * p.seg_rows, jend = min(p.G, jbeg + p.seg_rows);
  const int nsteps = int((jend - jbeg + NF_GT - 1) / NF_GT);  // >= 1: the launcher leaves no segment empty
  const int nkg = ((p.D + NF_KG - 1) / NF_KG + NF_PF - 1) / NF_PF * NF_PF;  // whole turns of the ring

  for (int i = tid; i < NF_QT; i += 256) {
    sthr[i] = 0ull;
    sflag[i] = 0;
  }
  for (int i = tid; i < NF_QT * p.k; i += 256) stop[i] = 0ull;
  for (int i = tid; i < NF_QT * NF_GT; i += 256) scand[i] = NF_ABSENT;

  // the tile's d from c0 on, rounded to f16: a wave per row, a lane per group of four
  auto stage = [&](int c0) __attribute__((always_inline)) {
    for (int r = wave; r < NF_QT; r += 4) {
      const long long qi = q0 + r;
      const float* const row = p.q + qi * p.q_stride;
      for (int g4 = lane; 4 * g4 < clen; g4 += 64) {
        const floatx4 v = nf_load4<VQ>(qi < p.n, row, c0 + 4 * g4, p.D);
        *reinterpret_cast<halfx4*>(sq + r * pitch + 4 * g4) = halfx4{(_Float16)v[0], (_Float16)v[1], (_Float16)v[2], (_Float16)v[3]};
      }
    }
  };

  // k-group kg of step st of this wave's rows: lane l takes the 8 d from 32 kg + 8 (l >> 4) of rows (l & 15), + 16
  halfx8 ring[NF_PF][2];
  const long long jl = jbeg + NF_WR * wave + lr;  // this lane's first row of step 0
  const _Float16* const gl = p.g + jl * p.D;
  auto fetch = [&](int slot, int st, int kg) __attribute__((always_inline)) {
    const long long sj = (long long)st * NF_GT;  // st == nsteps: past jend, nothing of it is read
#pragma unroll
    for (int rb = 0; rb < 2; ++rb)
      ring[slot][rb] = nf_load8<VG>(jl + sj + 16 * rb < jend, gl + (sj + 16 * rb) * p.D, NF_KG * kg + 8 * kq, p.D, p.g);
  };

  const _Float16* const bq = sq + lr * pitch + 8 * kq;
#pragma unroll
  for (int u = 0; u < NF_PF; ++u) {
    fetch(u, 0, u);
    __builtin_amdgcn_sched_barrier(0);
  }
  for (int st = 0; st < nsteps; ++st) {
    const long long j0 = jbeg + (long long)st * NF_GT;
    floatx4 acc[4][2];
#pragma unroll
    for (int qb = 0; qb < 4; ++qb) acc[qb][0] = acc[qb][1] = floatx4{0.0f, 0.0f, 0.0f, 0.0f};
    for (int kg0 = 0; kg0 < nkg; kg0 += NF_PF) {
      if (resident ? (st == 0 && kg0 == 0) : kg0 % (NF_DC / NF_KG) == 0) {  // uniform
        __syncthreads();  // the previous chunk's operand reads (and, first, the state's initialisation) are done
        stage(NF_KG * kg0);
        __syncthreads();
      }
      // one turn of the ring, without a branch: k-group kg0 + u is consumed from slot u, which then takes the k-group
      // NF_PF further on (into the next step at the end of this one).  The tile is staged in whole turns, so the
      // k-groups past D that fill the last turn multiply +0 by +0
#pragma unroll
      for (int u = 0; u < NF_PF; ++u) {
        const int kg = kg0 + u;
        const halfx8 a0 = nf_mask8<VG>(ring[u][0], jl + (j0 - jbeg) < jend, NF_KG * kg + 8 * kq, p.D);
        const halfx8 a1 = nf_mask8<VG>(ring[u][1], jl + (j0 - jbeg) + 16 < jend, NF_KG * kg + 8 * kq, p.D);
        const _Float16* const b = bq + (resident ? NF_KG * kg : NF_KG * (kg % (NF_DC / NF_KG)));
#pragma unroll
        for (int qb = 0; qb < 4; ++qb) {
          const halfx8 bv = *reinterpret_cast<const halfx8*>(b + 16 * qb * pitch);
          acc[qb][0] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a0, bv, acc[qb][0], 0, 0, 0);
          acc[qb][1] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a1, bv, acc[qb][1], 0, 0, 0);
        }
        const bool wrap = kg + NF_PF >= nkg;
        fetch(u, st + wrap, kg + NF_PF - (wrap ? nkg : 0));
        __builtin_amdgcn_sched_barrier(0);  // the loads stay in the ring's order: the waits count on it
      }
    }
    // the step's scores against the thresholds: acc[qb][rb][i] is query 16 qb + lr against row j0 + slot
#pragma unroll
    for (int qb = 0; qb < 4; ++qb) {
      const int ql = 16 * qb + lr;
      const u64 thr = sthr[ql];
      const bool q_ok = q0 + ql < p.n;
#pragma unroll
      for (int rb = 0; rb < 2; ++rb)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int slot = NF_WR * wave + 16 * rb + 4 * kq + i;
          const long long j = j0 + slot;
          const u64 key = topk_key(__float_as_uint(acc[qb][rb][i]), int(j));
          if (q_ok && j < jend && key > thr) {
            scand[ql * NF_GT + slot] = unsigned(key >> 32);
            sflag[ql] = 1;
          }
        }
    }
    __syncthreads();
    for (int t = 0; t < 16; ++t) {  // this wave's share of the queries that gained a candidate: k held + slots -> k held
      const int qi = 16 * wave + t;
      if (__builtin_amdgcn_readfirstlane(sflag[qi]) == 0) continue;  // wave-uniform
      u64 key[3];
      key[0] = lane < p.k ? stop[qi * p.k + lane] : 0ull;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int slot = lane + 64 * h;
        const unsigned hi = scand[qi * NF_GT + slot];
        key[1 + h] = hi != NF_ABSENT ? (u64(hi) << 32) | u64(~unsigned(j0 + slot)) : 0ull;
        scand[qi * NF_GT + slot] = NF_ABSENT;
      }
      const u64 mine = topk_rounds<3>(key, p.k, lane);
      if (lane < p.k) stop[qi * p.k + lane] = mine;
      if (lane == p.k - 1) sthr[qi] = mine;  // 0 while fewer than k are held: every key passes
      if (lane == 0) sflag[qi] = 0;
    }
    __syncthreads();
  }

  // the k best of the segment, rank = lane
  for (int t = 0; t < 16; ++t) {
    const int qi = 16 * wave + t;
    const long long row = q0 + qi;
    if (row >= p.n || lane >= p.k) continue;
    const u64 key = stop[qi * p.k + lane];
    if (p.S > 1) {
      p.part[(row * p.S + seg) * p.k + lane] = key;
    } else if (key != 0ull) {  // G >= k: every rank is held
      reinterpret_cast<unsigned*>(p.values)[row * p.k + lane] = topk_key_bits(key);
      p.indices[row * p.k + lane] = topk_key_index(key);
    }
  }
}

// f32 -> f16, round to nearest even, no clamp.  VEC (D % 8 == 0, both bases 16-byte aligned): a thread takes eight
// elements, two 16-byte loads and one 16-byte store; otherwise one element
template <bool VEC>
__global__ __launch_bounds__(256) void gallery_f16_kernel(const float* __restrict__ src, _Float16* __restrict__ dst, long long total) {
  const long long t0 = (long long)blockIdx.x * 256 + threadIdx.x, stride = (long long)gridDim.x * 256;
  if (VEC) {
    for (long long i = 8 * t0; i < total; i += 8 * stride) {
      const floatx4 a = *reinterpret_cast<const floatx4*>(src + i), b = *reinterpret_cast<const floatx4*>(src + i + 4);
      *reinterpret_cast<halfx8*>(dst + i) = halfx8{(_Float16)a[0], (_Float16)a[1], (_Float16)a[2], (_Float16)a[3],
                                                   (_Float16)b[0], (_Float16)b[1], (_Float16)b[2], (_Float16)b[3]};
    }
  } else {
    for (long long i = t0; i < total; i += stride) dst[i] = (_Float16)src[i];
  }
}

template <bool VQ, bool VG>
void nearest_f16_launch(const NearestF16Args& a, hipStream_t s) {
  static std::atomic<unsigned long long> raised{0};
  ore_raise_lds_once(raised, reinterpret_cast<const void*>(nearest_f16_kernel<VQ, VG>), int(nf_lds_bytes(NF_DRES, 64)));
  const dim3 grid((unsigned)((a.n + NF_QT - 1) / NF_QT), (unsigned)a.S);
  hipLaunchKernelGGL((nearest_f16_kernel<VQ, VG>), grid, dim3(256), nf_lds_bytes(a.D, a.k), s, a);
}

}  // namespace

int nearest_f16_step_rows() { return NF_GT; }

int nearest_f16_segments(long long n, long long G, int ncu) {
  const long long qt = std::max<long long>((n + NF_QT - 1) / NF_QT, 1), steps = (G + NF_GT - 1) / NF_GT;
  // the f32 split: about two workgroups per CU, at most NF_SMAX segments and a step each
  const long long want = std::min<long long>(std::min(std::max<long long>(2LL * ncu / qt, 1), steps), NF_SMAX);
  const long long per = (steps + want - 1) / want;
  return int((steps + per - 1) / per);  // no segment is empty
}

void launch_gallery_f16(const float* src, long long G, long long D, void* dst, hipStream_t s) {
  const long long total = G * D;
  const bool vec = D % 8 == 0 && ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 15) == 0;
  const dim3 grid((unsigned)std::min<long long>(((vec ? total / 8 : total) + 255) / 256, 1 << 16));
  if (vec) hipLaunchKernelGGL(gallery_f16_kernel<true>, grid, dim3(256), 0, s, src, static_cast<_Float16*>(dst), total);
  else hipLaunchKernelGGL(gallery_f16_kernel<false>, grid, dim3(256), 0, s, src, static_cast<_Float16*>(dst), total);
}

void launch_nearest_f16(const float* q, long long q_stride, int n, int D, const void* gallery, long long G, int k, int S,
                        void* part, float* values, int* indices, hipStream_t s) {
  if (n <= 0) return;
  const long long steps = (G + NF_GT - 1) / NF_GT, per = (steps + S - 1) / S;
  const NearestF16Args a{q, static_cast<const _Float16*>(gallery), static_cast<u64*>(part), values, indices, q_stride, G,
                         per * NF_GT, n, D, k, S};
  const bool vg = D % 8 == 0 && (reinterpret_cast<uintptr_t>(gallery) & 15) == 0;
  const bool vq = D % 4 == 0 && q_stride % 4 == 0 && (reinterpret_cast<uintptr_t>(q) & 15) == 0;
  if (vq && vg) nearest_f16_launch<true, true>(a, s);
  else if (vg) nearest_f16_launch<false, true>(a, s);
  else if (vq) nearest_f16_launch<true, false>(a, s);
  else nearest_f16_launch<false, false>(a, s);
  if (S > 1) launch_nearest_merge(part, n, S, k, values, indices, s);
}

}  // namespace ore
