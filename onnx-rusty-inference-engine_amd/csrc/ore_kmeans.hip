// One Lloyd iteration of spherical k-means (extension, ore_kmeans_step_f32): every sample row goes to
// the centroid with the largest inner product, scored to the bit as ore_nearest_f16 with k = 1 scores it, and a
// centroid becomes the normalised sum of its rows.  Two kernels behind launch_gallery_f16's rounding of the centroids.
//
// 1. Assignment.  grid = ceil(S / 64), four waves.  The workgroup rounds its 64 sample rows once to f16 into LDS, the B
//    operand: ore_nearest.h's tile, rows of D (in whole ring turns) + 8 halves, an odd multiple of 4 banks apart; D <=
//    512, so it is always resident.  Then it walks all L centroids by itself, the A operand, as ore_nearest.h walks a
//    segment: steps of 128 rows, wave w rows 32 w .. 32 w + 31 as two A operands, straight from global memory (L2: the
//    centroids are a few MB and every workgroup reads them) through a ring of 8 k-groups of registers, a turn of the
//    ring straight-line code, addresses masked and not branched (a row past L or a d past D reads the centroids' first
//    bytes and is zeroed on its bits when consumed).  There is no selection state in LDS: with k = 1 a lane folds the
//    eight scores it holds per sample column into one running ore_topk_key.h key per column, in registers, across all
//    steps.  The key order is associative, so the fold across the four lanes that share a column waits for the end of
//    the walk (two swaps), and the four waves' keys meet once through 2 KB of LDS.  No slots, no partial buffer, no
//    merge launch: LDS is the tile + 2 KB, twice on a compute unit at D = 512.
//
// 2. Update.  grid = ceil(L / KM_UC): a workgroup owns KM_UC consecutive centroids and reads assign[0 .. S) in ascending
//    order, 2048 rows a batch (thread t rows b + 256 j + t).  Per centroid and j a ballot per wave gives the lane's
//    place among the wave's matches and the wave's count; the counts go through LDS (double buffered: one barrier a
//    batch) and every thread walks them in (j, wave) order, so a matching row lands in its centroid's queue in ascending
//    row order.  A queue that holds KM_UQ rows or more is drained: the f32 loads of KM_UL rows are issued together and
//    added in queue order into f64 accumulators, thread t columns t and t + 256.  At the end count, norm^2 = sum_d
//    sum_d^2 (f64: lanes by a butterfly, waves in order) and out = (float)(sum_d / sqrt(norm^2)); no row, or a norm^2
//    that is 0 or not finite: the input centroid's bits.  No atomics: the bits depend on the inputs alone.
#include "../../include/ore.h"
#include "ore_nearest.h"

namespace ore {

namespace {

typedef _Float16 halfx4 __attribute__((ext_vector_type(4)));
typedef _Float16 halfx8 __attribute__((ext_vector_type(8)));
typedef unsigned uintx4 __attribute__((ext_vector_type(4)));
typedef int intx4 __attribute__((ext_vector_type(4)));

constexpr int KM_KG = 32, KM_OE = 8, KM_PAD = 8;  // d per MFMA, halves per operand, halves added to the tile's pitch
constexpr int KM_UC = 1;                          // update: centroids per workgroup (1, 2, 4 measured)
constexpr int KM_UB = 8;                          // rows of assign per thread and batch
constexpr int KM_UL = 8;                          // row loads in flight per thread and column
constexpr int KM_UQ = 32;                         // queued rows from which a queue is drained
constexpr int KM_QCAP = 256 * KM_UB + KM_UQ;      // a batch on top of what stayed below KM_UQ

struct KmeansArgs {
  const float* x;
  const _Float16* c16;  // [L][D], the rounded centroids
  const float* cent;    // [L][D]
  float* out;           // [L][D], may be cent
  int* assign;          // [S]
  float* scores;        // [S] or null
  int* counts;          // [L]
  long long x_stride;
  int S, D, L;
};

// one centroid operand without a branch, and its zeroing when it is consumed: FmtF16's pair (ore_nearest_f16.hip)
template <bool VEC>
__device__ __forceinline__ halfx8 km_load(bool row_ok, const _Float16* __restrict__ row, int d, int D, const _Float16* __restrict__ safe) {
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
__device__ __forceinline__ halfx8 km_mask(halfx8 v, bool row_ok, int d, int D) {
  if (VEC) {
    const unsigned m = row_ok && d < D ? ~0u : 0u;  // on the bits: a masked NaN or inf becomes +0 too
    return __builtin_bit_cast(halfx8, __builtin_bit_cast(uintx4, v) & uintx4{m, m, m, m});
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) v[e] = row_ok && d + e < D ? v[e] : (_Float16)0.0f;
  return v;
}

// the largest key of the four lanes l & 15, + 16, + 32, + 48, in each of them: wave_max's two steps across rows
__device__ __forceinline__ u64 km_rows_max(u64 v) {
  const unsigned lo = unsigned(v), hi = unsigned(v >> 32);
  auto l16 = __builtin_amdgcn_permlane16_swap(lo, lo, false, false);
  auto h16 = __builtin_amdgcn_permlane16_swap(hi, hi, false, false);
  const u64 a = (u64(h16[0]) << 32) | l16[0], b = (u64(h16[1]) << 32) | l16[1];
  v = a > b ? a : b;
  auto l32 = __builtin_amdgcn_permlane32_swap(unsigned(v), unsigned(v), false, false);
  auto h32 = __builtin_amdgcn_permlane32_swap(unsigned(v >> 32), unsigned(v >> 32), false, false);
  const u64 c = (u64(h32[0]) << 32) | l32[0], d = (u64(h32[1]) << 32) | l32[1];
  return c > d ? c : d;
}

__host__ __device__ constexpr int km_tile_d(int D) { return (D + KM_KG * NS_PF - 1) / (KM_KG * NS_PF) * (KM_KG * NS_PF); }
// dynamic LDS: the tile, then one key per wave and sample column
__host__ __device__ constexpr size_t km_lds_bytes(int D) { return size_t(NN_QT) * (km_tile_d(D) + KM_PAD) * 2 + 4 * NN_QT * 8; }
static_assert(2 * km_lds_bytes(ORE_KMEANS_MAX_D) <= 160 * 1024, "two workgroups per compute unit");

template <bool VX, bool VC>  // 16-byte loads of the samples / of the centroids
__global__ __launch_bounds__(256, 2) void kmeans_assign_kernel(KmeansArgs p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char km_lds[];
  const int clen = km_tile_d(p.D), pitch = clen + KM_PAD, nkg = clen / KM_KG;
  _Float16* const sx = reinterpret_cast<_Float16*>(km_lds);
  u64* const sbest = reinterpret_cast<u64*>(km_lds + size_t(NN_QT) * pitch * 2);  // [4][NN_QT]

  const int tid = threadIdx.x, lane = tid & 63, lr = lane & 15, kq = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const long long i0 = (long long)blockIdx.x * NN_QT;
  const int nsteps = (p.L + NS_GT - 1) / NS_GT;

  // the sample rows, rounded once: a wave per row, a lane per group of four d; a row past S and d past D are zero
  for (int r = wave; r < NN_QT; r += 4) {
    const float* const row = p.x + (i0 + r) * p.x_stride;
    for (int g4 = lane; 4 * g4 < clen; g4 += 64) {
      const floatx4 v = nn_load4<VX>(i0 + r < p.S, row, 4 * g4, p.D);
      *reinterpret_cast<halfx4*>(sx + r * pitch + 4 * g4) = halfx4{(_Float16)v[0], (_Float16)v[1], (_Float16)v[2], (_Float16)v[3]};
    }
  }

  // k-group kg of step st of this wave's rows: lane l takes the 8 d from 32 kg + 8 (l >> 4) of rows (l & 15), + 16
  halfx8 ring[NS_PF][2];
  const int jl = NS_WR * wave + lr;  // this lane's first row of step 0
  const _Float16* const gl = p.c16 + (long long)jl * p.D;
  auto fetch = [&](int slot, int st, int kg) __attribute__((always_inline)) {
    const int sj = st * NS_GT;  // st == nsteps: past L, nothing of it is read
#pragma unroll
    for (int rb = 0; rb < 2; ++rb)
      ring[slot][rb] = km_load<VC>(jl + sj + 16 * rb < p.L, gl + (long long)(sj + 16 * rb) * p.D, KM_KG * kg + KM_OE * kq, p.D, p.c16);
  };
  const _Float16* const bq = sx + lr * pitch + KM_OE * kq;
#pragma unroll
  for (int u = 0; u < NS_PF; ++u) {
    fetch(u, 0, u);
    __builtin_amdgcn_sched_barrier(0);
  }
  __syncthreads();  // the tile is whole

  u64 best[4] = {0ull, 0ull, 0ull, 0ull};  // column 16 qb + lr over this lane's rows so far; 0: none
  for (int st = 0; st < nsteps; ++st) {
    const int j0 = st * NS_GT;
    floatx4 acc[4][2];
#pragma unroll
    for (int qb = 0; qb < 4; ++qb) acc[qb][0] = acc[qb][1] = floatx4{0.0f, 0.0f, 0.0f, 0.0f};
    for (int kg0 = 0; kg0 < nkg; kg0 += NS_PF) {
      // one turn of the ring, without a branch: k-group kg0 + u is consumed from slot u, which then takes the k-group
      // NS_PF further on (into the next step at the end of this one); the k-groups past D multiply zero by zero
#pragma unroll
      for (int u = 0; u < NS_PF; ++u) {
        const int kg = kg0 + u;
        const halfx8 a0 = km_mask<VC>(ring[u][0], jl + j0 < p.L, KM_KG * kg + KM_OE * kq, p.D);
        const halfx8 a1 = km_mask<VC>(ring[u][1], jl + j0 + 16 < p.L, KM_KG * kg + KM_OE * kq, p.D);
#pragma unroll
        for (int qb = 0; qb < 4; ++qb) {
          const halfx8 bv = *reinterpret_cast<const halfx8*>(bq + KM_KG * kg + 16 * qb * pitch);
          acc[qb][0] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a0, bv, acc[qb][0], 0, 0, 0);
          acc[qb][1] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a1, bv, acc[qb][1], 0, 0, 0);
        }
        const bool wrap = kg + NS_PF >= nkg;
        fetch(u, st + wrap, kg + NS_PF - (wrap ? nkg : 0));
        __builtin_amdgcn_sched_barrier(0);  // the loads stay in the ring's order
      }
    }
    // acc[qb][rb][i] is sample 16 qb + lr against centroid j0 + 32 w + 16 rb + 4 kq + i: the lane's eight into its key
#pragma unroll
    for (int qb = 0; qb < 4; ++qb) {
      u64 b = best[qb];
#pragma unroll
      for (int rb = 0; rb < 2; ++rb)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int j = j0 + NS_WR * wave + 16 * rb + 4 * kq + i;
          const u64 key = j < p.L ? topk_key(__float_as_uint(acc[qb][rb][i]), j) : 0ull;
          b = key > b ? key : b;
        }
      best[qb] = b;
    }
  }
  // the four lanes of a column, then the four waves: L >= 1, so every column holds a key
#pragma unroll
  for (int qb = 0; qb < 4; ++qb) {
    const u64 v = km_rows_max(best[qb]);
    if (kq == 0) sbest[wave * NN_QT + 16 * qb + lr] = v;
  }
  __syncthreads();
  if (tid < NN_QT && i0 + tid < p.S) {
    u64 v = sbest[tid];
#pragma unroll
    for (int w = 1; w < 4; ++w) v = sbest[w * NN_QT + tid] > v ? sbest[w * NN_QT + tid] : v;
    p.assign[i0 + tid] = topk_key_index(v);
    if (p.scores) reinterpret_cast<unsigned*>(p.scores)[i0 + tid] = topk_key_bits(v);
  }
}

__global__ __launch_bounds__(256) void kmeans_update_kernel(KmeansArgs p) {
  __shared__ int squeue[KM_UC][KM_QCAP];
  __shared__ __attribute__((aligned(16))) int scnt[2][KM_UC][KM_UB][4];
  __shared__ double sred[KM_UC][4];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l0 = blockIdx.x * KM_UC;
  const bool d0 = tid < p.D, d1 = tid + 256 < p.D;
  double acc[KM_UC][2];
  int qn[KM_UC], total[KM_UC];  // rows queued, rows seen: uniform over the workgroup
#pragma unroll
  for (int c = 0; c < KM_UC; ++c) acc[c][0] = acc[c][1] = 0.0, qn[c] = total[c] = 0;

  // the queue of centroid c into its sums, in queue order; the loads of KM_UL rows at a time
  auto drain = [&](int c) __attribute__((always_inline)) {
    const int n = qn[c];
    int g = 0;
    for (; g + KM_UL <= n; g += KM_UL) {
      float v[KM_UL][2];
#pragma unroll
      for (int u = 0; u < KM_UL; ++u) {
        const float* const row = p.x + (long long)squeue[c][g + u] * p.x_stride;
        v[u][0] = d0 ? row[tid] : 0.0f;
        v[u][1] = d1 ? row[tid + 256] : 0.0f;
      }
#pragma unroll
      for (int u = 0; u < KM_UL; ++u) acc[c][0] += double(v[u][0]), acc[c][1] += double(v[u][1]);
    }
    for (; g < n; ++g) {
      const float* const row = p.x + (long long)squeue[c][g] * p.x_stride;
      acc[c][0] += double(d0 ? row[tid] : 0.0f);
      acc[c][1] += double(d1 ? row[tid + 256] : 0.0f);
    }
    total[c] += n;
    qn[c] = 0;
  };

  int buf = 0, next[KM_UB];  // the batch after this one, loaded a batch ahead: -1 past S
#pragma unroll
  for (int j = 0; j < KM_UB; ++j) next[j] = 256 * j + tid < p.S ? p.assign[256 * j + tid] : -1;
  for (long long b = 0; b < p.S; b += 256 * KM_UB, buf ^= 1) {
    int m[KM_UB], pre[KM_UB];  // the row's centroid relative to l0, and its place among the wave's matches
#pragma unroll
    for (int j = 0; j < KM_UB; ++j) {
      const long long i = b + 256 * (KM_UB + j) + tid;
      m[j] = next[j] - l0;
      next[j] = i < p.S ? p.assign[i] : -1;
      pre[j] = 0;
    }
#pragma unroll
    for (int c = 0; c < KM_UC; ++c)
#pragma unroll
      for (int j = 0; j < KM_UB; ++j) {
        const unsigned long long hit = __ballot(m[j] == c);
        if (m[j] == c) pre[j] = __popcll(hit & ((1ull << lane) - 1ull));
        if (lane == 0) scnt[buf][c][j][wave] = __popcll(hit);
      }
    __syncthreads();  // the counts are whole; the drains of the batch before are done
    bool full = false;
#pragma unroll
    for (int c = 0; c < KM_UC; ++c) {
      int at = qn[c];
#pragma unroll
      for (int j = 0; j < KM_UB; ++j) {
        const intx4 n = *reinterpret_cast<const intx4*>(scnt[buf][c][j]);
        const int mine = at + (wave > 0 ? n[0] : 0) + (wave > 1 ? n[1] : 0) + (wave > 2 ? n[2] : 0);  // behind the waves before
        if (m[j] == c) squeue[c][mine + pre[j]] = int(b + 256 * j + tid);
        at += n[0] + n[1] + n[2] + n[3];
      }
      qn[c] = at;
      full |= at >= KM_UQ;
    }
    if (full) {  // uniform
      __syncthreads();
#pragma unroll
      for (int c = 0; c < KM_UC; ++c)
        if (qn[c] >= KM_UQ) drain(c);
    }
  }
  __syncthreads();
#pragma unroll
  for (int c = 0; c < KM_UC; ++c) drain(c);

#pragma unroll
  for (int c = 0; c < KM_UC; ++c) {  // norm^2: the thread's two columns, the lanes by a butterfly, the waves in order
    double s = acc[c][0] * acc[c][0] + acc[c][1] * acc[c][1];
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o);
    if (lane == 0) sred[c][wave] = s;
  }
  __syncthreads();
#pragma unroll
  for (int c = 0; c < KM_UC; ++c) {
    const int l = l0 + c;
    if (l >= p.L) break;  // uniform
    const double n2 = ((sred[c][0] + sred[c][1]) + sred[c][2]) + sred[c][3];
    const bool ok = total[c] > 0 && n2 > 0.0 && n2 < __builtin_inf();  // false for a NaN
    const double r = sqrt(n2);
    if (tid == 0) p.counts[l] = total[c];
    const long long at = (long long)l * p.D + tid;
    if (d0) p.out[at] = ok ? float(acc[c][0] / r) : p.cent[at];
    if (d1) p.out[at + 256] = ok ? float(acc[c][1] / r) : p.cent[at + 256];
  }
}

}  // namespace

size_t kmeans_scratch_bytes(int L, int D) { return size_t(L) * D * 2; }

void launch_kmeans_assign(const float* x, long long x_stride, int S, int D, const void* centroids_f16, int L, int* assign,
                          float* scores, hipStream_t s) {
  if (S <= 0) return;
  static std::atomic<unsigned long long> raised[4];
  const KmeansArgs a{x, static_cast<const _Float16*>(centroids_f16), nullptr, nullptr, assign, scores, nullptr, x_stride, S, D, L};
  const bool vc = D % 8 == 0 && (reinterpret_cast<uintptr_t>(centroids_f16) & 15) == 0;
  const bool vx = D % 4 == 0 && x_stride % 4 == 0 && (reinterpret_cast<uintptr_t>(x) & 15) == 0;
  const auto kernel = vx ? (vc ? &kmeans_assign_kernel<true, true> : &kmeans_assign_kernel<true, false>)
                         : (vc ? &kmeans_assign_kernel<false, true> : &kmeans_assign_kernel<false, false>);
  ore_raise_lds_once(raised[2 * vx + vc], reinterpret_cast<const void*>(kernel), int(km_lds_bytes(ORE_KMEANS_MAX_D)));
  hipLaunchKernelGGL(kernel, dim3((unsigned)((S + NN_QT - 1) / NN_QT)), dim3(256), km_lds_bytes(D), s, a);
}

void launch_kmeans_update(const float* x, long long x_stride, int S, int D, const float* centroids, int L, const int* assign,
                          float* centroids_out, int* counts, hipStream_t s) {
  const KmeansArgs a{x, nullptr, centroids, centroids_out, const_cast<int*>(assign), nullptr, counts, x_stride, S, D, L};
  hipLaunchKernelGGL(kmeans_update_kernel, dim3((unsigned)((L + KM_UC - 1) / KM_UC)), dim3(256), 0, s, a);
}

}  // namespace ore
