// Nearest neighbours by inner product (extension, ore_nearest_f32): for every query row the k
// best of its G scores against a gallery [G][D], without the [n][G] score matrix ever existing.  An f32 MFMA
// GEMM whose epilogue is a running selection under ore_topk_f32's order (the key of ore_topk_key.h).
//
// Split.  grid = (ceil(n / 64) query tiles, S gallery segments).  A workgroup of four waves owns QT = 64
// queries -- wave w the 16 queries 16 w .. 16 w + 15, as the B operand of v_mfma_f32_16x16x4_f32 -- and walks
// its segment in steps of GT = 64 gallery rows, the A operand of four MFMAs per k-step.  Lane l of a wave
// holds query l & 15 against gallery rows 16 b + 4 (l >> 4) + i of the step, b, i = 0 .. 3: 16 accumulators
// over the whole of D.  Segments only exist so that few queries still fill the chip (nearest_segments).
//
// Data movement.  Per chunk of KC = 32 d the 64 x 32 query tile and the 64 x 32 gallery tile are staged in LDS
// (pitch 36 floats: the 16 rows of a quarter wave start 4 banks apart, so the 16-byte operand reads are
// conflict-free).  Each thread moves two 16-byte groups per tile and chunk, loaded into registers one chunk
// ahead of the MFMAs (16-byte loads where base and row stride allow, four masked 4-byte loads otherwise).
// Rows past n or the segment and d past D are masked at the load and enter LDS as +0: no element outside the
// operands is read, and a pad never meets a NaN or an inf by a multiplication.
//
// Position independence.  K is never split across waves or workgroups.  Score (i, j) is one accumulator's
// chain over the chunks in ascending order, within a chunk two groups of 16 d, within a group four MFMAs of
// which MFMA s takes d = 4 kq + s (kq = l >> 4) -- an order that depends on D alone.  Padded products are +0
// and leave the accumulator unchanged (an accumulator is never -0: it starts at +0).  So the bits of s[i, j]
// depend only on q[i, :] and gallery[j, :], not on n, G, k, the row's place, the segments or the load path.
//
// Selection.  Per query, in LDS: the k best keys so far (descending), the k-th of them as the threshold (0
// while fewer than k are held), a candidate buffer of GT keys and its counter.  After a step a lane compares
// each of its 16 fresh keys with its query's threshold; a survivor takes a slot through an LDS atomic add.  A
// query of a wave is only ever touched by that wave.  A buffer may overflow on the next step as soon as it
// holds anything (GT survivors per step, GT slots), so every query that gained a candidate is compacted at
// the end of the step: the k rounds of topk_rounds over (k held + candidates), lane j keeping rank j, and the
// new threshold.  Keys are unique, so the order of insertions never shows.  After warm-up nearly every key fails
// the compare and no query is compacted; a gallery sorted ascending by score compacts every query every step.
//
// Merge.  S == 1: the workgroup writes values and indices itself.  S > 1: it writes its k keys (0 where the
// segment held fewer rows) to part[n][S][k]; nearest_merge_kernel, one wave per query, merges the S sorted
// lists through their heads held in registers (S + k keys read).  Every slot of part it reads was written by the
// first kernel.  values are decoded from the keys (topk_key_bits).
#include <algorithm>

#include "ore_nearest.h"

namespace ore {

namespace {

constexpr int NN_GT = 64;             // gallery rows per step
constexpr int NN_KC = 32;             // d per staged chunk
constexpr int NN_PITCH = NN_KC + 4;   // LDS row pitch in floats
constexpr int NN_CB = NN_GT;          // candidate slots per query
constexpr int NN_ML = NN_SMAX / 64;    // lists per lane of the merge's wave
constexpr int NN_STAGE = NN_QT * NN_PITCH;  // floats of one staged tile (NN_QT == NN_GT)
static_assert(NN_QT == NN_GT && NN_QT * NN_KC == 2 * 256 * 4, "two 16-byte groups per thread, tile and chunk");

// dynamic LDS: the two staged tiles, then per query the threshold, k keys, NN_CB candidates and the counter
__host__ __device__ constexpr size_t nn_lds_bytes(int k) {
  return size_t(2) * NN_STAGE * 4 + size_t(NN_QT) * (8 + 8 * size_t(k) + 8 * NN_CB + 4);
}

template <bool VQ, bool VG>  // 16-byte loads of the queries / of the gallery
__global__ __launch_bounds__(256) void nearest_kernel(NearestArgs p) {
  extern __shared__ __attribute__((aligned(16))) float nn_lds[];
  float* const sq = nn_lds;
  float* const sg = nn_lds + NN_STAGE;
  u64* const sthr = reinterpret_cast<u64*>(nn_lds + 2 * NN_STAGE);
  u64* const stop = sthr + NN_QT;                 // [NN_QT][k]
  u64* const scand = stop + NN_QT * p.k;          // [NN_QT][NN_CB]
  int* const scnt = reinterpret_cast<int*>(scand + NN_QT * NN_CB);

  const int tid = threadIdx.x, lane = tid & 63, lr = lane & 15, kq = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const long long q0 = (long long)blockIdx.x * NN_QT;
  const int seg = blockIdx.y;
  const long long jbeg = (long long)seg * p.seg_rows, jend = min(p.G, jbeg + p.seg_rows);
  const int nsteps = int((jend - jbeg + NN_GT - 1) / NN_GT);  // >= 1: the launcher leaves no segment empty
  const int nchunks = (p.D + NN_KC - 1) / NN_KC;
  const float* const g = static_cast<const float*>(p.g);

  for (int i = tid; i < NN_QT; i += 256) {
    sthr[i] = 0ull;
    scnt[i] = 0;
  }
  for (int i = tid; i < NN_QT * p.k; i += 256) stop[i] = 0ull;

  // this thread's two groups of a tile: rows tid >> 3 and (tid >> 3) + 32, d offset 4 (tid & 7)
  const int srow = tid >> 3, sd = 4 * (tid & 7);
  floatx4 rq[2], rg[2];
  auto fetch = [&](long long j0, int c) __attribute__((always_inline)) {
    const int d = c * NN_KC + sd;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const long long qi = q0 + srow + 32 * u, gj = j0 + srow + 32 * u;
      rq[u] = nn_load4<VQ>(qi < p.n, p.q + qi * p.q_stride, d, p.D);
      rg[u] = nn_load4<VG>(gj < jend, g + gj * p.D, d, p.D);
    }
  };

  const int ql = 16 * wave + lr;  // this lane's query within the tile
  const bool q_ok = q0 + ql < p.n;
  const float* const bq = sq + ql * NN_PITCH + 4 * kq;
  const float* const ag = sg + lr * NN_PITCH + 4 * kq;

  fetch(jbeg, 0);
  for (int st = 0; st < nsteps; ++st) {
    const long long j0 = jbeg + (long long)st * NN_GT;
    floatx4 acc[4];
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[b] = floatx4{0.0f, 0.0f, 0.0f, 0.0f};
    for (int c = 0; c < nchunks; ++c) {
      __syncthreads();  // the previous chunk's operand reads (and, first, the state's initialisation) are done
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        *reinterpret_cast<floatx4*>(sq + (srow + 32 * u) * NN_PITCH + sd) = rq[u];
        *reinterpret_cast<floatx4*>(sg + (srow + 32 * u) * NN_PITCH + sd) = rg[u];
      }
      __syncthreads();
      if (c + 1 < nchunks) fetch(j0, c + 1);           // the next chunk's loads under this chunk's MFMAs
      else if (st + 1 < nsteps) fetch(j0 + NN_GT, 0);
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        if (c * NN_KC + 16 * h < p.D) {  // a group of 16 d that is all padding adds nothing (uniform; D alone decides)
          const floatx4 bv = *reinterpret_cast<const floatx4*>(bq + 16 * h);
          floatx4 av[4];
#pragma unroll
          for (int b = 0; b < 4; ++b) av[b] = *reinterpret_cast<const floatx4*>(ag + 16 * b * NN_PITCH + 16 * h);
#pragma unroll
          for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int b = 0; b < 4; ++b) acc[b] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[b][s], bv[s], acc[b], 0, 0, 0);
        }
      }
    }
    // the step's scores against the thresholds: acc[b][i] is query ql against gallery row j0 + 16 b + 4 kq + i
    const u64 thr = sthr[ql];
#pragma unroll
    for (int b = 0; b < 4; ++b)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const long long j = j0 + 16 * b + 4 * kq + i;
        const u64 key = topk_key(__float_as_uint(acc[b][i]), int(j));
        if (q_ok && j < jend && key > thr) {
          const int slot = atomicAdd(&scnt[ql], 1);  // < NN_CB: the buffer was empty and a step brings NN_GT keys
          scand[ql * NN_CB + slot] = key;
        }
      }
    __syncthreads();
    for (int t = 0; t < 16; ++t) {  // this wave's queries that gained a candidate: k held + candidates -> k held
      const int qi = 16 * wave + t;
      const int cnt = __builtin_amdgcn_readfirstlane(scnt[qi]);
      if (cnt == 0) continue;  // wave-uniform
      u64 key[2];
      key[0] = lane < p.k ? stop[qi * p.k + lane] : 0ull;
      key[1] = lane < cnt ? scand[qi * NN_CB + lane] : 0ull;
      const u64 mine = topk_rounds<2>(key, p.k, lane);
      if (lane < p.k) stop[qi * p.k + lane] = mine;
      if (lane == p.k - 1) sthr[qi] = mine;  // 0 while fewer than k are held: every key passes
      if (lane == 0) scnt[qi] = 0;
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

// One wavefront per query: the k best of its S partial lists.  A list is k keys in descending order, 0 from the
// first empty slot on.  Lane l owns lists l, l + 64, ... (at most NN_ML: S <= NN_SMAX) and keeps the first
// unconsumed key of each in a register; a round takes the largest head of the wave, and the one lane that held it
// (keys are unique) loads that list's next key.  S + k keys are read in all, not S k per round.
__global__ __launch_bounds__(256) void nearest_merge_kernel(const u64* __restrict__ part, long long n, int S, int k,
                                                            float* __restrict__ values, int* __restrict__ indices) {
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= n) return;  // wave-uniform; no barrier in this kernel
  const u64* pr = part + row * S * k;
  u64 head[NN_ML];
  int pos[NN_ML];
#pragma unroll
  for (int t = 0; t < NN_ML; ++t) {
    const int s = lane + 64 * t;
    head[t] = s < S ? pr[(long long)s * k] : 0ull;
    pos[t] = 0;
  }
  u64 mine = 0ull;
  for (int j = 0; j < k; ++j) {  // wave-uniform trip count
    u64 best = 0ull;
#pragma unroll
    for (int t = 0; t < NN_ML; ++t) best = head[t] > best ? head[t] : best;
    const u64 win = wave_max(best);  // never 0: G >= k keys are held in all
    mine = lane == j ? win : mine;
#pragma unroll
    for (int t = 0; t < NN_ML; ++t)
      if (win != 0ull && head[t] == win) {  // a head that is not 0 belongs to a list below S
        ++pos[t];
        head[t] = pos[t] < k ? pr[(long long)(lane + 64 * t) * k + pos[t]] : 0ull;
      }
  }
  if (lane < k && mine != 0ull) {
    reinterpret_cast<unsigned*>(values)[row * k + lane] = topk_key_bits(mine);
    indices[row * k + lane] = topk_key_index(mine);
  }
}

// e[r, :] /= sqrt(sum e[r, :]^2), one wavefront per row; a zero row stays zero
__global__ __launch_bounds__(256) void l2_normalize_kernel(float* __restrict__ e, long long rows, int C) {
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  float* er = e + row * C;
  float s = 0.0f;
  for (int i = lane; i < C; i += 64) s = fmaf(er[i], er[i], s);
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o);
  if (s == 0.0f) return;
  const float norm = sqrtf(s);
  for (int i = lane; i < C; i += 64) er[i] = er[i] / norm;
}

struct NearestF32 {
  static constexpr int GT = NN_GT, VGE = 4;
  static constexpr size_t LDS_MAX = nn_lds_bytes(64);
  static constexpr size_t lds(int, int k) { return nn_lds_bytes(k); }
  template <bool VQ, bool VG>
  static auto kernel() { return &nearest_kernel<VQ, VG>; }
};

}  // namespace

int nearest_step_rows(NearestFmt f) { return f == NearestFmt::F32 ? NN_GT : NS_GT; }

int nearest_segments(long long n, long long G, int ncu, int step_rows) {
  const long long qt = std::max<long long>((n + NN_QT - 1) / NN_QT, 1), steps = (G + step_rows - 1) / step_rows;
  // about two workgroups per CU, at most NN_SMAX segments (the merge's lists per lane) and a step each
  const long long want = std::min<long long>(std::min(std::max<long long>(2LL * ncu / qt, 1), steps), NN_SMAX);
  const long long per = (steps + want - 1) / want;
  return int((steps + per - 1) / per);  // no segment is empty
}

size_t nearest_partial_bytes(long long n, int S, int k) { return S > 1 ? size_t(n) * size_t(S) * size_t(k) * 8 : 0; }

void launch_nearest(const float* q, long long q_stride, int n, int D, const void* gallery, const float* scales, long long G, int k,
                    int S, void* part, float* values, int* indices, hipStream_t s) {
  nearest_launch<NearestF32>(q, q_stride, n, D, gallery, scales, G, k, S, part, values, indices, s);
}

void launch_nearest_merge(const void* part, long long n, int S, int k, float* values, int* indices, hipStream_t s) {
  hipLaunchKernelGGL(nearest_merge_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, s, static_cast<const u64*>(part), n, S,
                     k, values, indices);
}

void launch_l2_normalize(float* e, long long rows, int C, hipStream_t s) {
  if (rows <= 0) return;
  hipLaunchKernelGGL(l2_normalize_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, e, rows, C);
}

}  // namespace ore
