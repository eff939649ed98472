// Inverted-file search on an f16 gallery stored list by list (extension, ore_nearest_lists_f16): per
// query the k best rows of the union of the lists its row of probes names, scored to the bit as ore_nearest_f16
// scores them.  Every other search reads the whole gallery; this one reads the probed lists, and a list once per 64
// queries that probe it, however many those are.
//
// Three stages, six launches, all sized from host-known numbers (n, P, L, the chunk table's length, C = ceil(
// max_list_rows / IVF_R)); the scratch is cnt [L], start [L + 1], pairs [n P] and part [n P][C][k] keys.
//
// 1. Inversion.  Pair e = i P + p is query i's p-th probe.  ivf_pair_list gives its list, or -1 for padding (an entry
//    outside [0, L)) and for a list that an earlier entry of the same row names: that rule is evaluated wherever a
//    pair is looked at (count, fill, merge) and nothing of it is stored.  count: atomicAdd per valid pair into cnt
//    (cleared by a kernel: a memset node is not recorded into a capture).  scan: one workgroup, an exclusive scan over
//    L in tiles of 1024 with a carry; it leaves start and clears cnt again, which fill then uses as the lists'
//    cursors: pairs[start[l] + atomicAdd(cnt + l, 1)] = e.  The order of the pairs of a list varies from run to run;
//    which group and which MFMA column a pair lands in varies with it, and the output does not: a score is one
//    accumulator's chain over its own two rows, and keys are unique.
//
// 2. List-major scan.  grid = the chunk table, four waves.  Workgroup b takes chunk (list l, first row): at most
//    IVF_R rows of one list.  Everything it reads from the tables is clipped: l to [0, L), the list's rows to [0, G],
//    `first` to a whole chunk inside the list, the slot to C, start to [0, n P], a pair id to [0, n P) -- a workgroup
//    that finds its entry out of range returns, as does one whose list has no pair.  It walks the list's pairs in
//    groups of up to 64.  A group's query rows are gathered through the pair ids, rounded once to f16 and kept in LDS
//    as ore_nearest.h's tile: rows of D (in whole ring turns) + 8 halves, an odd multiple of 4 banks apart.  Then the
//    chunk's rows stream against it as in ore_nearest.h: steps of 128 rows, wave w rows 32 w .. 32 w + 31 as two A
//    operands, straight from global memory through a ring of 8 k-groups, a turn of the ring straight-line code,
//    addresses masked and not branched (a row past the chunk or a d past D reads the gallery's first bytes and is
//    zeroed on its bits when consumed).  A group of <= 16, <= 32, <= 48 pairs runs the instance of the step with one,
//    two, three B blocks: the choice is a branch around the group's whole K walk (16-byte path; the element-load path
//    always runs four: with the choice it spilled).  Selection is ore_nearest.h's (the
//    slots are the rows, a running k best per pair across the chunk's steps); the k keys of the chunk go to
//    part[e][slot][0 .. k), all k of them (0 = empty).
//
// 3. Merge.  One wave per query.  Lane p knows pair p's list and so how many chunk slots the scan wrote for it
//    (ceil(rows / IVF_R), at most C); only those are read, so what the buffer held before is never looked at.  The
//    P C k keys go through topk_rounds 128 at a time beside the k held; a batch with no key is skipped.  Equal keys
//    collapse in the rounds; ranks past the union keep key 0: index -1 and the NaN 0x7fc00000.
#include <algorithm>

#include "../../include/ore.h"
#include "ore_nearest.h"

namespace ore {

namespace {

typedef _Float16 halfx4 __attribute__((ext_vector_type(4)));
typedef _Float16 halfx8 __attribute__((ext_vector_type(8)));
typedef unsigned uintx4 __attribute__((ext_vector_type(4)));

constexpr int IVF_R = ORE_IVF_CHUNK_ROWS;  // two steps
constexpr int IVF_MAX_D = ORE_IVF_MAX_D;   // the tile is resident
constexpr int IVF_KG = 32, IVF_OE = 8, IVF_PAD = 8;
static_assert(IVF_R % NS_GT == 0, "chunks of whole steps");

struct IvfArgs {
  const float* q;
  const _Float16* g;
  const int* offsets;  // [L + 1]
  const int* chunks;   // [n_chunks][2]
  const int* probes;   // [n][probe_stride]
  int* cnt;            // [L]
  int* start;          // [L + 1]
  int* pairs;          // [n P]
  u64* part;           // [n P][C][k]
  float* values;
  int* indices;
  long long q_stride, G, probe_stride;
  int n, D, k, L, P, C;
};

// the list of pair (i, p), or -1: padding, or named by an earlier entry of the row
__device__ __forceinline__ int ivf_pair_list(const int* __restrict__ row, int p, int L) {
  const int l = row[p];
  if (l < 0 || l >= L) return -1;
  for (int t = 0; t < p; ++t)
    if (row[t] == l) return -1;
  return l;
}

// the rows of list l, clipped to the gallery
__device__ __forceinline__ void ivf_list_rows(const int* __restrict__ offsets, int l, long long G, int& lo, int& hi) {
  lo = int(min((long long)max(offsets[l], 0), G));
  hi = int(min((long long)max(offsets[l + 1], lo), G));
}

__global__ __launch_bounds__(256) void ivf_clear_kernel(int* __restrict__ cnt, int L) {
  const int l = blockIdx.x * 256 + threadIdx.x;
  if (l < L) cnt[l] = 0;
}

template <bool FILL>
__global__ __launch_bounds__(256) void ivf_invert_kernel(IvfArgs p) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= (long long)p.n * p.P) return;
  const int l = ivf_pair_list(p.probes + (e / p.P) * p.probe_stride, int(e % p.P), p.L);
  if (l < 0) return;
  const int at = atomicAdd(p.cnt + l, 1);
  if (FILL) p.pairs[p.start[l] + at] = int(e);
}

// start[l] = the pairs of the lists before l, start[L] = all of them; cnt back to 0.  One workgroup of 1024
__global__ __launch_bounds__(1024) void ivf_scan_kernel(int* __restrict__ cnt, int* __restrict__ start, int L) {
  __shared__ int s[1024];
  const int tid = threadIdx.x;
  int carry = 0;
  for (int l0 = 0; l0 < L; l0 += 1024) {
    const int l = l0 + tid, c = l < L ? cnt[l] : 0;
    s[tid] = c;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {
      const int v = tid >= d ? s[tid - d] : 0;
      __syncthreads();
      s[tid] += v;
      __syncthreads();
    }
    if (l < L) {
      start[l] = carry + s[tid] - c;
      cnt[l] = 0;
    }
    carry += s[1023];
    __syncthreads();
  }
  if (tid == 0) start[L] = carry;
}

// one gallery operand without a branch, and its zeroing when it is consumed: FmtF16's pair (ore_nearest_f16.hip)
template <bool VEC>
__device__ __forceinline__ halfx8 ivf_load(bool row_ok, const _Float16* __restrict__ row, int d, int D, const _Float16* __restrict__ safe) {
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
__device__ __forceinline__ halfx8 ivf_mask(halfx8 v, bool row_ok, int d, int D) {
  if (VEC) {
    const unsigned m = row_ok && d < D ? ~0u : 0u;  // on the bits: a masked NaN or inf becomes +0 too
    return __builtin_bit_cast(halfx8, __builtin_bit_cast(uintx4, v) & uintx4{m, m, m, m});
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) v[e] = row_ok && d + e < D ? v[e] : (_Float16)0.0f;
  return v;
}

__host__ __device__ constexpr int ivf_tile_d(int D) { return (D + IVF_KG * NS_PF - 1) / (IVF_KG * NS_PF) * (IVF_KG * NS_PF); }
// dynamic LDS: the tile, then per pair of the group the threshold, k keys, NS_GT slots, the flag and the pair id
__host__ __device__ constexpr size_t ivf_lds_bytes(int D, int k) {
  return size_t(NN_QT) * (ivf_tile_d(D) + IVF_PAD) * 2 + size_t(NN_QT) * (8 + 8 * size_t(k) + 4 * NS_GT + 4 + 4);
}
static_assert(ivf_lds_bytes(IVF_MAX_D, 64) <= 160 * 1024, "LDS");

struct IvfLds {
  const _Float16* sq;
  u64* sthr;
  u64* stop;
  unsigned* scand;
  int* sflag;
};

// One group against the chunk's rows [jbeg, jend): ore_nearest.h's resident K walk and selection with NB query blocks
template <int NB, bool VG>
__device__ __forceinline__ void ivf_group(const IvfArgs& p, const IvfLds& s, long long jbeg, long long jend, int npairs, int pitch, int nkg,
                                          int wave, int lane) {
  const int lr = lane & 15, kq = lane >> 4;
  const int nsteps = int((jend - jbeg + NS_GT - 1) / NS_GT);
  halfx8 ring[NS_PF][2];
  const long long jl = jbeg + NS_WR * wave + lr;  // this lane's first row of step 0
  const _Float16* const gl = p.g + jl * p.D;
  auto fetch = [&](int slot, int st, int kg) __attribute__((always_inline)) {
    const int sj = st * NS_GT;  // st == nsteps: past jend, nothing of it is read
#pragma unroll
    for (int rb = 0; rb < 2; ++rb)
      ring[slot][rb] = ivf_load<VG>(jl + sj + 16 * rb < jend, gl + (long long)(sj + 16 * rb) * p.D, IVF_KG * kg + IVF_OE * kq, p.D, p.g);
  };
  const _Float16* const bq = s.sq + lr * pitch + IVF_OE * kq;
#pragma unroll
  for (int u = 0; u < NS_PF; ++u) {
    fetch(u, 0, u);
    __builtin_amdgcn_sched_barrier(0);
  }
  for (int st = 0; st < nsteps; ++st) {
    const long long j0 = jbeg + st * NS_GT;
    floatx4 acc[NB][2];
#pragma unroll
    for (int qb = 0; qb < NB; ++qb) acc[qb][0] = acc[qb][1] = floatx4{0.0f, 0.0f, 0.0f, 0.0f};
    for (int kg0 = 0; kg0 < nkg; kg0 += NS_PF) {
      // one turn of the ring, without a branch: k-group kg0 + u is consumed from slot u, which then takes the k-group
      // NS_PF further on (into the next step at the end of this one); the k-groups past D multiply zero by zero
#pragma unroll
      for (int u = 0; u < NS_PF; ++u) {
        const int kg = kg0 + u;
        const halfx8 a0 = ivf_mask<VG>(ring[u][0], jl + (j0 - jbeg) < jend, IVF_KG * kg + IVF_OE * kq, p.D);
        const halfx8 a1 = ivf_mask<VG>(ring[u][1], jl + (j0 - jbeg) + 16 < jend, IVF_KG * kg + IVF_OE * kq, p.D);
#pragma unroll
        for (int qb = 0; qb < NB; ++qb) {
          const halfx8 bv = *reinterpret_cast<const halfx8*>(bq + IVF_KG * kg + 16 * qb * pitch);
          acc[qb][0] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a0, bv, acc[qb][0], 0, 0, 0);
          acc[qb][1] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a1, bv, acc[qb][1], 0, 0, 0);
        }
        const bool wrap = kg + NS_PF >= nkg;
        fetch(u, st + wrap, kg + NS_PF - (wrap ? nkg : 0));
        __builtin_amdgcn_sched_barrier(0);  // the loads stay in the ring's order
      }
    }
    // the step's scores against the thresholds: acc[qb][rb][i] is pair 16 qb + lr against row j0 + slot
#pragma unroll
    for (int qb = 0; qb < NB; ++qb) {
      const int ql = 16 * qb + lr;
      const u64 thr = s.sthr[ql];
#pragma unroll
      for (int rb = 0; rb < 2; ++rb)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int slot = NS_WR * wave + 16 * rb + 4 * kq + i;
          const long long j = j0 + slot;
          const u64 key = topk_key(__float_as_uint(acc[qb][rb][i]), int(j));
          if (ql < npairs && j < jend && key > thr) {
            s.scand[ql * NS_GT + slot] = unsigned(key >> 32);
            s.sflag[ql] = 1;
          }
        }
    }
    __syncthreads();
    for (int t = 0; t < 16; ++t) {  // this wave's share of the pairs that gained a candidate: k held + slots -> k held
      const int qi = 16 * wave + t;
      if (__builtin_amdgcn_readfirstlane(s.sflag[qi]) == 0) continue;  // wave-uniform
      u64 key[3];
      key[0] = lane < p.k ? s.stop[qi * p.k + lane] : 0ull;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int slot = lane + 64 * h;
        const unsigned hi = s.scand[qi * NS_GT + slot];
        key[1 + h] = hi != NS_ABSENT ? (u64(hi) << 32) | u64(~unsigned(j0 + slot)) : 0ull;
        s.scand[qi * NS_GT + slot] = NS_ABSENT;
      }
      const u64 mine = topk_rounds<3>(key, p.k, lane);
      if (lane < p.k) s.stop[qi * p.k + lane] = mine;
      if (lane == p.k - 1) s.sthr[qi] = mine;  // 0 while fewer than k are held: every key passes
      if (lane == 0) s.sflag[qi] = 0;
    }
    __syncthreads();
  }
}

template <bool VG>  // 16-byte loads of the gallery
__global__ __launch_bounds__(256) void ivf_lists_kernel(IvfArgs p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char ivf_lds[];
  const int clen = ivf_tile_d(p.D), pitch = clen + IVF_PAD, nkg = clen / IVF_KG;
  _Float16* const sq = reinterpret_cast<_Float16*>(ivf_lds);
  u64* const sthr = reinterpret_cast<u64*>(ivf_lds + size_t(NN_QT) * pitch * 2);
  u64* const stop = sthr + NN_QT;                                           // [NN_QT][k]
  unsigned* const scand = reinterpret_cast<unsigned*>(stop + NN_QT * p.k);  // [NN_QT][NS_GT]
  int* const sflag = reinterpret_cast<int*>(scand + NN_QT * NS_GT);
  int* const spair = sflag + NN_QT;
  const IvfLds s{sq, sthr, stop, scand, sflag};

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  // the chunk, clipped: everything below is uniform over the workgroup
  const int l = p.chunks[2 * blockIdx.x], first = p.chunks[2 * blockIdx.x + 1];
  if (l < 0 || l >= p.L) return;
  int lo, hi;
  ivf_list_rows(p.offsets, l, p.G, lo, hi);
  if (first < lo || first >= hi || (first - lo) % IVF_R != 0) return;
  const int slot = (first - lo) / IVF_R;
  if (slot >= p.C) return;
  const long long jbeg = first, jend = min(jbeg + IVF_R, (long long)hi);
  const long long np_all = (long long)p.n * p.P;
  const int pb = int(min((long long)max(p.start[l], 0), np_all)), pe = int(min((long long)max(p.start[l + 1], pb), np_all));
  const bool vq = p.D % 4 == 0 && p.q_stride % 4 == 0 && (reinterpret_cast<uintptr_t>(p.q) & 15) == 0;

  for (int g0 = pb; g0 < pe; g0 += NN_QT) {
    const int npairs = min(NN_QT, pe - g0), nb = (npairs + 15) / 16;
    __syncthreads();  // the group before is written out
    if (tid < NN_QT) {
      int e = tid < npairs ? p.pairs[g0 + tid] : -1;
      if (e < 0 || e >= np_all) e = -1;
      spair[tid] = e;
      sthr[tid] = 0ull;
      sflag[tid] = 0;
    }
    for (int i = tid; i < NN_QT * p.k; i += 256) stop[i] = 0ull;
    for (int i = tid; i < NN_QT * NS_GT; i += 256) scand[i] = NS_ABSENT;
    __syncthreads();
    // the group's query rows, rounded once: a wave per row, a lane per group of four d; a row without a pair is zero
    for (int r = wave; r < 16 * nb; r += 4) {
      const int e = spair[r];
      const float* const row = p.q + (long long)(max(e, 0) / p.P) * p.q_stride;
      for (int g4 = lane; 4 * g4 < clen; g4 += 64) {
        const floatx4 v = vq ? nn_load4<true>(e >= 0, row, 4 * g4, p.D) : nn_load4<false>(e >= 0, row, 4 * g4, p.D);
        *reinterpret_cast<halfx4*>(sq + r * pitch + 4 * g4) = halfx4{(_Float16)v[0], (_Float16)v[1], (_Float16)v[2], (_Float16)v[3]};
      }
    }
    __syncthreads();
    // wave-uniform, outside the turn.  The element-load path runs all four blocks: with the four instances beside its
    // 128 loads per turn it spilled
    if (!VG || nb == 4) ivf_group<4, VG>(p, s, jbeg, jend, npairs, pitch, nkg, wave, lane);
    else if (nb == 1) ivf_group<1, VG>(p, s, jbeg, jend, npairs, pitch, nkg, wave, lane);
    else if (nb == 2) ivf_group<2, VG>(p, s, jbeg, jend, npairs, pitch, nkg, wave, lane);
    else ivf_group<3, VG>(p, s, jbeg, jend, npairs, pitch, nkg, wave, lane);
    // the k best of the chunk per pair, rank = lane: all k, 0 where the chunk has fewer rows (ivf_group ends on a barrier)
    for (int t = 0; t < 16; ++t) {
      const int qi = 16 * wave + t, e = spair[qi];
      if (e >= 0 && lane < p.k) p.part[((long long)e * p.C + slot) * p.k + lane] = stop[qi * p.k + lane];
    }
  }
}

__global__ __launch_bounds__(256) void ivf_merge_kernel(IvfArgs p) {
  __shared__ int snch[4][64];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const long long i = (long long)blockIdx.x * 4 + wave;
  if (i >= p.n) return;  // wave-uniform; no barrier below
  int nch = 0;           // the chunk slots the scan wrote for pair (i, lane)
  if (lane < p.P) {
    const int l = ivf_pair_list(p.probes + i * p.probe_stride, lane, p.L);
    if (l >= 0) {
      int lo, hi;
      ivf_list_rows(p.offsets, l, p.G, lo, hi);
      nch = min((hi - lo + IVF_R - 1) / IVF_R, p.C);
    }
  }
  snch[wave][lane] = nch;  // read by this wave alone
  const long long total = (long long)p.P * p.C * p.k;
  const u64* const part = p.part + i * total;
  u64 held = 0ull;  // rank = lane
  for (long long t0 = 0; t0 < total; t0 += 128) {
    u64 key[3];
    key[0] = held;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const long long t = t0 + lane + 64 * h;
      key[1 + h] = 0ull;
      if (t < total) {
        const long long pc = t / p.k;
        if (int(pc % p.C) < snch[wave][pc / p.C]) key[1 + h] = part[t];
      }
    }
    if (__ballot((key[1] | key[2]) != 0ull) == 0ull) continue;
    held = topk_rounds<3>(key, p.k, lane);
  }
  if (lane < p.k) {  // 0 past the union: the quiet NaN and index -1
    reinterpret_cast<unsigned*>(p.values)[i * p.k + lane] = topk_key_bits(held);
    p.indices[i * p.k + lane] = topk_key_index(held);
  }
}

}  // namespace

int nearest_lists_chunk_rows() { return IVF_R; }
int nearest_lists_max_d() { return IVF_MAX_D; }

// cnt [L], start [L + 1] and pairs [n P] as int, then part [n P][C][k] at the next multiple of 8 bytes
static size_t ivf_part_offset(long long n, int P, int L) { return (size_t(2 * (long long)L + 1 + n * P) * 4 + 7) / 8 * 8; }

size_t nearest_lists_bytes(long long n, int P, int L, int C, int k) {
  return ivf_part_offset(n, P, L) + size_t(n) * P * C * k * 8;
}

void launch_nearest_lists_f16(const float* q, long long q_stride, int n, int D, const void* gallery, long long G, const int* offsets,
                              int L, const int* chunks, int n_chunks, int C, const int* probes, long long probe_stride, int P, int k,
                              void* scratch, float* values, int* indices, hipStream_t s) {
  if (n <= 0) return;
  static std::atomic<unsigned long long> raised[2];
  int* const cnt = static_cast<int*>(scratch);
  const IvfArgs a{q, static_cast<const _Float16*>(gallery), offsets, chunks, probes, cnt, cnt + L, cnt + 2 * (long long)L + 1,
                  reinterpret_cast<u64*>(static_cast<char*>(scratch) + ivf_part_offset(n, P, L)), values, indices, q_stride, G,
                  probe_stride, n, D, k, L, P, C};
  const dim3 pairs((unsigned)(((long long)n * P + 255) / 256)), block(256);
  hipLaunchKernelGGL(ivf_clear_kernel, dim3((unsigned)((L + 255) / 256)), block, 0, s, a.cnt, L);
  hipLaunchKernelGGL(ivf_invert_kernel<false>, pairs, block, 0, s, a);
  hipLaunchKernelGGL(ivf_scan_kernel, dim3(1), dim3(1024), 0, s, a.cnt, a.start, L);
  hipLaunchKernelGGL(ivf_invert_kernel<true>, pairs, block, 0, s, a);
  const bool vg = D % 8 == 0 && (reinterpret_cast<uintptr_t>(gallery) & 15) == 0;
  const auto kernel = vg ? &ivf_lists_kernel<true> : &ivf_lists_kernel<false>;
  ore_raise_lds_once(raised[vg], reinterpret_cast<const void*>(kernel), int(ivf_lds_bytes(IVF_MAX_D, 64)));
  if (n_chunks > 0) hipLaunchKernelGGL(kernel, dim3((unsigned)n_chunks), block, ivf_lds_bytes(D, k), s, a);
  hipLaunchKernelGGL(ivf_merge_kernel, dim3((unsigned)((n + 3) / 4)), block, 0, s, a);
}

}  // namespace ore
