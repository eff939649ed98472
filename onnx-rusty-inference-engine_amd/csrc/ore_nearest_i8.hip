// Nearest neighbours on an int8 gallery with one scale per row (extension, ore_nearest_i8 and ore_gallery_i8;
// DESIGN.md 3.13c): the k best of s[i, j] = fmul(fmul((float)dot, tq[i]), tg[j]), dot = sum_d cq[i, d] cg[j, d] an
// exact int32 sum of v_mfma_i32_16x16x64_i8, cq and tq the query row quantised by include/ore.h's rule inside the
// kernel, under ore_topk_f32's order (ore_topk_key.h) -- and the packer that makes codes and scales by the same rule.
//
// Split.  grid = (ceil(n / 64) query tiles, S gallery segments), four waves.  A step is NI_GT = 128 gallery rows:
// wave w takes rows 32 w .. 32 w + 31 of it, as two A operands of 16 rows, against all 64 queries of the tile, the
// B operands of four query blocks -- eight MFMAs per k-group of 64 d, 32 int32 accumulators over the whole of D.
// Lane l holds query 16 qb + (l & 15) against rows 32 w + 16 rb + 4 (l >> 4) + i.  A gallery byte is used by one wave.
//
// Queries.  Before the first step a wave takes the maximum |x| of each of its 16 rows over the whole row (NaNs
// skipped: fmaxf), lane-strided and reduced over the wave, and leaves t = a / 127 and 127 / a in LDS.  The codes are
// then written to LDS by the wave that took the maximum, four d per lane: 64 rows of D bytes, D rounded up to a whole
// turn of the ring below (512), at a pitch of 16 bytes more: a row starts 128 m + 4 dwords after the one before, so
// the 16 rows of a 16-byte operand read fall on 16 different bank quads.  Up to NI_DRES = 1024 d the tile is resident
// for the segment; above it the tile is staged in chunks of NI_DC d, every step, between two barriers per chunk, the
// accumulators carrying across -- the scales are still those of the whole row.  Query rows past n and d past D enter
// LDS as code 0.  No int8 copy of q reaches memory.
//
// Gallery.  It never passes through LDS: a lane loads the 16 bytes of its row and k-group straight into the A operand
// (sixteen 1-byte loads when D % 16 != 0 or the base is not 16-byte aligned), NI_PF k-groups ahead of the MFMAs that
// consume them, through a ring of registers that runs on across the steps.  A turn of the ring is straight-line code
// without a branch (ore_nearest_f16.hip found why), so a byte that is not there (a row past the segment, d past D)
// is read from the gallery's first bytes instead and made 0 on its bits before the MFMA; the k-groups past D that
// fill the last turn multiply zero codes, which is exact.  The eight scales of a lane's rows are loaded in the first
// slot of every turn, at the index clamped to G - 1, so that their place among the ring's loads is fixed and the
// epilogue's wait for them leaves the ring in flight.
//
// Position independence.  The dot product is exact, so the bits of s[i, j] depend on q[i, :], gallery[j, :] and
// tg[j] alone, whatever the order of the d, the load path, resident or chunked.
//
// Selection and merge: ore_nearest_f16.hip's.  Per query, in LDS: the threshold, the k best keys so far, NI_GT slots
// (slot r holds the 32-bit score image of row r of the step, or NI_ABSENT) and a flag; behind the step's barrier the
// flagged queries are dealt out over the waves and compacted by topk_rounds<3>.  S == 1: the workgroup writes values
// and indices.  S > 1: part[n][S][k] and ore_nearest.hip's merge.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>

#include "ore_kernels.h"
#include "ore_topk_key.h"

// every product of the definition is rounded on its own
#pragma clang fp contract(off)

namespace ore {

namespace {

typedef float floatx4 __attribute__((ext_vector_type(4)));
typedef int intx4 __attribute__((ext_vector_type(4)));
typedef unsigned uintx4 __attribute__((ext_vector_type(4)));

constexpr int NI_QT = 64;               // queries per workgroup
constexpr int NI_WR = 32;               // gallery rows per wave and step
constexpr int NI_GT = 4 * NI_WR;        // gallery rows per step
constexpr int NI_KG = 64;               // d per MFMA
constexpr int NI_PF = 8;                // k-groups the gallery loads run ahead of the MFMAs
constexpr int NI_TURN = NI_KG * NI_PF;  // d per turn of the ring
constexpr int NI_DRES = 1024;           // the largest D whose query tile is resident
constexpr int NI_DC = 1024;             // d per staged chunk above it
constexpr int NI_PAD = 16;              // bytes added to the LDS row pitch
constexpr int NI_SMAX = 512;            // segments at most: the merge kernel's lists
constexpr int NI_DMAX = 131072;         // 127 * 128 * D < 2^31
constexpr unsigned NI_ABSENT = 0xffffffffu;
static_assert(NI_DC % NI_TURN == 0 && NI_DRES % NI_TURN == 0 && NI_GT == 128, "chunks of whole ring turns; two slots per lane");
static_assert(127LL * 128 * NI_DMAX < (1LL << 31), "the dot product stays in int32");

// the d of the tile that are staged at once: D in whole turns of the ring, or a chunk
__host__ __device__ constexpr int ni_chunk(int D) { return D <= NI_DRES ? (D + NI_TURN - 1) / NI_TURN * NI_TURN : NI_DC; }
// dynamic LDS: the code tile, then per query the threshold, k keys, NI_GT slots, the flag, t and 127 / a
__host__ __device__ constexpr size_t ni_lds_bytes(int D, int k) {
  return size_t(NI_QT) * (ni_chunk(D) + NI_PAD) + size_t(NI_QT) * (8 + 8 * size_t(k) + 4 * NI_GT + 4 + 8);
}
static_assert(ni_lds_bytes(NI_DRES, 64) <= 160 * 1024 && ni_lds_bytes(NI_DRES + 1, 64) <= ni_lds_bytes(NI_DRES, 64), "LDS");
static_assert(ni_lds_bytes(NI_DRES, 64) + size_t(NI_QT) * NI_TURN > 160 * 1024, "a resident tile one turn longer does not fit");

struct NearestI8Args {
  const float* q;
  const signed char* g;
  const float* scales;
  u64* part;       // [n][S][k], S > 1
  float* values;   // [n][k]
  int* indices;
  long long q_stride, G, seg_rows;  // seg_rows: gallery rows per segment, a multiple of NI_GT
  int n, D, k, S;
};

// the maximum over the wave, in every lane
__device__ __forceinline__ float ni_wave_fmax(float a) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) a = fmaxf(a, __shfl_xor(a, m));
  return a;
}

// one code of include/ore.h's rule: x inv rounded on its own, clamped, ties to even; a NaN quotient is 0
__device__ __forceinline__ unsigned ni_code(float x, float inv) {
  const float r = x * inv;
  const int c = r != r ? 0 : int(__builtin_rintf(fminf(fmaxf(r, -127.0f), 127.0f)));
  return unsigned(c) & 0xffu;
}
__device__ __forceinline__ unsigned ni_code4(floatx4 v, float inv) {
  return ni_code(v[0], inv) | ni_code(v[1], inv) << 8 | ni_code(v[2], inv) << 16 | ni_code(v[3], inv) << 24;
}

// four consecutive d of a query row, masked: nothing past D or of a row that is not there
template <bool VEC>
__device__ __forceinline__ floatx4 ni_load4(bool row_ok, const float* __restrict__ row, int d, int D) {
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

// The gallery loads sit in the K loop, far ahead of their use, so they are masked without a branch: a byte that is not
// there is read from `safe` instead (the gallery's first byte, or its first sixteen: always there), and ni_mask16
// makes it 0 when the operand is consumed.
template <bool VEC>
__device__ __forceinline__ intx4 ni_load16(bool row_ok, const signed char* __restrict__ row, int d, int D,
                                           const signed char* __restrict__ safe) {
  if (VEC)  // D % 16 == 0: the group is inside the row or outside it
    return *reinterpret_cast<const intx4*>(row_ok && d < D ? row + d : safe);
  intx4 v;
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    unsigned x = 0u;
#pragma unroll
    for (int b = 0; b < 4; ++b)
      x |= unsigned(static_cast<unsigned char>(*(row_ok && d + 4 * w + b < D ? row + d + 4 * w + b : safe))) << (8 * b);
    v[w] = int(x);
  }
  return v;
}

template <bool VEC>
__device__ __forceinline__ intx4 ni_mask16(intx4 v, bool row_ok, int d, int D) {
  if (VEC) {
    const unsigned m = row_ok && d < D ? ~0u : 0u;
    return __builtin_bit_cast(intx4, __builtin_bit_cast(uintx4, v) & uintx4{m, m, m, m});
  }
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    const int left = row_ok ? D - (d + 4 * w) : 0;  // bytes of this dword that are there
    v[w] &= left >= 4 ? -1 : left <= 0 ? 0 : int((1u << (8 * left)) - 1u);
  }
  return v;
}

template <bool VQ, bool VG>  // 16-byte loads of the queries / of the gallery
__global__ __launch_bounds__(256) void nearest_i8_kernel(NearestI8Args p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char ni_lds[];
  const bool resident = p.D <= NI_DRES;
  const int clen = ni_chunk(p.D), pitch = clen + NI_PAD;
  unsigned char* const sq = ni_lds;
  u64* const sthr = reinterpret_cast<u64*>(ni_lds + size_t(NI_QT) * pitch);
  u64* const stop = sthr + NI_QT;                                           // [NI_QT][k]
  unsigned* const scand = reinterpret_cast<unsigned*>(stop + NI_QT * p.k);  // [NI_QT][NI_GT]
  int* const sflag = reinterpret_cast<int*>(scand + NI_QT * NI_GT);
  float* const stq = reinterpret_cast<float*>(sflag + NI_QT);
  float* const sinv = stq + NI_QT;

  const int tid = threadIdx.x, lane = tid & 63, lr = lane & 15, kq = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const long long q0 = (long long)blockIdx.x * NI_QT;
  const int seg = blockIdx.y;
  const long long jbeg = (long long)seg * p.seg_rows, jend = min(p.G, jbeg + p.seg_rows);
  const int nsteps = int((jend - jbeg + NI_GT - 1) / NI_GT);  // >= 1: the launcher leaves no segment empty
  const int nkg = ((p.D + NI_KG - 1) / NI_KG + NI_PF - 1) / NI_PF * NI_PF;  // whole turns of the ring

  for (int i = tid; i < NI_QT; i += 256) {
    sthr[i] = 0ull;
    sflag[i] = 0;
  }
  for (int i = tid; i < NI_QT * p.k; i += 256) stop[i] = 0ull;
  for (int i = tid; i < NI_QT * NI_GT; i += 256) scand[i] = NI_ABSENT;

  // the scales of the tile's rows: a wave per row, the maximum over the whole row, NaNs skipped
  for (int r = wave; r < NI_QT; r += 4) {
    const long long qi = q0 + r;
    const float* const row = p.q + qi * p.q_stride;
    float a = 0.0f;
    for (int d = 4 * lane; d < p.D; d += 256) {
      const floatx4 v = ni_load4<VQ>(qi < p.n, row, d, p.D);
#pragma unroll
      for (int e = 0; e < 4; ++e) a = fmaxf(a, fabsf(v[e]));
    }
    a = ni_wave_fmax(a);
    if (lane == 0) {
      stq[r] = a / 127.0f;
      sinv[r] = 127.0f / a;
    }
  }

  // the tile's d from c0 on as codes: the wave that took a row's maximum, a lane per group of four
  auto stage = [&](int c0) __attribute__((always_inline)) {
    for (int r = wave; r < NI_QT; r += 4) {
      const long long qi = q0 + r;
      const float* const row = p.q + qi * p.q_stride;
      const float inv = sinv[r];
      for (int g4 = lane; 4 * g4 < clen; g4 += 64)
        *reinterpret_cast<unsigned*>(sq + r * pitch + 4 * g4) = ni_code4(ni_load4<VQ>(qi < p.n, row, c0 + 4 * g4, p.D), inv);
    }
  };

  // k-group kg of step st of this wave's rows: lane l takes the 16 d from 64 kg + 16 (l >> 4) of rows (l & 15), + 16
  intx4 ring[NI_PF][2];
  const long long jl = jbeg + NI_WR * wave + lr;  // this lane's first row of step 0
  const signed char* const gl = p.g + jl * p.D;
  auto fetch = [&](int slot, int st, int kg) __attribute__((always_inline)) {
    const long long sj = (long long)st * NI_GT;  // st == nsteps: past jend, nothing of it is read
#pragma unroll
    for (int rb = 0; rb < 2; ++rb)
      ring[slot][rb] = ni_load16<VG>(jl + sj + 16 * rb < jend, gl + (sj + 16 * rb) * p.D, NI_KG * kg + 16 * kq, p.D, p.g);
  };

  const unsigned char* const bq = sq + lr * pitch + 16 * kq;
#pragma unroll
  for (int u = 0; u < NI_PF; ++u) {
    fetch(u, 0, u);
    __builtin_amdgcn_sched_barrier(0);
  }
  for (int st = 0; st < nsteps; ++st) {
    const long long j0 = jbeg + (long long)st * NI_GT;
    intx4 acc[4][2];
    float tg[2][4];
#pragma unroll
    for (int qb = 0; qb < 4; ++qb) acc[qb][0] = acc[qb][1] = intx4{0, 0, 0, 0};
    for (int kg0 = 0; kg0 < nkg; kg0 += NI_PF) {
      if (resident ? (st == 0 && kg0 == 0) : kg0 % (NI_DC / NI_KG) == 0) {  // uniform
        __syncthreads();  // the previous chunk's operand reads (and, first, the state's initialisation) are done
        stage(NI_KG * kg0);
        __syncthreads();
      }
      // one turn of the ring, without a branch: k-group kg0 + u is consumed from slot u, which then takes the k-group
      // NI_PF further on (into the next step at the end of this one)
#pragma unroll
      for (int u = 0; u < NI_PF; ++u) {
        const int kg = kg0 + u;
        const intx4 a0 = ni_mask16<VG>(ring[u][0], jl + (j0 - jbeg) < jend, NI_KG * kg + 16 * kq, p.D);
        const intx4 a1 = ni_mask16<VG>(ring[u][1], jl + (j0 - jbeg) + 16 < jend, NI_KG * kg + 16 * kq, p.D);
        const unsigned char* const b = bq + (resident ? NI_KG * kg : NI_KG * (kg % (NI_DC / NI_KG)));
#pragma unroll
        for (int qb = 0; qb < 4; ++qb) {
          const intx4 bv = *reinterpret_cast<const intx4*>(b + 16 * qb * pitch);
          acc[qb][0] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a0, bv, acc[qb][0], 0, 0, 0);
          acc[qb][1] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a1, bv, acc[qb][1], 0, 0, 0);
        }
        if (u == 0) {  // the scales of this lane's eight rows, at a fixed place among the ring's loads
#pragma unroll
          for (int rb = 0; rb < 2; ++rb)
#pragma unroll
            for (int i = 0; i < 4; ++i)
              tg[rb][i] = p.scales[min(j0 + NI_WR * wave + 16 * rb + 4 * kq + i, p.G - 1)];
        }
        const bool wrap = kg + NI_PF >= nkg;
        fetch(u, st + wrap, kg + NI_PF - (wrap ? nkg : 0));
        __builtin_amdgcn_sched_barrier(0);  // the loads stay in the ring's order: the waits count on it
      }
    }
    // the step's scores against the thresholds: acc[qb][rb][i] is query 16 qb + lr against row j0 + slot
#pragma unroll
    for (int qb = 0; qb < 4; ++qb) {
      const int ql = 16 * qb + lr;
      const u64 thr = sthr[ql];
      const float tq = stq[ql];
      const bool q_ok = q0 + ql < p.n;
#pragma unroll
      for (int rb = 0; rb < 2; ++rb)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int slot = NI_WR * wave + 16 * rb + 4 * kq + i;
          const long long j = j0 + slot;
          const float s = (float(acc[qb][rb][i]) * tq) * tg[rb][i];  // two roundings, nothing to fuse them with
          const u64 key = topk_key(__float_as_uint(s), int(j));
          if (q_ok && j < jend && key > thr) {
            scand[ql * NI_GT + slot] = unsigned(key >> 32);
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
        const unsigned hi = scand[qi * NI_GT + slot];
        key[1 + h] = hi != NI_ABSENT ? (u64(hi) << 32) | u64(~unsigned(j0 + slot)) : 0ull;
        scand[qi * NI_GT + slot] = NI_ABSENT;
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

// f32 rows -> codes and a scale per row by include/ore.h's rule: a wave per row, four rows per workgroup.  Pass 1 takes
// the row's maximum, pass 2 writes the codes (the row comes from the cache) and lane 0 the scale.  VEC (D % 4 == 0,
// src 16-byte and dst 4-byte aligned): a lane takes four elements, one 16-byte load and one packed store; otherwise one
template <bool VEC>
__global__ __launch_bounds__(256) void gallery_i8_kernel(const float* __restrict__ src, signed char* __restrict__ dst,
                                                         float* __restrict__ scales, long long G, long long D) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (long long r = 4LL * blockIdx.x + wave; r < G; r += 4LL * gridDim.x) {
    const float* const row = src + r * D;
    signed char* const out = dst + r * D;
    float a = 0.0f;
    if (VEC) {
      for (long long d = 4 * lane; d < D; d += 256) {
        const floatx4 v = *reinterpret_cast<const floatx4*>(row + d);
#pragma unroll
        for (int e = 0; e < 4; ++e) a = fmaxf(a, fabsf(v[e]));
      }
    } else {
      for (long long d = lane; d < D; d += 64) a = fmaxf(a, fabsf(row[d]));
    }
    a = ni_wave_fmax(a);
    const float inv = 127.0f / a;
    if (VEC) {
      for (long long d = 4 * lane; d < D; d += 256)
        *reinterpret_cast<unsigned*>(out + d) = ni_code4(*reinterpret_cast<const floatx4*>(row + d), inv);
    } else {
      for (long long d = lane; d < D; d += 64) out[d] = static_cast<signed char>(ni_code(row[d], inv));
    }
    if (lane == 0) scales[r] = a / 127.0f;
  }
}

template <bool VQ, bool VG>
void nearest_i8_launch(const NearestI8Args& a, hipStream_t s) {
  static std::atomic<unsigned long long> raised{0};
  ore_raise_lds_once(raised, reinterpret_cast<const void*>(nearest_i8_kernel<VQ, VG>), int(ni_lds_bytes(NI_DRES, 64)));
  const dim3 grid((unsigned)((a.n + NI_QT - 1) / NI_QT), (unsigned)a.S);
  hipLaunchKernelGGL((nearest_i8_kernel<VQ, VG>), grid, dim3(256), ni_lds_bytes(a.D, a.k), s, a);
}

}  // namespace

int nearest_i8_step_rows() { return NI_GT; }
int nearest_i8_max_d() { return NI_DMAX; }

int nearest_i8_segments(long long n, long long G, int ncu) {
  const long long qt = std::max<long long>((n + NI_QT - 1) / NI_QT, 1), steps = (G + NI_GT - 1) / NI_GT;
  // the f32 split: about two workgroups per CU, at most NI_SMAX segments and a step each
  const long long want = std::min<long long>(std::min(std::max<long long>(2LL * ncu / qt, 1), steps), NI_SMAX);
  const long long per = (steps + want - 1) / want;
  return int((steps + per - 1) / per);  // no segment is empty
}

void launch_gallery_i8(const float* src, long long G, long long D, void* dst, float* scales, hipStream_t s) {
  const bool vec = D % 4 == 0 && (reinterpret_cast<uintptr_t>(src) & 15) == 0 && (reinterpret_cast<uintptr_t>(dst) & 3) == 0;
  const dim3 grid((unsigned)std::min<long long>((G + 3) / 4, 1 << 20));
  if (vec) hipLaunchKernelGGL(gallery_i8_kernel<true>, grid, dim3(256), 0, s, src, static_cast<signed char*>(dst), scales, G, D);
  else hipLaunchKernelGGL(gallery_i8_kernel<false>, grid, dim3(256), 0, s, src, static_cast<signed char*>(dst), scales, G, D);
}

void launch_nearest_i8(const float* q, long long q_stride, int n, int D, const void* gallery, const float* scales, long long G,
                       int k, int S, void* part, float* values, int* indices, hipStream_t s) {
  if (n <= 0) return;
  const long long steps = (G + NI_GT - 1) / NI_GT, per = (steps + S - 1) / S;
  const NearestI8Args a{q, static_cast<const signed char*>(gallery), scales, static_cast<u64*>(part), values, indices, q_stride, G,
                        per * NI_GT, n, D, k, S};
  const bool vg = D % 16 == 0 && (reinterpret_cast<uintptr_t>(gallery) & 15) == 0;
  const bool vq = D % 4 == 0 && q_stride % 4 == 0 && (reinterpret_cast<uintptr_t>(q) & 15) == 0;
  if (vq && vg) nearest_i8_launch<true, true>(a, s);
  else if (vg) nearest_i8_launch<false, true>(a, s);
  else if (vq) nearest_i8_launch<true, false>(a, s);
  else nearest_i8_launch<false, false>(a, s);
  if (S > 1) launch_nearest_merge(part, n, S, k, values, indices, s);
}

}  // namespace ore
