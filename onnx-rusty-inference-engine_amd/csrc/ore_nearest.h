// Nearest neighbours by inner product, the parts the three searches share.  Device code and its
// launch, for ore_nearest.hip (f32 gallery), ore_nearest_f16.hip and ore_nearest_i8.hip:
//   1. what every search has: the kernel arguments, the masked query loader and the launch (the four-way choice of
//      the load paths, the one-time LDS raise, the merge launch);
//   2. the streaming kernel of the f16 and the int8 gallery, written once over a format type.
// The f32 kernel (ore_nearest.hip) stages both operands through LDS and appends candidates through a counter: another
// data movement and another selection, so it is a kernel of its own on part 1.  The write of a segment's k best stands
// in both kernels: as a shared function, fields or struct passed, it changed the order of the int8 byte-load instances'
// last ring slot.
//
// The streaming kernel: the k best of s[i, j] per query row under ore_topk_f32's order (ore_topk_key.h), s the format's
// score of its MFMA's sum over d.
//
// Split.  grid = (ceil(n / 64) query tiles, S gallery segments), four waves.  A step is NS_GT = 128 gallery rows:
// wave w takes rows 32 w .. 32 w + 31 of it, as two A operands of 16 rows, against all 64 queries of the tile, the
// B operands of four query blocks -- eight MFMAs per k-group of F::KG d, 32 accumulators over the whole of D.  Lane l
// holds query 16 qb + (l & 15) against rows 32 w + 16 rb + 4 (l >> 4) + i, and supplies the 16 bytes d = KG kg +
// (KG / 4) (l >> 4) + e of its row to both operands.  A gallery element is used by one wave.
//
// Data movement.  The query tile is converted to the format once per workgroup (F::stage4, behind F::prologue) and
// stays in LDS for the whole segment: 64 rows of D elements, D rounded up to a whole turn of the ring below, at a pitch
// of F::PAD elements (16 bytes) more: a row starts an odd multiple of 4 banks after the one before, so the 16 rows of
// a 16-byte operand read fall on 16 different bank quads.  The gallery never passes through LDS: a lane loads the 16
// bytes of its row and k-group straight into the A operand (element by element when D is no multiple of an operand's
// elements or the base is not 16-byte aligned), NS_PF k-groups ahead of the MFMAs that consume them, through a ring of
// registers that runs on across the steps.  The K loop has no barrier and no branch: a turn of the ring is
// straight-line code, so the waits count the loads in flight (vmcnt 15 and 14 before a k-group's MFMAs) -- with a
// branch around a load or around a k-group's MFMAs the compiler drained the ring once per turn.  So a gallery element
// that is not there (a row past the segment, d past D) is read from the gallery's first elements instead and made +0
// on its bits before the MFMA (F::load, F::mask), and the k-groups past D that fill the last turn multiply the zero of
// that mask by the zero the tile holds there.  Above F::DRES the tile no longer fits beside the selection state: it is
// then staged in chunks of F::DC d, every step, between two barriers per chunk, and the accumulators carry across the
// chunks.  Query rows past n and d past D are masked at the load and enter LDS as zero.  Nothing outside q's rows and
// the gallery's G D elements (and, with scales, its G scales) is read.
//
// Scales (F::SCALES, a compile-time property: no format adds a run-time branch).  A lane needs the scales of its eight
// rows once per step.  They are loaded in the first slot of every turn, at the index clamped to G - 1, so that their
// place among the ring's loads is fixed and the epilogue's wait for them leaves the ring in flight (vmcnt 23 and 22
// before the other k-groups of a turn, 23 .. 16 in the epilogue).  In front of the step's K loop they would sit
// between ring loads whose number differs between the loop's entry and its back edge.  The queries' scales are left in
// LDS by F::prologue, F::QX bytes per query behind the flags.
//
// Position independence.  K is never split across waves or workgroups.  A score is one accumulator's chain over the
// k-groups in ascending order: an order that depends on D alone (so does resident or chunked, and the number of
// turns).  Padded products are zero and leave the accumulator unchanged.
//
// Selection.  Per query, in LDS: the threshold, the k best keys so far, NS_GT candidate slots and a flag.  Several
// waves score the same query, so a candidate is not appended through a counter: slot r of a query belongs to row r
// of the step and holds the 32-bit score image of the key (the index is j0 + r), or NS_ABSENT, which no image
// equals (an image is at most +inf's 0xff800000).  A buffer cannot overflow: the slots are the rows.  A key above
// its query's threshold is stored and the flag set; behind the step's barrier the flagged queries are dealt out
// over the waves, 16 each, and compacted by topk_rounds over (k held, two slots per lane), which also empties the
// slots.  8-byte slots behind the f32 kernel's atomic counter would need 128 of them per query: with k = 64 that
// is 97 KB of state beside the 65 KB tile of an f16 D = 512, past the 160 KB.
//
// Merge.  S == 1: the workgroup writes values and indices.  S > 1: part[n][S][k] and ore_nearest.hip's merge.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>

#include "ore_kernels.h"
#include "ore_topk_key.h"

namespace ore {

namespace {

typedef float floatx4 __attribute__((ext_vector_type(4)));

constexpr int NN_QT = 64;     // queries per workgroup: wave w writes the k best of queries 16 w .. 16 w + 15
constexpr int NN_SMAX = 512;  // segments at most: the merge kernel's lists

struct NearestArgs {
  const float* q;
  const void* g;   // [G][D] in the kernel's format
  u64* part;       // [n][S][k], S > 1
  float* values;   // [n][k]
  int* indices;
  long long q_stride, G, seg_rows;  // seg_rows: gallery rows per segment, a multiple of the kernel's step
  int n, D, k, S;
  const float* scales;  // [G], int8 gallery; null otherwise.  Last: the f32 and f16 kernels read the fields above where
                        // they were before the struct was shared
};

// four consecutive d of a query (or f32 gallery) row, masked: nothing past D or of a row that is not there is read
template <bool VEC>
__device__ __forceinline__ floatx4 nn_load4(bool row_ok, const float* __restrict__ row, int d, int D) {
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

// The launch of a search.  K names the kernel: kernel<VQ, VG>() (16-byte loads of the queries / of the gallery), GT its
// gallery rows per step, VGE the gallery elements of a 16-byte load, lds(D, k) its dynamic LDS and LDS_MAX the most of it.
template <class K, bool VQ, bool VG>
void nearest_launch_instance(const NearestArgs& a, hipStream_t s) {
  static std::atomic<unsigned long long> raised{0};
  const auto kernel = K::template kernel<VQ, VG>();
  ore_raise_lds_once(raised, reinterpret_cast<const void*>(kernel), int(K::LDS_MAX));
  const dim3 grid((unsigned)((a.n + NN_QT - 1) / NN_QT), (unsigned)a.S);
  hipLaunchKernelGGL(kernel, grid, dim3(256), K::lds(a.D, a.k), s, a);
}

template <class K>
void nearest_launch(const float* q, long long q_stride, int n, int D, const void* gallery, const float* scales, long long G,
                    int k, int S, void* part, float* values, int* indices, hipStream_t s) {
  if (n <= 0) return;
  const long long steps = (G + K::GT - 1) / K::GT, per = (steps + S - 1) / S;
  const NearestArgs a{q, gallery, static_cast<u64*>(part), values, indices, q_stride, G, per * K::GT, n, D, k, S, scales};
  const bool vg = D % K::VGE == 0 && (reinterpret_cast<uintptr_t>(gallery) & 15) == 0;
  const bool vq = D % 4 == 0 && q_stride % 4 == 0 && (reinterpret_cast<uintptr_t>(q) & 15) == 0;
  if (vq && vg) nearest_launch_instance<K, true, true>(a, s);
  else if (vg) nearest_launch_instance<K, false, true>(a, s);
  else if (vq) nearest_launch_instance<K, true, false>(a, s);
  else nearest_launch_instance<K, false, false>(a, s);
  if (S > 1) launch_nearest_merge(part, n, S, k, values, indices, s);
}

// ---- the streaming kernel.  A format type F supplies:
//   elem, opnd, accum       an element of the gallery and of the LDS tile, a 16-byte MFMA operand, four accumulators
//   KG, DRES, DC, PAD, QX   d per MFMA, the largest resident D, d per chunk above it, elements added to the LDS row
//                           pitch, LDS bytes per query behind the selection state
//   SCALES                  whether a score is scaled by a factor per query (t, 127 / a in LDS) and per gallery row
//   load<VEC>, mask<VEC>    one gallery operand, read without a branch, and its zeroing when it is consumed
//   prologue<VQ>            what the tile's conversion needs of whole query rows (the int8 scales; empty for f16)
//   stage4                  four staged d as elements of the tile
//   mfma, score             one k-group of a 16 x 16 block, and an accumulator as the f32 score

constexpr int NS_WR = 32;         // gallery rows per wave and step
constexpr int NS_GT = 4 * NS_WR;  // gallery rows per step
constexpr int NS_PF = 8;          // k-groups the gallery loads run ahead of the MFMAs
constexpr unsigned NS_ABSENT = 0xffffffffu;
static_assert(NS_GT == 128, "two slots per lane");

// the d of the tile that are staged at once: D in whole turns of the ring, or a chunk
template <class F>
__host__ __device__ constexpr int ns_chunk(int D) {
  return D <= F::DRES ? (D + F::KG * NS_PF - 1) / (F::KG * NS_PF) * (F::KG * NS_PF) : F::DC;
}
// dynamic LDS: the query tile, then per query the threshold, k keys, NS_GT slots, the flag and the format's QX bytes
template <class F>
__host__ __device__ constexpr size_t ns_lds_bytes(int D, int k) {
  return size_t(NN_QT) * (ns_chunk<F>(D) + F::PAD) * sizeof(typename F::elem) + size_t(NN_QT) * (8 + 8 * size_t(k) + 4 * NS_GT + 4 + F::QX);
}

template <class F, bool VQ, bool VG>  // 16-byte loads of the queries / of the gallery
__global__ __launch_bounds__(256) void nearest_stream_kernel(NearestArgs p) {
  typedef typename F::elem elem;
  typedef typename F::opnd opnd;
  typedef typename F::accum accum;
  constexpr int KG = F::KG, OE = KG / 4;  // d per MFMA and per operand register group (16 bytes)
  static_assert(F::DC % (KG * NS_PF) == 0 && F::DRES % (KG * NS_PF) == 0, "chunks of whole ring turns");
  extern __shared__ __attribute__((aligned(16))) unsigned char ns_lds[];
  const bool resident = p.D <= F::DRES;
  const int clen = ns_chunk<F>(p.D), pitch = clen + F::PAD;
  elem* const sq = reinterpret_cast<elem*>(ns_lds);
  u64* const sthr = reinterpret_cast<u64*>(ns_lds + size_t(NN_QT) * pitch * sizeof(elem));
  u64* const stop = sthr + NN_QT;                                           // [NN_QT][k]
  unsigned* const scand = reinterpret_cast<unsigned*>(stop + NN_QT * p.k);  // [NN_QT][NS_GT]
  int* const sflag = reinterpret_cast<int*>(scand + NN_QT * NS_GT);
  [[maybe_unused]] float* const stq = reinterpret_cast<float*>(sflag + NN_QT);  // SCALES: t and 127 / a of the queries
  [[maybe_unused]] float* const sinv = stq + NN_QT;

  const int tid = threadIdx.x, lane = tid & 63, lr = lane & 15, kq = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const long long q0 = (long long)blockIdx.x * NN_QT;
  const int seg = blockIdx.y;
  const long long jbeg = (long long)seg * p.seg_rows, jend = min(p.G, jbeg + p.seg_rows);
  const int nsteps = int((jend - jbeg + NS_GT - 1) / NS_GT);  // >= 1: the launcher leaves no segment empty
  const int nkg = ((p.D + KG - 1) / KG + NS_PF - 1) / NS_PF * NS_PF;  // whole turns of the ring

  for (int i = tid; i < NN_QT; i += 256) {
    sthr[i] = 0ull;
    sflag[i] = 0;
  }
  for (int i = tid; i < NN_QT * p.k; i += 256) stop[i] = 0ull;
  for (int i = tid; i < NN_QT * NS_GT; i += 256) scand[i] = NS_ABSENT;

  F::template prologue<VQ>(p.q, p.q_stride, p.n, p.D, q0, wave, lane, stq, sinv);

  // the tile's d from c0 on in the format: a wave per row (the wave that ran the row's prologue), a lane per group of four
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

  // k-group kg of step st of this wave's rows: lane l takes the OE d from KG kg + OE (l >> 4) of rows (l & 15), + 16
  opnd ring[NS_PF][2];
  const long long jl = jbeg + NS_WR * wave + lr;  // this lane's first row of step 0
  const elem* const g0 = static_cast<const elem*>(p.g);
  const elem* const gl = g0 + jl * p.D;
  auto fetch = [&](int slot, int st, int kg) __attribute__((always_inline)) {
    const long long sj = (long long)st * NS_GT;  // st == nsteps: past jend, nothing of it is read
#pragma unroll
    for (int rb = 0; rb < 2; ++rb)
      ring[slot][rb] = F::template load<VG>(jl + sj + 16 * rb < jend, gl + (sj + 16 * rb) * p.D, KG * kg + OE * kq, p.D, g0);
  };

  const elem* const bq = sq + lr * pitch + OE * kq;
#pragma unroll
  for (int u = 0; u < NS_PF; ++u) {
    fetch(u, 0, u);
    __builtin_amdgcn_sched_barrier(0);
  }
  for (int st = 0; st < nsteps; ++st) {
    const long long j0 = jbeg + (long long)st * NS_GT;
    accum acc[4][2];
    [[maybe_unused]] float tg[2][4];
#pragma unroll
    for (int qb = 0; qb < 4; ++qb) acc[qb][0] = acc[qb][1] = accum{};
    for (int kg0 = 0; kg0 < nkg; kg0 += NS_PF) {
      if (resident ? (st == 0 && kg0 == 0) : kg0 % (F::DC / KG) == 0) {  // uniform
        __syncthreads();  // the previous chunk's operand reads (and, first, the state's initialisation) are done
        stage(KG * kg0);
        __syncthreads();
      }
      // one turn of the ring, without a branch: k-group kg0 + u is consumed from slot u, which then takes the k-group
      // NS_PF further on (into the next step at the end of this one).  The tile is staged in whole turns, so the
      // k-groups past D that fill the last turn multiply zero by zero
#pragma unroll
      for (int u = 0; u < NS_PF; ++u) {
        const int kg = kg0 + u;
        const opnd a0 = F::template mask<VG>(ring[u][0], jl + (j0 - jbeg) < jend, KG * kg + OE * kq, p.D);
        const opnd a1 = F::template mask<VG>(ring[u][1], jl + (j0 - jbeg) + 16 < jend, KG * kg + OE * kq, p.D);
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
              for (int i = 0; i < 4; ++i)
                tg[rb][i] = p.scales[min(j0 + NS_WR * wave + 16 * rb + 4 * kq + i, p.G - 1)];
          }
        }
        const bool wrap = kg + NS_PF >= nkg;
        fetch(u, st + wrap, kg + NS_PF - (wrap ? nkg : 0));
        __builtin_amdgcn_sched_barrier(0);  // the loads stay in the ring's order: the waits count on it
      }
    }
    // the step's scores against the thresholds: acc[qb][rb][i] is query 16 qb + lr against row j0 + slot
#pragma unroll
    for (int qb = 0; qb < 4; ++qb) {
      const int ql = 16 * qb + lr;
      const u64 thr = sthr[ql];
      float tq = 0.0f;
      if constexpr (F::SCALES) tq = stq[ql];
      const bool q_ok = q0 + ql < p.n;
#pragma unroll
      for (int rb = 0; rb < 2; ++rb)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int slot = NS_WR * wave + 16 * rb + 4 * kq + i;
          const long long j = j0 + slot;
          float s;
          if constexpr (F::SCALES) s = F::score(acc[qb][rb][i], tq, tg[rb][i]);
          else s = F::score(acc[qb][rb][i]);
          const u64 key = topk_key(__float_as_uint(s), int(j));
          if (q_ok && j < jend && key > thr) {
            scand[ql * NS_GT + slot] = unsigned(key >> 32);
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
        const unsigned hi = scand[qi * NS_GT + slot];
        key[1 + h] = hi != NS_ABSENT ? (u64(hi) << 32) | u64(~unsigned(j0 + slot)) : 0ull;
        scand[qi * NS_GT + slot] = NS_ABSENT;
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

// the streaming kernel of a format, for nearest_launch
template <class F>
struct NearestStream {
  static constexpr int GT = NS_GT, VGE = 16 / int(sizeof(typename F::elem));
  static constexpr size_t LDS_MAX = ns_lds_bytes<F>(F::DRES, 64);
  static constexpr size_t lds(int D, int k) { return ns_lds_bytes<F>(D, k); }
  template <bool VQ, bool VG>
  static auto kernel() { return &nearest_stream_kernel<F, VQ, VG>; }
};

}  // namespace

}  // namespace ore
