// Candidate search on an MXFP4 gallery (extension, ore_nearest_bins_mxfp4 and ore_gallery_mxfp4): the
// best gallery row of every bin of B consecutive rows per query under ore_topk_f32's order (ore_topk_key.h) of
//   s[i, j] = sum over blocks of 32 d of 2^(eq + eg) sum_d cq cg,
// 4-bit E2M1 codes with one E8M0 scale byte per block on both sides, on v_mfma_scale_f32_16x16x128_f8f6f4 -- and the
// packer that makes codes and scale bytes by include/ore.h's rule.  The winners go to ore_nearest_bins.hip's select.
//
// Split: ore_nearest_bins.h's.  grid = (ceil(n / 64) query tiles, S gallery segments), four waves, wave w walks the
// quarter [jbeg + w wr, jbeg + (w + 1) wr) of its segment, 32 rows per step as two A operands of 16 rows against the
// four query blocks of the tile: eight MFMAs per k-group of 128 d, 32 accumulators, the running best of the open bin
// in registers, the permlane wave-max and one 8-byte store per lane at a bin's end, no barrier in the step loop.
//
// Operands.  Lane l supplies row l & 15 and the 32 d from 128 kg + 32 (l >> 4): 16 bytes, one MX block, and its scale
// byte applies to exactly that row and block.  The gallery row is A, the query B; acc[i] of lane l is query l & 15
// against row 4 (l >> 4) + i.
//
// Query tile.  Quantised once per workgroup into LDS: a wave per row, eight lanes per block (four d each, the block
// maximum by three DPP exchanges), 64 rows of 64 nkg code bytes at a pitch of 16 bytes more (a row starts an odd
// multiple of 4 banks after the one before), then the scale bytes as dwords [row][l >> 4][kg / 4]: byte kg & 3 of a
// dword is the scale of block 4 kg + (l >> 4), so a lane reads one dword per query block for four consecutive k-groups
// and the MFMA's opsel picks the k-group.  Up to D = 512 (NKG = 1, 2, 4 k-groups, compiled in) those four dwords are
// read once and opsel_b is the unrolled slot's k-group, an immediate; above (NKG = 0: any number of k-groups) the dword
// is read per k-group and shifted by a wave-uniform count.  Blocks past D hold code 0 and scale byte 0.
//
// Gallery.  16-byte loads straight into the A operand through a ring of F4_PF = 8 slots that counts (step, k-group)
// pairs and runs on across the steps: pair p is consumed from slot p % 8, which then takes pair p + 8.  With NKG
// compiled in, a turn of the ring is 8 / NKG whole steps, straight-line; with NKG = 0 the step's end is a wave-uniform
// branch in each slot (around the scoring only, never around a load).  No k-group of padding is ever issued: a step is
// ceil(D / 128) pairs.  A row past the wave's range or a block past D is read from the gallery's first bytes and made
// 0 when it is consumed.
//
// Gallery scale bytes.  In the ring, at a fixed place.  VS (D in 481..512, scales 16-byte aligned): a row's 16 scale
// bytes in one load per row and step, issued with the step's first pair two steps ahead; dword kg shifted right by
// 8 (l >> 4) puts the lane's byte into byte 0, opsel_a = 0.  Otherwise one byte load per row and pair beside the
// pair's code loads, at the address clamped to the array's first byte, made 0 (2^-127, times code 0) when masked.
//
// Position independence.  K is never split; a score is one accumulator's chain over the k-groups ascending from +0.
#include <algorithm>
#include <utility>

#include "ore_nearest.h"

namespace ore {

namespace {

typedef int intx4 __attribute__((ext_vector_type(4)));
typedef int intx8 __attribute__((ext_vector_type(8)));

constexpr int F4_DMAX = 4096;  // the query tile is always resident: 64 rows of D / 2 + 16 bytes and the scales, 140 KB
constexpr int F4_WR = 32;      // gallery rows per wave and step
constexpr int F4_PF = 8;       // (step, k-group) pairs the gallery loads run ahead of the MFMAs
constexpr int F4_WG_CU = 2;    // workgroups per compute unit the kernel is compiled and the segments are cut for (the VGPRs)

// ---- include/ore.h's block rule, shared by the packer and the kernel's query path

template <int CTRL>
__device__ __forceinline__ float f4_dpp_fmax(float a) {
  return fmaxf(a, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(a), CTRL, 0xf, 0xf, false)));
}
// the maximum over the eight lanes of a block (a >= 0), in each of them
__device__ __forceinline__ float f4_block_fmax(float a) {
  a = f4_dpp_fmax<0xb1>(a);     // quad_perm [1,0,3,2]
  a = f4_dpp_fmax<0x4e>(a);     // quad_perm [2,3,0,1]
  return f4_dpp_fmax<0x141>(a);  // row_half_mirror
}
__device__ __forceinline__ float f4_fmax4(floatx4 v) {
  return fmaxf(fmaxf(fmaxf(fabsf(v[0]), fabsf(v[1])), fabsf(v[2])), fabsf(v[3]));  // NaNs skipped
}
__device__ __forceinline__ unsigned f4_scale_byte(float a) {
  const int e = int(__float_as_uint(fminf(a, 3.402823466e+38f)) >> 23) - 2;
  return unsigned(min(max(e, 0), 254));
}
// sign and E2M1 magnitude of x / 2^(b - 127): ties to the even code, saturated at 6 (code 7); a NaN is code 0
__device__ __forceinline__ unsigned f4_code(float x, unsigned b) {
  const float m = __builtin_ldexpf(fabsf(x), 127 - int(b));  // exact
  const float c = m < 2.0f ? __builtin_rintf(2.0f * m) : m < 4.0f ? 2.0f + __builtin_rintf(m) : fminf(4.0f + __builtin_rintf(0.5f * m), 7.0f);
  return x != x ? 0u : unsigned(int(c)) | (__float_as_uint(x) >> 31) << 3;
}
__device__ __forceinline__ unsigned f4_code4(floatx4 v, unsigned b) {
  return f4_code(v[0], b) | f4_code(v[1], b) << 4 | f4_code(v[2], b) << 8 | f4_code(v[3], b) << 12;
}

// f32 rows -> codes and scale bytes: eight lanes per block of 32 d, four d each, one pass -- the maximum over the eight
// lanes, then the codes from the registers that hold the block: 2 packed bytes per lane and a scale byte per block
template <bool VEC>
__global__ __launch_bounds__(256) void gallery_mxfp4_kernel(const float* __restrict__ src, unsigned char* __restrict__ codes,
                                                            unsigned char* __restrict__ scales, long long G, int D, int nb) {
  const int sub = threadIdx.x & 7;
  const long long total = G * nb;
  for (long long t = 32LL * blockIdx.x + (threadIdx.x >> 3); t < total; t += 32LL * gridDim.x) {  // whole blocks of lanes
    const long long r = t / nb;
    const int blk = int(t - r * nb);
    const floatx4 v = nn_load4<VEC>(true, src + r * D, 32 * blk + 4 * sub, D);
    const unsigned b = f4_scale_byte(f4_block_fmax(f4_fmax4(v)));
    *reinterpret_cast<unsigned short*>(codes + 16 * t + 2 * sub) = static_cast<unsigned short>(f4_code4(v, b));
    if (sub == 0) scales[t] = static_cast<unsigned char>(b);
  }
}

// ---- the search

struct Fp4Args {
  const float* q;
  const unsigned char* codes;   // [G][16 nb]
  const unsigned char* scales;  // [G][nb]
  u64* win;                     // [n][NB]
  long long q_stride, G, NB, seg_rows;  // seg_rows: gallery rows per segment, a multiple of 4 B
  int n, D, lgR;                        // B = 32 << lgR
};

__host__ __device__ constexpr int f4_nkg(int D) { return (D + 127) / 128; }
__host__ __device__ constexpr size_t f4_lds_bytes(int nkg) {
  return size_t(NN_QT) * (64 * nkg + 16) + size_t(NN_QT) * 16 * ((nkg + 3) / 4);
}
static_assert(f4_lds_bytes(f4_nkg(F4_DMAX)) <= 160 * 1024 && F4_WG_CU * f4_lds_bytes(4) <= 160 * 1024, "LDS");

template <int OPB>
__device__ __forceinline__ floatx4 f4_mfma(intx4 a, intx4 b, floatx4 c, unsigned sa, unsigned sb) {
  const intx8 a8 = {a[0], a[1], a[2], a[3], 0, 0, 0, 0}, b8 = {b[0], b[1], b[2], b[3], 0, 0, 0, 0};  // FP4: four registers
  return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a8, b8, c, 4, 4, 0, int(sa), OPB, int(sb));
}

template <class F, int... U>
__device__ __forceinline__ void f4_each(F&& f, std::integer_sequence<int, U...>) {
  (f(std::integral_constant<int, U>{}), ...);
}

// NKG: the k-groups of a step, 1, 2 or 4, or 0 for any number; VQ: 16-byte loads of the queries; VS: of the scales
template <int NKG, bool VQ, bool VS>
__global__ __launch_bounds__(256, F4_WG_CU) void nearest_bins_fp4_kernel(Fp4Args p) {
  static_assert(!VS || NKG == 4, "a row's scale bytes in one load: 16 blocks");
  extern __shared__ __attribute__((aligned(16))) unsigned char f4_lds[];
  const int nb = (p.D + 31) >> 5, nkg = NKG ? NKG : (nb + 3) >> 2, nkg4 = (nkg + 3) >> 2;
  const int pitch = 64 * nkg + 16;
  unsigned char* const sq = f4_lds;
  unsigned* const sqs = reinterpret_cast<unsigned*>(f4_lds + NN_QT * pitch);  // [64][4][nkg4]

  const int tid = threadIdx.x, lane = tid & 63, lr = lane & 15, kq = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const long long q0 = (long long)blockIdx.x * NN_QT;
  const long long jbeg = (long long)blockIdx.y * p.seg_rows, wr = p.seg_rows >> 2;
  const int R = 1 << p.lgR;
  // the steps of wave 0, in whole bins: no other wave has more rows below G (jbeg < G: no segment is empty)
  const int nsteps = int((min(wr, p.G - jbeg) + F4_WR * R - 1) >> (5 + p.lgR)) << p.lgR;
  const long long jw = jbeg + wr * wave, jlim = min(p.G, jw + (long long)F4_WR * nsteps);  // this wave's rows: [jw, jlim)

  // the tile: a wave per row, eight lanes per block
  for (int r = wave; r < NN_QT; r += 4) {
    const long long qi = q0 + r;
    const float* const row = p.q + qi * p.q_stride;
    for (int d = 4 * lane; d < 128 * nkg; d += 256) {  // whole blocks of lanes
      const floatx4 v = nn_load4<VQ>(qi < p.n, row, d, p.D);
      const unsigned b = f4_scale_byte(f4_block_fmax(f4_fmax4(v)));
      *reinterpret_cast<unsigned short*>(sq + r * pitch + (d >> 1)) = static_cast<unsigned short>(f4_code4(v, b));
      if ((lane & 7) == 0) {
        const int blk = d >> 5, kg = blk >> 2;
        reinterpret_cast<unsigned char*>(sqs)[(((r * 4 + (blk & 3)) * nkg4 + (kg >> 2)) << 2) + (kg & 3)] = static_cast<unsigned char>(b);
      }
    }
  }
  __syncthreads();

  // the ring: pair (st, kg) of this wave's rows; lane l takes block 4 kg + (l >> 4) of rows (l & 15), + 16
  intx4 ring[F4_PF][2];
  [[maybe_unused]] unsigned rsc[F4_PF][2];  // !VS: the pair's scale bytes
  [[maybe_unused]] intx4 sv[2][2];          // VS: the step's 16 scale bytes per row, and the lane's four of them
  [[maybe_unused]] unsigned sa[2][4];
  const long long jl = jw + lr;  // this lane's A row of step 0, rb 0
  const int lleft = int(max(min(jlim - jl, 1LL << 30), -1LL));  // rows e of the lane with e < lleft are there
  // an address is a wave-uniform base (the wave's row jw + e, or the array's first bytes past the wave's range) and
  // a 32-bit lane part, 0 where the lane's own row or block is not there
  const int wleft = int(max(min(jlim - jw, 1LL << 30), -1LL));
  const unsigned gvo = unsigned(lr * nb + kq) * 16u, svo = unsigned(lr * nb + kq);
  auto fetch = [&](auto uc, int st, int kg) __attribute__((always_inline)) {
    constexpr int u = decltype(uc)::value;
#pragma unroll
    for (int rb = 0; rb < 2; ++rb) {
      const int e = F4_WR * st + 16 * rb;
      const bool uok = e < wleft, ok = e < lleft && 4 * kg + kq < nb;
      const long long ublk = uok ? (jw + e) * nb + 4 * kg : 0LL;
      ring[u][rb] = *reinterpret_cast<const intx4*>(p.codes + ublk * 16 + (ok ? gvo : 0u));
      if constexpr (VS) {
        if (u % 4 == 0) sv[u / 4][rb] = *reinterpret_cast<const intx4*>(p.scales + ublk + (e < lleft ? 16u * lr : 0u));
      } else {
        rsc[u][rb] = p.scales[ublk + (ok ? svo : 0u)];
      }
    }
  };

  // the running best of the open bin per query block (ore_nearest_bins.h)
  unsigned bimg[4] = {0u, 0u, 0u, 0u};
  int brow[4];
  const int jmine = int(jw) + 4 * kq;  // the first row this lane scores (G < 2^31)
#pragma unroll
  for (int qb = 0; qb < 4; ++qb) brow[qb] = jmine;

  floatx4 acc[4][2];
#pragma unroll
  for (int qb = 0; qb < 4; ++qb) acc[qb][0] = acc[qb][1] = floatx4{};

  // the step's scores against the running best, this lane's rows in ascending order, and the bin's end
  auto finish = [&](int st) __attribute__((always_inline)) {
    const long long js = (long long)st * F4_WR;
    const int j0 = jmine + F4_WR * st;
    const int left = int(max(min(jlim - (jw + js + 4 * kq), (long long)F4_WR), 0LL));
#pragma unroll
    for (int qb = 0; qb < 4; ++qb)
#pragma unroll
      for (int rb = 0; rb < 2; ++rb)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          unsigned img = unsigned(topk_key(__float_as_uint(acc[qb][rb][i]), 0) >> 32);
          img = 16 * rb + i < left ? img : 0u;
          const bool up = img > bimg[qb];
          bimg[qb] = up ? img : bimg[qb];
          brow[qb] = up ? j0 + 16 * rb + i : brow[qb];
        }
    if (((st + 1) & (R - 1)) == 0) {  // the bin ends: wave-uniform
      const bool have = jw + js - F4_WR * (R - 1) + 4 * kq < jlim;  // this lane's first row of the bin is there
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
        brow[qb] = jmine + F4_WR * (st + 1);
      }
      const long long bin = (jw >> (5 + p.lgR)) + (st >> p.lgR), qi = q0 + lane;  // lane l: query block l >> 4, row l & 15
      if (qi < p.n && bin < p.NB) p.win[qi * p.NB + bin] = mine;
    }
  };

  const unsigned char* const bq = sq + lr * pitch + 16 * kq;
  const unsigned* const bs = sqs + (lr * 4 + kq) * nkg4;
  [[maybe_unused]] unsigned qs[4];  // NKG: the lane's query scales of the whole of D
  if constexpr (NKG != 0) {
#pragma unroll
    for (int qb = 0; qb < 4; ++qb) qs[qb] = bs[64 * qb * nkg4];
  }

  int st = 0;                                      // NKG: the turn's first step; otherwise the step of the slot
  [[maybe_unused]] int kg = 0, fst = 0, fkg = 0;  // !NKG: the slot's k-group, and the pair F4_PF ahead
  auto advance = [&](int& s, int& k) __attribute__((always_inline)) {
    const bool wrap = k + 1 == nkg;
    k = wrap ? 0 : k + 1;
    s += wrap;
  };
  f4_each([&](auto uc) __attribute__((always_inline)) {
    constexpr int u = decltype(uc)::value;
    if constexpr (NKG != 0) {
      fetch(uc, u / NKG, u % NKG);
    } else {
      fetch(uc, fst, fkg);
      advance(fst, fkg);
    }
    __builtin_amdgcn_sched_barrier(0);
  }, std::make_integer_sequence<int, F4_PF>{});

  // one slot of a turn: pair (sst, skg) is consumed from slot u, which then takes the pair F4_PF further on
  auto slot = [&](auto uc) __attribute__((always_inline)) {
    constexpr int u = decltype(uc)::value;
    constexpr int OPB = NKG ? u % (NKG ? NKG : 1) : 0;
    const int sst = NKG ? st + u / (NKG ? NKG : 1) : st, skg = NKG ? OPB : kg;
    if constexpr (VS) {
      if (u % 4 == 0) {
#pragma unroll
        for (int rb = 0; rb < 2; ++rb)
#pragma unroll
          for (int k = 0; k < 4; ++k) sa[rb][k] = unsigned(sv[u / 4][rb][k]) >> (8 * kq);
      }
    }
    intx4 a[2];
    unsigned as[2];
#pragma unroll
    for (int rb = 0; rb < 2; ++rb) {
      const bool ok = F4_WR * sst + 16 * rb < lleft && 4 * skg + kq < nb;
      const int m = ok ? -1 : 0;
      a[rb] = ring[u][rb] & intx4{m, m, m, m};
      if constexpr (VS) as[rb] = sa[rb][OPB];
      else as[rb] = ok ? rsc[u][rb] : 0u;
    }
    const unsigned char* const b = bq + 64 * skg;
#pragma unroll
    for (int qb = 0; qb < 4; ++qb) {
      const intx4 bv = *reinterpret_cast<const intx4*>(b + 16 * qb * pitch);
      unsigned sb;
      if constexpr (NKG != 0) sb = qs[qb];
      else sb = bs[64 * qb * nkg4 + (skg >> 2)] >> (8 * (skg & 3));
      acc[qb][0] = f4_mfma<OPB>(a[0], bv, acc[qb][0], as[0], sb);
      acc[qb][1] = f4_mfma<OPB>(a[1], bv, acc[qb][1], as[1], sb);
    }
    if constexpr (NKG != 0) {
      fetch(uc, sst + F4_PF / (NKG ? NKG : 1), skg);
    } else {
      fetch(uc, fst, fkg);
      advance(fst, fkg);
    }
    __builtin_amdgcn_sched_barrier(0);  // the loads stay in the ring's order: the waits count on it
    if (skg == nkg - 1) {               // the step ends: compiled in, or wave-uniform
      if (sst < nsteps) finish(sst);    // the pairs that fill the last turn belong to no step
#pragma unroll
      for (int qb = 0; qb < 4; ++qb) acc[qb][0] = acc[qb][1] = floatx4{};
    }
    if constexpr (NKG == 0) advance(st, kg);
  };
  while (st < nsteps) {
    f4_each(slot, std::make_integer_sequence<int, F4_PF>{});
    if constexpr (NKG != 0) st += F4_PF / (NKG ? NKG : 1);
  }
}

template <int NKG, bool VQ, bool VS>
void nearest_bins_fp4_instance(const Fp4Args& a, int S, hipStream_t s) {
  static std::atomic<unsigned long long> raised{0};
  const auto kernel = &nearest_bins_fp4_kernel<NKG, VQ, VS>;
  if (NKG == 0) ore_raise_lds_once(raised, reinterpret_cast<const void*>(kernel), int(f4_lds_bytes(f4_nkg(F4_DMAX))));
  const dim3 grid((unsigned)((a.n + NN_QT - 1) / NN_QT), (unsigned)S);
  hipLaunchKernelGGL(kernel, grid, dim3(256), f4_lds_bytes(f4_nkg(a.D)), s, a);
}

template <int NKG, bool VS>
void nearest_bins_fp4_vq(const Fp4Args& a, int S, hipStream_t s) {
  const bool vq = a.D % 4 == 0 && a.q_stride % 4 == 0 && (reinterpret_cast<uintptr_t>(a.q) & 15) == 0;
  if (vq) nearest_bins_fp4_instance<NKG, true, VS>(a, S, s);
  else nearest_bins_fp4_instance<NKG, false, VS>(a, S, s);
}

}  // namespace

int nearest_mxfp4_max_d() { return F4_DMAX; }

int nearest_bins_segments_mxfp4(long long n, long long G, int ncu, int bin_rows) {
  const long long qt = std::max<long long>((n + NN_QT - 1) / NN_QT, 1), unit = 4LL * bin_rows, units = (G + unit - 1) / unit;
  const long long want = std::min<long long>(std::min(std::max<long long>((long long)F4_WG_CU * ncu / qt, 1), units), 65535);
  const long long per = (units + want - 1) / want;
  return int((units + per - 1) / per);  // no segment is empty
}

void launch_gallery_mxfp4(const float* src, long long G, long long D, void* codes, void* scales, hipStream_t s) {
  const int nb = int((D + 31) / 32);
  const dim3 grid((unsigned)std::min<long long>((G * nb + 31) / 32, 1 << 20));
  const auto c = static_cast<unsigned char*>(codes), t = static_cast<unsigned char*>(scales);
  if (D % 4 == 0 && (reinterpret_cast<uintptr_t>(src) & 15) == 0)
    hipLaunchKernelGGL(gallery_mxfp4_kernel<true>, grid, dim3(256), 0, s, src, c, t, G, int(D), nb);
  else
    hipLaunchKernelGGL(gallery_mxfp4_kernel<false>, grid, dim3(256), 0, s, src, c, t, G, int(D), nb);
}

void launch_nearest_bins_mxfp4(const float* q, long long q_stride, int n, int D, const void* codes, const void* scales, long long G,
                               int bin_rows, int S, void* win, hipStream_t s) {
  if (n <= 0) return;
  const long long unit = 4LL * bin_rows, units = (G + unit - 1) / unit, per = (units + S - 1) / S;
  int lgR = 0;
  while ((32 << lgR) < bin_rows) ++lgR;
  const Fp4Args a{q, static_cast<const unsigned char*>(codes), static_cast<const unsigned char*>(scales), static_cast<u64*>(win),
                  q_stride, G, (G + bin_rows - 1) / bin_rows, per * unit, n, D, lgR};
  const int nkg = f4_nkg(D);
  if (nkg == 4 && (D + 31) / 32 == 16 && (reinterpret_cast<uintptr_t>(scales) & 15) == 0) nearest_bins_fp4_vq<4, true>(a, S, s);
  else if (nkg == 4) nearest_bins_fp4_vq<4, false>(a, S, s);
  else if (nkg == 2) nearest_bins_fp4_vq<2, false>(a, S, s);
  else if (nkg == 1) nearest_bins_fp4_vq<1, false>(a, S, s);
  else nearest_bins_fp4_vq<0, false>(a, S, s);
}

}  // namespace ore
