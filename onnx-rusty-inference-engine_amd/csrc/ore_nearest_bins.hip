// Candidate search for the rerank, kernel 2: the c best of a query's NB bin winners, exact, at a
// cost that does not grow with c.  ore_nearest_bins.h's kernel leaves one 64-bit key (ore_topk_key.h) per query and
// bin; keys are unique and larger is better, so the answer is the c largest keys in descending order.
//
// One workgroup per query.  A radix select from the top byte of the key down finds the cut: a pass counts, in an LDS
// histogram, the byte at `shift` of every key whose bytes above it equal the prefix found so far; a scan from bucket
// 255 down finds the bucket in which the count of keys crosses the ranks still wanted; that bucket's byte joins the
// prefix.  The four bytes of the image come first and the four of the complemented row after them, so equal images
// are resolved by the lower row with no code of their own.  The passes stop as soon as the keys at or above the cut
// bucket are at most NBS_CAP (the last pass leaves one key in its bucket, keys being unique): typically after two or
// three of the eight.  Any pass but the last can be the one that ends it: the last never is, the cut bucket of the
// pass before it holding the bins of 256 consecutive rows, at most 8; the pass over the row's top byte is only on a
// gallery past 2^24 rows (tests/test_nearest_select_gpu.py takes the select to each of the seven).  Those survivors
// -- the c wanted ones among them -- go to LDS through a counter, each is ranked by counting the survivors above it
// (unique keys: rank = position) and the ranks below c are written.  Work: O(passes NB + NBS_CAP^2 / 256) per thread
// row, whatever c is; NB of any size by striding over the row.
#include "ore_kernels.h"
#include "ore_nearest.h"

namespace ore {

namespace {

constexpr int NBS_CAP = 512;  // survivors ranked in LDS: at least twice the largest c, so that a pass whose cut bucket
                              // holds up to 256 keys already ends the select

__global__ __launch_bounds__(256) void nearest_bins_select_kernel(const u64* __restrict__ win, long long NB, int c,
                                                                  float* __restrict__ values, int* __restrict__ indices) {
  __shared__ unsigned hist[256];
  __shared__ unsigned cut[3];  // the cut bucket, the keys above it, the keys in it
  __shared__ unsigned count;
  __shared__ u64 surv[NBS_CAP];
  const int tid = threadIdx.x;
  const u64* const keys = win + (long long)blockIdx.x * NB;
  u64 prefix = 0ull, himask = 0ull;
  unsigned want = unsigned(c);  // ranks still to be found among the keys that match the prefix
  for (int shift = 56;; shift -= 8) {
    hist[tid] = 0u;
    if (tid == 0) count = 0u;
    __syncthreads();
    for (long long j = tid; j < NB; j += 256) {
      const u64 k = keys[j];
      if ((k & himask) == prefix) atomicAdd(&hist[unsigned(k >> shift) & 255u], 1u);
    }
    __syncthreads();
    unsigned above = 0u;  // the matching keys in the buckets above this thread's
    for (int d = tid + 1; d < 256; ++d) above += hist[d];
    if (above < want && want <= above + hist[tid]) {  // one thread: the matching keys are at least `want`
      cut[0] = unsigned(tid);
      cut[1] = above;
      cut[2] = hist[tid];
    }
    __syncthreads();
    prefix |= u64(cut[0]) << shift;
    himask |= 255ull << shift;
    want -= cut[1];
    // the keys above the cut bucket number c - want < c, those in it cut[2]
    if (unsigned(c) - want + cut[2] <= unsigned(NBS_CAP) || shift == 0) break;  // the next write of cut is two barriers on
  }
  for (long long j = tid; j < NB; j += 256) {
    const u64 k = keys[j];
    if ((k & himask) >= prefix) surv[atomicAdd(&count, 1u)] = k;
  }
  __syncthreads();
  const int m = int(count);  // c <= m <= NBS_CAP
  for (int e = tid; e < m; e += 256) {
    const u64 k = surv[e];
    int rank = 0;
    for (int o = 0; o < m; ++o) rank += surv[o] > k;
    if (rank < c) {
      reinterpret_cast<unsigned*>(values)[(long long)blockIdx.x * c + rank] = topk_key_bits(k);
      indices[(long long)blockIdx.x * c + rank] = topk_key_index(k);
    }
  }
}

}  // namespace

int nearest_bins_segments(long long n, long long G, int ncu, int bin_rows) { return nearest_segments(n, G, ncu, 4 * bin_rows); }

size_t nearest_bins_bytes(long long n, long long G, int bin_rows) { return size_t(n) * size_t((G + bin_rows - 1) / bin_rows) * 8; }

void launch_nearest_bins_select(const void* win, int n, long long NB, int c, float* values, int* indices, hipStream_t s) {
  if (n <= 0) return;
  hipLaunchKernelGGL(nearest_bins_select_kernel, dim3((unsigned)n), dim3(256), 0, s, static_cast<const u64*>(win), NB, c, values,
                     indices);
}

}  // namespace ore
