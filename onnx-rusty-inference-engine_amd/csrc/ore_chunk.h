// Image chunks of a batched launch (host only, no HIP: compiled alone by tests/test_chunk.py).
// The kernels address activations through buffer resources (32-bit byte offsets, plus up to a few KB
// read before x by the 3x3 tap loads): a batch whose input or output extent does not fit is launched
// in image chunks that do.
#pragma once
#include <algorithm>
#include <cstdint>

namespace ore {

constexpr int64_t CHUNK_LIMIT = (int64_t(1) << 31) - (int64_t(1) << 21);

// one side of a launch: images `nstride` elements of `es` bytes apart, `img_bytes` valid in each
struct ChunkSide {
  int64_t nstride, img_bytes;
  int es;
  int64_t bytes(int64_t nb) const { return (nb - 1) * nstride * es + img_bytes; }  // extent of nb images
};

// images per chunk: N when the whole batch fits, else N halved (rounding up) until a chunk does;
// 0: one image alone is too large
inline int64_t image_chunk(int64_t N, const ChunkSide& x, const ChunkSide& y) {
  auto fits = [&](int64_t nb) { return x.bytes(nb) < CHUNK_LIMIT && y.bytes(nb) < CHUNK_LIMIT; };
  if (!fits(1)) return 0;
  int64_t nb = N;
  while (nb > 1 && !fits(nb)) nb = (nb + 1) / 2;
  return nb;
}

// images [i0, i0 + nc) of a batch of N taken nb at a time; nc 0 past the end:
// for (Chunk c = chunk_at(0, N, nb); c.nc > 0; c = chunk_at(c.i0 + c.nc, N, nb))
struct Chunk {
  int64_t i0, nc;
};
inline Chunk chunk_at(int64_t i0, int64_t N, int64_t nb) { return {i0, std::max<int64_t>(0, std::min(nb, N - i0))}; }

// The model's passes over n images, run_batch at the most in each, in whole groups of `views` consecutive images
// (ore_model_set_views; n a multiple of views, 1 <= views <= run_batch): with G = n / views groups and gb =
// run_batch / views groups per pass, ceil(G / gb) equal chunks of ceil(G / nchunks) groups.  chunk is in images;
// walk it with chunk_at(i0, n, chunk).  At views == 1: equal chunks of consecutive images, at most run_batch each.
struct GroupChunks {
  int64_t nchunks, chunk;
};
inline GroupChunks group_chunks(int64_t n, int64_t run_batch, int64_t views) {
  const int64_t G = n / views, gb = run_batch / views;
  const int64_t nchunks = G > gb ? (G + gb - 1) / gb : 1;
  return {nchunks, (G + nchunks - 1) / nchunks * views};
}

}  // namespace ore
