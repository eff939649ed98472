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

}  // namespace ore
