// Host driver around the runners' image chunking (csrc/ore_chunk.h), built and run by tests/test_chunk.py with
// the plain host compiler.
// usage: chunk_dump N x_nstride x_img_bytes x_es y_nstride y_img_bytes y_es [the same seven again ...]
// per case: "case nb", then one "i0 nc" line per chunk in launch order
#include <cstdio>
#include <cstdlib>

#include "ore_chunk.h"

int main(int argc, char** argv) {
  if (argc < 8 || (argc - 1) % 7 != 0) return 2;
  for (int a = 1; a + 6 < argc; a += 7) {
    long long v[7];
    for (int i = 0; i < 7; ++i) v[i] = std::atoll(argv[a + i]);
    const ore::ChunkSide x{v[1], v[2], int(v[3])}, y{v[4], v[5], int(v[6])};
    const long long nb = ore::image_chunk(v[0], x, y);
    std::printf("case %lld\n", nb);
    for (ore::Chunk c = ore::chunk_at(0, v[0], nb); c.nc > 0; c = ore::chunk_at(c.i0 + c.nc, v[0], nb))
      std::printf("%lld %lld\n", (long long)c.i0, (long long)c.nc);
  }
  return 0;
}
