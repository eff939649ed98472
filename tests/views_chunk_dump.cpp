// Host driver around the classify entries' group chunking (csrc/ore_chunk.h: group_chunks), built and run by
// tests/test_views_abi.py with the plain host compiler.
// usage: views_chunk_dump run_batch views nmax [the same three again ...]
// per case and per n = views, 2 views, ... <= nmax: "n nchunks chunk", then one "i0 nc" line per chunk in the
// walker's order (chunk c starts at c * chunk and takes what is left, chunk images at the most)
#include <cstdio>
#include <cstdlib>

#include "ore_chunk.h"

int main(int argc, char** argv) {
  if (argc < 4 || (argc - 1) % 3 != 0) return 2;
  for (int a = 1; a + 2 < argc; a += 3) {
    const long long run_batch = std::atoll(argv[a]), views = std::atoll(argv[a + 1]), nmax = std::atoll(argv[a + 2]);
    if (run_batch < 1 || views < 1 || views > run_batch) return 2;
    std::printf("case %lld %lld\n", run_batch, views);
    for (long long n = views; n <= nmax; n += views) {
      const ore::GroupChunks g = ore::group_chunks(n, run_batch, views);
      std::printf("n %lld %lld %lld\n", n, (long long)g.nchunks, (long long)g.chunk);
      long long done = 0;
      for (ore::Chunk c = ore::chunk_at(0, n, g.chunk); c.nc > 0; c = ore::chunk_at(c.i0 + c.nc, n, g.chunk), ++done)
        std::printf("%lld %lld\n", (long long)c.i0, (long long)c.nc);
      if (done != g.nchunks) return 3;
    }
  }
  return 0;
}
