// Host driver around the LDS Winograd kernel's workgroup geometry (csrc/ore_wino_geom.h), built and run by
// tests/test_wino_geom.py with the plain host compiler.
// usage: wino_geom_dump NCU N H W M [N H W M ...]
// per case: "case N H W M ok ntg mtiles mbs nmg nsmall grid", then one "bid tg mb0 mb1" line per workgroup
#include <cstdio>
#include <cstdlib>

#include "ore_wino_geom.h"

int main(int argc, char** argv) {
  if (argc < 6 || (argc - 2) % 4 != 0) return 2;
  const int ncu = std::atoi(argv[1]);
  for (int a = 2; a + 3 < argc; a += 4) {
    const int N = std::atoi(argv[a]), H = std::atoi(argv[a + 1]), W = std::atoi(argv[a + 2]), M = std::atoi(argv[a + 3]);
    const long long T = (long long)N * ((H + 1) / 2) * ((W + 1) / 2);
    ore::WmGroups g;
    const bool ok = ore::wm_groups(T, M, ncu, &g);
    if (!ok) {
      std::printf("case %d %d %d %d 0 0 0 0 0 0 0\n", N, H, W, M);
      continue;
    }
    std::printf("case %d %d %d %d 1 %d %d %d %d %d %d\n", N, H, W, M, g.ntg, g.mtiles, g.mbs, g.nmg, g.nsmall, g.grid);
    for (int bid = 0; bid < g.grid; ++bid) {
      const ore::WmWg w = ore::wm_wg_map(g, bid);
      std::printf("%d %d %d %d\n", bid, w.tg, w.mb0, w.mb1);
    }
  }
  return 0;
}
