// Workgroup geometry of the LDS-staged Winograd kernel (conv_winol_kernel, ore_conv_wino.hip): how a
// launch's (tile group, 32-channel block) pairs are shared out over its workgroups.  Plain C++ besides
// the __host__ __device__ marks, so a host test can compile it alone (tests/test_wino_geom.py).
#pragma once

#if defined(__HIPCC__)
#define ORE_WM_HD __host__ __device__
#else
#define ORE_WM_HD
#endif

namespace ore {

constexpr int WM_TILES = 64;  // 2x2 tiles per workgroup (16 per wave)
constexpr int WM_CH = 32;     // output channels per m-block
// workgroups the m-grouping keeps at least (4 per resident slot of a 256-CU part at two per CU): the blocks of
// a tile group are shared out only as far as the launch stays this wide
constexpr long long WM_MIN_WG = 2048;
constexpr int WM_MAX_MBS = 8;
constexpr int WM_XCDS = 8;  // consecutive workgroup ids go round the XCDs

// A tile group's mtiles m-blocks go to nmg workgroups of mbs blocks each ("large"), or, for the last nsmall
// tile groups of every XCD, to mtiles workgroups of one block each.  XCD x = blockIdx % 8 owns a contiguous
// range of tile groups (ntg / 8, the first ntg % 8 XCDs one more) and walks it in the order of its local
// workgroup index blockIdx / 8: first the large workgroups, tile group by tile group (the workgroups of a
// tile group consecutive: they share its staged rows in the XCD's L2), then the single-block ones.
struct WmGroups {
  int ntg;        // tile groups of WM_TILES
  int mtiles;     // 32-channel m-blocks
  int mbs;        // m-blocks per large workgroup
  int nmg;        // large workgroups per tile group = ceil(mtiles / mbs)
  int nsmall;     // tile groups per XCD on single-block workgroups (fewer where the XCD owns fewer)
  int grid;       // workgroups launched: 8 x the largest XCD's count (the others' spares do nothing)
  float rNMG, rMT;  // 1 / nmg, 1 / mtiles (wm_div)
};

// n / d for 0 <= n < 2^22 from a float reciprocal rd = 1 / d: the float quotient is within
// (n / d) 2^-23 < 1 / (2 d) of n / d, so the truncation is the quotient or one below, fixed by the remainder
ORE_WM_HD inline int wm_div(int n, int d, float rd) {
  int q = (int)((float)n * rd);
  q += n - q * d >= d ? 1 : 0;
  return q;
}

// The grouping rule.  mbs: the largest divisor of the block count that keeps >= WM_MIN_WG workgroups.  nsmall:
// the dispatcher hands a freed slot the next workgroup id, so an XCD's ncu / 8 CUs take its large workgroups
// ceil(large / CUs) deep, mbs blocks each, and the single blocks then level the CUs; the most loaded CU ends at
// ceil(blocks / CUs) -- what single-block workgroups throughout would give -- as long as the large phase stays
// within that: nsmall is the smallest count for which it does.  false: outside wm_div's range.
inline bool wm_groups(long long T, int M, int ncu, WmGroups* g) {
  if (T <= 0 || T >= (1LL << 22) || M <= 0) return false;  // wm_div's range (4M tiles: 5,700 images at 54 x 54)
  g->ntg = (int)((T + WM_TILES - 1) / WM_TILES);
  g->mtiles = (M + WM_CH - 1) / WM_CH;
  g->mbs = 1;
  for (int b = 2; b <= (g->mtiles < WM_MAX_MBS ? g->mtiles : WM_MAX_MBS); ++b)
    if (g->mtiles % b == 0 && (long long)g->ntg * (g->mtiles / b) >= WM_MIN_WG) g->mbs = b;
  g->nmg = (g->mtiles + g->mbs - 1) / g->mbs;
  const int ntgx = (g->ntg + WM_XCDS - 1) / WM_XCDS;  // the largest XCD's tile groups
  g->nsmall = 0;
  if (g->mbs > 1) {
    const long long cus = ncu / WM_XCDS > 0 ? ncu / WM_XCDS : 1;
    const long long target = ((long long)ntgx * g->mtiles + cus - 1) / cus;  // blocks on the most loaded CU
    const long long large = (target / g->mbs) * cus / g->nmg;               // tile groups the large phase may take
    g->nsmall = large >= ntgx ? 0 : (int)(ntgx - large);
  }
  const long long per_xcd = (long long)(ntgx - g->nsmall) * g->nmg + (long long)g->nsmall * g->mtiles;
  if (per_xcd * WM_XCDS >= (1LL << 22)) return false;  // wm_div's range for the local workgroup index
  g->grid = (int)(per_xcd * WM_XCDS);
  g->rNMG = 1.0f / (float)g->nmg;
  g->rMT = 1.0f / (float)g->mtiles;
  return true;
}

struct WmWg {
  int tg;        // tile group
  int mb0, mb1;  // m-blocks [mb0, mb1); empty: a spare workgroup
};

// workgroup (blockIdx) -> its tile group and m-blocks: the kernel's and the host's one definition
ORE_WM_HD inline WmWg wm_wg_map(const WmGroups& g, int bid) {
  const int xcd = bid & (WM_XCDS - 1), li = bid / WM_XCDS;
  const int q = g.ntg / WM_XCDS, r = g.ntg % WM_XCDS;
  const int ntgx = q + (xcd < r ? 1 : 0), tg0 = xcd * q + (xcd < r ? xcd : r);
  const int ns = g.nsmall < ntgx ? g.nsmall : ntgx, nl = ntgx - ns;
  const int nlarge = nl * g.nmg;
  WmWg w;
  if (li < nlarge) {
    const int t = wm_div(li, g.nmg, g.rNMG), mg = li - t * g.nmg;
    w.tg = tg0 + t;
    w.mb0 = mg * g.mbs;
    w.mb1 = w.mb0 + g.mbs < g.mtiles ? w.mb0 + g.mbs : g.mtiles;
  } else {
    const int j = li - nlarge, t = wm_div(j, g.mtiles, g.rMT);
    w.tg = tg0 + nl + t;
    w.mb0 = j - t * g.mtiles;
    w.mb1 = t < ns ? w.mb0 + 1 : w.mb0;
  }
  return w;
}

}  // namespace ore
