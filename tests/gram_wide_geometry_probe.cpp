// gram_wide_geometry_probe.cpp — plan_gram_wide's decisions on a CPU box (tests/test_gram_wide_host.py).
// One query "n_clients ncols cus forced" per line on stdin, one answer line each:
//   tiles panels pairs kc lc chunks slices share chain workspace_bytes sized_bytes empty breaks widest
// sized_bytes is gram_wide_workspace_bytes; the last three walk the kernel's own split (slice s: chunks
// [s * chunks / slices, (s + 1) * chunks / slices)): the slices left empty, the places where one
// slice's end is not the next one's begin (the first at 0, the last at `chunks`), and the widest
// slice in columns.  Every pair takes every slice, so this covers every (pair, chunk) once.
#include "fa_gramwide_geometry.hpp"

#include <cstdio>

int main() {
  long long ncols = 0;
  int n = 0, cus = 0, forced = 0;
  while (std::scanf("%d %lld %d %d", &n, &ncols, &cus, &forced) == 4) {
    const fa::GramWidePlan p = fa::plan_gram_wide(n, ncols, cus, forced);
    long long empty = 0, breaks = 0, widest = 0, end = 0;
    for (long long s = 0; s < p.slices; ++s) {
      const long long cb = s * p.chunks / p.slices, ce = (s + 1) * p.chunks / p.slices;
      empty += ce <= cb;
      breaks += cb != end;
      end = ce;
      if ((ce - cb) * p.kc > widest) widest = (ce - cb) * p.kc;
    }
    breaks += end != p.chunks;
    std::printf("%d %d %d %d %d %lld %lld %lld %lld %lld %lld %lld %lld %lld\n", p.tiles, p.panels, p.pairs, p.kc, p.lc,
                (long long)p.chunks, (long long)p.slices, (long long)p.share, (long long)p.chain,
                (long long)p.workspace_bytes, (long long)(p.tiles ? fa::gram_wide_workspace_bytes(n, ncols) : 0), empty,
                breaks, widest);
  }
  return 0;
}
