// gram_geometry_probe.cpp — plan_gram_window's decisions on a CPU box (tests/test_gram_host.py).
// One query per line on stdin, one answer line each:
//   "plan n_clients ncols cus forced" -> np kc lc chunks grid share chain workspace_bytes
//   "cover n_clients ncols cus forced" -> blocks_with_no_chunk gaps_or_overlaps widest_share
// `cover` walks the kernel's own split (block b: chunks [b * chunks / grid, (b + 1) * chunks / grid))
// and counts the blocks it leaves empty and the places where one block's end is not the next one's
// begin (with the first at 0 and the last at `chunks`); widest_share is in columns.
#include "fa_geometry.hpp"

#include <cstdio>
#include <cstring>

int main() {
  char line[256];
  while (std::fgets(line, sizeof line, stdin)) {
    const bool plan = std::strncmp(line, "plan ", 5) == 0, cover = std::strncmp(line, "cover ", 6) == 0;
    if (!plan && !cover) {
      std::printf("bad query\n");
      return 2;
    }
    long long ncols = 0;
    int n = 0, cus = 0, forced = 0;
    if (std::sscanf(line + (plan ? 5 : 6), "%d %lld %d %d", &n, &ncols, &cus, &forced) != 4) return 2;
    const fa::GramPlan p = fa::plan_gram_window(n, ncols, cus, forced);
    if (plan) {
      std::printf("%d %d %d %lld %lld %lld %lld %lld\n", p.np, p.kc, p.lc, (long long)p.chunks, (long long)p.grid,
                  (long long)p.share, (long long)p.chain, (long long)p.workspace_bytes);
      continue;
    }
    long long empty = 0, breaks = 0, widest = 0, end = 0;
    for (long long b = 0; b < p.grid; ++b) {
      const long long cb = b * p.chunks / p.grid, ce = (b + 1) * p.chunks / p.grid;
      empty += ce <= cb;
      breaks += cb != end;
      end = ce;
      if ((ce - cb) * p.kc > widest) widest = (ce - cb) * p.kc;
    }
    breaks += end != p.chunks;
    std::printf("%lld %lld %lld\n", empty, breaks, widest);
  }
  return 0;
}
