// noise_geometry_probe — plan_gauss_add (flearn_amd/csrc/fa_geometry.hpp) on a CPU box, for
// tests/test_noise_host.py.  Reads queries from stdin, one per line, and answers each with one line:
//   plan  ncols cus forced -> quads blocks grid steps
//   cover ncols cus forced -> uncovered_or_twice written_outside busiest_lane_steps
// `cover` walks the window as gauss_add_kernel does (lane t of block b: quads b * 256 + t, + grid *
// 256, ...; whole quads as four columns, the ragged last one column by column) and counts the
// columns written other than once and the writes past the window.
#include <cstdio>
#include <cstring>
#include <vector>

#include "fa_geometry.hpp"

int main() {
  char what[16];
  long long ncols, cus, forced;
  while (std::scanf("%15s %lld %lld %lld", what, &ncols, &cus, &forced) == 4) {
    const fa::NoisePlan p = fa::plan_gauss_add(ncols, (int)cus, (int)forced);
    if (!std::strcmp(what, "plan")) {
      std::printf("%lld %lld %lld %lld\n", (long long)p.quads, (long long)p.blocks, (long long)p.grid, (long long)p.steps);
      continue;
    }
    const int64_t whole = ncols / 4, nquads = (ncols + 3) / 4, step = p.grid * fa::kNoiseBlock;
    std::vector<unsigned char> seen((size_t)ncols + 8, 0);
    long long busiest = 0;
    for (int64_t lane = 0; lane < step; ++lane) {
      long long mine = 0;
      for (int64_t q = lane; q < nquads; q += step) {
        ++mine;
        const int cols = q < whole ? 4 : (int)(ncols - q * 4);
        for (int e = 0; e < cols; ++e) ++seen[(size_t)(q * 4 + e)];
      }
      if (mine > busiest) busiest = mine;
    }
    long long bad = 0, outside = 0;
    for (size_t c = 0; c < seen.size(); ++c) {
      if (c < (size_t)ncols) bad += seen[c] != 1;
      else outside += seen[c] != 0;
    }
    std::printf("%lld %lld %lld\n", bad, outside, busiest);
  }
  return 0;
}
