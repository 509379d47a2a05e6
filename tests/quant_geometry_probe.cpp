// quant_geometry_probe — plan_q8_window (flearn_amd/csrc/fa_quant_geometry.hpp) on a CPU box, for
// tests/test_quant_host.py.  Reads queries from stdin, one per line, and answers each with one line:
//   plan  ncols cus forced -> V W D grid
//   cover ncols cus forced -> pc pieces uncovered_or_twice widest_block_pieces
// `cover` walks the window as deq_fold_kernel does (k rounds, pieces of pc chunks, block b: pieces b,
// b + grid, ..., piece p: chunks [p * pc, min((p + 1) * pc, chunks))) and counts the columns covered
// other than once.
#include <cstdio>
#include <cstring>
#include <vector>

#include "fa_quant_geometry.hpp"

int main() {
  char what[16];
  long long ncols, cus, forced;
  while (std::scanf("%15s %lld %lld %lld", what, &ncols, &cus, &forced) == 4) {
    const fa::Plan p = fa::plan_q8_window(ncols, (int)cus, (int)forced);
    if (!std::strcmp(what, "plan")) {
      std::printf("%d %d %d %lld\n", p.V, p.W, p.D, (long long)p.grid);
      continue;
    }
    const int64_t chunks = (ncols + 1023) / 1024, gr = p.grid;
    const int64_t k = (chunks + gr * p.W * p.V - 1) / (gr * p.W * p.V);
    const int64_t pc = (chunks + gr * k - 1) / (gr * k);
    const int64_t pieces = (chunks + pc - 1) / pc;
    std::vector<unsigned char> seen((size_t)ncols, 0);
    long long widest = 0;
    for (int64_t b = 0; b < gr; ++b) {
      long long mine = 0;
      for (int64_t q = b; q < pieces; q += gr) {
        const int64_t cb = q * pc, ce = cb + pc < chunks ? cb + pc : chunks;
        const int64_t cend = ce * 1024 < ncols ? ce * 1024 : ncols;
        if (cend <= cb * 1024) continue;
        ++mine;
        for (int64_t c = cb * 1024; c < cend; ++c) ++seen[(size_t)c];
      }
      if (mine > widest) widest = mine;
    }
    long long bad = 0;
    for (unsigned char s : seen) bad += s != 1;
    std::printf("%lld %lld %lld %lld\n", (long long)pc, (long long)pieces, bad, widest);
  }
  return 0;
}
