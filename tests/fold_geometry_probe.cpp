// fold_geometry_probe.cpp — plan_fold_window's decisions on a CPU box (tests/test_fold_host.py).
// One query per line on stdin, "kind ncols cus forced", one answer line each:
//   family V W D grid chunks rounds piece_chunks pieces
// rounds, piece_chunks and pieces restate fold_kernel_rows' work split for that grid (block b takes
// pieces b, b + grid, ...; piece p is chunks [p * piece_chunks, ...)); 0 for the element-wise kernel.
#include "fa_geometry.hpp"

#include <cstdio>

int main() {
  char line[256];
  while (std::fgets(line, sizeof line, stdin)) {
    long long ncols = 0;
    int kind = 0, cus = 0, forced = 0;
    if (std::sscanf(line, "%d %lld %d %d", &kind, &ncols, &cus, &forced) != 4) {
      std::printf("bad query\n");
      return 2;
    }
    const fa::Plan p = fa::plan_fold_window(kind, ncols, cus, forced);
    long long chunks = 0, k = 0, pc = 0, pieces = 0;
    if (p.family == fa::kFamFoldRows) {
      chunks = fa::row_chunks(ncols);
      const long long g = p.grid;
      k = (chunks + g * p.W * p.V - 1) / (g * p.W * p.V);
      pc = (chunks + g * k - 1) / (g * k);
      pieces = (chunks + pc - 1) / pc;
    }
    std::printf("%s %d %d %d %lld %lld %lld %lld %lld\n", p.family == fa::kFamFoldRows ? "fold_rows" : "fold_elem", p.V, p.W,
                p.D, (long long)p.grid, chunks, k, pc, pieces);
  }
  return 0;
}
