// clip_geometry_probe — plan_rownorm_window (flearn_amd/csrc/fa_geometry.hpp) on a CPU box, for
// tests/test_clip_host.py.  Reads queries from stdin, one per line, and answers each with one line:
//   plan  n ncols cus forced -> V W D chunks pc pieces grid per_block chain workspace_bytes cap_bytes
//   cover n ncols cus forced -> empty_blocks uncovered_or_twice widest_block_pieces
// `cover` walks the window as rownorm_kernel does (block b: pieces b, b + grid, ..., piece p: quads
// [p * pc * 64, min((p + 1) * pc * 64, nquads))) and counts the columns covered other than once.
#include <cstdio>
#include <cstring>
#include <vector>

#include "fa_geometry.hpp"

int main() {
  char what[16];
  long long n, ncols, cus, forced;
  while (std::scanf("%15s %lld %lld %lld %lld", what, &n, &ncols, &cus, &forced) == 5) {
    const fa::RownormPlan p = fa::plan_rownorm_window((int)n, ncols, (int)cus, (int)forced);
    if (!std::strcmp(what, "plan")) {
      std::printf("%d %d %d %lld %lld %lld %lld %lld %lld %lld %lld\n", p.V, p.W, p.D, (long long)p.chunks,
                  (long long)p.pc, (long long)p.pieces, (long long)p.grid, (long long)p.per_block, (long long)p.chain,
                  (long long)p.workspace_bytes, (long long)fa::rownorm_workspace_bytes((int)n, ncols));
      continue;
    }
    const int64_t nquads = (ncols + 3) / 4;
    std::vector<unsigned char> seen((size_t)ncols, 0);
    long long empty = 0, widest = 0;
    for (int64_t b = 0; b < p.grid; ++b) {
      long long mine = 0;
      for (int64_t q = b; q < p.pieces; q += p.grid) {
        const int64_t qb = q * p.pc * 64;
        const int64_t qe = qb + p.pc * 64 < nquads ? qb + p.pc * 64 : nquads;
        const int64_t cend = qe * 4 < ncols ? qe * 4 : ncols;
        if (cend <= qb * 4) continue;
        ++mine;
        for (int64_t c = qb * 4; c < cend; ++c) ++seen[(size_t)c];
      }
      if (mine == 0) ++empty;
      if (mine > widest) widest = mine;
    }
    long long bad = 0;
    for (unsigned char s : seen) bad += s != 1;
    std::printf("%lld %lld %lld\n", empty, bad, widest);
  }
  return 0;
}
