// trim_geometry_probe.cpp — plan_trim_window's decisions and trim_kernel_rows' sorting network on a
// CPU box (tests/test_robust_host.py).  One query per line on stdin, one answer line each:
//   "plan n_clients ncols cus forced" -> np pieces grid waves_per_simd elem_grid
//   "net np seed rounds"              -> exchanges bad
// `net` runs the network trim_net_pair describes (the layers in trim_sort's order) over `rounds`
// random arrays of np keys, ties and the padding key included, and over every 0/1 input for
// np <= 16; `bad` counts arrays that did not come out sorted or lost a key.
#include "fa_geometry.hpp"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

static long long run_net(int np, std::vector<int>& key) {
  long long exchanges = 0;
  for (int p = 1; p < np; p *= 2)
    for (int k = p; k >= 1; k /= 2)
      for (int m = 0; m < np / 2; ++m) {
        const fa::TrimPair c = fa::trim_net_pair(np, p, k, m);
        if (!c.on) continue;
        ++exchanges;
        const int lo = std::min(key[c.a], key[c.b]), hi = std::max(key[c.a], key[c.b]);
        key[c.a] = lo;
        key[c.b] = hi;
      }
  return exchanges;
}

int main() {
  char line[256];
  while (std::fgets(line, sizeof line, stdin)) {
    if (std::strncmp(line, "plan ", 5) == 0) {
      long long ncols = 0;
      int n = 0, cus = 0, forced = 0;
      if (std::sscanf(line + 5, "%d %lld %d %d", &n, &ncols, &cus, &forced) != 4) return 2;
      const fa::TrimPlan p = fa::plan_trim_window(n, ncols, cus, forced);
      std::printf("%d %lld %lld %d %lld\n", p.np, (long long)p.pieces, (long long)p.grid,
                  fa::trim_waves_per_simd(p.np ? p.np : 4), (long long)fa::trim_elem_grid(ncols, cus, forced));
    } else if (std::strncmp(line, "net ", 4) == 0) {
      int np = 0, rounds = 0;
      unsigned seed = 0;
      if (std::sscanf(line + 4, "%d %u %d", &np, &seed, &rounds) != 3) return 2;
      std::mt19937 rng(seed);
      long long exchanges = 0, bad = 0;
      std::vector<int> key(np), want(np);
      auto check = [&]() {
        want = key;
        std::sort(want.begin(), want.end());
        exchanges = run_net(np, key);
        bad += key != want;
      };
      for (int r = 0; r < rounds; ++r) {
        const int span = r % 3 == 0 ? 4 : 1 << 30;  // every third round: many ties
        for (int i = 0; i < np; ++i) key[i] = (int)(rng() % (unsigned)(2 * span)) - span;
        for (int i = np - r % (np / 2 + 1); i < np; ++i) key[i] = 0x7fffffff;  // padded slots
        check();
      }
      if (np <= 16)
        for (unsigned bits = 0; bits < (1u << np); ++bits) {  // the 0/1 principle, exhaustively
          for (int i = 0; i < np; ++i) key[i] = (bits >> i) & 1;
          check();
        }
      std::printf("%lld %lld\n", exchanges, bad);
    } else {
      std::printf("bad query\n");
      return 2;
    }
  }
  return 0;
}
