// geometry_probe.cpp — the reduce geometry's decisions on a CPU box (tests/test_geometry_plan.py).
// One query per line on stdin, one answer line each:
//   f32 mode op n ncols cus forced splitn -> family V W D KG EPIB wide16 grid
//   f16 vmax ncols cus [forced]           -> family V W D KG EPIB wide16 grid   (no forced: 0)
//   win op ncols                          -> window count and width
//   bal chunks slots                      -> grid
#include "fa_geometry.hpp"

#include <cstdio>
#include <cstring>

static void show(const fa::Plan& p) {
  static const char* const names[] = {"rows", "narrow", "rowmajor", "splitn", "balanced", "rows_h16"};
  std::printf("%s %d %d %d %d %d %d %lld\n", names[p.family], p.V, p.W, p.D, p.KG, p.EPIB, (int)p.wide16,
              (long long)p.grid);
}

int main() {
  char line[256], kind[8];
  while (std::fgets(line, sizeof line, stdin)) {
    long long a = 0, b = 0;
    int mode = 0, op = 0, n = 0, cus = 0, forced = 0, splitn = 0;
    if (std::sscanf(line, "%7s", kind) != 1) continue;
    if (!std::strcmp(kind, "f32") &&
        std::sscanf(line, "%*s %d %d %d %lld %d %d %d", &mode, &op, &n, &a, &cus, &forced, &splitn) == 7) {
      show(fa::plan_f32_window(mode, op, n, a, cus, forced, splitn != 0));
    } else if (!std::strcmp(kind, "f16") && std::sscanf(line, "%*s %d %lld %d %d", &mode, &a, &cus, &forced) >= 3) {
      show(fa::plan_f16_window(mode, a, cus, forced));
    } else if (!std::strcmp(kind, "win") && std::sscanf(line, "%*s %d %lld", &op, &a) == 2) {
      const int count = fa::window_count(op, a);
      std::printf("%d %lld\n", count, (long long)fa::window_width(a, count));
    } else if (!std::strcmp(kind, "bal") && std::sscanf(line, "%*s %lld %lld", &a, &b) == 2) {
      std::printf("%lld\n", (long long)fa::balanced_grid(a, b));
    } else {
      std::printf("bad query\n");
      return 2;
    }
  }
  return 0;
}
