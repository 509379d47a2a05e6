// quot_rule_probe.cpp — the reciprocal quotient's enable rule on a CPU box (tests/test_quot_rule_host.py).
// One denominator per line on stdin as the 16 hex digits of its float64 bits; one answer line each:
// 1 where fa::recip_quot_exact takes the reciprocal form, 0 where the launch keeps the IEEE divide.
#include "fa_geometry.hpp"

#include <cinttypes>
#include <cstdio>
#include <cstring>

int main() {
  char line[64];
  while (std::fgets(line, sizeof line, stdin)) {
    uint64_t u = 0;
    if (std::sscanf(line, "%" SCNx64, &u) != 1) {
      std::printf("bad query\n");
      return 2;
    }
    double d;
    std::memcpy(&d, &u, sizeof d);
    std::printf("%d\n", fa::recip_quot_exact(d) ? 1 : 0);
  }
  return 0;
}
