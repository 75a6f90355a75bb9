// locali_core_main.cpp -- the cases of locali_core_cases.h as a program of its
// own, so that they run under -fsanitize=address,undefined on the CPU
// (tests/test_locali_core.py builds and starts it): a cell written or read
// outside a column ends the run there.
#include "locali_core_cases.h"

int main() {
  const lccases::Tally t = lccases::run();
  printf("%llu walks, %llu columns, %llu matches, %llu failures\n", t.walks, t.columns, t.matches, t.failures);
  return t.failures == 0 && t.walks > 0 ? 0 : 1;
}
