// ivwalk_main.cpp -- the cases of ivwalk_cases.h as a program of its own, so that
// they run under -fsanitize=address,undefined on the CPU (tests/test_ivwalk.py
// builds and starts it): a probe that wraps near 2^32, or one read behind a
// table, ends the run there.
#include "ivwalk_cases.h"

int main() {
  const ivcases::Tally t = ivcases::run();
  printf("%llu cases, at most %u rounds, %llu failures\n", t.cases, t.max_rounds, t.failures);
  return t.failures == 0 && t.cases > 0 ? 0 : 1;
}
