// tagmatch_core_main.cpp -- the cases of tagmatch_core_cases.h as a program of its
// own, so that they run under -fsanitize=address,undefined on the CPU
// (tests/test_tagmatch_core.py builds and starts it): a shift by 64 at m = 64
// and a read behind the sequence end the run there.
#include "tagmatch_core_cases.h"

int main() {
  const tmcases::Tally t = tmcases::run();
  printf("%llu walks, %llu columns, %llu matches, %llu failures\n", t.walks, t.columns, t.matches, t.failures);
  return t.failures == 0 && t.walks > 0 ? 0 : 1;
}
