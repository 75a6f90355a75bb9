// tagmatch_core_shim.cpp -- genometools_amd/csrc/esa_tagmatch_core.h compiled for
// the CPU, for tests/test_tagmatch_core.py: the walk of one suffix and the
// columns of one text as the lanes compute them, and the cases of
// tagmatch_core_cases.h in one call.
#include "tagmatch_core_cases.h"

extern "C" {

// the match of start position p: its length, *dist its distance; 0 for none
uint32_t tm_shim_walk(const uint8_t *tag, uint32_t m, uint32_t K, int wild, const uint8_t *enc, uint64_t n, uint64_t p,
                      uint32_t *dist) {
  u64 eq[TM_LETTERS];
  tm_eq_table(tag, m, eq);
  return tm_walk(tm_first_column(K), eq, enc, n, p, 0, m, K, wild != 0, dist);
}

// (row, val) of the column after each of the first symbols of text, until it is
// dead or has reached row m; the number of columns
uint32_t tm_shim_columns(const uint8_t *tag, uint32_t m, uint32_t K, const uint8_t *text, uint32_t len, uint32_t *rows,
                         uint32_t *vals) {
  u64 eq[TM_LETTERS];
  tm_eq_table(tag, m, eq);
  TmColumn c = tm_first_column(K);
  uint32_t d = 0;
  while (d < len && !tm_dead(c) && !tm_success(c, m)) {
    tm_step(c, text[d] < TM_LETTERS ? eq[text[d]] : 0, K);
    rows[d] = c.row;
    vals[d] = c.val;
    d++;
  }
  return d;
}

// figures[4]: walks, columns, matches, failures
void tm_shim_cases(unsigned long long *figures) {
  const tmcases::Tally t = tmcases::run();
  figures[0] = t.walks; figures[1] = t.columns; figures[2] = t.matches; figures[3] = t.failures;
}

}
