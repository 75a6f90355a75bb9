// ivwalk_shim.cpp -- genometools_amd/csrc/esa_ivwalk.h compiled for the CPU, for
// tests/test_ivwalk.py: one search over a table in memory with its rounds, and
// the cases of ivwalk_cases.h in one call.
#include "ivwalk_cases.h"

extern "C" {

// the right bound of the child of the symbol at cur in [cur, end) at depth d; *rounds: what the search took
uint32_t iv_shim_right_bound(const uint8_t *enc, uint64_t n, const void *suf, uint32_t suf_bytes, uint32_t cur,
                             uint32_t end, uint32_t d, uint32_t *rounds) {
  ivcases::rounds_of_call = 0;
  uint32_t e;
  if (suf_bytes == 4) {
    const IvText<u32> text = { enc, n, (const u32 *) suf };
    e = iv_right_bound(text, cur, end, d, iv_symbol(text, cur, d));
  } else {
    const IvText<u64> text = { enc, n, (const u64 *) suf };
    e = iv_right_bound(text, cur, end, d, iv_symbol(text, cur, d));
  }
  *rounds = ivcases::rounds_of_call;
  return e;
}

// figures[10]: the fields of ivcases::Tally in their order
void iv_shim_cases(unsigned long long *figures) {
  const ivcases::Tally t = ivcases::run();
  const unsigned long long f[10] = { t.cases, t.failures, t.small, t.large, t.tables, t.no_index, t.no_position,
                                     t.behind_the_end, t.letters, t.max_rounds };
  for (int i = 0; i < 10; i++) figures[i] = f[i];
}

}
