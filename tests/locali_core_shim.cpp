// locali_core_shim.cpp -- genometools_amd/csrc/esa_locali_core.h compiled for the
// CPU, for tests/test_locali_core.py: the walk of one suffix as the lanes
// compute it, and the cases of locali_core_cases.h in one call.
#include "locali_core_cases.h"

extern "C" {

// the match of start position p: out[4] = dblen, score, qstart, qlen; 0 for none
uint32_t lc_shim_walk(const uint8_t *q, uint32_t m, const uint8_t *enc, uint64_t n, uint64_t p, int match, int mismatch,
                      int gapextend, uint32_t T, uint32_t *out) {
  std::vector<u32> a(m), b(m);
  const LcMatch hit = lc_walk(nullptr, LcColumn{ 0, 0, 0, 0, 0 }, 0, enc, n, p, q, m, LcScores{ match, mismatch, -gapextend },
                              T, a.data(), b.data());
  out[0] = hit.dblen; out[1] = hit.score; out[2] = hit.qstart; out[3] = hit.e - hit.qstart;
  return hit.dblen;
}

uint32_t lc_shim_max_depth(uint32_t m, int match, int gapextend) { return lc_max_depth(m, LcScores{ match, -1, -gapextend }); }

// figures[22]: the members of lccases::Tally in their order
void lc_shim_cases(unsigned long long *figures) {
  const lccases::Tally t = lccases::run();
  memcpy(figures, &t, sizeof t);
}

}
