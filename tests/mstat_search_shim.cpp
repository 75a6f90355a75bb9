// Test shim (CPU): the search of one query position of the matching statistics
// kernel (genometools_amd/csrc/esa_mstat_search.h), run over every position of a
// query as the lanes of k_mstat run it.
#include "../genometools_amd/csrc/esa_mstat_search.h"

template <typename S, bool MATSTAT>
static uint64_t run(const uint8_t *enc, uint64_t n, const S *suf, const uint8_t *q, uint64_t m, uint32_t limit,
                    uint32_t *len, uint64_t *pos, uint64_t *compared) {
  uint64_t reruns = 0;
  *compared = 0;
  for (uint64_t i = 0; i < m; i++) {
    Lane c = { q, m, i, enc, n, 0 };
    reruns += mst_position<S, MATSTAT>(c, suf, n + 1, limit, pos != nullptr, &len[i], &pos[i]);
    *compared += c.compared;
  }
  return reruns;
}

// suf_bytes 4 or 8; limit: max_len + 1, or 2^32 - 1 for no cap.  Returns the
// number of positions searched again without the cut.
extern "C" uint64_t mst_shim_run(const uint8_t *enc, uint64_t n, const void *suf, int suf_bytes,
                                 const uint8_t *q, uint64_t m, uint32_t limit, int matstat, uint32_t *len,
                                 uint64_t *pos, uint64_t *compared) {
  if (suf_bytes == 4)
    return matstat ? run<uint32_t, true>(enc, n, (const uint32_t *) suf, q, m, limit, len, pos, compared)
                   : run<uint32_t, false>(enc, n, (const uint32_t *) suf, q, m, limit, len, pos, compared);
  return matstat ? run<uint64_t, true>(enc, n, (const uint64_t *) suf, q, m, limit, len, pos, compared)
                 : run<uint64_t, false>(enc, n, (const uint64_t *) suf, q, m, limit, len, pos, compared);
}
