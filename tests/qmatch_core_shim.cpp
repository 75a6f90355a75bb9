// Test shim (CPU): what one lane of the query match kernels does
// (genometools_amd/csrc/esa_qmatch_core.h), run over every query position and
// every candidate as the lanes of k_qm_intervals and k_qm_emit run it.
#include "../genometools_amd/csrc/esa_qmatch_core.h"

enum { F_CANDIDATES = 0, F_SEEDS, F_MAXWIDTH, F_SEARCH, F_EXTENSION, F_WORDS };

// the intervals of all positions into lo and width, then their candidates in
// order; the records of the kept ones go to out (rows dbpos, qpos, len of 32
// bits) when it is not NULL.  Returns their number.
template <typename S>
static uint64_t run(const uint8_t *enc, uint64_t n, const S *suf, const uint8_t *q, uint64_t m, uint32_t L,
                    uint32_t *lo, uint32_t *width, int32_t *out, uint64_t *fig) {
  uint64_t kept = 0;
  for (int k = 0; k < F_WORDS; k++) fig[k] = 0;
  for (uint64_t i = 0; i < m; i++) {
    Lane c = { q, m, i, enc, n, 0 };
    qm_interval(c, suf, n + 1, L, &lo[i], &width[i]);
    fig[F_SEARCH] += c.compared;
    fig[F_CANDIDATES] += width[i];
    fig[F_SEEDS] += width[i] != 0;
    if (width[i] > fig[F_MAXWIDTH]) fig[F_MAXWIDTH] = width[i];
  }
  for (uint64_t i = 0; i < m; i++)
    for (uint32_t k = 0; k < width[i]; k++) {
      Lane c = { q, m, i, enc, n, 0 };
      uint64_t p;
      if (!qm_kept(c, suf, lo[i], k, &p)) continue;
      if (out != nullptr) {
        QmRecord rec;
        qm_extend(c, p, L, &rec);
        fig[F_EXTENSION] += c.compared;
        out[3 * kept] = (int32_t) rec.dbpos;
        out[3 * kept + 1] = (int32_t) rec.qpos;
        out[3 * kept + 2] = (int32_t) rec.len;
      }
      kept++;
    }
  return kept;
}

extern "C" uint64_t qm_shim_run(const uint8_t *enc, uint64_t n, const void *suf, int suf_bytes, const uint8_t *q,
                                uint64_t m, uint32_t L, uint32_t *lo, uint32_t *width, int32_t *out,
                                uint64_t *fig) {
  return suf_bytes == 4 ? run(enc, n, (const uint32_t *) suf, q, m, L, lo, width, out, fig)
                        : run(enc, n, (const uint64_t *) suf, q, m, L, lo, width, out, fig);
}
