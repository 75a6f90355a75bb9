// Test shim (CPU): the segment pass and the two walks of the maximal-pairs
// kernels (genometools_amd/csrc/esa_maxpairs_walk.h), run over every segment
// and every entry as the lanes of esa_maxpairs.hip run them.
#include <vector>
#include "../genometools_amd/csrc/esa_maxpairs_walk.h"

// figures[0..4): pairs, largest count of one entry, largest length, steps of the
// count pass.  out == NULL: count only.  Returns the number of pairs.
template <typename S>
static uint64_t run(const uint32_t *idx, const uint32_t *val, const uint8_t *cls, uint32_t M,
                    const uint32_t *seg_first, const uint32_t *seg_of, uint32_t nseg, const S *suf,
                    MpRecord *out, uint64_t *figures) {
  std::vector<uint32_t> tmin(M), seg_min(nseg), cnt(M);
  std::vector<uint16_t> seg_info(nseg);
  for (uint32_t s = 0; s < nseg; s++)
    mp_segment_fill(val, cls, seg_first, s, tmin.data(), seg_min.data(), seg_info.data());
  const MpSegments g = { val, tmin.data(), seg_of, seg_first, seg_min.data(), seg_info.data(), nseg };
  uint64_t z = 0;
  figures[0] = figures[1] = figures[2] = figures[3] = 0;
  for (uint32_t k = 0; k < M; k++) {
    uint32_t longest, steps;
    cnt[k] = mp_walk_count(g, k, cls[k], &longest, &steps);
    z += cnt[k];
    if (cnt[k] > figures[1]) figures[1] = cnt[k];
    if (longest > figures[2]) figures[2] = longest;
    figures[3] += steps;
  }
  figures[0] = z;
  if (out != nullptr) {
    uint64_t at = 0;
    for (uint32_t k = 0; k < M; k++) {
      mp_walk_emit<S>(g, k, cls[k], idx[k], suf, out + at);
      at += cnt[k];
    }
  }
  return z;
}

extern "C" uint64_t mp_shim_run(const uint32_t *idx, const uint32_t *val, const uint8_t *cls, uint32_t M,
                                const uint32_t *seg_first, const uint32_t *seg_of, uint32_t nseg,
                                const void *suf, int suf_bytes, MpRecord *out, uint64_t *figures) {
  if (suf_bytes == 4)
    return run<uint32_t>(idx, val, cls, M, seg_first, seg_of, nseg, (const uint32_t *) suf, out, figures);
  return run<uint64_t>(idx, val, cls, M, seg_first, seg_of, nseg, (const uint64_t *) suf, out, figures);
}
