// Test shim (CPU): what one lane of the contained-read kernels does
// (genometools_amd/csrc/esa_contained_core.h), run over every read start, every
// read and every symbol of the compacted set as the lanes of k_ct_starts,
// k_ct_images, k_ct_verdicts and k_ct_compact run it.  The lists of read starts
// and separators are made as tests/spm_core_shim.cpp makes them.
#include <algorithm>
#include <vector>
#include "../genometools_amd/csrc/esa_contained_core.h"

// verdict[r] for the R reads of the mirrored set of 2R sequences; count[v] = the
// reads of verdict v.  Returns R, or -1 for a set that is no mirrored one.
template <typename S> static int64_t run(const SpIndex<S> &x, uint8_t *verdict, uint64_t *count) {
  std::vector<u32> starts, seps;
  const u64 N = x.n + 1;
  for (u64 i = 0; i < N; i++) {
    if (sp_read_start(x, i)) starts.push_back((u32) i);
    if (i < x.n && x.enc[i] == 255) seps.push_back((u32) i);
  }
  const u64 K = x.n ? seps.size() + 1 : 0;
  if (K % 2 || starts.size() != K) return -1;
  std::vector<u32> spos(K), slen(K);
  for (u64 j = 0; j < K; j++) sr_start(x, starts.data(), seps.data(), seps.size(), j, &spos[j], &slen[j]);
  const CtLists a = { starts.data(), spos.data(), slen.data(), K, seps.data(), seps.size() };
  std::vector<u8> image(K, 0);
  for (u64 j = 0; j < K; j++) {
    u64 s;
    const u8 f = ct_image(x, a, j, &s);
    image[s] = f;
  }
  for (u32 v = 0; v < CT_VERDICTS; v++) count[v] = 0;
  for (u64 r = 0; r < K / 2; r++) {
    verdict[r] = ct_verdict(image[r], image[K - 1 - r]);
    count[verdict[r]]++;
  }
  return (int64_t) (K / 2);
}

extern "C" int64_t ct_shim_run(const uint8_t *enc, uint64_t n, const void *suf, int suf_bytes, const uint8_t *lcp,
                               const uint64_t *llv, uint64_t llv_pairs, uint8_t *verdict, uint64_t *count) {
  if (suf_bytes == 4) return run(SpIndex<uint32_t>{ enc, n, (const uint32_t *) suf, lcp, llv, llv_pairs }, verdict, count);
  return run(SpIndex<uint64_t>{ enc, n, (const uint64_t *) suf, lcp, llv, llv_pairs }, verdict, count);
}

// The n symbols at enc without the reads whose verdict is a bit of mask, to out
// (n bytes of room); seps: the separators of the set, or those of its mirrored
// set.  Returns the symbols written.
extern "C" uint64_t ct_shim_compact(const uint8_t *enc, uint64_t n, const uint32_t *seps, uint64_t nseps, uint64_t R,
                                    const uint8_t *verdict, uint32_t mask, uint8_t *out) {
  std::vector<u64> off(R + 1, 0);
  for (u64 r = 0; r < R; r++) off[r + 1] = off[r] + ct_kept_symbols(verdict, mask, seps, nseps, n, r);
  const u64 total = off[R] ? off[R] - 1 : 0;             // no separator behind the last read
  for (u64 e = 0; e < total; e++) {
    const u64 r = (u64) (std::upper_bound(off.begin(), off.end(), e) - off.begin()) - 1;
    out[e] = ct_symbol(enc, seps, nseps, n, off.data(), r, e);
  }
  return total;
}

// the mirrored set of the n symbols at enc, 2n + 1 symbols to out
extern "C" void ct_shim_mirror(const uint8_t *enc, uint64_t n, uint8_t *out) {
  for (u64 e = 0; e < 2 * n + 1; e++) out[e] = ct_mirror_symbol(enc, n, e);
}
