// Test shim (CPU): what one lane of the irreducible suffix-prefix match kernels
// does (genometools_amd/csrc/esa_spmred_core.h), run over every read start, every
// pair and every kept record as the lanes of k_sr_starts, k_sr_decide and
// k_sr_emit run it: the lists of steps 1 to 4 are made as tests/spm_core_shim.cpp
// makes them, the verdicts go through a bitmap of 64-bit words, and the kept
// records are found again from that bitmap by sr_select.
#include <algorithm>
#include <numeric>
#include <vector>
#include "../genometools_amd/csrc/esa_spmred_core.h"

enum { F_PAIRS = 0, F_KEPT, F_SAME, F_OTHER, F_CONTAINED, F_CANDIDATES, F_MAXCAND, F_LETTERS, F_WORDS };

// verdict[g] (when not NULL) = 1 transitive, 0 not, for every pair g in order; the
// kept records in order go to out (rows of four 64-bit numbers) when it is not
// NULL.  Returns their number.
template <typename S>
static uint64_t run(const SpIndex<S> &x, uint32_t L, uint32_t flags, uint8_t *verdict, int64_t *out, uint64_t *fig) {
  std::vector<u32> idx, len, starts, seps, first, cnt;
  const u64 N = x.n + 1;
  for (int k = 0; k < F_WORDS; k++) fig[k] = 0;
  for (u64 i = 0; i < N; i++) {
    u32 h = 0;
    if (sp_terminal(x, i, L, &h)) { idx.push_back((u32) i); len.push_back(h); }
    if (sp_read_start(x, i)) starts.push_back((u32) i);
    if (i < x.n && x.enc[i] == 255) seps.push_back((u32) i);
  }
  const u64 M = idx.size(), R = starts.size();
  std::vector<u64> off(M + 1, 0);
  first.resize(M); cnt.resize(M);
  for (u64 k = 0; k < M; k++) {
    u32 lo, width;
    u64 compared = 0;
    sp_interval(x, (u64) idx[k], len[k], &lo, &width, &compared);
    cnt[k] = sp_starts_inside(starts.data(), R, lo, width, &first[k]);
    off[k + 1] = off[k] + cnt[k];
  }
  // step 5
  std::vector<u32> spos(R), slen(R), tpos(M), tperm(M);
  for (u64 j = 0; j < R; j++) {
    sr_start(x, starts.data(), seps.data(), seps.size(), j, &spos[j], &slen[j]);
    fig[F_CONTAINED] += sr_contained(x, starts.data(), j, L);
  }
  std::iota(tperm.begin(), tperm.end(), 0u);
  std::stable_sort(tperm.begin(), tperm.end(), [&](u32 a, u32 b) { return x.suf[idx[a]] < x.suf[idx[b]]; });
  for (u64 u = 0; u < M; u++) tpos[u] = (u32) x.suf[idx[tperm[u]]];
  const SrLists a = { idx.data(), len.data(), first.data(), cnt.data(), M, starts.data(), spos.data(), slen.data(), R,
                      seps.data(), seps.size(), tpos.data(), tperm.data() };
  // step 6
  const u64 Z = off[M], W = (Z + 63) / 64, K = seps.size() + 1;
  std::vector<u64> bitmap(W, 0), woff(W + 1, 0);
  fig[F_PAIRS] = Z;
  for (u64 k = 0, g = 0; k < M; k++)
    for (u64 j = 0; j < cnt[k]; j++, g++) {
      bool kept = true;
      if (flags & SR_ELIMTRANS) {
        SrWalk walk = { 0, 0 };
        const bool t = sr_transitive(x, a, L, k, j, &walk);
        if (verdict != nullptr) verdict[g] = t;
        fig[F_CANDIDATES] += walk.candidates;
        fig[F_LETTERS] += walk.letters;
        if (walk.candidates > fig[F_MAXCAND]) fig[F_MAXCAND] = walk.candidates;
        if (t) {
          SpRecord rec;
          bool d;
          sp_record(x, a.starts, a.seps, a.nseps, a.idx[k], a.len[k], a.first[k], j, &rec);
          const bool same = (flags & SR_MIRRORED) ? sr_read_of(rec.suffix_seq, K, &d) == sr_read_of(rec.prefix_seq, K, &d)
                                                  : rec.suffix_seq == rec.prefix_seq;
          fig[same ? F_SAME : F_OTHER]++;
          kept = false;
        }
      } else if (verdict != nullptr) verdict[g] = 0;
      if (kept && (flags & SR_MIRRORED)) kept = sr_pair_kept(x, a, k, j);
      if (kept) bitmap[g >> 6] |= 1ull << (g & 63);
    }
  // step 7
  for (u64 v = 0; v < W; v++) woff[v + 1] = woff[v] + (u64) __builtin_popcountll(bitmap[v]);
  fig[F_KEPT] = woff[W];
  // step 8
  for (u64 e = 0; e < woff[W] && out != nullptr; e++) {
    const u64 v = (u64) (std::upper_bound(woff.begin(), woff.end(), e) - woff.begin()) - 1;
    const u64 g = v * 64 + sr_select(bitmap[v], (u32) (e - woff[v]));
    const u64 k = (u64) (std::upper_bound(off.begin(), off.end(), g) - off.begin()) - 1;
    SrRecord rec;
    sr_record(x, a, flags, k, g - off[k], &rec);
    out[4 * e] = (int64_t) rec.suffix_read;
    out[4 * e + 1] = (int64_t) rec.prefix_read;
    out[4 * e + 2] = (int64_t) rec.len;
    out[4 * e + 3] = (int64_t) rec.flags;
  }
  return woff[W];
}

extern "C" uint64_t sr_shim_run(const uint8_t *enc, uint64_t n, const void *suf, int suf_bytes, const uint8_t *lcp,
                                const uint64_t *llv, uint64_t llv_pairs, uint32_t L, uint32_t flags, uint8_t *verdict,
                                int64_t *out, uint64_t *fig) {
  if (suf_bytes == 4)
    return run(SpIndex<uint32_t>{ enc, n, (const uint32_t *) suf, lcp, llv, llv_pairs }, L, flags, verdict, out, fig);
  return run(SpIndex<uint64_t>{ enc, n, (const uint64_t *) suf, lcp, llv, llv_pairs }, L, flags, verdict, out, fig);
}

// sr_select alone: the place of the r-th set bit of b
extern "C" uint32_t sr_shim_select(uint64_t b, uint32_t r) { return sr_select(b, r); }
