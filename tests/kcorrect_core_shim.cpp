// Test shim (CPU): what one lane of the k-mer correction kernels does
// (genometools_amd/csrc/esa_kcorrect_core.h), run over every table entry, every
// child and every record as the lanes of k_kc_heads, k_kc_groups, k_kc_emit,
// k_kc_first, k_kc_round and k_kc_finals run it; the scans and the sort between
// them are plain loops and std::sort here.
#include <algorithm>
#include <vector>
#include "../genometools_amd/csrc/esa_kcorrect_core.h"

struct Figures { uint64_t groups, untrusted_groups, records, dependent, rounds, changed; int64_t delta[4]; };

// triples: (entry, normalised position, letter) per record, room for `room`
// records; out: the corrected unmirrored symbols.  Returns the records, or -1
// when there is no room for them.
template <typename S>
static int64_t run(KcIndex<S> x, u32 k, u32 c, uint64_t *triples, uint64_t room, uint8_t *out, Figures *fig) {
  *fig = Figures();
  x.N = 0;
  for (u64 p = 0; p < x.n; p++) x.N += x.enc[p] < 254;
  for (u64 p = 0; p < x.first_mirror; p++) out[p] = x.enc[p];
  if (k < 2 || x.N == 0) return 0;
  std::vector<u32> heads;
  for (u64 i = 0; i < x.N; i++)
    if (kc_is_head(x.lcp, i, k)) heads.push_back((u32) i);
  const u64 C = heads.size();
  heads.push_back((u32) x.N);
  std::vector<u32> rcount(C), src(C), first(C);
  std::vector<u64> roff(C + 1, 0);
  for (u64 j = 0; j < C; j++) {
    rcount[j] = kc_child(x, heads.data(), C, k, c, j, &src[j], &first[j]);
    if (kc_group_start(x, heads.data(), j, k)) {
      const KcGroup g = kc_group(x, heads.data(), C, k, c, j);
      fig->groups += g.examined;
      fig->untrusted_groups += g.emits;
    }
    roff[j + 1] = roff[j] + rcount[j];
  }
  const u64 R = fig->records = roff[C];
  if (R > room) return -1;
  if (R == 0) return 0;
  u32 rbits = 1;
  while (rbits < 64 && (R - 1) >> rbits) rbits++;
  std::vector<u64> target(R), source(R), keys(R), gf(R), entry(R);
  for (u64 j = 0; j < C; j++) {
    if (rcount[j] == 0) continue;
    const u64 s = kc_normalised(x, (u64) x.suf[src[j]] + k - 1);
    for (u32 t = 0; t < rcount[j]; t++) {
      const u64 r = roff[j] + t, e = (u64) heads[j] + t;
      entry[r] = e;
      target[r] = kc_normalised(x, (u64) x.suf[e] + k - 1);
      source[r] = s;
      gf[r] = roff[first[j]];
      keys[r] = (target[r] >> 1) << rbits | r;
    }
  }
  std::sort(keys.begin(), keys.end());
  std::vector<u64> state(R), next(R);
  u64 open = 0;
  for (u64 r = 0; r < R; r++) {
    state[r] = kc_first_state(x.enc, keys.data(), R, rbits, target[r], source[r], gf[r]);
    open += !(state[r] & KC_DONE);
  }
  fig->dependent = open;
  while (open) {
    open = 0;
    for (u64 r = 0; r < R; r++) {
      next[r] = state[r] & KC_DONE ? state[r] : kc_next_state(state.data(), state[r]);
      open += !(next[r] & KC_DONE);
    }
    state.swap(next);
    if (++fig->rounds > 64) return -2;
  }
  for (u64 s = 0; s < R; s++) {
    if (!kc_is_final(keys.data(), R, rbits, s)) continue;
    const u64 pos = keys[s] >> rbits;
    const u8 f = (u8) (state[keys[s] & ((1ull << rbits) - 1)] & 3);
    if (x.enc[pos] != f) {
      fig->changed++;
      fig->delta[x.enc[pos]]--;
      fig->delta[f]++;
    }
    out[pos] = f;
  }
  for (u64 r = 0; r < R; r++) {
    triples[3 * r] = entry[r];
    triples[3 * r + 1] = target[r] >> 1;
    triples[3 * r + 2] = state[r] & 3;
  }
  return (int64_t) R;
}

extern "C" int64_t kc_shim_run(const uint8_t *enc, uint64_t n, const void *suf, int suf_bytes, const uint8_t *lcp,
                               int mirrored, uint32_t k, uint32_t c, uint64_t *triples, uint64_t room, uint8_t *out,
                               Figures *fig) {
  const u64 fm = mirrored ? n >> 1 : n;
  if (suf_bytes == 4) return run(KcIndex<uint32_t>{ enc, n, (const uint32_t *) suf, lcp, 0, fm }, k, c, triples, room, out, fig);
  return run(KcIndex<uint64_t>{ enc, n, (const uint64_t *) suf, lcp, 0, fm }, k, c, triples, room, out, fig);
}
