// esa_kcorrect_core.h -- what one lane of esa_kcorrect.hip does (definition and
// algorithm: include/gtamd_kcorrect.h), apart from the kernels so that a test can
// compile it for the CPU (tests/kcorrect_core_shim.cpp) and run the very code
// the lanes run against the restatement without a device: what a child of a
// group of k-mers finds out about its group (step 3), the records it gives
// (step 4), and the letter of a record from the records in front of it (step 5).
#pragma once
#include "esa_mstat_search.h"

// n symbols, the N non-special suffixes of .suf with .lcp; first_mirror: n >> 1
// for a mirrored set, n otherwise
template <typename S> struct KcIndex {
  const u8 *enc; u64 n;
  const S *suf; const u8 *lcp;
  u64 N, first_mirror;
};

// ---- steps 1 to 3 ------------------------------------------------------------------
// entry i < N starts a child: another k-mer than the entry before
MST_HD bool kc_is_head(const u8 *lcp, u64 i, u32 k) { return i == 0 || lcp[i] < k; }

// child j starts a group: other k - 1 letters than the child before.  heads: the
// C child heads in table order, heads[C] = N
template <typename S> MST_HD bool kc_group_start(const KcIndex<S> &x, const u32 *heads, u64 j, u32 k) {
  const u32 h = heads[j];
  return h == 0 || x.lcp[h] < k - 1;
}

// the k-th symbol of the suffixes of the child with head h is a letter
template <typename S> MST_HD bool kc_valid(const KcIndex<S> &x, u32 h, u32 k) {
  const u64 p = (u64) x.suf[h] + k - 1;
  return p < x.n && x.enc[p] < 254;
}

// the group whose first child is `first`: its nv valid children in front of the
// first invalid one or the next group, their widths, the trusted one (-1: none)
struct KcGroup {
  u32 nv, width[4];
  int trusted;
  bool examined;            // it has an interval of depth k - 1: two children at least
  bool emits;               // not all four trusted, one trusted, one not
};

template <typename S> MST_HD KcGroup kc_group(const KcIndex<S> &x, const u32 *heads, u64 C, u32 k, u32 c, u64 first) {
  KcGroup g;
  g.nv = 0;
  g.trusted = -1;
  g.examined = first + 1 < C && !kc_group_start(x, heads, first + 1, k);
  bool untrusted = false, all = true;
  for (u32 t = 0; t < 4; t++) {
    const u64 j = first + t;
    g.width[t] = 0;
    if (g.nv != t || j >= C || (t && kc_group_start(x, heads, j, k)) || !kc_valid(x, heads[j], k)) continue;
    g.width[t] = heads[j + 1] - heads[j];
    g.nv = t + 1;
    if (g.width[t] >= c) { if (g.trusted < 0) g.trusted = (int) t; }
    else untrusted = true;
  }
  all = g.nv == 4 && !untrusted;
  g.emits = g.examined && !all && g.trusted >= 0 && untrusted;
  return g;
}

// The records child j gives, one per entry of it; *src: the head of the trusted
// child of its group, *first: the first child of its group.  A valid child is one
// of the first four of its group: three steps to the left find the group's start.
template <typename S>
MST_HD u32 kc_child(const KcIndex<S> &x, const u32 *heads, u64 C, u32 k, u32 c, u64 j, u32 *src, u32 *first) {
  *src = 0;
  *first = (u32) j;
  if (!kc_valid(x, heads[j], k)) return 0;
  u64 f = j;
  for (u32 s = 0; !kc_group_start(x, heads, f, k); s++) {
    if (s == 3) return 0;                                // behind an invalid child (or a table that is none)
    f--;                                                 // (child 0 starts a group)
  }
  const KcGroup g = kc_group(x, heads, C, k, c, f);
  const u32 t = (u32) (j - f);
  if (!g.emits || t >= g.nv || g.width[t] >= c) return 0;
  *src = heads[f + (u32) g.trusted];
  *first = (u32) f;
  return g.width[t];
}

// ---- steps 4 and 5 -----------------------------------------------------------------
// position p of the text, normalised: the position in the first half and whether
// the letter is complemented; both in one word, the flag in bit 0
template <typename S> MST_HD u64 kc_normalised(const KcIndex<S> &x, u64 p) {
  return p >= x.first_mirror ? (x.n - 1 - p) << 1 | 1 : p << 1;
}

// the state of a record during the resolution: its letter (KC_DONE), or the
// earlier record its letter comes from with the parity of the complements between
constexpr u64 KC_DONE = 1ull << 63, KC_PARITY = 1ull << 32;

// The sorted keys are (target << rbits | order) of the R records.  The last
// record in front of record `bound` that wrote position `pos`: its order, or
// R for none.
MST_HD u64 kc_writer(const u64 *keys, u64 R, u32 rbits, u64 pos, u64 bound) {
  const u64 limit = pos << rbits | bound;
  u64 lo = 0, hi = R;                                    // the first key that is not below limit
  while (lo < hi) {
    const u64 mid = (lo + hi) >> 1;
    if (keys[mid] < limit) lo = mid + 1; else hi = mid;
  }
  if (lo == 0 || keys[lo - 1] >> rbits != pos) return R;
  return keys[lo - 1] & ((1ull << rbits) - 1);
}

// the first state of a record: target and source normalised (kc_normalised),
// group_first the first record of its group; enc: the original symbols
MST_HD u64 kc_first_state(const u8 *enc, const u64 *keys, u64 R, u32 rbits, u64 target, u64 source, u64 group_first) {
  const u64 parity = (target ^ source) & 1;
  const u64 w = kc_writer(keys, R, rbits, source >> 1, group_first);
  if (w == R) return KC_DONE | (u64) (enc[source >> 1] ^ (parity ? 3 : 0));
  return w | (parity ? KC_PARITY : 0);
}

// one round of the pointer doubling for a record that is not done: state is
// its own, of the round before, as is everything at `before`
MST_HD u64 kc_next_state(const u64 *before, u64 state) {
  const u64 other = before[state & 0xFFFFFFFFull];
  if (other & KC_DONE) return KC_DONE | ((other & 3) ^ (state & KC_PARITY ? 3 : 0));
  return (other & 0xFFFFFFFFull) | ((state ^ other) & KC_PARITY);
}

// sorted record s of R is the last of its target: its letter stands in the end
MST_HD bool kc_is_final(const u64 *keys, u64 R, u32 rbits, u64 s) {
  return s + 1 == R || keys[s + 1] >> rbits != keys[s] >> rbits;
}
