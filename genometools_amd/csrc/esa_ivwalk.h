// esa_ivwalk.h -- what the lanes of a depth-first walk over the intervals of
// .suf share (esa_tagmatch.hip, esa_locali.hip): the two special
// codes, the symbol of a table entry at a depth, and the search for the right
// bound of a child.  Apart from the kernels so that a test can compile it for
// the CPU (tests/test_ivwalk.py): there the 64 lanes are a loop and the ballot
// is made of their answers; everything else is the same text.
#pragma once
#include <stdint.h>

typedef uint64_t u64;
typedef uint32_t u32;
typedef uint8_t u8;

constexpr u32 IV_BATCH = 64;             // probes of one round: the lanes of a wave
constexpr u32 IV_WILDCARD = 254, IV_SEPARATOR = 255;      // the specials, behind all letters

// iv_ballot: bit l is what lane l answers; on the device the lane as the kernels
// have it already (their workgroups are rows of whole waves)
#if defined(__HIPCC__)
#define IV_HD __device__ __forceinline__
template <typename A> IV_HD u64 iv_ballot(A answer) { return __ballot(answer(threadIdx.x & 63)); }
#else
#define IV_HD inline
template <typename A> IV_HD u64 iv_ballot(A answer) {
  u64 mask = 0;
  for (u32 l = 0; l < IV_BATCH; l++) mask |= (u64) (answer(l) ? 1 : 0) << l;
  return mask;
}
#endif
#if !defined(IV_ROUND)
#define IV_ROUND() ((void) 0)            // a test counts the rounds of a search here
#endif

template <typename S> struct IvText { const u8 *enc; u64 n; const S *suf; };

// the symbol `d` behind the start of the suffix at table index idx < N; a separator
// where there is none: behind the end, or for an entry that is no position
template <typename S> IV_HD u32 iv_symbol(const IvText<S> &t, u32 idx, u32 d) {
  const u64 p = t.suf[idx];
  if (p >= t.n) return IV_SEPARATOR;
  const u64 x = p + d;
  return x < t.n ? t.enc[x] : IV_SEPARATOR;
}

// The right bound of the child that starts at table index cur of a level that
// ends at `end`: the first index behind cur whose entry differs(q) from the one
// at cur.  The symbols at one depth ascend inside an interval, the specials
// behind all letters, so this is a search: 64 probes a round, spread over the
// range [lo, hi) that is left; the range behind the last probe that still
// holds the symbol and in front of the first that does not is what the next
// round gets.  A round leaves fewer than span / 64 + 1 < span entries, whatever
// the table holds; the result lies in (cur, end].  The whole wave calls this
// with the same arguments.
template <typename D> IV_HD u32 iv_right_bound_by(D differs, u32 cur, u32 end) {
  u32 lo = cur + 1, hi = end;
  while (lo < hi) {
    IV_ROUND();
    const u32 span = hi - lo;
    const u32 step = span <= IV_BATCH ? 1 : (span + IV_BATCH - 1) / IV_BATCH;
    const u64 mask = iv_ballot([&](u32 lane) {
      const u64 q = (u64) lo + (u64) lane * step;
      return q >= hi || differs((u32) q);
    });
    const u32 f = mask ? (u32) __builtin_ctzll(mask) : IV_BATCH;
    if (f == 0) return lo;
    const u64 next = (u64) lo + (u64) f * step;          // the first probe that differs, if there is one
    if (f < IV_BATCH && next < hi) hi = (u32) next;
    lo = lo + (f - 1) * step + 1;
  }
  return lo;
}

// ... of the child of letter s at depth d of a table in memory
template <typename S> IV_HD u32 iv_right_bound(const IvText<S> &t, u32 cur, u32 end, u32 d, u32 s) {
  return iv_right_bound_by([&](u32 q) { return iv_symbol(t, q, d) != s; }, cur, end);
}
