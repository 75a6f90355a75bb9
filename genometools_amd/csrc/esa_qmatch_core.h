// esa_qmatch_core.h -- what one lane of esa_qmatch.hip does (semantics and
// algorithm: include/gtamd_qmatch.h), apart from the kernels so that a test can
// compile it for the CPU (tests/qmatch_core_shim.cpp) and run the very code the
// lanes run against the brute force without a device.  The comparisons and the
// binary search with carried shared prefixes are those of esa_mstat_search.h.
#pragma once
#include "esa_mstat_search.h"

struct QmRecord { u64 dbpos, qpos, len; };

// The table indices [*lo, *lo + *width) of the suffixes that start with the L >= 1
// symbols from query position c.i; width 0 when one of the symbols is a special
// or lies at or beyond m.  Two binary searches: the place of the L symbols among
// the suffixes, then the first suffix behind it that does not start with them.
template <typename S> MST_HD void qm_interval(Lane &c, const S *suf, u64 N, u32 L, u32 *lo, u32 *width) {
  *lo = 0;
  *width = 0;
  if (c.m - c.i < L) return;
  const Place pl = place_of(c, suf, N, L);
  if (pl.R < L) return;               // (a special among the L symbols ends every comparison in front of it)
  // suffixes [pl.lb, a) start with the L symbols, suffix b shares lb < L of them;
  // entry N - 1, the subject's end, shares none
  u64 a = pl.lb + 1, b = N - 1;
  u32 lb = 0;
  while (a < b) {
    const u64 mid = (a + b) >> 1;
    const u32 k = c.shared(suffix_at(suf, mid, c.n), lb, L);
    if (k >= L) a = mid + 1; else { b = mid; lb = k; }
  }
  *lo = (u32) pl.lb;
  *width = (u32) (a - pl.lb);
}

// occurrence p of the L symbols from query position c.i is left-maximal
// (gt_mmsearch_isleftmaximal): a special never equals anything
MST_HD bool qm_left_maximal(const Lane &c, u64 p) {
  if (c.i == 0 || p == 0) return true;
  const u32 x = c.enc[p - 1];
  return x >= 254 || x != c.q[c.i - 1];
}

// Candidate k < width of query position c.i: the suffix at table index lo + k.
// False when it is not left-maximal (or the entry lies beyond n); else *p = its
// position.
template <typename S> MST_HD bool qm_kept(const Lane &c, const S *suf, u32 lo, u32 k, u64 *p) {
  *p = suf[(u64) lo + k];
  return *p < c.n && qm_left_maximal(c, *p);
}

// the record of a kept candidate: its L letters extended to the right
MST_HD void qm_extend(Lane &c, u64 p, u32 L, QmRecord *rec) {
  rec->dbpos = p;
  rec->qpos = c.i;
  rec->len = c.shared(p, L, (u32) (c.m - c.i));       // (m - i <= 2^32 - 1)
}
