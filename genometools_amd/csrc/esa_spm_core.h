// esa_spm_core.h -- what one lane of esa_spm.hip does (semantics and algorithm:
// include/gtamd_spm.h), apart from the kernels so that a test can compile it for
// the CPU (tests/spm_core_shim.cpp) and run the very code the lanes run against
// the brute force without a device.
#pragma once
#include "esa_qmatch_core.h"

struct SpRecord { u64 suffix_seq, prefix_seq, len; };

// the index the lanes read: n symbols, N = n + 1 table entries, m .llv pairs
template <typename S> struct SpIndex {
  const u8 *enc; u64 n; const S *suf;
  const u8 *lcp; const u64 *llv; u64 m;
};

// the first of the count ascending values that is not below x
MST_HD u64 sp_lower_bound(const u32 *a, u64 count, u64 x) {
  u64 lo = 0, hi = count;
  while (lo < hi) {
    const u64 mid = (lo + hi) >> 1;
    if (a[mid] < x) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// the LCP value of table index i < N: byte 255 is looked up in .llv
template <typename S> MST_HD u32 sp_lcp_value(const SpIndex<S> &x, u64 i) {
  const u32 b = x.lcp[i];
  if (b != 255) return b;
  // (llv_lower_bound of esa_devutil.h, written out: this header also compiles with g++ alone)
  u64 lo = 0, hi = x.m;
  while (lo < hi) {
    const u64 mid = (lo + hi) >> 1;
    if (x.llv[2 * mid] < i) lo = mid + 1; else hi = mid;
  }
  return lo < x.m && x.llv[2 * lo] == i ? (u32) x.llv[2 * lo + 1] : 255u;
}

// Table index i < N is a TERMINAL suffix of minimum length L: its h >= L letters
// run up to a separator or the end, and another suffix starts with them.  h is
// the larger LCP value of the entry's two sides: a value never counts a special,
// so it equals the letters in front of the separator exactly when a neighbour
// shares all of them.
template <typename S> MST_HD bool sp_terminal(const SpIndex<S> &x, u64 i, u32 L, u32 *h) {
  const u64 p = x.suf[i];
  if (p >= x.n) return false;
  // (a byte below 255 is the value itself: most entries end here without a look-up)
  if (L <= 255 && x.lcp[i] < L && (i >= x.n || x.lcp[i + 1] < L)) return false;
  const u32 a = sp_lcp_value(x, i), b = i < x.n ? sp_lcp_value(x, i + 1) : 0;
  *h = mst_max(a, b);
  if (*h < L || *h > x.n - p) return false;
  return p + *h == x.n || x.enc[p + *h] == 255;
}

// table index i < N is a READ START: its suffix begins a sequence with a letter
template <typename S> MST_HD bool sp_read_start(const SpIndex<S> &x, u64 i) {
  const u64 p = x.suf[i];
  return p < x.n && x.enc[p] < 254 && (p == 0 || x.enc[p - 1] == 255);
}

constexpr u32 SP_WALK = 64;            // table entries a lane walks over to either side before it searches

// does the LCP value of table index i < N reach h?  (A byte below 255 is the value.)
template <typename S> MST_HD bool sp_lcp_reaches(const SpIndex<S> &x, u64 i, u32 h) {
  const u32 b = x.lcp[i];
  return b != 255 ? b >= h : sp_lcp_value(x, i) >= h;
}

// The table indices [*lo, *lo + *width) of the suffixes that start with the h
// letters of the terminal suffix at table index i: those around it whose LCP
// values reach h.  Most intervals are a few entries wide: a walk over .lcp to
// both sides, one byte a step, finds their ends without a look at the text.
// An interval that reaches further than SP_WALK entries to either side is
// searched for in the text instead, by the two binary searches of
// esa_qmatch_core.h with the sequence as its own query; *compared += their
// symbol comparisons.
template <typename S> MST_HD void sp_interval(const SpIndex<S> &x, u64 i, u32 h, u32 *lo, u32 *width, u64 *compared) {
  const u64 N = x.n + 1;
  u64 a = i, b = i + 1;
  u32 steps = 0;
  while (steps < SP_WALK && a > 0 && sp_lcp_reaches(x, a, h)) { a--; steps++; }
  if (steps < SP_WALK) {
    steps = 0;
    while (steps < SP_WALK && b < N && sp_lcp_reaches(x, b, h)) { b++; steps++; }
  }
  if (steps < SP_WALK) {
    *lo = (u32) a;
    *width = (u32) (b - a);
    return;
  }
  const u64 p = x.suf[i];
  Lane c = { x.enc, x.n, p < x.n ? p : x.n, x.enc, x.n, 0 };
  qm_interval(c, x.suf, N, h, lo, width);
  *compared += c.compared;
}

// the read starts (ascending table indices, `count` of them) inside [lo, lo +
// width): their number, *first = the place of the first in the list
MST_HD u32 sp_starts_inside(const u32 *starts, u64 count, u32 lo, u32 width, u32 *first) {
  const u64 a = sp_lower_bound(starts, count, lo), b = sp_lower_bound(starts, count, (u64) lo + width);
  *first = (u32) a;
  return (u32) (b - a);
}

// the number of the sequence that holds position p, which is no separator:
// the separators (ascending positions, `count` of them) in front of it
MST_HD u64 sp_sequence_of(const u32 *seps, u64 count, u64 p) { return sp_lower_bound(seps, count, p); }

// candidate r of a terminal suffix at table index i whose first read start is
// starts[first]
template <typename S>
MST_HD void sp_record(const SpIndex<S> &x, const u32 *starts, const u32 *seps, u64 nseps, u32 i, u32 h, u32 first,
                      u64 r, SpRecord *rec) {
  u64 p = x.suf[i], q = x.suf[starts[(u64) first + r]];
  if (p > x.n) p = x.n;              // (a table that is none cannot lead outside the lists)
  if (q > x.n) q = x.n;
  rec->suffix_seq = sp_sequence_of(seps, nseps, p);
  rec->prefix_seq = sp_sequence_of(seps, nseps, q);
  rec->len = h;
}
