// esa_contained_core.h -- what one lane of esa_contained.hip does (definition,
// tie rule and algorithm: include/gtamd_contained.h), apart from the kernels so
// that a test can compile it for the CPU (tests/contained_core_shim.cpp) and run
// the very code the lanes run against the brute force without a device: what one
// sequence of the mirrored set finds out about itself, the verdict of a read from
// its two images, and the symbols of the compacted set.
#pragma once
#include "esa_spmred_core.h"

// the verdict of a read (GTAMD_CONTAINED_*): the first that applies
constexpr u8 CT_KEPT = 0, CT_DUPLICATE = 1, CT_AFFIX = 2, CT_INTERNAL = 3, CT_SELF_COMPLEMENTARY = 4;
constexpr u32 CT_VERDICTS = 5;

// what a sequence of the mirrored set finds out: a longer sequence starts with
// it; the lowest read of its class is another one; it stands at a place that is no
// sequence start; its class holds its own mirror image
constexpr u8 CT_IMG_PREFIX = 1, CT_IMG_DUPLICATE = 2, CT_IMG_ELSEWHERE = 4, CT_IMG_SELF = 8;

// the R read starts of the mirrored set in table order, position and length of the
// sequence of each (sr_start), and the separators
struct CtLists {
  const u32 *starts, *spos, *slen; u64 R;
  const u32 *seps; u64 nseps;
};

// Read start j, sequence *seq of K = nseps + 1, m letters at table index i.  If
// neither LCP value beside i reaches m, the letters stand nowhere else: nothing is
// found out, after two byte loads.  Otherwise [lo, lo + width) are the suffixes
// that start with the m letters and starts[first .. first + c) the sequences that
// do.  A separator is larger than every letter, so the sequences of more than m
// letters come first and the whole sequences equal to this one last, in text
// order: the direct copies by ascending read number, then the mirror images by
// descending read number.  The lowest read of the class is therefore that of the
// first or of the last of that run, and a lane looks at no other member of it.
template <typename S> MST_HD u8 ct_image(const SpIndex<S> &x, const CtLists &a, u64 j, u64 *seq) {
  const u64 i = a.starts[j], K = a.nseps + 1;
  const u32 m = a.slen[j];
  const u64 s = sp_sequence_of(a.seps, a.nseps, a.spos[j]);
  *seq = s;
  if (!sp_lcp_reaches(x, i, m) && !(i < x.n && sp_lcp_reaches(x, i + 1, m))) return 0;
  u32 lo, width, first;
  u64 compared = 0;
  sp_interval(x, i, m, &lo, &width, &compared);
  const u32 c = sp_starts_inside(a.starts, a.R, lo, width, &first);
  u64 eq = first, end = (u64) first + c;
  while (eq < end) {                                      // the first of the run of m letters
    const u64 mid = (eq + end) >> 1;
    if (a.slen[mid] > m) eq = mid + 1; else end = mid;
  }
  end = (u64) first + c;
  u8 f = 0;
  if (eq > first) f |= CT_IMG_PREFIX;
  if (width > c) f |= CT_IMG_ELSEWHERE;
  if (eq >= end) return f;                                // (a table that is none: the run holds j)
  const u64 s0 = sp_sequence_of(a.seps, a.nseps, a.spos[eq]), s1 = sp_sequence_of(a.seps, a.nseps, a.spos[end - 1]);
  bool d, d0, d1;
  const u64 r = sr_read_of(s, K, &d), r0 = sr_read_of(s0, K, &d0), r1 = sr_read_of(s1, K, &d1);
  if ((r0 < r1 ? r0 : r1) != r) f |= CT_IMG_DUPLICATE;
  if ((d ? s1 : s0) == K - 1 - s) f |= CT_IMG_SELF;       // (said of the lowest read of a class only)
  return f;
}

// The verdict of a read from what its sequence (f) and its mirror image (g) found
// out.  A proper suffix of a sequence is a proper prefix of that sequence's mirror
// image, found by g.  Once no longer sequence starts or ends with the read, every
// place it stands at beside the whole sequences of its class is strictly inside
// a sequence.
MST_HD u8 ct_verdict(u8 f, u8 g) {
  if (f & CT_IMG_DUPLICATE) return CT_DUPLICATE;
  if ((f | g) & CT_IMG_PREFIX) return CT_AFFIX;
  if ((f | g) & CT_IMG_ELSEWHERE) return CT_INTERNAL;
  if (f & CT_IMG_SELF) return CT_SELF_COMPLEMENTARY;
  return CT_KEPT;
}

// ---- the compaction ------------------------------------------------------------
// read r of a set of n symbols: its letters stand at [*begin, *begin + *len).  seps:
// ascending separators, nseps of them not below r -- those of the set itself (one
// fewer than its reads) or those of its mirrored set
MST_HD void ct_read_span(const u32 *seps, u64 nseps, u64 n, u64 r, u64 *begin, u32 *len) {
  *begin = r ? (u64) seps[r - 1] + 1 : 0;
  *len = (u32) ((r < nseps ? seps[r] : n) - *begin);
}

// the symbols read r gives to the compacted set: its letters and a separator, or
// nothing when bit verdict[r] of mask is set
MST_HD u32 ct_kept_symbols(const u8 *verdict, u32 mask, const u32 *seps, u64 nseps, u64 n, u64 r) {
  u64 begin;
  u32 len;
  if (mask >> verdict[r] & 1) return 0;
  ct_read_span(seps, nseps, n, r, &begin, &len);
  return len + 1;
}

// symbol e of the compacted set, which read r gives (off[r] <= e < off[r + 1])
MST_HD u8 ct_symbol(const u8 *enc, const u32 *seps, u64 nseps, u64 n, const u64 *off, u64 r, u64 e) {
  u64 begin;
  u32 len;
  ct_read_span(seps, nseps, n, r, &begin, &len);
  const u64 k = e - off[r];
  return k < len ? enc[begin + k] : (u8) 255;
}

// symbol e of the 2n + 1 of the mirrored set of n symbols (gtamd_mirror)
MST_HD u8 ct_mirror_symbol(const u8 *enc, u64 n, u64 e) {
  if (e < n) return enc[e];
  if (e == n) return 255;
  const u8 c = enc[2 * n - e];
  return c < 254 ? (u8) (3 - c) : c;
}
