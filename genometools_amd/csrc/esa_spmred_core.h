// esa_spmred_core.h -- what one lane of esa_spmred.hip does (semantics and
// algorithm: include/gtamd_spmred.h), apart from the kernels so that a test can
// compile it for the CPU (tests/spmred_core_shim.cpp) and run the very code the
// lanes run against the brute force without a device: the decision for one
// (terminal suffix, read start) pair, the mirror filter, the k-th kept pair of a
// bitmap word and the record of a kept pair.
#pragma once
#include "esa_spm_core.h"

// flags of a prepare (GTAMD_SPMRED_ELIMTRANS, GTAMD_SPMRED_MIRRORED) and of a record
constexpr u32 SR_ELIMTRANS = 1, SR_MIRRORED = 2;
constexpr u64 SR_PREFIX_DIRECT = 1, SR_SUFFIX_DIRECT = 2;

struct SrRecord { u64 suffix_read, prefix_read, len, flags; };

// What steps 1 to 4 of include/gtamd_spm.h leave (M terminal suffixes in table
// order, R read starts, nseps separators), and beside it: position and length of
// the sequence of every read start; the terminal suffixes by text position (tpos
// ascending, tperm[u] = the place in table order of the one at tpos[u]), which
// puts those of one sequence side by side, the longest first.
struct SrLists {
  const u32 *idx, *len, *first, *cnt; u64 M;
  const u32 *starts, *spos, *slen; u64 R;
  const u32 *seps; u64 nseps;
  const u32 *tpos, *tperm;
};

// the walk of one pair: read starts looked at, letters compared
struct SrWalk { u64 candidates, letters; };

// position and length of the sequence that starts at read start j
template <typename S> MST_HD void sr_start(const SpIndex<S> &x, const u32 *starts, const u32 *seps, u64 nseps, u64 j,
                                           u32 *pos, u32 *len) {
  u64 q = x.suf[starts[j]];
  if (q > x.n) q = x.n;              // (a table that is none cannot lead outside the lists)
  const u64 s = sp_sequence_of(seps, nseps, q);
  *pos = (u32) q;
  *len = (u32) ((s < nseps ? seps[s] : x.n) - q);
}

// the sequence that starts at read start j stands at another place of the set as
// well: its whole length is a terminal suffix of step 1
template <typename S> MST_HD bool sr_contained(const SpIndex<S> &x, const u32 *starts, u64 j, u32 L) {
  u32 h;
  return sp_terminal(x, (u64) starts[j], L, &h);
}

// Pair j of terminal suffix k -- the last l letters of sequence r are the first l
// of sequence w -- is TRANSITIVE: some sequence t has a suffix-prefix match (t,
// w, l') with l' > l whose left part, t without its last l' letters, ends the
// left part of r.  Aligned on w, t then starts inside r: its first m letters are
// the last m of r for an m >= l, and l' = |t| - m + l.  So the lane walks the
// terminal suffixes of r of m >= l letters, the longest first, and the read starts
// t inside the interval of each: t qualifies when |t| > m (l' > l), when l' <= |w|
// and when the letters t[m .. |t|) are w[l .. l'); the l letters in front of them
// are r's.  It stops at the first that does.  (m = l is the empty left part: t is
// the first l' letters of w.  t = w with l' = |w| is the trivial triple, a match
// only when w stands at another place too: include/gtamd_spm.h.)
template <typename S>
MST_HD bool sr_transitive(const SpIndex<S> &x, const SrLists &a, u32 L, u64 k, u64 j, SrWalk *walk) {
  const u32 l = a.len[k];
  u64 p = x.suf[a.idx[k]];
  if (p > x.n) p = x.n;
  const u64 end = p + l;                                  // the separator behind r, or n
  const u64 s = sp_sequence_of(a.seps, a.nseps, p);
  const u64 begin = s ? (u64) a.seps[s - 1] + 1 : 0;
  const u64 jw = (u64) a.first[k] + j;
  const u64 q = a.spos[jw], wl = a.slen[jw];
  const u64 u0 = sp_lower_bound(a.tpos, a.M, begin), u1 = sp_lower_bound(a.tpos, a.M, p);
  for (u64 u = u0; u <= u1 && u < a.M; u++) {
    const u64 kk = a.tperm[u], m = end - a.tpos[u], f = a.first[kk];
    const u32 c = a.cnt[kk];
    for (u32 e = 0; e < c; e++) {
      const u64 tl = a.slen[f + e];
      walk->candidates++;
      if (tl <= m) continue;
      const u64 lp = tl - m + l;
      if (lp > wl) continue;
      const u64 tq = a.spos[f + e];
      if (tq == q && lp == wl) {                           // t is w, in its whole length
        if (sr_contained(x, a.starts, jw, L)) return true;
        continue;
      }
      const u32 more = (u32) (tl - m);
      u32 o = 0;
      while (o < more) {
        const u32 piece = more - o < MST_WORD ? more - o : MST_WORD;
        const u32 bad = first_bad16(x.enc, x.n, tq + m + o, x.enc, x.n, q + l + o, piece);
        walk->letters += bad < piece ? bad + 1 : piece;
        if (bad < piece) break;
        o += piece;
      }
      if (o >= more) return true;
    }
  }
  return false;
}

// Sequence s of K = 2R, the mirrored set of R reads: its read number; *direct =
// it is the read itself, not the reverse complement (GT_READJOINER_CORRECT_REVCOMPL)
MST_HD u64 sr_read_of(u64 s, u64 K, bool *direct) {
  *direct = s < K / 2;
  return *direct ? s : K - 1 - s;
}

// of the two mirror images of one overlap, the one that is kept
// (GT_READJOINER_IS_CORRECT_REVCOMPL_CASE)
MST_HD bool sr_mirror_kept(u64 sn, bool sd, u64 pn, bool pd) {
  return (sd && pd) || (sn == pn && (sd || pd)) || (sd && !pd && pn > sn) || (!sd && pd && pn < sn);
}

// the mirror filter for pair j of terminal suffix k
template <typename S> MST_HD bool sr_pair_kept(const SpIndex<S> &x, const SrLists &a, u64 k, u64 j) {
  SpRecord rec;
  bool sd, pd;
  sp_record(x, a.starts, a.seps, a.nseps, a.idx[k], a.len[k], a.first[k], j, &rec);
  const u64 sn = sr_read_of(rec.suffix_seq, a.nseps + 1, &sd), pn = sr_read_of(rec.prefix_seq, a.nseps + 1, &pd);
  return sr_mirror_kept(sn, sd, pn, pd);
}

// the place of the r-th set bit of b, r below the number of its set bits
MST_HD u32 sr_select(u64 b, u32 r) {
  u32 at = 0;
  for (u32 half = 32; half != 0; half >>= 1) {
    const u32 c = (u32) __builtin_popcountll(b & ((1ull << half) - 1));
    if (r >= c) { r -= c; b >>= half; at += half; }
  }
  return at;
}

// the record of pair j of terminal suffix k
template <typename S>
MST_HD void sr_record(const SpIndex<S> &x, const SrLists &a, u32 flags, u64 k, u64 j, SrRecord *out) {
  SpRecord rec;
  sp_record(x, a.starts, a.seps, a.nseps, a.idx[k], a.len[k], a.first[k], j, &rec);
  out->suffix_read = rec.suffix_seq;
  out->prefix_read = rec.prefix_seq;
  out->len = rec.len;
  out->flags = SR_SUFFIX_DIRECT | SR_PREFIX_DIRECT;
  if (flags & SR_MIRRORED) {
    bool sd, pd;
    out->suffix_read = sr_read_of(rec.suffix_seq, a.nseps + 1, &sd);
    out->prefix_read = sr_read_of(rec.prefix_seq, a.nseps + 1, &pd);
    out->flags = (sd ? SR_SUFFIX_DIRECT : 0) | (pd ? SR_PREFIX_DIRECT : 0);
  }
}
