// esa_mstat_search.h -- the search of one query position of esa_mstat.hip
// (semantics and algorithm: include/gtamd_mstat.h), apart from the kernel so
// that a test can compile it for the CPU (tests/mstat_search_shim.cpp) and run
// the very code the lanes run against the brute force without a device.
#pragma once
#include <stdint.h>

typedef uint64_t u64;
typedef uint32_t u32;
typedef uint8_t u8;

#if defined(__HIPCC__)
#define MST_HD __device__ __forceinline__
#define MST_ALIGNBYTE(hi, lo, shift) __builtin_amdgcn_alignbyte(hi, lo, shift)
#else
#define MST_HD inline
#define MST_ALIGNBYTE(hi, lo, shift) ((u32) (((((u64) (hi)) << 32) | (lo)) >> (8 * (shift))))
#endif

constexpr u32 MST_WORD = 16;             // symbols of one wide comparison
constexpr u32 MST_WORD_MIN = 8;          // fewer symbols go byte by byte

MST_HD u32 mst_min(u32 a, u32 b) { return a < b ? a : b; }
MST_HD u32 mst_max(u32 a, u32 b) { return a > b ? a : b; }
// index of the lowest byte of x that is not zero, 4 for none
MST_HD u32 mst_first_byte(u32 x) { return x ? (u32) __builtin_ctz(x) >> 3 : 4; }

// 0x80 in every byte of x that is zero
MST_HD u32 zero_bytes(u32 x) {
  return ~(((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x | 0x7f7f7f7fu);
}

// the first of cnt <= MST_WORD offsets at which a[xa + k] and b[xb + k] are not
// equal letters, or cnt; the caller keeps xa + cnt <= na and xb + cnt <= nb.
// Whole words where all 20 bytes around each side lie inside its sequence.
MST_HD u32 first_bad16(const u8 *a, u64 na, u64 xa, const u8 *b, u64 nb, u64 xb,
                                           u32 cnt) {
  if (cnt >= MST_WORD_MIN && xa >= 3 && xb >= 3 && xa + MST_WORD + 4 <= na && xb + MST_WORD + 4 <= nb) {
    const uintptr_t pa = (uintptr_t) a + xa, pb = (uintptr_t) b + xb;
    const u32 ma = pa & 3, mb = pb & 3;
    const u32 *wa = (const u32 *) (pa - ma), *wb = (const u32 *) (pb - mb);
    u32 va[5], vb[5];
#pragma unroll
    for (int k = 0; k < 5; k++) { va[k] = wa[k]; vb[k] = wb[k]; }
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const u32 x = MST_ALIGNBYTE(va[k + 1], va[k], ma);
      const u32 y = MST_ALIGNBYTE(vb[k + 1], vb[k], mb);
      // a byte differs, or is a special (>= 254: all of its upper seven bits set)
      const u32 d = x ^ y, sp = zero_bytes((x & 0xfefefefeu) ^ 0xfefefefeu);
      if (d | sp) {
        const u32 at = 4 * k + mst_min(mst_first_byte(d), mst_first_byte(sp));
        return at < cnt ? at : cnt;
      }
    }
    return cnt;
  }
  for (u32 k = 0; k < cnt; k++) {
    const u32 x = a[xa + k], y = b[xb + k];
    if (x != y || x >= 254) return k;
  }
  return cnt;
}

// one query position against the subject
struct Lane {
  const u8 *q; u64 m, i;
  const u8 *enc; u64 n;
  u64 compared;

  // the letters the query suffix, cut to qlen symbols, shares with subject suffix
  // p <= n, of which the first `from` are known to be shared
  MST_HD u32 shared(u64 p, u32 from, u32 qlen) {
    const u64 room = n - p;
    const u32 to = room < qlen ? (u32) room : qlen;
    u32 k = to;
    for (u32 o = from; o < to; o += MST_WORD) {
      const u32 cnt = to - o < MST_WORD ? to - o : MST_WORD;
      const u32 bad = first_bad16(q, m, i + o, enc, n, p + o, cnt);
      if (bad < cnt) { k = o + bad; break; }
    }
    if (k >= from) compared += k - from + 1;
    return k;
  }

  // is subject suffix p smaller than the query suffix of qlen symbols, which
  // shares k letters with it?  The query's end sorts in front of everything, a
  // special of the subject and its end behind every letter.
  MST_HD bool subject_smaller(u64 p, u32 k, u32 qlen) const {
    if (k >= qlen) return false;
    const u32 a = q[i + k];
    if (a >= 254 || p + k >= n) return false;
    return enc[p + k] < a;
  }
};

template <typename S> MST_HD u64 suffix_at(const S *suf, u64 r, u64 n) {
  const u64 p = suf[r];
  return p < n ? p : n;        // (a table that is none cannot lead outside the sequence)
}

struct Place { u64 lb; u32 L, R; };

// lb: the first table index whose suffix is not smaller than the query suffix
// of qlen symbols; L, R: the letters it shares with the suffixes at lb - 1
// (0: none) and lb.  The entry N - 1 is the subject's end: never smaller.
template <typename S> MST_HD Place place_of(Lane &c, const S *suf, u64 N, u32 qlen) {
  u64 lo = 0, hi = N - 1;
  u32 llo = 0, lhi = 0;
  while (lo < hi) {
    const u64 mid = (lo + hi) >> 1, p = suffix_at(suf, mid, c.n);
    const u32 k = c.shared(p, mst_min(llo, lhi), qlen);
    if (c.subject_smaller(p, k, qlen)) { lo = mid + 1; llo = k; }
    else { hi = mid; lhi = k; }
  }
  return { lo, llo, lhi };
}

// the smallest l >= 1 for which exactly one suffix starts with l letters of
// the query suffix, 0 if there is none among its qlen symbols
template <typename S> MST_HD u32 unique_of(Lane &c, const S *suf, u64 N, const Place &pl, u32 qlen) {
  if (pl.L == pl.R) return 0;
  u32 best, other, next = 0;
  if (pl.L > pl.R) {
    best = pl.L; other = pl.R;
    if (pl.lb >= 2) next = c.shared(suffix_at(suf, pl.lb - 2, c.n), 0, best);
  } else {
    best = pl.R; other = pl.L;
    if (pl.lb + 1 < N) next = c.shared(suffix_at(suf, pl.lb + 1, c.n), 0, best);
  }
  const u32 v = mst_max(other, next) + 1;      // (both below best <= 2^32 - 2)
  return v <= best ? v : 0;
}

// One query position i < m.  MATSTAT: ms(i) -> *len and, if want_pos, the witness
// -> *pos; else mu(i) -> *len.  limit: symbols of a query suffix that are looked
// at, max_len + 1 or 2^32 - 1.  Returns 1 if the position was searched again
// without the cut.
template <typename S, bool MATSTAT>
MST_HD u32 mst_position(Lane &c, const S *suf, u64 N, u32 limit, bool want_pos, u32 *len_out, u64 *pos_out) {
  const u64 n = c.n, rest = c.m - c.i;                    // rest <= 2^32 - 1
  u32 qlen = rest < limit ? (u32) rest : limit;
  u32 len = 0, reruns = 0;
  u64 pos = 0;
  if (c.q[c.i] < 254) {
    Place pl = place_of(c, suf, N, qlen);
    const u32 ms = mst_max(pl.L, pl.R);
    if (MATSTAT) {
      len = ms;
      if (ms > 0 && want_pos) {
        u64 at = pl.lb;
        if (pl.L >= pl.R) {
          // the first index of [0, lb - 1] whose suffix shares ms letters
          u64 lo = 0, hi = pl.lb - 1;
          u32 llo = 0;
          while (lo < hi) {
            const u64 mid = (lo + hi) >> 1;
            const u32 k = c.shared(suffix_at(suf, mid, n), llo, ms);
            if (k >= ms) hi = mid; else { lo = mid + 1; llo = k; }
          }
          at = lo;
        }
        pos = suf[at];
      }
    } else {
      len = unique_of(c, suf, N, pl, qlen);
      if (len == 0 && ms == limit && rest > limit) {
        // the cut suffix occurs twice: mu(i) is 0 or beyond the cap
        qlen = (u32) rest;
        pl = place_of(c, suf, N, qlen);
        len = unique_of(c, suf, N, pl, qlen) ? limit : 0;
        reruns = 1;
      }
    }
  }
  *len_out = len;
  *pos_out = pos;
  return reruns;
}
