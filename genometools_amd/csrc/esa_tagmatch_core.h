// esa_tagmatch_core.h -- what one lane of esa_tagmatch.hip computes on its own
// (semantics and algorithm: include/gtamd_tagmatch.h): the bit-vector column of
// a tag against one more symbol, the tests for success and for the end of a
// walk, and the walk of a single suffix in the text.  Apart from the kernels so
// that a test can compile it for the CPU (tests/tagmatch_core_shim.cpp,
// tests/tagmatch_core_main.cpp) and run the very code the lanes run against a
// plain table of edit distances without a device.
//
// The column is the one of Myers' bit-vector algorithm for a tag of m <= 64
// letters anchored at a start position: after d symbols, row i (0..m) holds the
// edit distance of the tag's first i letters and the d symbols; row 0 is d.  Pv
// and Mv hold, in bit i - 1, whether row i is one more or one less than row
// i - 1.  No shift in here has a count of 64: bit m - 1 <= 63 is the highest
// one that is looked at.
#pragma once
#include "esa_ivwalk.h"

#if defined(__HIPCC__)
#define TM_HD __device__ __forceinline__
#else
#define TM_HD inline
#endif

constexpr u32 TM_MAX_TAG = 64;           // letters of a tag: the bits of a word
constexpr u32 TM_LETTERS = 32;           // letters an alphabet may have here: the entries of an Eq table
constexpr u32 TM_NONE = 0xffffffffu;     // no row of the column is <= K
constexpr u32 TM_WILDCARD = IV_WILDCARD, TM_SEPARATOR = IV_SEPARATOR;      // (as the cases of tests/ name them)

// row: the largest row whose value is <= K, val: that value.  While row < m the
// value is K itself (the row above holds K + 1 and rows differ by at most one).
struct TmColumn { u64 Pv, Mv; u32 row, val; };

// depth 0: row i holds i
TM_HD TmColumn tm_first_column(u32 K) { return TmColumn{ ~0ull, 0, K, K }; }

// eq[c]: bit i set where tag letter i is c; a letter >= TM_LETTERS is in no tag
TM_HD void tm_eq_table(const u8 *tag, u32 m, u64 *eq) {
  for (u32 c = 0; c < TM_LETTERS; c++) eq[c] = 0;
  for (u32 i = 0; i < m && i < TM_MAX_TAG; i++)
    if (tag[i] < TM_LETTERS) eq[tag[i]] |= 1ull << i;
}

// One more symbol whose Eq word is Eq (0 for a wildcard).  Asks for c.row <
// m: a column that has reached row m is a match and is not stepped.
TM_HD void tm_step(TmColumn &c, u64 Eq, u32 K) {
  const u64 Pv = c.Pv, Mv = c.Mv;
  const u64 Xv = Eq | Mv;
  const u64 Xh = (((Eq & Pv) + Pv) ^ Pv) | Eq;
  const u64 Mh = Pv & Xh;                       // bit i - 1: row i is one less than it was
  const u64 Ph = ((Mv | ~(Xh | Pv)) << 1) | 1;  // shifted: bit i: row i is one more; row 0 always is
  c.Pv = (Mh << 1) | ~(Xv | Ph);
  c.Mv = Ph & Xv;
  const u64 above = 1ull << c.row;              // bit of row c.row + 1; c.row <= m - 1 <= 63
  if ((Eq | Mh) & above) {
    // row + 1 takes the value K: along the diagonal from (row, K), or K + 1 less one
    c.row += 1;
    return;
  }
  if (!(Ph & above)) return;                    // row c.row keeps its value
  // row c.row is K + 1 now: down to the first row that holds K
  u32 score = K + 1;
  u64 bit = above;
  for (u32 r = c.row; r > 0; r--) {
    bit >>= 1;                                  // the bit of row r: row r against row r - 1
    if (c.Pv & bit) score -= 1;
    else if (c.Mv & bit) score += 1;
    if (score <= K) { c.row = r - 1; c.val = score; return; }
  }
  c.row = TM_NONE;
}

TM_HD bool tm_dead(const TmColumn &c) { return c.row == TM_NONE; }
TM_HD bool tm_success(const TmColumn &c, u32 m) { return c.row == m; }

// Suffix p whose first `depth` symbols gave column c (alive, no success yet) goes
// on alone in the text.  The length of its match, *dist = its distance; 0 if it
// has none.  A separator and the end never pass, a wildcard only with `wild`, as
// a symbol that equals nothing.  At most m + K symbols are part of a match (row
// m holds at least depth - m), so the loop ends there whatever the text holds.
TM_HD u32 tm_walk(TmColumn c, const u64 *eq, const u8 *enc, u64 n, u64 p, u32 depth, u32 m, u32 K, bool wild,
                  u32 *dist) {
  while (depth < m + K && p + depth < n) {
    const u32 s = enc[p + depth];
    if (s == IV_SEPARATOR || (s == IV_WILDCARD && !wild)) return 0;
    tm_step(c, s < TM_LETTERS ? eq[s] : 0, K);
    depth += 1;
    if (tm_dead(c)) return 0;
    if (tm_success(c, m)) { *dist = c.val; return depth; }
  }
  return 0;
}
