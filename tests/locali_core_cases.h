// locali_core_cases.h -- the cases of tests/test_locali_core.py for
// genometools_amd/csrc/esa_locali_core.h, shared by the shim the test loads and
// the program it starts under the sanitizers.  The judge is the statement with
// stored traces (lc_plain_column, lc_traceback): full columns, no band, no
// prefix maximum, no start row that travels.  Against it, for every column of
// every walk: the cells > 0, their start rows, the band, M and e; and for the
// walk: the match.  The tally counts the events the cases are there for, so
// that the test can see that they happened; it counts them from the plain
// columns, never from what lc_column answers.  The long queries (191 to 16384
// letters) are walked for some 70 columns each; only the longest exact copy
// goes all the 16384 columns down.  For m > 1024 the traceback from the
// maximum, which walks d columns back, is held against the start row in the
// first 300 columns, in every 61st and in the last one, not in every column;
// the start rows themselves are followed from the traces in every cell of
// every column at any m.  That walk keeps all its traces, 16384 * 16385 bytes
// (268 MB), in the sanitized program and in the process that loads the shim
// alike: lc_traceback reads columns back to the first.
#pragma once
#include <stdio.h>
#include <string.h>
#include <vector>
#include "../genometools_amd/csrc/esa_locali_core.h"

namespace lccases {

struct Tally {
  unsigned long long walks, columns, matches, failures;
  unsigned long long tie_del_rep, tie_del_ins, tie_rep_ins;     // equal candidates whose start rows differ
  unsigned long long delete_across, two_maxima, zero_cells, depth_one, deepest_reached, stopped_by_special;
  // the long queries, all counted from the plain columns: a band of more than three chunks; a column that starts at
  // a row r0 that is no multiple of 64 plus 1 and whose band begins below r0, for the third column in a row; a band
  // that ends a chunk or more before row m; a Delete run over more than two chunk boundaries (the chunks count from
  // r0); a maximum or its start row above 16000; a maximum above 65000; a Delete run that ends beyond the last row
  // with a candidate of its own, on the first and on the last row of a chunk
  unsigned long long columns_past_three_chunks, band_starts_unaligned, stopped_before_last_row, delete_across_three;
  unsigned long long row_above_16000, score_above_65000, chain_dies_on_first_row, chain_dies_on_last_row;
  unsigned long long tie_with_last_row;       // equal maxima, one of them in row 16384: the smaller row has to win
};

// the largest key a lane can form: the largest score in the last row a chunk can reach, with the largest gap
static_assert((long long) LC_MAX_SCORE + (long long) (LC_MAX_QUERY + LC_CHUNK - 1) * LC_MAX_WEIGHT < (1ll << 31),
              "key = score + row * gap must fit an int");

inline void fail(Tally &t, const char *what, u32 m, u32 d, u32 i) {
  if (t.failures++ < 10) fprintf(stderr, "locali core: %s (m = %u, column %u, row %u)\n", what, m, d, i);
}

// every column of start position p, both ways; the walk of the lanes once per threshold of Ts (ascending), the
// columns until the largest of them is reached
inline void walk_many(Tally &t, const std::vector<u8> &q, const std::vector<u8> &enc, u64 p, LcScores sc,
                      const std::vector<u32> &Ts) {
  const u32 m = (u32) q.size();
  const u64 n = enc.size();
  const u32 deepest = lc_max_depth(m, sc);
  std::vector<int> prev(m + 1), cur(m + 1);
  std::vector<u8> traces;
  // the start rows of the cells > 0 of column d and of column d - 1, LC_NO_ROW for the other cells
  std::vector<u32> scur(m + 1, LC_NO_ROW), sprev(m + 1, LC_NO_ROW);
  std::vector<u32> a(m + 1, 0xdeadbeefu), b(m + 1, 0xdeadbeefu);
  LcColumn band = { 0, 0, 0, 0, 0 };
  const u32 *src = nullptr;
  std::vector<LcMatch> want(Ts.size(), LcMatch{ 0, 0, 0, 0 });
  u32 plo = 0, phi = 0, moving = 0;                      // the plain band of column d - 1; columns in a row whose band moved
  u32 d = 0;
  for (;;) {
    if (p + d >= n || enc[p + d] >= LC_WILDCARD) { t.stopped_by_special++; break; }
    const u32 c = enc[p + d];
    d += 1;
    traces.resize((u64) d * (m + 1));
    const u8 *tr = traces.data() + (u64) (d - 1) * (m + 1);
    lc_plain_column(d == 1 ? nullptr : prev.data(), c, q.data(), m, sc, cur.data(), traces.data() + (u64) (d - 1) * (m + 1));
    const int *cu = cur.data(), *pv = prev.data();
    u32 *s1 = scur.data();
    const u32 *s2 = sprev.data();
    const u32 r0 = d == 1 ? 1 : plo;                     // where the chunks of lc_column count from
    u32 M = 0, e = 0, lo = LC_NO_ROW, hi = 0, maxima = 0, hangs_from = 0, elast = 0;
    unsigned long long zeros = 0;
    for (u32 i = 1; i <= m; i++) {
      s1[i] = LC_NO_ROW;
      if (cu[i] <= 0) { zeros += cu[i] == 0; continue; }
      if (lo == LC_NO_ROW) lo = i;
      hi = i + 1;
      if ((u32) cu[i] > M) { M = (u32) cu[i]; e = elast = i; maxima = 1; }
      else if ((u32) cu[i] == M) { maxima++; elast = i; }
      // where lc_traceback from (i, d) ends: its first step, then the end known for the cell it comes to
      const u8 bit = tr[i];
      s1[i] = bit == LC_TRACE_DELETE ? s1[i - 1]
              : bit == LC_TRACE_REPLACE ? (d == 1 ? i - 1 : s2[i - 1])
              : bit == LC_TRACE_INSERT && d > 1 ? s2[i] : LC_NO_ROW;
      if (s1[i] == LC_NO_ROW) fail(t, "a cell > 0 without a trace", m, d, i);
      // equal candidates with different ends of their tracebacks
      const int r = q[i - 1] == c ? sc.match : sc.mismatch;
      const bool del = cu[i - 1] > 0 && cu[i - 1] - sc.gap == cu[i];
      const bool rep = d == 1 ? r == cu[i] : pv[i - 1] > 0 && pv[i - 1] + r == cu[i];
      const bool ins = d > 1 && pv[i] > 0 && pv[i] - sc.gap == cu[i];
      const u32 sdel = del ? s1[i - 1] : 0, srep = rep ? (d == 1 ? i - 1 : s2[i - 1]) : 0;
      const u32 sins = ins ? s2[i] : 0;
      if (del && rep && sdel != srep) t.tie_del_rep++;
      if (del && ins && sdel != sins) t.tie_del_ins++;
      if (rep && ins && srep != sins) t.tie_rep_ins++;
      if (i == 65 && tr[65] == LC_TRACE_DELETE && tr[64] == LC_TRACE_DELETE && cu[63] > 0) t.delete_across++;
      // a Delete run hangs from the last cell above it that is none; counted as it crosses its third boundary
      if (bit != LC_TRACE_DELETE) hangs_from = i;
      else if ((i - r0) % LC_CHUNK == 0 && (i - r0) / LC_CHUNK - (hangs_from - r0) / LC_CHUNK == 3) t.delete_across_three++;
    }
    t.zero_cells += zeros;
    if (maxima > 1) t.two_maxima++;
    if (maxima > 1 && elast == LC_MAX_QUERY) t.tie_with_last_row++;
    if (M) {
      if (hi - lo > 3 * LC_CHUNK) t.columns_past_three_chunks++;
      if (hi + LC_CHUNK <= m) t.stopped_before_last_row++;
      if (e > 16000 || s1[e] > 16000) t.row_above_16000++;
      if (M > 65000) t.score_above_65000++;
      // the last cell > 0 lies beyond the rows with a candidate of their own (those up to phi) and above row m
      if (d > 1 && hi - 1 > phi && hi - 1 < m && tr[hi - 1] == LC_TRACE_DELETE) {
        if ((hi - 1 - r0) % LC_CHUNK == 0) t.chain_dies_on_first_row++;
        if ((hi - 1 - r0) % LC_CHUNK == LC_CHUNK - 1) t.chain_dies_on_last_row++;
      }
    }
    moving = d > 1 && M && plo % LC_CHUNK != 1 && lo > plo ? moving + 1 : 0;
    if (moving >= 3) t.band_starts_unaligned++;
    // (the traceback from the maximum walks d columns back: for m > 1024 in the first 300 columns, in every 61st
    // and in the last one; the start rows above are the same traces, followed one step a column.  It is why all
    // the traces of a walk are kept: 268 MB for the 16384 columns of the longest exact copy)
    if (M && (m <= 1024 || d <= 300 || d % 61 == 0 || M >= Ts.back()) && lc_traceback(traces.data(), m, d, e) != s1[e])
      fail(t, "the traceback from the maximum", m, d, e);
    // the column of the lanes
    const bool first = d == 1;
    std::fill(a.begin(), a.end(), 0xdeadbeefu);
    const LcColumn got = lc_column(src, band.lo, band.hi, first, c, q.data(), m, sc, a.data());
    t.columns++;
    if (got.M != M || (M && (got.e != e || got.qstart != s1[e]))) fail(t, "M, e or qstart", m, d, e);
    if (got.lo != lo || (M && got.hi != hi)) fail(t, "the band", m, d, lo);
    if (M) {
      const u32 *cells = a.data() + lc_band_offset(got, first, band.lo);
      for (u32 i = lo; i < hi; i++) {
        const u32 cell = cells[i - lo];
        if (cu[i] > 0 ? cell != ((u32) cu[i] << 16 | s1[i]) : cell != 0) fail(t, "a cell", m, d, i);
      }
    }
    for (size_t k = 0; k < Ts.size(); k++)
      if (!want[k].dblen && M >= Ts[k]) { want[k] = LcMatch{ d, M, e, s1[e] }; if (d == 1) t.depth_one++; }
    if (M >= Ts.back()) break;
    if (M == 0) break;
    if (d == deepest) t.deepest_reached++;
    if (d > deepest) { fail(t, "a cell > 0 beyond lc_max_depth", m, d, e); break; }
    src = a.data() + lc_band_offset(got, first, band.lo);
    band = got;
    plo = lo;
    phi = hi;
    a.swap(b);
    prev.swap(cur);
    sprev.swap(scur);
  }
  // the walk of the lanes, from depth 0
  for (size_t k = 0; k < Ts.size(); k++) {
    t.walks++;
    std::fill(a.begin(), a.end(), 0xdeadbeefu);
    std::fill(b.begin(), b.end(), 0xdeadbeefu);
    const LcMatch got = lc_walk(nullptr, LcColumn{ 0, 0, 0, 0, 0 }, 0, enc.data(), n, p, q.data(), m, sc, Ts[k], a.data(), b.data());
    if (got.dblen != want[k].dblen || got.score != want[k].score || got.e != want[k].e || got.qstart != want[k].qstart)
      fail(t, "the match of a walk", m, want[k].dblen, want[k].e);
    if (want[k].dblen) t.matches++;
  }
}

inline void walk(Tally &t, const std::vector<u8> &q, const std::vector<u8> &enc, u64 p, LcScores sc, u32 T) {
  walk_many(t, q, enc, p, sc, std::vector<u32>{ T });
}

struct Rng {
  u64 s;
  u32 next(u32 below) { s = s * 6364136223846793005ull + 1442695040888963407ull; return (u32) ((s >> 33) % below); }
};

inline std::vector<u8> letters(Rng &r, u32 count, u32 sigma) {
  std::vector<u8> v(count);
  for (u8 &x : v) x = (u8) r.next(sigma);
  return v;
}

inline Tally run() {
  Tally t;
  memset(&t, 0, sizeof t);
  Rng r = { 17 };
  const LcScores scores[] = { { 1, -1, 1 }, { 2, -1, 1 }, { 3, -2, 2 }, { 5, -3, 1 }, { 1, -2, 3 } };
  // every m around the chunks, queries cut from the subject and edited, sigma 2 and 4, a special at every distance
  for (u32 m : { 1u, 2u, 3u, 63u, 64u, 65u, 127u, 128u, 129u })
    for (u32 sigma : { 2u, 4u })
      for (const LcScores &sc : scores) {
        if (m > 65 && ((&sc - scores) % 2 == 1 || sigma == 2)) continue;      // (the long queries: three of the five, four letters)
        std::vector<u8> enc = letters(r, m + 40, sigma);
        std::vector<u8> q(enc.begin() + 3, enc.begin() + 3 + m);
        for (u32 k = 0; k < 1 + m / 16; k++) q[r.next(m)] = (u8) r.next(sigma);
        if (m > 8) { q.erase(q.begin() + r.next(m - 1)); q.insert(q.begin() + r.next(m - 1), (u8) r.next(sigma)); }
        if (m > 20) q[m / 2] = LC_WILDCARD;
        const u32 high = sc.match * (m > 4 ? m - m / 4 : m);
        for (u32 T : { 1u, (u32) sc.match, (u32) sc.match + 1, high / 2 + 1, high, (u32) sc.match * m + 1 })
          for (u64 p : { (u64) 0, (u64) 3, (u64) 4, (u64) enc.size() - 1, (u64) enc.size() }) walk(t, q, enc, p, sc, T);
        // the end, a wildcard and a separator at every distance from p = 3, under a T that only the whole query reaches
        // (the long queries: around the end of the first chunk only)
        for (u32 dist = m > 65 ? 62 : 0; dist <= m + 2 && dist < 70; dist++)
          for (u32 special : { 0u, LC_WILDCARD, LC_SEPARATOR }) {
            std::vector<u8> cut(enc.begin(), enc.begin() + 3 + dist + (special ? 1 : 0));
            if (special) cut.back() = (u8) special;
            walk(t, q, cut, 3, sc, high);
          }
      }
  // a Delete run from row 60 down across rows 63, 64, 65: one letter of the query matches, the gap is cheap
  {
    std::vector<u8> q(129, 0), enc = { 1, 0, 0, 0 };
    q[59] = 1;
    walk(t, q, enc, 0, LcScores{ 10, -1, 1 }, 100);
    q.assign(129, 0); q[62] = 1;                          // ... and one that starts in lane 62 and ends in the next chunk
    walk(t, q, enc, 0, LcScores{ 4, -1, 1 }, 100);
  }
  // equal candidates: short queries over two letters with every small score set, all subjects of 6 symbols
  for (u32 m : { 2u, 3u, 4u, 5u })
    for (u32 code = 0; code < (1u << m); code++)
      for (u32 text = 0; text < 64; text++)
        for (const LcScores &sc : { LcScores{ 1, -1, 1 }, LcScores{ 2, -1, 1 }, LcScores{ 2, -1, 2 }, LcScores{ 3, -1, 1 } }) {
          std::vector<u8> q(m), enc(6);
          for (u32 i = 0; i < m; i++) q[i] = code >> i & 1;
          for (u32 i = 0; i < 6; i++) enc[i] = text >> i & 1;
          walk(t, q, enc, 0, sc, 1000);
        }
  // the deepest walk the bound allows: four matches, then an insertion per column until the score is 1
  {
    std::vector<u8> q(4, 0), enc(40, 1);
    for (u32 i = 0; i < 4; i++) enc[i] = 0;
    const unsigned long long before = t.deepest_reached;
    walk(t, q, enc, 0, LcScores{ 5, -3, 1 }, 21);
    if (t.deepest_reached != before + 1 || lc_max_depth(4, LcScores{ 5, -3, 1 }) != 23) fail(t, "the deepest walk", 4, 23, 0);
  }
  // the long queries: around the end of the third chunk and up to the longest, cut from the subject and edited.  From
  // where the last 36 letters of the query align the bands sit in the last chunk, and the subject ends 73 symbols on;
  // from where its head aligns they stay in the first chunks, and the subject is cut after 72 columns.  Three
  // thresholds a walk: one that the first dozen letters reach, a later one, and one out of reach.
  for (u32 m : { 191u, 192u, 193u, 1000u, 4097u, LC_MAX_QUERY })
    for (const LcScores &sc : { LcScores{ 1, -2, 2 }, LcScores{ 2, -1, 1 } }) {
      const std::vector<u8> enc = letters(r, m + 40, 4);
      std::vector<u8> q(enc.begin() + 3, enc.begin() + 3 + m);
      for (u32 k = 0; k < 1 + m / 64; k++) q[r.next(m)] = (u8) r.next(4);
      q.erase(q.begin() + r.next(m - 1));
      q.insert(q.begin() + r.next(m - 1), (u8) r.next(4));
      q[m / 2] = LC_WILDCARD;
      const std::vector<u32> Ts = { 12 * (u32) sc.match, 24 * (u32) sc.match, (u32) sc.match * m + 1 };
      const std::vector<u8> head(enc.begin(), enc.begin() + 3 + 72);
      for (u64 p : { (u64) 2, (u64) 3, (u64) 4 }) {
        if (p != 3 && m > 1000) continue;
        walk_many(t, q, enc, p + m - 36, sc, Ts);
        walk_many(t, q, head, p, sc, Ts);
      }
    }
  // Delete runs over many chunks.  One letter of the query, in row 100, equals the subject's; it is worth 200 and the
  // gap costs 1, so the first column runs down 200 rows from there ...
  {
    const unsigned long long before = t.delete_across_three;
    std::vector<u8> q(600, (u8) LC_WILDCARD), enc = { 1, 0, 0 };
    q[99] = 1;
    walk(t, q, enc, 0, LcScores{ 200, -1, 1 }, 100000);
    if (t.delete_across_three < before + 1) fail(t, "no Delete run over three chunk boundaries", 600, 1, 100);
  }
  // ... and the second column, whose chunks count from row 70 - a, gets twice the match score in row 71 and no other
  // candidate below row 70 + match: the run ends in row 70 + 2 * match, on every row of a chunk as a goes from 0 to
  // 63, and the loop over the chunks has to stop right there
  {
    const unsigned long long first = t.chain_dies_on_first_row, last = t.chain_dies_on_last_row;
    for (int match : { 96, 100 })
      for (u32 a = 0; a < LC_CHUNK; a++) {
        std::vector<u8> q(600, (u8) LC_WILDCARD), enc = { 1, 1, 0, 0 };
        q[70 - a - 1] = q[70 - 1] = q[71 - 1] = 1;
        walk(t, q, enc, 0, LcScores{ match, -1, 1 }, 100000);
      }
    if (t.chain_dies_on_first_row < first + 2 || t.chain_dies_on_last_row < last + 2)
      fail(t, "no Delete run that ends on the first and on the last row of a chunk", 600, 2, 70);
  }
  // the top of a cell: exact copies whose score is the largest the 16 bits hold, under a threshold equal to it and
  // one above it; the longest of them with the largest gap, which makes key = score + row * gap as large as it gets
  {
    const unsigned long long before = t.score_above_65000;
    struct { int match, mismatch, gap; u32 m; } const tops[] = {
      { 2047, -1, 1, 32 }, { 1023, -1, 1, 64 }, { 511, -1, 1, 128 }, { 32767, -1, 1, 2 },
      { 3, -3, LC_MAX_WEIGHT, LC_MAX_QUERY }, { 3, -1, 1, 600 } };
    for (const auto &top : tops) {
      const std::vector<u8> q = letters(r, top.m, 4);
      const u32 whole = (u32) top.match * top.m;
      const unsigned long long matches = t.matches;
      walk_many(t, q, q, 0, LcScores{ top.match, top.mismatch, top.gap }, { whole, whole + 1 });
      if (t.matches != matches + 1) fail(t, "an exact copy under T and T + 1", top.m, top.m, top.m);
    }
    if (t.score_above_65000 < before + 4) fail(t, "no score above 65000", 0, 0, 0);
  }
  // equal maxima in the last rows: the maximum keeps 0xffff - row beside the score so that the smaller row wins.  One
  // letter of the longest query in row 5 (then in row 16383) and one in row 16384 equal the subject's first symbol,
  // and the second column has the tie again, one higher, in rows 16383 and 16384
  {
    const unsigned long long before = t.tie_with_last_row;
    for (u32 other : { 5u, LC_MAX_QUERY - 1 })
      for (u32 T : { 1u, 3u }) {
        std::vector<u8> q(LC_MAX_QUERY, (u8) LC_WILDCARD), enc = { 1, 1, 0 };
        q[other - 1] = q[LC_MAX_QUERY - 1] = 1;
        if (other > 5) q[other - 2] = 1;
        walk(t, q, enc, 0, LcScores{ 1, -3, 3 }, T);
      }
    if (t.tie_with_last_row < before + 5) fail(t, "no tie of maxima with row 16384", LC_MAX_QUERY, 1, LC_MAX_QUERY);
  }
  return t;
}

}  // namespace lccases
