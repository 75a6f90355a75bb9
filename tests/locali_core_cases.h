// locali_core_cases.h -- the cases of tests/test_locali_core.py for
// genometools_amd/csrc/esa_locali_core.h, shared by the shim the test loads and
// the program it starts under the sanitizers.  The judge is the statement with
// stored traces (lc_plain_column, lc_traceback): full columns, no band, no
// prefix maximum, no start row that travels.  Against it, for every column of
// every walk: the cells > 0, their start rows, the band, M and e; and for the
// walk: the match.  The tally counts the events the cases are there for, so
// that the test can see that they happened.
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
};

inline void fail(Tally &t, const char *what, u32 m, u32 d, u32 i) {
  if (t.failures++ < 10) fprintf(stderr, "locali core: %s (m = %u, column %u, row %u)\n", what, m, d, i);
}

// every column of start position p, both ways
inline void walk(Tally &t, const std::vector<u8> &q, const std::vector<u8> &enc, u64 p, LcScores sc, u32 T) {
  const u32 m = (u32) q.size();
  const u64 n = enc.size();
  const u32 deepest = lc_max_depth(m, sc);
  std::vector<int> prev(m + 1), cur(m + 1);
  std::vector<u8> traces;
  std::vector<u32> flat;                                 // the start rows of the cells > 0 of every column
  std::vector<u32> a(m + 1, 0xdeadbeefu), b(m + 1, 0xdeadbeefu);
  LcColumn band = { 0, 0, 0, 0, 0 };
  const u32 *src = nullptr;
  LcMatch want = { 0, 0, 0, 0 };
  t.walks++;
  u32 d = 0;
  for (;;) {
    if (p + d >= n || enc[p + d] >= LC_WILDCARD) { t.stopped_by_special++; break; }
    const u32 c = enc[p + d];
    d += 1;
    traces.resize((u64) d * (m + 1));
    lc_plain_column(d == 1 ? nullptr : prev.data(), c, q.data(), m, sc, cur.data(), traces.data() + (u64) (d - 1) * (m + 1));
    flat.resize((u64) d * (m + 1), LC_NO_ROW);
    const auto starts = [&](u32 col) { return flat.data() + (u64) col * (m + 1); };
    u32 M = 0, e = 0, lo = LC_NO_ROW, hi = 0, maxima = 0;
    for (u32 i = 1; i <= m; i++) {
      if (cur[i] == 0) t.zero_cells++;
      if (cur[i] <= 0) continue;
      if (lo == LC_NO_ROW) lo = i;
      hi = i + 1;
      if ((u32) cur[i] > M) { M = (u32) cur[i]; e = i; maxima = 1; }
      else if ((u32) cur[i] == M) maxima++;
      // where lc_traceback from (i, d) ends: its first step, then the end known for the cell it comes to
      const u8 bit = traces[(u64) (d - 1) * (m + 1) + i];
      starts(d - 1)[i] = bit == LC_TRACE_DELETE ? starts(d - 1)[i - 1]
                         : bit == LC_TRACE_REPLACE ? (d == 1 ? i - 1 : starts(d - 2)[i - 1])
                         : bit == LC_TRACE_INSERT && d > 1 ? starts(d - 2)[i] : LC_NO_ROW;
      if (starts(d - 1)[i] == LC_NO_ROW) fail(t, "a cell > 0 without a trace", m, d, i);
      // equal candidates with different ends of their tracebacks
      const int r = q[i - 1] == c ? sc.match : sc.mismatch;
      const bool del = cur[i - 1] > 0 && cur[i - 1] - sc.gap == cur[i];
      const bool rep = d == 1 ? r == cur[i] : prev[i - 1] > 0 && prev[i - 1] + r == cur[i];
      const bool ins = d > 1 && prev[i] > 0 && prev[i] - sc.gap == cur[i];
      const u32 sdel = del ? starts(d - 1)[i - 1] : 0, srep = rep ? (d == 1 ? i - 1 : starts(d - 2)[i - 1]) : 0;
      const u32 sins = ins ? starts(d - 2)[i] : 0;
      if (del && rep && sdel != srep) t.tie_del_rep++;
      if (del && ins && sdel != sins) t.tie_del_ins++;
      if (rep && ins && srep != sins) t.tie_rep_ins++;
      if (i == 65 && traces[(u64) (d - 1) * (m + 1) + 65] == LC_TRACE_DELETE &&
          traces[(u64) (d - 1) * (m + 1) + 64] == LC_TRACE_DELETE && cur[63] > 0)
        t.delete_across++;
    }
    if (maxima > 1) t.two_maxima++;
    if (M && lc_traceback(traces.data(), m, d, e) != starts(d - 1)[e]) fail(t, "the traceback from the maximum", m, d, e);
    // the column of the lanes
    const bool first = d == 1;
    std::fill(a.begin(), a.end(), 0xdeadbeefu);
    const LcColumn got = lc_column(src, band.lo, band.hi, first, c, q.data(), m, sc, a.data());
    t.columns++;
    if (got.M != M || (M && (got.e != e || got.qstart != starts(d - 1)[e]))) fail(t, "M, e or qstart", m, d, e);
    if (got.lo != lo || (M && got.hi != hi)) fail(t, "the band", m, d, lo);
    if (M) {
      const u32 *cells = a.data() + lc_band_offset(got, first, band.lo);
      for (u32 i = lo; i < hi; i++) {
        const u32 cell = cells[i - lo];
        if (cur[i] > 0 ? cell != ((u32) cur[i] << 16 | starts(d - 1)[i]) : cell != 0) fail(t, "a cell", m, d, i);
      }
    }
    if (M >= T) { want = LcMatch{ d, M, e, starts(d - 1)[e] }; if (d == 1) t.depth_one++; break; }
    if (M == 0) break;
    if (d == deepest) t.deepest_reached++;
    if (d > deepest) { fail(t, "a cell > 0 beyond lc_max_depth", m, d, e); break; }
    src = a.data() + lc_band_offset(got, first, band.lo);
    band = got;
    a.swap(b);
    prev.swap(cur);
  }
  // the walk of the lanes, from depth 0
  std::fill(a.begin(), a.end(), 0xdeadbeefu);
  std::fill(b.begin(), b.end(), 0xdeadbeefu);
  const LcMatch got = lc_walk(nullptr, LcColumn{ 0, 0, 0, 0, 0 }, 0, enc.data(), n, p, q.data(), m, sc, T, a.data(), b.data());
  if (got.dblen != want.dblen || got.score != want.score || got.e != want.e || got.qstart != want.qstart)
    fail(t, "the match of a walk", m, want.dblen, want.e);
  if (want.dblen) t.matches++;
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
  return t;
}

}  // namespace lccases
