// esa_locali_core.h -- what the lanes of esa_locali.hip compute (semantics:
// include/gtamd_locali.h): one column of the local-alignment matrix of a query
// against one more symbol of the subject, 64 rows at a time with one row per
// lane, its largest cell, and the walk of a single suffix in the text.  Apart
// from the kernels so that a test can compile it for the CPU
// (tests/locali_core_shim.cpp, tests/locali_core_main.cpp): there the 64 lanes
// of a chunk are a loop, and the two operations that cross lanes, lc_scan and
// lc_max, run over an array; everything else is the same text.
//
// THE CELL.  Only a cell > 0 is ever extended, is ever the maximum of its
// column, or is ever reached by a traceback, so every cell <= 0 is stored as 0.
// A cell > 0 is score << 16 | start, where `start` is the row in which the
// traceback from this cell ends (qstart): it travels with the score along the
// very candidate that gives the cell its trace, so no trace is stored and no
// column is read twice.  lc_plain_column / lc_traceback below are the stored
// traces as the header states them; the test holds the two against each other.
//
// THE DELETE CHAIN.  C[i] = max(h[i], C[i-1] - gap) with h the better of
// Replace and Insert is, with key[i] = h[i] + i * gap, the prefix maximum of
// the keys: C[i] = max_{j <= i} key[j] - i * gap.  A strict comparison with
// Delete tried first means that on equal keys the EARLIER row wins, which is
// what lc_combine does; Replace before Insert is settled inside the lane.  A
// chain that has fallen to <= 0 stays there (its value only falls), so
// clamping to 0 loses nothing.  The carry from one chunk of 64 rows into the
// next is the last lane's key.
//
// THE DEPTH.  A cell > 0 of column d aligns d symbols of the subject with at
// most m letters of the query: at most m replacements, which give at most
// match * m, and at least d - m insertions, which cost gap each.  So it needs
// match * m - gap * (d - m) > 0, that is d <= lc_max_depth(m) = m +
// ceil(match * m / gap) - 1.  Every walk stops there whatever the text holds.
#pragma once
#include "esa_ivwalk.h"

#if defined(__HIPCC__)
#define LC_HD __device__ __forceinline__
#define LC_LANES_BEGIN { const u32 l = __lane_id(); const u32 li = 0;
#define LC_LANES_END }
// cells one lane wrote are read by its neighbours: the stores are done before a load goes out
#define LC_WAVE_FENCE() __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup")
#define LC_UNI(v) ((u32) __builtin_amdgcn_readfirstlane((int) (v)))      // the same in every lane, and known to be
constexpr u32 LC_PER = 1;                // lanes one thread of execution stands for
#else
#define LC_HD inline
#define LC_LANES_BEGIN for (u32 l = 0; l < 64; l++) { const u32 li = l;
#define LC_LANES_END }
#define LC_WAVE_FENCE() ((void) 0)
#define LC_UNI(v) ((u32) (v))
constexpr u32 LC_PER = 64;
#endif

constexpr u32 LC_CHUNK = 64;             // rows of one step: the lanes of a wave
constexpr u32 LC_MAX_QUERY = 16384;      // letters of a query
constexpr u32 LC_MAX_SCORE = 65535;      // match * m must fit the 16 bits of a cell
constexpr int LC_MAX_WEIGHT = 32767;     // match, -mismatch, -gapextend
constexpr u32 LC_LETTERS = 32;
constexpr u32 LC_WILDCARD = IV_WILDCARD, LC_SEPARATOR = IV_SEPARATOR;      // (as the cases of tests/ name them)
constexpr u32 LC_NO_ROW = 0xffffffffu;

struct LcScores { int match, mismatch, gap; };      // gap = -gapextend > 0
struct LcKey { int key; u32 start; };               // key = score + row * gap; 0: no candidate
// what a column leaves: the rows [lo, hi) hold all its cells > 0 (lo = LC_NO_ROW
// without any), M its largest cell, e the smallest row that holds it, qstart
// where the traceback from there ends
struct LcColumn { u32 lo, hi, M, e, qstart; };

LC_HD u32 lc_max_depth(u32 m, LcScores sc) {
  return m + (u32) (((u64) sc.match * m + (u64) sc.gap - 1) / (u64) sc.gap) - 1;
}

// earlier: rows above; on equal keys the earlier row wins (Delete before Replace)
LC_HD LcKey lc_combine(LcKey earlier, LcKey later) { return earlier.key >= later.key ? earlier : later; }

// the better of Replace and Insert for row i; pd = C_{d-1}[i-1], pi = C_{d-1}[i] as cells
LC_HD LcKey lc_candidate(u32 pd, u32 pi, bool same, u32 i, LcScores sc) {
  const int rep = pd ? (int) (pd >> 16) + (same ? sc.match : sc.mismatch) : 0;
  const int ins = pi ? (int) (pi >> 16) - sc.gap : 0;
  if (rep > 0 && rep >= ins) return LcKey{ rep + (int) i * sc.gap, pd & 0xffffu };
  if (ins > 0) return LcKey{ ins + (int) i * sc.gap, pi & 0xffffu };
  return LcKey{ 0, 0 };
}

// the first column: Replace is the bare score of the pair, Insert never wins
LC_HD LcKey lc_first_candidate(bool same, u32 i, LcScores sc) {
  return same ? LcKey{ sc.match + (int) i * sc.gap, i - 1 } : LcKey{ 0, 0 };
}

// ---- what crosses lanes ----------------------------------------------------------
#if defined(__HIPCC__)
// inclusive scan of lc_combine over the wave
LC_HD void lc_scan(LcKey *k) {
  const u32 lane = __lane_id();
  for (u32 s = 1; s < 64; s <<= 1) {
    LcKey o;
    o.key = __shfl_up(k[0].key, s);
    o.start = __shfl_up(k[0].start, s);
    if (lane >= s) k[0] = lc_combine(o, k[0]);
  }
}
LC_HD LcKey lc_last(const LcKey *k) {
  return LcKey{ (int) LC_UNI(__shfl(k[0].key, 63)), LC_UNI(__shfl((int) k[0].start, 63)) };
}
LC_HD u64 lc_max(const u64 *v) {
  u64 x = v[0];
  for (u32 s = 32; s > 0; s >>= 1) {
    const u64 o = __shfl_xor(x, s);
    x = o > x ? o : x;
  }
  return (u64) LC_UNI((u32) (x >> 32)) << 32 | LC_UNI((u32) x);
}
LC_HD u64 lc_ballot(const bool *b) { return __ballot(b[0]); }
#else
LC_HD void lc_scan(LcKey *k) {
  for (u32 s = 1; s < 64; s <<= 1)                   // the same steps, from the top so that a step reads old values
    for (u32 l = 63; l >= s; l--) k[l] = lc_combine(k[l - s], k[l]);
}
LC_HD LcKey lc_last(const LcKey *k) { return k[63]; }
LC_HD u64 lc_max(const u64 *v) {
  u64 x = 0;
  for (u32 l = 0; l < 64; l++) x = v[l] > x ? v[l] : x;
  return x;
}
LC_HD u64 lc_ballot(const bool *b) {
  u64 m = 0;
  for (u32 l = 0; l < 64; l++) m |= (u64) (b[l] ? 1 : 0) << l;
  return m;
}
#endif

// Column d of query q[0..m) for the subject letter c < sigma.  first: d = 1; else
// src holds the cells of rows [slo, shi) of column d - 1 (src[0] is row slo; all
// other rows are 0).  The cells of rows r0 .. min(m, what the Delete chain
// reaches) go to dst, dst[0] being row r0 = first ? 1 : slo: dst needs room for
// m + 1 - r0 cells and is not src.  The whole wave calls this with the same
// arguments.
LC_HD LcColumn lc_column(const u32 *src, u32 slo, u32 shi, bool first, u32 c, const u8 *q, u32 m, LcScores sc,
                         u32 *dst) {
  const u32 r0 = first ? 1 : slo;
  const u32 last_h = first ? m : (shi < m ? shi : m);         // the last row with a candidate of its own
  LcKey carry = { 0, 0 };
  u64 best[LC_PER];
  LC_LANES_BEGIN (void) l; best[li] = 0; LC_LANES_END
  LcColumn col = { LC_NO_ROW, 0, 0, 0, 0 };
  for (u32 base = r0; base <= m; base += LC_CHUNK) {
    if (base > last_h && carry.key - (int) base * sc.gap <= 0) break;
    LcKey k[LC_PER];
    bool pos[LC_PER];
    LC_LANES_BEGIN
      const u32 i = base + l;
      k[li] = LcKey{ 0, 0 };
      if (i <= last_h) {
        const bool same = q[i - 1] == c;
        if (first) k[li] = lc_first_candidate(same, i, sc);
        else {
          const u32 pd = i - 1 >= slo && i - 1 < shi ? src[i - 1 - slo] : 0;
          const u32 pi = i < shi ? src[i - slo] : 0;
          k[li] = lc_candidate(pd, pi, same, i, sc);
        }
      }
    LC_LANES_END
    lc_scan(k);
    LC_LANES_BEGIN
      const u32 i = base + l;
      k[li] = lc_combine(carry, k[li]);
      const int v = k[li].key - (int) i * sc.gap;
      pos[li] = i <= m && k[li].key > 0 && v > 0;
      if (i <= m) dst[i - r0] = pos[li] ? (u32) v << 16 | k[li].start : 0;
      if (pos[li]) {
        const u64 mine = (u64) v << 32 | (u64) (0xffffu - i) << 16 | k[li].start;   // larger: a larger cell, then a smaller row
        if (mine > best[li]) best[li] = mine;
      }
    LC_LANES_END
    carry = lc_last(k);
    const u64 mask = lc_ballot(pos);
    if (mask) {
      if (col.lo == LC_NO_ROW) col.lo = base + (u32) __builtin_ctzll(mask);
      col.hi = base + 64 - (u32) __builtin_clzll(mask);
    }
  }
  LC_WAVE_FENCE();
  const u64 top = lc_max(best);
  if (top) {
    col.M = (u32) (top >> 32);
    col.e = 0xffffu - (u32) (top >> 16 & 0xffffu);
    col.qstart = (u32) (top & 0xffffu);
  }
  return col;
}

// where the cells of [col.lo, col.hi) begin in a dst that lc_column filled from row r0 on
LC_HD u32 lc_band_offset(const LcColumn &col, bool first, u32 slo) { return col.lo - (first ? 1 : slo); }

struct LcMatch { u32 dblen, score, e, qstart; };             // dblen 0: none

// Suffix p, whose first `depth` symbols gave the column `cur` in src (depth 0:
// none yet), goes on alone in the text until a column reaches T, dies, or a
// special, the end or lc_max_depth stops it.  a and b: two buffers of m cells
// each, neither of them src.  The whole wave calls this with the same arguments.
LC_HD LcMatch lc_walk(const u32 *src, LcColumn cur, u32 depth, const u8 *enc, u64 n, u64 p, const u8 *q, u32 m,
                      LcScores sc, u32 T, u32 *a, u32 *b) {
  const u32 deepest = lc_max_depth(m, sc);
  while (depth < deepest && p + depth < n) {
    const u32 c = LC_UNI((u32) enc[p + depth]);
    if (c >= IV_WILDCARD) break;
    const bool first = depth == 0;
    const LcColumn next = lc_column(src, cur.lo, cur.hi, first, c, q, m, sc, a);
    depth += 1;
    if (next.M >= T) return LcMatch{ depth, next.M, next.e, next.qstart };
    if (next.M == 0) break;
    src = a + lc_band_offset(next, first, cur.lo);
    cur = next;
    u32 *t = a; a = b; b = t;
  }
  return LcMatch{ 0, 0, 0, 0 };
}

// ---- the statement with stored traces, one lane, for the tests ---------------------
enum { LC_TRACE_NONE = 0, LC_TRACE_INSERT = 1, LC_TRACE_REPLACE = 2, LC_TRACE_DELETE = 3 };

// column d as include/gtamd_locali.h states it: out[0..m] scores, trace[0..m];
// in: column d - 1, or nullptr for d = 1
LC_HD void lc_plain_column(const int *in, u32 c, const u8 *q, u32 m, LcScores sc, int *out, u8 *trace) {
  out[0] = -1;
  trace[0] = LC_TRACE_NONE;
  for (u32 i = 1; i <= m; i++) {
    const int r = q[i - 1] == c ? sc.match : sc.mismatch;
    int v = -1;
    u8 t = LC_TRACE_NONE;
    if (out[i - 1] > 0 && out[i - 1] - sc.gap > v) { v = out[i - 1] - sc.gap; t = LC_TRACE_DELETE; }
    if (in == nullptr) {
      if (r > v) { v = r; t = LC_TRACE_REPLACE; }
      if (-sc.gap > v) { v = -sc.gap; t = LC_TRACE_INSERT; }
    } else {
      if (in[i - 1] > 0 && in[i - 1] + r > v) { v = in[i - 1] + r; t = LC_TRACE_REPLACE; }
      if (in[i] > 0 && in[i] - sc.gap > v) { v = in[i] - sc.gap; t = LC_TRACE_INSERT; }
    }
    out[i] = v;
    trace[i] = t;
  }
}

// traces: column d at trace + (d - 1) * (m + 1), d = 1 .. dblen; from (e, dblen)
// until d is 0: the row left over; LC_NO_ROW for a cell without a trace
LC_HD u32 lc_traceback(const u8 *traces, u32 m, u32 dblen, u32 e) {
  u32 d = dblen, i = e;
  while (d > 0) {
    switch (traces[(u64) (d - 1) * (m + 1) + i]) {
      case LC_TRACE_INSERT: d -= 1; break;
      case LC_TRACE_REPLACE: d -= 1; i -= 1; break;
      case LC_TRACE_DELETE: i -= 1; break;
      default: return LC_NO_ROW;
    }
  }
  return i;
}
