// esa_pckidx_dec.h -- the decoded form of the packed index as the kernels see it,
// and what one lane asks of it: rank, rank pair, BWT symbol, locate (the form and
// the semantics: include/gtamd_pckidx.h).  esa_pckidx.hip decodes into it and
// searches it for matstat and uniquesub; esa_tagmatch.hip and esa_locali.hip walk
// it depth first (include/gtamd_pcktag.h, include/gtamd_pcklocali.h), through
// esa_jobs.h, which has the step of such a walk that needs the window of records.
// Only .hip files include this.
#pragma once
#include "esa_common.h"
#include "esa_pckidx_core.h"

constexpr u32 LINE_ROWS = 192;           // 2-bit lines: 4 counters + 12 words of 16 rows
constexpr u32 LINE_WORDS = 16;
constexpr u32 CP_ROWS = 64;              // byte rows: a counter row every 64 rows

// the decoded form as the kernels see it
struct PkxDec {
  u64 N, rot0, first_special_row, nmarks;
  u32 sigma, two_bit, locint, reversible;
  u32 *lines, *flags;          // two_bit: N / 192 + 1 lines; one flag bit per line
  u8 *sym; u32 *cp;            // else: N rows (padded to whole 64), (N / 64 + 1) x sigma counters
  u32 *count;                  // sigma + 1: letters smaller than s in the text
  u64 *mk; u32 *mkpre, *mkpos; // marked rows, marks before each word (+ the total), stored numbers
  u32 *sprank;                 // stored rank of every special row, in row order
  u32 *totals;                 // sigma: what the decode counted
  PkxRegions rg;
};

struct gtamd_pckidx;
// the decoded form of a reader with an open image (esa_pckidx.hip); it holds
// device pointers of the reader, which the next open of the reader replaces
const PkxDec &pckidx_dec(const gtamd_pckidx *px);

namespace {

__device__ __forceinline__ void dev_fail(u32 *err, u32 code) { if (code) atomicCAS(err, 0u, code); }

// special rows in [a, b)
__device__ inline u32 specials_between(const PkxRegions &rg, u64 a, u64 b) {
  u32 c = 0;
  for (u32 ri = pkx_region_from(rg, a); ri < rg.n && rg.start[ri] < b; ri++) {
    const u64 s = rg.start[ri] > a ? rg.start[ri] : a, e = pkx_region_end(rg, ri) < b ? pkx_region_end(rg, ri) : b;
    c += (u32) (e - s);
  }
  return c;
}
// 254 / 255 if row lies in a region, else `letter`
__device__ inline u32 special_or(const PkxRegions &rg, u64 row, u32 letter) {
  const u32 ri = pkx_region_from(rg, row);
  return ri < rg.n && rg.start[ri] <= row ? 254u + rg.sym[ri] : letter;
}

// ---- 2-bit lines -----------------------------------------------------------------
struct Line { uint4 v[4]; };
__device__ __forceinline__ Line load_line(const PkxDec &d, u32 line) {
  const uint4 *p = reinterpret_cast<const uint4 *>(d.lines + (u64) line * LINE_WORDS);
  Line l;
#pragma unroll
  for (int k = 0; k < 4; k++) l.v[k] = p[k];
  return l;
}
__device__ __forceinline__ u32 line_word(const Line &l, int k) {     // k: compile-time after unrolling
  const uint4 &v = l.v[k >> 2];
  return (k & 3) == 0 ? v.x : (k & 3) == 1 ? v.y : (k & 3) == 2 ? v.z : v.w;
}
// counter of letter s plus its occurrences among the first o rows of the line
__device__ __forceinline__ u32 line_rank(const Line &l, u32 s, u32 o) {
  u32 c = s == 0 ? l.v[0].x : s == 1 ? l.v[0].y : s == 2 ? l.v[0].z : l.v[0].w;
  const u32 pat = s * 0x55555555u;
#pragma unroll
  for (int k = 0; k < 12; k++) {
    const u32 have = o > 16u * k ? o - 16u * k : 0u;
    const u32 mask = have >= 16 ? 0x55555555u : ((1u << (2 * have)) - 1u) & 0x55555555u;
    const u32 x = line_word(l, 4 + k) ^ pat;
    c += (u32) __popc(~(x | (x >> 1)) & mask);
  }
  return c;
}
__device__ __forceinline__ bool line_flagged(const PkxDec &d, u32 line) { return (d.flags[line >> 5] >> (line & 31)) & 1u; }

// ---- byte rows -------------------------------------------------------------------
// 0x80 in every byte of x that is zero
__device__ __forceinline__ u32 zero_bytes32(u32 x) { return ~(((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x | 0x7f7f7f7fu); }
__device__ __forceinline__ u32 bytes_rank(const PkxDec &d, u32 s, u64 row) {
  const u64 blk = row / CP_ROWS;
  const u32 o = (u32) (row % CP_ROWS);
  u32 c = d.cp[blk * d.sigma + s];
  const uint4 *p = reinterpret_cast<const uint4 *>(d.sym + blk * CP_ROWS);
  const u32 pat = s * 0x01010101u;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    if (o <= 16u * k) break;
    const uint4 v = p[k];
    const u32 w[4] = { v.x, v.y, v.z, v.w };
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const u32 at = 16u * k + 4u * j, have = o > at ? o - at : 0u;
      const u32 mask = have >= 4 ? 0x80808080u : have ? 0x80808080u >> (8 * (4 - have)) : 0u;
      c += (u32) __popc(zero_bytes32(w[j] ^ pat) & mask);
    }
  }
  return c;
}

// occurrences of letter s < sigma in rows [0, row), row <= N
__device__ __forceinline__ u32 dec_rank(const PkxDec &d, u32 s, u64 row) {
  if (!d.two_bit) return bytes_rank(d, s, row);
  const u32 line = (u32) (row / LINE_ROWS), o = (u32) (row % LINE_ROWS);
  u32 c = line_rank(load_line(d, line), s, o);
  if (s == 0 && o && line_flagged(d, line)) c -= specials_between(d.rg, (u64) line * LINE_ROWS, row);
  return c;
}
// both bounds of an interval, from one line load when they share the line
__device__ __forceinline__ void dec_rank_pair(const PkxDec &d, u32 s, u64 lo, u64 hi, u32 *a, u32 *b) {
  if (!d.two_bit) { *a = bytes_rank(d, s, lo); *b = bytes_rank(d, s, hi); return; }
  const u32 la = (u32) (lo / LINE_ROWS), lb = (u32) (hi / LINE_ROWS);
  if (la != lb) { *a = dec_rank(d, s, lo); *b = dec_rank(d, s, hi); return; }
  const Line l = load_line(d, la);
  const u32 oa = (u32) (lo % LINE_ROWS), ob = (u32) (hi % LINE_ROWS);
  u32 ca = line_rank(l, s, oa), cb = line_rank(l, s, ob);
  if (s == 0 && line_flagged(d, la)) {
    const u64 r0 = (u64) la * LINE_ROWS;
    ca -= specials_between(d.rg, r0, lo);
    cb -= specials_between(d.rg, r0, hi);
  }
  *a = ca; *b = cb;
}
// The rank part of the children step of a walk over intervals of rows, one letter
// a lane: lane c of `todo`, c < sigma and c < letters, gets the rows [*clo, *chi)
// of the child of letter c of the interval [lo, hi) -- one rank pair, all lanes in
// the same one or two lines.  True where the child is not empty; an empty child,
// and every other lane, has *clo == *chi.  count: count[] of the index.  Bounds
// that are none (the decoded form is inconsistent) leave the error word and an
// empty child.
__device__ __forceinline__ bool dec_children(const PkxDec &d, const u32 *count, u32 lo, u32 hi, u32 letters, u32 todo,
                                             u32 lane, u32 *clo, u32 *chi, u32 *err) {
  *clo = *chi = 0;
  if (lane < d.sigma && lane < letters && ((todo >> lane) & 1u)) {
    u32 a, b;
    dec_rank_pair(d, lane, lo, hi, &a, &b);
    const u64 l = (u64) count[lane] + a, h = (u64) count[lane] + b;
    if (l > h || h > d.N) dev_fail(err, PKX_E_WALK);
    else if (l < h) {
      *clo = (u32) l; *chi = (u32) h;
      return true;
    }
  }
  return false;
}
// BWT symbol of row < N: 0..sigma-1, 254, 255
__device__ __forceinline__ u32 dec_symbol(const PkxDec &d, u64 row) {
  if (!d.two_bit) return d.sym[row];
  const u32 line = (u32) (row / LINE_ROWS), o = (u32) (row % LINE_ROWS);
  const u32 c = (d.lines[(u64) line * LINE_WORDS + 4 + o / 16] >> (2 * (o % 16))) & 3u;
  return c == 0 && line_flagged(d, line) ? special_or(d.rg, row, 0) : c;
}

// gt_BWTSeqLocateMatch: text position of the suffix of row < N
__device__ inline u64 dec_locate(const PkxDec &d, u64 row, u32 *err) {
  for (u32 steps = 0;; steps++) {
    const u64 w = d.mk[row >> 6];
    const u32 bit = (u32) (row & 63);
    if ((w >> bit) & 1) {
      const u32 idx = d.mkpre[row >> 6] + (u32) __popcll(w & ((1ull << bit) - 1));
      return (u64) d.mkpos[idx] * (d.reversible ? d.locint : 1u) + steps;
    }
    // (every locint-th text position is marked)
    if (steps >= d.locint) { dev_fail(err, PKX_E_WALK); return 0; }
    const u32 c = dec_symbol(d, row);
    if (c >= 254) {
      if (!d.reversible) { dev_fail(err, PKX_E_WALK); return 0; }
      const u32 ri = pkx_region_from(d.rg, row);
      row = d.first_special_row + d.sprank[d.rg.pre[ri] + (u32) (row - d.rg.start[ri])];
    } else
      row = (u64) d.count[c] + dec_rank(d, c, row);
    if (row >= d.N) { dev_fail(err, PKX_E_WALK); return 0; }
  }
}

// ---- the row steps of a walk over intervals of rows --------------------------------
// dbstart of the match of `len` letters found at `row`: the suffix of the row
// begins with them, last letter first (gen_pck_overinterval, pck_overcontext)
__device__ __forceinline__ u64 dec_dbstart(const PkxDec &d, u32 row, u32 len, u32 *err) {
  const u64 end = dec_locate(d, row, err) + len;
  if (end > d.N - 1) { dev_fail(err, PKX_E_WALK); return 0; }
  return d.N - 1 - end;
}

// count[0 .. sigma] of the index to `count`, the LDS of a wave; sigma, which is
// returned: the letters of the index, at most `letters`
__device__ __forceinline__ u32 dec_count_to_lds(const PkxDec &d, u32 *count, u32 letters) {
  const u32 sigma = d.sigma < letters ? d.sigma : letters;
  for (u32 c = 0; c <= sigma; c++) count[c] = d.count[c];       // (every lane the same word)
  return sigma;
}

// the `todo` of dec_children for a level that has not been expanded yet
__device__ __forceinline__ u32 dec_all_letters(u32 sigma) { return sigma >= 32 ? ~0u : (1u << sigma) - 1u; }

}  // namespace
