// esa_strgraph_core.h -- what one lane of esa_strgraph.hip does (semantics and
// algorithm: include/gtamd_strgraph.h), apart from the kernels so that a test
// can compile it for the CPU (tests/strgraph_core_shim.cpp) and run the very
// code the lanes run against the brute force without a device: the two edges of
// a match, the kind of a vertex, one step of the pointer doubling, the choice
// between the two orientations of a path, and the symbol of a contig from the
// element that covers it.
#pragma once
#include "esa_mstat_search.h"

constexpr u64 SG_PREFIX_DIRECT = 1, SG_SUFFIX_DIRECT = 2;      // the flags of a gtamd_spmred_record
constexpr u32 SG_NONE = 0xffffffffu;

struct SgRecord { u64 suffix_read, prefix_read, len, flags; };
struct SgContig { u64 length, depth, first, last, offset; };

// vertices of read r, and the one at the other end of the read
MST_HD u32 sg_b(u32 r) { return r << 1; }
MST_HD u32 sg_e(u32 r) { return (r << 1) | 1; }
MST_HD u32 sg_other(u32 v) { return v ^ 1; }

// a record adds edges: it is at least L long, no match of a read with itself,
// and it lies inside the set (*bad: it does not -- a read number beyond the R
// reads, flags that are none, or more letters than either read has)
MST_HD bool sg_record_counts(const SgRecord &m, const u32 *rlen, u64 R, u32 L, bool *bad) {
  *bad = m.suffix_read >= R || m.prefix_read >= R || m.flags > 3 || m.flags == 0 ||
         m.len > rlen[m.suffix_read] || m.len > rlen[m.prefix_read];
  return !*bad && m.len >= L && m.suffix_read != m.prefix_read;
}

// edge `second` (0, 1) of the pair a record adds, in the order they are added:
// the cases of gt_spmproc_strgraph_add; the two are mirror images of each other.
// Its fourth case, both reads reversed, is stated in the reference and asserted
// never to occur there; sg_record_counts refuses such a record (flags 0), so
// three cases are left here.
MST_HD void sg_edge(const SgRecord &m, u32 second, u32 *from, u32 *to) {
  const u32 s = (u32) m.suffix_read, p = (u32) m.prefix_read;
  const bool sd = m.flags & SG_SUFFIX_DIRECT, pd = m.flags & SG_PREFIX_DIRECT;
  if (sd && pd) { *from = second ? sg_b(p) : sg_e(s); *to = second ? sg_b(s) : sg_e(p); }
  else if (sd)  { *from = second ? sg_e(p) : sg_e(s); *to = second ? sg_b(s) : sg_b(p); }
  else          { *from = second ? sg_b(p) : sg_b(s); *to = second ? sg_e(s) : sg_e(p); }
}

// the length of an edge: the letters of the destination read the match leaves
MST_HD u32 sg_edge_length(const SgRecord &m, const u32 *rlen, u32 to) { return rlen[to >> 1] - (u32) m.len; }

// the kind of a vertex from its out-degree and that of the other end.  The
// kinds from SG_INTERNAL on are internal vertices; the last three are given to
// those the first ranking leaves on a cycle.
enum : u8 { SG_ISOLATED = 0, SG_END = 1, SG_INTERNAL = 2, SG_CYCLE = 3, SG_LEADER = 4, SG_MIRROR_CYCLE = 5 };
MST_HD u8 sg_kind(u32 outdeg, u32 indeg) {
  if (outdeg == 1 && indeg == 1) return SG_INTERNAL;
  return outdeg ? SG_END : SG_ISOLATED;
}
// GT_STRGRAPH_V_IS_JUNCTION
MST_HD bool sg_junction(u32 outdeg, u32 indeg) { return (outdeg > 1 && indeg > 0) || (outdeg == 1 && indeg > 1); }

// What the ranking knows of an internal vertex v after k rounds: the vertex
// `hops` edges ahead (at most 2^k), the sum of the lengths of those edges, the
// lowest and the last internal vertex among v and those passed.  A vertex that
// is not ranked holds { itself, 0, 0, SG_NONE, SG_NONE }.
struct SgRank { u32 nxt, hops, sum, low, last; };

MST_HD SgRank sg_rank_start(u32 v, bool ranked, u32 succ, u32 length) {
  return ranked ? SgRank{ succ, 1, length, v, v } : SgRank{ v, 0, 0, SG_NONE, SG_NONE };
}
// one doubling step of a: b is the state of a.nxt, which is itself ranked (a
// vertex whose a.nxt is the end of its path keeps what it has)
MST_HD SgRank sg_rank_step(const SgRank &a, const SgRank &b) {
  return SgRank{ b.nxt, a.hops + b.hops, a.sum + b.sum, a.low < b.low ? a.low : b.low, b.last };
}

// Of a path from (i, j) -- vertex i, its j-th edge -- to the end t, and its
// mirror image from (other(t), jm): this one is written.  A hairpin has i =
// other(t), and j decides.
MST_HD bool sg_written(u32 i, u32 j, u32 t, u32 jm) {
  const u32 im = sg_other(t);
  return i < im || (i == im && j < jm);
}
// a path of one edge from i to t, neither internal: the reference's marks skip it when t was visited before i
MST_HD bool sg_single_written(u32 i, u32 t) { return t > i; }
// of a cycle with lowest vertex low and its mirror image with lowest vertex low_mirror: this one is written
MST_HD bool sg_cycle_written(u32 low, u32 low_mirror) { return low < low_mirror; }

MST_HD bool sg_kept(u64 depth, u64 length, u32 depthcutoff, u32 lengthcutoff) {
  return depth >= depthcutoff && length >= lengthcutoff;
}

// the element that holds symbol s: the last of [a, b) whose first symbol is not
// behind s; start[a] <= s, and start[b] is not read
MST_HD u64 sg_element_of(const u64 *start, u64 a, u64 b, u64 s) {
  while (b - a > 1) {
    const u64 mid = a + (b - a) / 2;
    if (start[mid] <= s) a = mid; else b = mid;
  }
  return a;
}

// Symbol s of the contigs: element e = sg_element_of covers symbols [start[e],
// start[e + 1]) with the LAST letters of the read of vertex vertex[e] as the
// contig reads it: an E vertex the read, a B vertex its reverse complement
// (GT_STRGRAPH_V_MIRROR_SEQNUM).
MST_HD u8 sg_symbol(const u8 *enc, const u32 *rstart, const u32 *rlen, const u32 *vertex, const u64 *start, u64 e, u64 s) {
  const u32 v = vertex[e], r = v >> 1, len = rlen[r];
  const u64 at = len - (start[e + 1] - start[e]) + (s - start[e]);       // in the read as the contig reads it
  if (v & 1) return enc[rstart[r] + at];
  const u8 c = enc[rstart[r] + (len - 1 - at)];
  return c < 4 ? (u8) (3 - c) : c;
}

// ---- the graph as the kernels after the sort see it -----------------------------
// E slots, two a record, sorted by source vertex (stable: the edges of a vertex
// in the order of the list); the Ev slots of records that count come first, the
// others have the key NV.  skey: source, sval: the slot before the sort (record
// * 2 + second), pos: where a slot stands now, edst and elen: destination and
// length, voff[v]: the first edge of vertex v (NV + 1 entries), kind and st:
// what the classification and the rankings leave.
struct SgGraph {
  const u32 *skey, *sval, *pos, *edst, *elen, *voff;
  const u8 *kind;
  const SgRank *st;
  const u32 *rlen;
  u32 NV, Ev;
};

// the first edge of vertex v: lower bound of v among the sorted keys
MST_HD u32 sg_first_edge(const u32 *skey, u32 E, u32 v) {
  u32 lo = 0, hi = E;
  while (lo < hi) {
    const u32 mid = lo + (hi - lo) / 2;
    if (skey[mid] < v) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// where the mirror image of the edge at p stands: the other edge of its record
MST_HD u32 sg_mirror_edge(const SgGraph &g, u32 p) { return g.pos[g.sval[p] ^ 1]; }

struct SgPath { u64 length; u32 first, last, depth, last_len; bool cycle; };

// The path that starts with the edge at p, if one is written from there: a
// cycle from its leader, a single edge between two vertices that are not
// internal, or a chain of internal vertices from the edge that enters it, in
// the orientation that is written.  last_len: the length of its last edge.
MST_HD bool sg_path(const SgGraph &g, u32 p, SgPath *o) {
  const u32 i = g.skey[p], t = g.edst[p];
  const u8 ki = g.kind[i];
  o->first = i;
  if (ki == SG_LEADER) {
    const SgRank a = g.st[i];
    o->cycle = true;
    o->last = i;
    o->depth = a.hops + 1;
    o->length = (u64) g.rlen[i >> 1] + a.sum;
    o->last_len = g.elen[sg_mirror_edge(g, g.voff[sg_other(i)])];
    return true;
  }
  if (ki != SG_END) return false;
  o->cycle = false;
  if (g.kind[t] < SG_INTERNAL) {
    if (!sg_single_written(i, t)) return false;
    o->last = t;
    o->depth = 2;
    o->length = (u64) g.rlen[i >> 1] + g.elen[p];
    o->last_len = g.elen[p];
    return true;
  }
  const SgRank a = g.st[t];                       // t is the first internal vertex of a chain
  const u32 q = g.voff[a.last];                   // the edge that leaves the chain
  if (!sg_written(i, p - g.voff[i], a.nxt, sg_mirror_edge(g, q) - g.voff[sg_other(a.nxt)])) return false;
  o->last = a.nxt;
  o->depth = a.hops + 2;
  o->length = (u64) g.rlen[i >> 1] + g.elen[p] + a.sum;
  o->last_len = g.elen[q];
  return true;
}

// Internal vertex v as an element of a path: *flag = the place of the path's
// verdict (the edge that starts it; cycles stand behind the Ev places of the
// others), *index = its number in the path (the start is 0), *tail = the letters
// of the path behind it, *letters = those it adds.  From the mirror symmetry:
// the ranking of other(v) runs to other(start), so its hops are v's number from
// the start and its last vertex is the other end of the path's first internal one.
MST_HD bool sg_element(const SgGraph &g, u32 v, u32 *flag, u32 *index, u32 *tail, u32 *letters) {
  const u8 k = g.kind[v];
  if (k != SG_INTERNAL && k != SG_CYCLE) return false;
  const SgRank a = g.st[v];
  *tail = a.sum;
  *letters = g.elen[sg_mirror_edge(g, g.voff[sg_other(v)])];
  if (k == SG_CYCLE) {
    *flag = g.Ev + g.voff[a.low];
    *index = g.st[a.low].hops - a.hops;
    return true;
  }
  const SgRank m = g.st[sg_other(v)];
  *flag = sg_mirror_edge(g, g.voff[m.last]);
  *index = m.hops;
  return true;
}
