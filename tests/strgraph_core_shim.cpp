// Test shim (CPU): what one lane of the string-graph kernels does
// (genometools_amd/csrc/esa_strgraph_core.h), run lane after lane in the steps of
// genometools_amd/csrc/esa_strgraph.hip: every round of the pointer doubling
// reads one buffer and writes the other, as the kernels do.  The sort is
// std::stable_sort, the scans are loops.
#include <algorithm>
#include <vector>
#include "../genometools_amd/csrc/esa_strgraph_core.h"

extern "C" {

void sg_shim_edge(const uint64_t *rec, uint32_t second, uint32_t *from, uint32_t *to) {
  const SgRecord m = { rec[0], rec[1], rec[2], rec[3] };
  sg_edge(m, second, from, to);
}

int sg_shim_kind(uint32_t outdeg, uint32_t indeg) { return sg_kind(outdeg, indeg); }
int sg_shim_junction(uint32_t outdeg, uint32_t indeg) { return sg_junction(outdeg, indeg); }

// a and b: nxt, hops, sum, low, last
void sg_shim_rank_step(const uint32_t *a, const uint32_t *b, uint32_t *out) {
  const SgRank r = sg_rank_step(SgRank{ a[0], a[1], a[2], a[3], a[4] }, SgRank{ b[0], b[1], b[2], b[3], b[4] });
  out[0] = r.nxt; out[1] = r.hops; out[2] = r.sum; out[3] = r.low; out[4] = r.last;
}

int sg_shim_written(uint32_t i, uint32_t j, uint32_t t, uint32_t jm) { return sg_written(i, j, t, jm); }
int sg_shim_single_written(uint32_t i, uint32_t t) { return sg_single_written(i, t); }
int sg_shim_cycle_written(uint32_t low, uint32_t low_mirror) { return sg_cycle_written(low, low_mirror); }
int sg_shim_kept(uint64_t depth, uint64_t length, uint32_t d, uint32_t c) { return sg_kept(depth, length, d, c); }
uint64_t sg_shim_element_of(const uint64_t *start, uint64_t a, uint64_t b, uint64_t s) { return sg_element_of(start, a, b, s); }

// The whole of steps 1 to 7.  contigs: five numbers a kept contig, symbols: all
// of them; figures: contigs, elements, symbols, rounds of the first ranking, of
// the second, written paths, written cycles, internal vertices, edges.  Returns
// the number of contigs, -1 for records outside the read set, -2 for an output
// that is too small.
int64_t sg_shim_run(const uint8_t *enc, uint64_t n, const uint64_t *recs, uint64_t Z, uint32_t L, uint32_t depthcutoff,
                    uint32_t lengthcutoff, uint64_t *contigs, uint64_t max_contigs, uint8_t *symbols, uint64_t max_symbols,
                    uint64_t *figures) {
  // 1
  std::vector<u32> seps;
  for (u64 i = 0; i < n; i++) if (enc[i] == 255) seps.push_back((u32) i);
  const u32 R = n ? (u32) seps.size() + 1 : 0, NV = 2 * R;
  std::vector<u32> rstart(R), rlen(R);
  for (u32 r = 0; r < R; r++) {
    rstart[r] = r ? seps[r - 1] + 1 : 0;
    rlen[r] = (r < seps.size() ? seps[r] : (u32) n) - rstart[r];
  }
  // 2
  const SgRecord *rec = reinterpret_cast<const SgRecord *>(recs);
  const u32 E = (u32) (2 * Z);
  std::vector<u32> key(E), val(E);
  for (u32 e = 0; e < E; e++) {
    bool bad;
    u32 from = NV, to;
    if (sg_record_counts(rec[e >> 1], rlen.data(), R, L, &bad)) sg_edge(rec[e >> 1], e & 1, &from, &to);
    if (bad) return -1;
    key[e] = from;
    val[e] = e;
  }
  std::stable_sort(val.begin(), val.end(), [&](u32 a, u32 b) { return key[a] < key[b]; });
  std::vector<u32> skey(E), edst(E), elen(E), pos(E), voff(NV + 1);
  for (u32 p = 0; p < E; p++) skey[p] = key[val[p]];
  for (u32 p = 0; p < E; p++) {
    const u32 e = val[p];
    pos[e] = p;
    u32 from, to = 0, len = 0;
    if (skey[p] < NV) {
      sg_edge(rec[e >> 1], e & 1, &from, &to);
      len = sg_edge_length(rec[e >> 1], rlen.data(), to);
    }
    edst[p] = to;
    elen[p] = len;
  }
  for (u32 v = 0; v <= NV; v++) voff[v] = sg_first_edge(skey.data(), E, v);
  const u32 Ev = voff[NV];
  // 3
  std::vector<u8> kind(NV + 1);
  u64 internal = 0;
  for (u32 v = 0; v < NV; v++) {
    kind[v] = sg_kind(voff[v + 1] - voff[v], voff[(v ^ 1) + 1] - voff[v ^ 1]);
    internal += kind[v] == SG_INTERNAL;
  }
  // 4
  std::vector<SgRank> a(NV + 1), b(NV + 1);
  for (u32 v = 0; v < NV; v++) {
    const bool ranked = kind[v] == SG_INTERNAL;
    a[v] = sg_rank_start(v, ranked, ranked ? edst[voff[v]] : 0, ranked ? elen[voff[v]] : 0);
  }
  auto rounds_of = [&](bool cycles, u64 most, u64 *left) {
    u32 limit = 1, rounds = 0;
    while ((1ull << (limit - 1)) < most) limit++;
    for (u32 r = 0; r < limit; r++) {
      *left = 0;
      for (u32 v = 0; v < NV; v++) {
        SgRank x = a[v];
        const u8 k = kind[v];
        if (cycles ? (k == SG_CYCLE || k == SG_LEADER) : k >= SG_INTERNAL) {
          const u8 ahead = kind[x.nxt];
          if (cycles ? ahead != SG_LEADER : ahead >= SG_INTERNAL) {
            x = sg_rank_step(x, a[x.nxt]);
            const u8 then = kind[x.nxt];
            *left += cycles ? then != SG_LEADER : then >= SG_INTERNAL;
          }
        }
        b[v] = x;
      }
      a.swap(b);
      rounds++;
      if (*left == 0) break;
    }
    return rounds;
  };
  u64 left = 0, cycles_written = 0;
  u32 rounds = 0, cycle_rounds = 0;
  if (internal) {
    rounds = rounds_of(false, NV, &left);
    if (left) {
      std::vector<u8> then(kind);
      for (u32 v = 0; v < NV; v++) {
        SgRank x = a[v];
        if (kind[v] == SG_INTERNAL && kind[x.nxt] >= SG_INTERNAL) {
          if (sg_cycle_written(x.low, a[v ^ 1].low)) {
            then[v] = x.low == v ? SG_LEADER : SG_CYCLE;
            cycles_written += x.low == v;
            const u32 low = x.low;
            x = sg_rank_start(v, true, edst[voff[v]], elen[voff[v]]);
            x.low = low;
          } else then[v] = SG_MIRROR_CYCLE;
        }
        b[v] = x;
      }
      kind = then;
      a.swap(b);
      cycle_rounds = rounds_of(true, left, &left);
    }
  }
  // 5
  const SgGraph g = { skey.data(), val.data(), pos.data(), edst.data(), elen.data(), voff.data(), kind.data(), a.data(),
                      rlen.data(), NV, Ev };
  std::vector<u32> flag(2 * (u64) Ev + 1, 0);
  u64 paths = 0;
  for (u32 p = 0; p < Ev; p++) {
    SgPath o;
    const bool written = sg_path(g, p, &o);
    const bool kept = written && sg_kept(o.depth, o.length, depthcutoff, lengthcutoff);
    paths += written && !o.cycle;
    flag[p] = kept && !o.cycle;
    flag[Ev + p] = kept && o.cycle;
  }
  std::vector<u64> foff(2 * (u64) Ev + 1, 0);
  for (u64 f = 0; f < 2 * (u64) Ev; f++) foff[f + 1] = foff[f] + flag[f];
  const u64 C = foff[2 * (u64) Ev];
  std::vector<u32> cstart(C), cdepth(C), clen(C);
  for (u64 f = 0; f < 2 * (u64) Ev; f++)
    if (flag[f]) {
      SgPath o;
      const u32 p = (u32) (f < Ev ? f : f - Ev);
      sg_path(g, p, &o);
      cstart[foff[f]] = p; cdepth[foff[f]] = o.depth; clen[foff[f]] = (u32) o.length;
    }
  std::vector<u64> eoff(C + 1, 0), soff(C + 1, 0);
  for (u64 c = 0; c < C; c++) { eoff[c + 1] = eoff[c] + cdepth[c]; soff[c + 1] = soff[c] + clen[c]; }
  const u64 T = eoff[C], S = soff[C];
  // 6
  std::vector<u32> el_v(T, SG_NONE);
  std::vector<u64> el_s(T + 1, ~0ull);
  if (C > max_contigs || S > max_symbols) return -2;
  for (u64 c = 0; c < C; c++) {
    SgPath o;
    sg_path(g, cstart[c], &o);
    const u64 row[5] = { o.length, o.depth, o.first, o.last, soff[c] };
    std::copy(row, row + 5, contigs + 5 * c);
    el_v[eoff[c]] = o.first; el_s[eoff[c]] = soff[c];
    el_v[eoff[c] + o.depth - 1] = o.last; el_s[eoff[c] + o.depth - 1] = soff[c] + o.length - o.last_len;
    if (c == C - 1) el_s[eoff[c] + o.depth] = soff[c] + o.length;
  }
  for (u32 v = 0; v < NV; v++) {
    u32 f, index, tail, letters;
    if (!sg_element(g, v, &f, &index, &tail, &letters) || !flag[f]) continue;
    const u64 c = foff[f];
    el_v[eoff[c] + index] = v;
    el_s[eoff[c] + index] = soff[c] + clen[c] - tail - letters;
  }
  for (u64 e = 0; e < T; e++) if (el_v[e] == SG_NONE || el_s[e] > el_s[e + 1]) return -3;      // every element was written once
  // 7
  for (u64 s = 0; s < S; s++)
    symbols[s] = sg_symbol(enc, rstart.data(), rlen.data(), el_v.data(), el_s.data(), sg_element_of(el_s.data(), 0, T, s), s);
  const u64 fig[9] = { C, T, S, rounds, cycle_rounds, paths, cycles_written, internal, Ev };
  std::copy(fig, fig + 9, figures);
  return (int64_t) C;
}

}
