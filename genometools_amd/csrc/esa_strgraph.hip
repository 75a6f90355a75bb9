// esa_strgraph.hip -- the contigs of a read set from its irreducible
// suffix-prefix matches on the device: `gt readjoiner assembly` with default
// options (C ABI, the semantics and the algorithm: include/gtamd_strgraph.h;
// DESIGN.md 9o).  What one lane does is in esa_strgraph_core.h.
//
//   1  k_sg_sep_count, offsets_u64_counted (esa_prims), k_sg_sep_write   the separators;
//      k_sg_reads            one lane per read: start and length
//   2  k_sg_slots            one lane per slot, two a record: (source, slot);
//      radix_sort_pairs (esa_prims)      stable, by source
//      k_sg_gather           one lane per sorted slot: destination, length, the way back
//      k_sg_first_edges      one lane per vertex: its first edge
//   3  k_sg_classify         one lane per vertex
//   4  k_sg_rank_init, k_sg_rank_round   pointer doubling; k_sg_cycle_init and
//      k_sg_rank_round again for the written cycles
//   5  k_sg_select           one lane per edge: a kept path starts here;
//      offsets_u64_counted   numbers the contigs; k_sg_contigs, one lane per
//      verdict, gives a kept one its figures; two scans more place elements and symbols
//   6  k_sg_ends             one lane per contig: its record, first and last element
//      k_sg_elements         one lane per vertex: the element it is
//   7  k_sg_spell            one lane per symbol of an emit call
#include "esa_common.h"
#include "esa_index.h"
#include "esa_prims.h"
#include "esa_devutil.h"
#include "esa_strgraph_core.h"
#include "../../include/gtamd_strgraph.h"

static_assert(SG_PREFIX_DIRECT == GTAMD_SPMRED_PREFIX_DIRECT && SG_SUFFIX_DIRECT == GTAMD_SPMRED_SUFFIX_DIRECT,
              "the flags of the lane header are those of the C ABI");
static_assert(sizeof(SgRecord) == sizeof(gtamd_spmred_record) && sizeof(SgContig) == sizeof(gtamd_strgraph_contig),
              "one record");
static_assert(GTAMD_STRGRAPH_DEPTHCUTOFF == 3 && GTAMD_STRGRAPH_LENGTHCUTOFF == 100, "the defaults of the tool");

namespace {

constexpr int SG_THREADS = SC_THREADS;
constexpr u32 SG_TILE = SG_THREADS;                  // lanes of one workgroup: one a record, edge, vertex, contig, symbol
constexpr u32 SG_LANE_SYMS = 16;                     // symbols one lane of step 1 looks at
constexpr u32 SG_SEP_TILE = SG_TILE * SG_LANE_SYMS;  // symbols of one workgroup of step 1
constexpr u64 SG_MIN_CAPACITY = SG_TILE;             // the smallest capacity of an emit call
constexpr u64 SG_MAX_SPELL = 1ull << 28;             // symbols of one launch of step 7
constexpr u64 SG_MAX_SYMBOLS = 1ull << 31, SG_MAX_READS = 1ull << 30, SG_MAX_RECORDS = 1ull << 30;
constexpr u32 SG_MAX_ROUNDS = 34;

enum { W_BAD = 0, W_INTERNAL, W_JUNCTIONS, W_PATHS, W_CYCLES, W_CYCLE_VERTICES, W_LONGEST, W_SEPS, W_CONTIGS,
       W_ELEMENTS, W_SYMBOLS, W_ROUND0, W_WORDS = W_ROUND0 + 2 * SG_MAX_ROUNDS };

// this workgroup's sum of one count a wave into *word
__device__ __forceinline__ void add_ballot(bool flag, u64 *word) {
  const u64 mask = __ballot(flag);
  if ((threadIdx.x & 63) == 0 && mask) atomicAdd((unsigned long long *) word, (unsigned long long) __popcll(mask));
}

// ---- step 1 ----------------------------------------------------------------------
// bit k: symbol i0 + k is a separator
__device__ __forceinline__ u32 sep_mask(const u8 *enc, u64 n, u64 i0) {
  u32 mask = 0;
  if (((uintptr_t) enc & 15) == 0 && i0 + SG_LANE_SYMS <= n) {      // one load of 16 bytes
    const uint4 w = *reinterpret_cast<const uint4 *>(enc + i0);
    const u32 x[4] = { w.x, w.y, w.z, w.w };
#pragma unroll
    for (u32 k = 0; k < SG_LANE_SYMS; k++)
      if (((x[k >> 2] >> (8 * (k & 3))) & 0xff) == 255) mask |= 1u << k;
    return mask;
  }
  for (u32 k = 0; k < SG_LANE_SYMS; k++)
    if (i0 + k < n && enc[i0 + k] == 255) mask |= 1u << k;
  return mask;
}

__global__ __launch_bounds__(SG_THREADS) void k_sg_sep_count(const u8 *enc, u64 n, u32 *cnt) {
  __shared__ u32 lds4[SG_THREADS / 64];
  u32 total;
  const u64 i0 = ((u64) blockIdx.x * SG_TILE + threadIdx.x) * SG_LANE_SYMS;
  block_scan_excl_sum((u32) __popc(sep_mask(enc, n, i0)), &total, lds4);
  if (threadIdx.x == 0) cnt[blockIdx.x] = total;
}

__global__ __launch_bounds__(SG_THREADS) void k_sg_sep_write(const u8 *enc, u64 n, const u64 *off, u32 *seps) {
  __shared__ u32 lds4[SG_THREADS / 64];
  u32 total;
  const u64 i0 = ((u64) blockIdx.x * SG_TILE + threadIdx.x) * SG_LANE_SYMS;
  u32 mask = sep_mask(enc, n, i0);
  u64 at = off[blockIdx.x] + block_scan_excl_sum((u32) __popc(mask), &total, lds4);
  for (; mask; mask &= mask - 1) seps[at++] = (u32) (i0 + (u32) __builtin_ctz(mask));
}

__global__ __launch_bounds__(SG_THREADS) void k_sg_reads(const u32 *seps, u32 nseps, u64 n, u32 R, u32 *rstart, u32 *rlen) {
  const u64 r = (u64) blockIdx.x * SG_TILE + threadIdx.x;
  if (r >= R) return;
  const u32 a = r ? seps[r - 1] + 1 : 0, b = r < nseps ? seps[r] : (u32) n;
  rstart[r] = a;
  rlen[r] = b - a;
}

// ---- step 2 ----------------------------------------------------------------------
__global__ __launch_bounds__(SG_THREADS) void k_sg_slots(const SgRecord *rec, u64 Z, const u32 *rlen, u32 R, u32 L, u32 NV,
                                                         u32 *key, u32 *val, u64 *w) {
  const u64 e = (u64) blockIdx.x * SG_TILE + threadIdx.x;
  bool bad = false;
  if (e < 2 * Z) {
    const SgRecord m = rec[e >> 1];
    u32 from = NV, to;
    if (sg_record_counts(m, rlen, R, L, &bad)) sg_edge(m, (u32) (e & 1), &from, &to);
    key[e] = from;
    val[e] = (u32) e;
    bad = bad && !(e & 1);
  }
  add_ballot(bad, &w[W_BAD]);
}

__global__ __launch_bounds__(SG_THREADS) void k_sg_gather(const SgRecord *rec, const u32 *rlen, const u32 *skey, const u32 *sval,
                                                          u32 E, u32 NV, u32 *edst, u32 *elen, u32 *pos) {
  const u64 p = (u64) blockIdx.x * SG_TILE + threadIdx.x;
  if (p >= E) return;
  const u32 e = sval[p];
  pos[e] = (u32) p;
  u32 from = NV, to = 0, len = 0;
  if (skey[p] < NV) {
    const SgRecord m = rec[e >> 1];
    sg_edge(m, e & 1, &from, &to);
    len = sg_edge_length(m, rlen, to);
  }
  edst[p] = to;
  elen[p] = len;
}

// voff[v] for v = 0 .. NV: voff[NV] = the edges
__global__ __launch_bounds__(SG_THREADS) void k_sg_first_edges(const u32 *skey, u32 E, u32 NV, u32 *voff) {
  const u64 v = (u64) blockIdx.x * SG_TILE + threadIdx.x;
  if (v <= NV) voff[v] = sg_first_edge(skey, E, (u32) v);
}

// ---- step 3 ----------------------------------------------------------------------
__global__ __launch_bounds__(SG_THREADS) void k_sg_classify(const u32 *voff, u32 NV, u8 *kind, u64 *w) {
  const u64 v = (u64) blockIdx.x * SG_TILE + threadIdx.x;
  bool internal = false, junction = false;
  if (v < NV) {
    const u64 o = v ^ 1;
    const u32 outdeg = voff[v + 1] - voff[v], indeg = voff[o + 1] - voff[o];
    const u8 k = sg_kind(outdeg, indeg);
    kind[v] = k;
    internal = k == SG_INTERNAL;
    junction = sg_junction(outdeg, indeg);
  }
  add_ballot(internal, &w[W_INTERNAL]);
  add_ballot(junction, &w[W_JUNCTIONS]);
}

// ---- step 4 ----------------------------------------------------------------------
__global__ __launch_bounds__(SG_THREADS) void k_sg_rank_init(const u8 *kind, const u32 *voff, const u32 *edst, const u32 *elen,
                                                             u32 NV, SgRank *st) {
  const u64 v = (u64) blockIdx.x * SG_TILE + threadIdx.x;
  if (v >= NV) return;
  const bool ranked = kind[v] == SG_INTERNAL;
  const u32 p = voff[v];
  st[v] = sg_rank_start((u32) v, ranked, ranked ? edst[p] : 0, ranked ? elen[p] : 0);
}

// One round.  CYCLES false: the internal vertices, an end is what is not
// internal; true: the vertices of the written cycles, the end is the leader.
// Every other vertex keeps what it has.  *left: vertices that have not reached their end.
template <bool CYCLES>
__global__ __launch_bounds__(SG_THREADS) void k_sg_rank_round(const u8 *kind, const SgRank *in, SgRank *out, u32 NV, u64 *left) {
  const u64 v = (u64) blockIdx.x * SG_TILE + threadIdx.x;
  bool more = false;
  if (v < NV) {
    SgRank a = in[v];
    const u8 k = kind[v];
    if (CYCLES ? (k == SG_CYCLE || k == SG_LEADER) : k >= SG_INTERNAL) {
      const u8 ahead = kind[a.nxt];
      if (CYCLES ? ahead != SG_LEADER : ahead >= SG_INTERNAL) {
        a = sg_rank_step(a, in[a.nxt]);
        const u8 then = kind[a.nxt];
        more = CYCLES ? then != SG_LEADER : then >= SG_INTERNAL;
      }
    }
    out[v] = a;
  }
  add_ballot(more, left);
}

// what the first ranking left on a cycle: of the cycle and its mirror image the
// one with the lowest vertex is written, and ranked again from that vertex
__global__ __launch_bounds__(SG_THREADS) void k_sg_cycle_init(u8 *kind, const SgRank *in, SgRank *out, const u32 *voff,
                                                              const u32 *edst, const u32 *elen, u32 NV, u64 *w) {
  const u64 v = (u64) blockIdx.x * SG_TILE + threadIdx.x;
  bool on_cycle = false, leader = false;
  if (v < NV) {
    SgRank a = in[v];
    // (the kinds of other vertices are read while they change: from internal to one of the cycle kinds, all >= SG_INTERNAL)
    on_cycle = kind[v] == SG_INTERNAL && kind[a.nxt] >= SG_INTERNAL;
    if (on_cycle) {
      const u32 low = a.low;
      if (sg_cycle_written(low, in[v ^ 1].low)) {
        leader = low == v;
        kind[v] = leader ? SG_LEADER : SG_CYCLE;
        const u32 p = voff[v];
        a = sg_rank_start((u32) v, true, edst[p], elen[p]);
        a.low = low;
      } else kind[v] = SG_MIRROR_CYCLE;
    }
    out[v] = a;
  }
  add_ballot(on_cycle, &w[W_CYCLE_VERTICES]);
  add_ballot(leader, &w[W_CYCLES]);
}

// ---- step 5 ----------------------------------------------------------------------
// flag[p]: a kept path that is no cycle starts with edge p; flag[Ev + p]: a kept cycle
__global__ __launch_bounds__(SG_THREADS) void k_sg_select(SgGraph g, u32 depthcutoff, u32 lengthcutoff, u32 *flag, u64 *w) {
  const u64 p = (u64) blockIdx.x * SG_TILE + threadIdx.x;
  bool path = false, cycle = false;
  if (p < g.Ev) {
    SgPath o;
    const bool written = sg_path(g, (u32) p, &o);
    const bool kept = written && sg_kept(o.depth, o.length, depthcutoff, lengthcutoff);
    path = written && !o.cycle;
    cycle = written && o.cycle;
    flag[p] = kept && path;
    flag[g.Ev + p] = kept && cycle;
  }
  add_ballot(path, &w[W_PATHS]);
}

// the kept contigs by number: where they start, their vertices and their letters
__global__ __launch_bounds__(SG_THREADS) void k_sg_contigs(SgGraph g, const u32 *flag, const u64 *foff, u32 *cstart, u32 *cdepth,
                                                           u32 *clen, u64 *w) {
  __shared__ u32 lds4[SG_THREADS / 64];
  const u64 f = (u64) blockIdx.x * SG_TILE + threadIdx.x;
  u32 length = 0, longest;
  if (f < 2ull * g.Ev && flag[f]) {
    SgPath o;
    const u32 p = (u32) (f < g.Ev ? f : f - g.Ev);
    sg_path(g, p, &o);
    const u64 c = foff[f];
    cstart[c] = p;
    cdepth[c] = o.depth;
    clen[c] = length = (u32) o.length;
  }
  block_scan_excl_max(length, &longest, lds4);
  if (threadIdx.x == 0 && longest) atomicMax((unsigned long long *) &w[W_LONGEST], (unsigned long long) longest);
}

// ---- step 6 ----------------------------------------------------------------------
// el_v, el_s: vertex and first symbol of every element, those of a contig side by
// side; el_s has one entry more, the symbols of all
__global__ __launch_bounds__(SG_THREADS) void k_sg_ends(SgGraph g, const u32 *cstart, const u64 *eoff, const u64 *soff, u64 C,
                                                        SgContig *crec, u32 *el_v, u64 *el_s) {
  const u64 c = (u64) blockIdx.x * SG_TILE + threadIdx.x;
  if (c >= C) return;
  SgPath o;
  sg_path(g, cstart[c], &o);
  const u64 e0 = eoff[c], s0 = soff[c];
  crec[c] = SgContig{ o.length, o.depth, o.first, o.last, s0 };
  el_v[e0] = o.first;
  el_s[e0] = s0;
  el_v[e0 + o.depth - 1] = o.last;
  el_s[e0 + o.depth - 1] = s0 + o.length - o.last_len;
  if (c == C - 1) el_s[e0 + o.depth] = s0 + o.length;
}

__global__ __launch_bounds__(SG_THREADS) void k_sg_elements(SgGraph g, const u32 *flag, const u64 *foff, const u64 *eoff,
                                                            const u64 *soff, const u32 *clen, u32 *el_v, u64 *el_s) {
  const u64 v = (u64) blockIdx.x * SG_TILE + threadIdx.x;
  u32 f, index, tail, letters;
  if (v >= g.NV || !sg_element(g, (u32) v, &f, &index, &tail, &letters) || !flag[f]) return;
  const u64 c = foff[f];
  el_v[eoff[c] + index] = (u32) v;
  el_s[eoff[c] + index] = soff[c] + clen[c] - tail - letters;
}

// ---- step 7 ----------------------------------------------------------------------
// symbols [s0, s1) of all to out, SG_TILE a workgroup
__global__ __launch_bounds__(SG_THREADS) void k_sg_spell(const u8 *enc, const u32 *rstart, const u32 *rlen, const u32 *el_v,
                                                         const u64 *el_s, u64 T, u64 s0, u64 s1, u8 *out) {
  __shared__ u64 span[2];                 // the elements of the workgroup's first and last symbol
  const u64 b0 = s0 + (u64) blockIdx.x * SG_TILE;
  const u64 last = (s1 - b0 < SG_TILE ? s1 : b0 + SG_TILE) - 1;
  if (threadIdx.x < 2) span[threadIdx.x] = sg_element_of(el_s, 0, T, threadIdx.x == 0 ? b0 : last);
  __syncthreads();
  const u64 s = b0 + threadIdx.x;
  if (s > last) return;
  out[s - s0] = sg_symbol(enc, rstart, rlen, el_v, el_s, sg_element_of(el_s, span[0], span[1] + 1, s), s);
}

}  // namespace

struct gtamd_strgraph : ConsumerBase<6> {
  bool prepared = false;
  // the inputs: the caller's device memory, or copies of host memory
  Dev<u8> own_enc;
  Dev<SgRecord> own_rec;
  const u8 *enc = nullptr;
  const SgRecord *rec = nullptr;
  u64 n = 0, Z = 0;
  bool reads_set = false;
  // what a prepare leaves for the emit calls
  Dev<u32> sepcnt, seps, rstart, rlen, key_a, key_b, val_a, val_b, sortws, edst, elen, pos, voff, flag, cstart, cdepth, clen,
      el_v;
  Dev<u64> tsum, sepoff, foff, eoff, soff, el_s;
  Dev<u8> kind, out;
  Dev<SgRank> st_a, st_b;
  Dev<SgContig> crec;
  u64 C = 0, T = 0, S = 0;
  gtamd_strgraph_info info = gtamd_strgraph_info();
};

namespace {

const char FEATURE[] = "contigs of the string graph";

u64 held_bytes(const gtamd_strgraph *sg) {
  u64 total = sg->own_enc.bytes + sg->own_rec.bytes + sg->tsum.bytes + sg->sepoff.bytes + sg->foff.bytes + sg->eoff.bytes +
              sg->soff.bytes + sg->el_s.bytes + sg->kind.bytes + sg->out.bytes + sg->st_a.bytes + sg->st_b.bytes +
              sg->crec.bytes + sg->words.bytes;
  for (const Dev<u32> *d : { &sg->sepcnt, &sg->seps, &sg->rstart, &sg->rlen, &sg->key_a, &sg->key_b, &sg->val_a, &sg->val_b,
                             &sg->sortws, &sg->edst, &sg->elen, &sg->pos, &sg->voff, &sg->flag, &sg->cstart, &sg->cdepth,
                             &sg->clen, &sg->el_v })
    total += d->bytes;
  return total;
}

u32 grid(u64 lanes) { return (u32) div_up(lanes ? lanes : 1, SG_TILE); }

// off[0 .. count] of the counts, total to the device word; count >= 1
int scan_counts(gtamd_strgraph *sg, const u32 *cnt, u64 count, Dev<u64> &off, u64 *total_dev, const char *of) {
  if (sg->tsum.grow(div_up(count, 256) * 8) != hipSuccess || off.grow((count + 1) * 8) != hipSuccess)
    return out_of_memory(FEATURE, count, of);
  return offsets_u64_counted(cnt, count, sg->tsum, off, total_dev, sg->st);
}

// the doubling rounds from `from`: the result and the rounds made
template <bool CYCLES>
int rank(gtamd_strgraph *sg, u32 NV, u64 most, SgRank **from, SgRank **to, u32 slot0, u32 *rounds) {
  u32 limit = 1;
  while ((1ull << (limit - 1)) < most) limit++;          // ceil(log2(most)) + 1
  *rounds = 0;
  for (u32 r = 0; r < limit && r < SG_MAX_ROUNDS; r++) {
    u64 *left = sg->words + slot0 + r;
    k_sg_rank_round<CYCLES><<<grid(NV), SG_THREADS, 0, sg->st>>>(sg->kind, *from, *to, NV, left);
    HIP_TRY(hipGetLastError());
    SgRank *t = *from; *from = *to; *to = t;
    ++*rounds;
    u64 h;
    TRY(fetch(sg->st, { { left, &h, sizeof h } }));
    if (h == 0) break;
  }
  return 0;
}

int prepare(gtamd_strgraph *sg, u32 L, u32 depthcutoff, u32 lengthcutoff) {
  hipStream_t st = sg->st;
  const u64 n = sg->n, Z = sg->Z, E = 2 * Z;
  gtamd_strgraph_info &o = sg->info;
  u64 h[W_WORDS];
  HIP_TRY(hipMemsetAsync(sg->words, 0, W_WORDS * sizeof(u64), st));
  HIP_TRY(hipEventRecord(sg->ev[0], st));

  // 1: the reads
  u32 R = 0, nseps = 0;
  if (n != 0) {
    const u64 tiles = div_up(n, SG_SEP_TILE);
    if (sg->sepcnt.grow(tiles * 4) != hipSuccess) return out_of_memory(FEATURE, tiles, "counts of separators");
    k_sg_sep_count<<<(u32) tiles, SG_THREADS, 0, st>>>(sg->enc, n, sg->sepcnt);
    HIP_TRY(hipGetLastError());
    TRY(scan_counts(sg, sg->sepcnt, tiles, sg->sepoff, sg->words + W_SEPS, "counts of separators"));
    TRY(fetch(st, { { sg->words + W_SEPS, &h[W_SEPS], sizeof(u64) } }));
    if (h[W_SEPS] >= SG_MAX_READS) {
      gtamd_set_error("%s: %llu reads are beyond the limit of %llu", FEATURE, (unsigned long long) h[W_SEPS] + 1,
                      (unsigned long long) SG_MAX_READS);
      return -1;
    }
    nseps = (u32) h[W_SEPS];
    R = nseps + 1;
    if (sg->seps.grow((nseps ? (u64) nseps : 1) * 4) != hipSuccess) return out_of_memory(FEATURE, nseps, "separators");
    k_sg_sep_write<<<(u32) tiles, SG_THREADS, 0, st>>>(sg->enc, n, sg->sepoff, sg->seps);
    HIP_TRY(hipGetLastError());
  }
  const u32 NV = 2 * R;
  if (sg->rstart.grow((R ? (u64) R : 1) * 4) != hipSuccess || sg->rlen.grow((R ? (u64) R : 1) * 4) != hipSuccess)
    return out_of_memory(FEATURE, R, "reads");
  if (R != 0) {
    k_sg_reads<<<grid(R), SG_THREADS, 0, st>>>(sg->seps, nseps, n, R, sg->rstart, sg->rlen);
    HIP_TRY(hipGetLastError());
  }

  // 2: the edges
  const u64 e4 = (E ? E : 1) * 4, v1 = (u64) NV + 1;
  if (sg->key_a.grow(e4) != hipSuccess || sg->key_b.grow(e4) != hipSuccess || sg->val_a.grow(e4) != hipSuccess ||
      sg->val_b.grow(e4) != hipSuccess || sg->edst.grow(e4) != hipSuccess || sg->elen.grow(e4) != hipSuccess ||
      sg->pos.grow(e4) != hipSuccess || sg->sortws.grow(radix_workspace_words(E ? E : 1) * sizeof(u32)) != hipSuccess)
    return out_of_memory(FEATURE, E, "edges");
  if (sg->voff.grow(v1 * 4) != hipSuccess || sg->kind.grow(v1) != hipSuccess || sg->st_a.grow(v1 * sizeof(SgRank)) != hipSuccess ||
      sg->st_b.grow(v1 * sizeof(SgRank)) != hipSuccess)
    return out_of_memory(FEATURE, NV, "vertices");
  const u32 *skey = sg->key_a, *sval = sg->val_a;
  if (E != 0) {
    k_sg_slots<<<grid(E), SG_THREADS, 0, st>>>(sg->rec, Z, sg->rlen, R, L, NV, sg->key_a, sg->val_a, sg->words);
    HIP_TRY(hipGetLastError());
    int shifts[4], widths[4], passes = 0;
    for (u64 top = NV; top != 0 && passes < 4; top >>= 8, passes++) {
      shifts[passes] = 8 * passes;
      widths[passes] = 8;
    }
    if (passes != 0)
      TRY(radix_sort_pairs<u32, u32>(sg->key_a, sg->val_a, sg->key_b, sg->val_b, E, shifts, widths, passes, sg->sortws, st,
                                     nullptr, nullptr));
    skey = (passes & 1) ? sg->key_b : sg->key_a;
    sval = (passes & 1) ? sg->val_b : sg->val_a;
    k_sg_gather<<<grid(E), SG_THREADS, 0, st>>>(sg->rec, sg->rlen, skey, sval, (u32) E, NV, sg->edst, sg->elen, sg->pos);
    HIP_TRY(hipGetLastError());
  }
  k_sg_first_edges<<<grid(v1), SG_THREADS, 0, st>>>(skey, (u32) E, NV, sg->voff);
  HIP_TRY(hipGetLastError());
  // 3: the vertices
  k_sg_classify<<<grid(NV), SG_THREADS, 0, st>>>(sg->voff, NV, sg->kind, sg->words);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(sg->ev[1], st));
  u32 Ev = 0;
  TRY(fetch(st, { { sg->words, h, W_ROUND0 * sizeof(u64) }, { sg->voff + NV, &Ev, sizeof Ev } }));
  if (h[W_BAD] != 0) {
    gtamd_set_error("%s: %llu of the %llu matches do not lie inside the read set of %u reads (a read number beyond it, "
                    "flags that are none, or more letters than either read has)", FEATURE, (unsigned long long) h[W_BAD],
                    (unsigned long long) Z, R);
    return -1;
  }

  // 4: the ranking
  SgRank *from = sg->st_a, *to = sg->st_b;
  u32 rounds = 0, cycle_rounds = 0;
  k_sg_rank_init<<<grid(NV), SG_THREADS, 0, st>>>(sg->kind, sg->voff, sg->edst, sg->elen, NV, from);
  HIP_TRY(hipGetLastError());
  if (h[W_INTERNAL] != 0) {
    TRY((rank<false>(sg, NV, NV, &from, &to, W_ROUND0, &rounds)));
    u64 left;
    TRY(fetch(st, { { sg->words + W_ROUND0 + rounds - 1, &left, sizeof left } }));
    if (left != 0) {
      k_sg_cycle_init<<<grid(NV), SG_THREADS, 0, st>>>(sg->kind, from, to, sg->voff, sg->edst, sg->elen, NV, sg->words);
      HIP_TRY(hipGetLastError());
      SgRank *t = from; from = to; to = t;
      TRY((rank<true>(sg, NV, left, &from, &to, W_ROUND0 + SG_MAX_ROUNDS, &cycle_rounds)));
    }
  }
  HIP_TRY(hipEventRecord(sg->ev[2], st));

  // 5: the paths that are written and kept
  const SgGraph g = { skey, sval, sg->pos, sg->edst, sg->elen, sg->voff, sg->kind, from, sg->rlen, NV, Ev };
  u64 C = 0, T = 0, S = 0;
  if (Ev != 0) {
    if (sg->flag.grow(2ull * Ev * 4) != hipSuccess) return out_of_memory(FEATURE, Ev, "verdicts of edges");
    k_sg_select<<<grid(Ev), SG_THREADS, 0, st>>>(g, depthcutoff, lengthcutoff, sg->flag, sg->words);
    HIP_TRY(hipGetLastError());
    TRY(scan_counts(sg, sg->flag, 2ull * Ev, sg->foff, sg->words + W_CONTIGS, "verdicts of edges"));
    TRY(fetch(st, { { sg->words + W_CONTIGS, &C, sizeof C } }));
  }
  if (C != 0) {
    if (sg->cstart.grow(C * 4) != hipSuccess || sg->cdepth.grow(C * 4) != hipSuccess || sg->clen.grow(C * 4) != hipSuccess ||
        sg->crec.grow(C * sizeof(SgContig)) != hipSuccess)
      return out_of_memory(FEATURE, C, "contigs");
    k_sg_contigs<<<grid(2ull * Ev), SG_THREADS, 0, st>>>(g, sg->flag, sg->foff, sg->cstart, sg->cdepth, sg->clen, sg->words);
    HIP_TRY(hipGetLastError());
    TRY(scan_counts(sg, sg->cdepth, C, sg->eoff, sg->words + W_ELEMENTS, "contigs"));
    TRY(scan_counts(sg, sg->clen, C, sg->soff, sg->words + W_SYMBOLS, "contigs"));
    TRY(fetch(st, { { sg->words + W_ELEMENTS, &T, sizeof T }, { sg->words + W_SYMBOLS, &S, sizeof S } }));
  }
  HIP_TRY(hipEventRecord(sg->ev[3], st));

  // 6: the elements
  if (C != 0) {
    if (sg->el_v.grow(T * 4) != hipSuccess || sg->el_s.grow((T + 1) * 8) != hipSuccess)
      return out_of_memory(FEATURE, T, "elements of contigs");
    k_sg_ends<<<grid(C), SG_THREADS, 0, st>>>(g, sg->cstart, sg->eoff, sg->soff, C, sg->crec, sg->el_v, sg->el_s);
    HIP_TRY(hipGetLastError());
    k_sg_elements<<<grid(NV), SG_THREADS, 0, st>>>(g, sg->flag, sg->foff, sg->eoff, sg->soff, sg->clen, sg->el_v, sg->el_s);
    HIP_TRY(hipGetLastError());
  }
  HIP_TRY(hipEventRecord(sg->ev[4], st));
  TRY(fetch(st, { { sg->words, h, W_ROUND0 * sizeof(u64) } }));
  sg->C = C; sg->T = T; sg->S = S;
  o.reads = R;
  o.vertices = NV;
  o.matches = Z;
  o.edges = Ev;
  o.internal_vertices = h[W_INTERNAL];
  o.junctions = h[W_JUNCTIONS];
  o.paths = h[W_PATHS];
  o.cycles = h[W_CYCLES];
  o.cycle_vertices = h[W_CYCLE_VERTICES];
  o.contigs = C;
  o.elements = T;
  o.total_length = S;
  o.longest_contig = h[W_LONGEST];
  o.doubling_rounds = rounds;
  o.cycle_rounds = cycle_rounds;
  HIP_TRY(hipEventElapsedTime(&o.device_ms, sg->ev[0], sg->ev[4]));
  HIP_TRY(hipEventElapsedTime(&o.build_ms, sg->ev[0], sg->ev[1]));
  HIP_TRY(hipEventElapsedTime(&o.rank_ms, sg->ev[1], sg->ev[2]));
  HIP_TRY(hipEventElapsedTime(&o.select_ms, sg->ev[2], sg->ev[3]));
  HIP_TRY(hipEventElapsedTime(&o.scatter_ms, sg->ev[3], sg->ev[4]));
  return 0;
}

int emit_contigs(gtamd_strgraph *sg, u64 *cursor, gtamd_strgraph_contig *out, u64 capacity, int out_on_device, u64 *written) {
  *written = 0;
  const u64 total = sg->C, cur = *cursor;
  TRY(refuse_window(FEATURE, "contigs", cur, total, capacity, SG_MIN_CAPACITY));
  if (cur == total) return 0;
  const u64 count = capacity < total - cur ? capacity : total - cur;
  HIP_TRY(hipMemcpyAsync(out, sg->crec + cur, count * sizeof(SgContig),
                         out_on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, sg->st));
  HIP_TRY(hipStreamSynchronize(sg->st));
  *cursor = cur + count;
  *written = count;
  return 0;
}

int emit_symbols(gtamd_strgraph *sg, u64 *cursor, u8 *out, u64 capacity, int out_on_device, u64 *written) {
  *written = 0;
  const u64 total = sg->S, cur = *cursor;
  TRY(refuse_window(FEATURE, "symbols", cur, total, capacity, SG_MIN_CAPACITY));
  if (cur == total) return 0;
  const u64 count = capacity < total - cur ? capacity : total - cur;
  u8 *dst = out;
  if (!out_on_device) {
    if (sg->out.grow(count) != hipSuccess) return out_of_memory(FEATURE, count, "symbols");
    dst = sg->out;
  }
  HIP_TRY(hipEventRecord(sg->ev[0], sg->st));
  for (u64 done = 0; done < count; done += SG_MAX_SPELL) {
    const u64 chunk = count - done < SG_MAX_SPELL ? count - done : SG_MAX_SPELL;
    k_sg_spell<<<grid(chunk), SG_THREADS, 0, sg->st>>>(sg->enc, sg->rstart, sg->rlen, sg->el_v, sg->el_s, sg->T, cur + done,
                                                       cur + done + chunk, dst + done);
    HIP_TRY(hipGetLastError());
  }
  HIP_TRY(hipEventRecord(sg->ev[5], sg->st));
  TRY(fetch(sg->st, { { dst, out, out_on_device ? 0 : count } }));
  float ms = 0;
  HIP_TRY(hipEventElapsedTime(&ms, sg->ev[0], sg->ev[5]));
  sg->info.spell_ms += ms;
  *cursor = cur + count;
  *written = count;
  return 0;
}

}  // namespace

extern "C" gtamd_strgraph *gtamd_strgraph_create(int device) {
  GTAMD_ABI_BEGIN
  return create_consumer<gtamd_strgraph>(device, W_WORDS, "the string graph");
  GTAMD_ABI_END(nullptr)
}

extern "C" void gtamd_strgraph_destroy(gtamd_strgraph *sg) { destroy_consumer(sg); }

extern "C" void gtamd_strgraph_geometry(uint32_t *tile, uint32_t *separator_tile, uint64_t *min_capacity) {
  if (tile != nullptr) *tile = SG_TILE;
  if (separator_tile != nullptr) *separator_tile = SG_SEP_TILE;
  if (min_capacity != nullptr) *min_capacity = SG_MIN_CAPACITY;
}

extern "C" int gtamd_strgraph_set_reads(gtamd_strgraph *sg, const uint8_t *enc, uint64_t n, int on_device) {
  GTAMD_ABI_BEGIN
  if (sg == nullptr || (enc == nullptr && n)) { gtamd_set_error("invalid argument to gtamd_strgraph_set_reads"); return -1; }
  sg->prepared = sg->reads_set = false;
  if (n >= SG_MAX_SYMBOLS) {
    gtamd_set_error("%s: a read set of %llu symbols is beyond the limit of %llu", FEATURE, (unsigned long long) n,
                    (unsigned long long) SG_MAX_SYMBOLS);
    return -1;
  }
  HIP_TRY(hipSetDevice(sg->device));
  sg->own_enc.reset();
  if (!on_device) TRY(upload(sg->own_enc, enc, n, FEATURE, "the read set"));
  sg->enc = on_device ? enc : (const u8 *) sg->own_enc;
  sg->n = n;
  sg->reads_set = true;
  return 0;
  GTAMD_ABI_END(-1)
}

extern "C" int gtamd_strgraph_set_matches(gtamd_strgraph *sg, const gtamd_spmred_record *rec, uint64_t count, int on_device) {
  GTAMD_ABI_BEGIN
  if (sg == nullptr || (rec == nullptr && count)) { gtamd_set_error("invalid argument to gtamd_strgraph_set_matches"); return -1; }
  sg->prepared = false;
  sg->Z = 0;
  if (count > SG_MAX_RECORDS) {
    gtamd_set_error("%s: a list of %llu matches is beyond the limit of %llu", FEATURE, (unsigned long long) count,
                    (unsigned long long) SG_MAX_RECORDS);
    return -1;
  }
  HIP_TRY(hipSetDevice(sg->device));
  sg->own_rec.reset();
  if (!on_device) TRY(upload(sg->own_rec, rec, count * sizeof(SgRecord), FEATURE, "the list of matches"));
  sg->rec = on_device ? (const SgRecord *) rec : (const SgRecord *) sg->own_rec;
  sg->Z = count;
  return 0;
  GTAMD_ABI_END(-1)
}

extern "C" int gtamd_strgraph_prepare(gtamd_strgraph *sg, uint32_t min_len, uint32_t depthcutoff, uint32_t lengthcutoff,
                                      gtamd_strgraph_info *info) {
  GTAMD_ABI_BEGIN
  if (sg == nullptr) { gtamd_set_error("invalid argument to gtamd_strgraph_prepare"); return -1; }
  sg->prepared = false;
  sg->info = gtamd_strgraph_info();
  sg->C = sg->T = sg->S = 0;
  if (!sg->reads_set) { gtamd_set_error("%s: no read set is set (gtamd_strgraph_set_reads)", FEATURE); return -1; }
  HIP_TRY(hipSetDevice(sg->device));
  TRY(prepare(sg, min_len, depthcutoff, lengthcutoff));
  sg->info.device_bytes = held_bytes(sg);
  sg->prepared = true;
  if (info != nullptr) *info = sg->info;
  return 0;
  GTAMD_ABI_END(-1)
}

static int refuse_emit(const gtamd_strgraph *sg, const void *cursor, const void *written, const void *out, u64 capacity,
                       const char *fn) {
  if (sg == nullptr || cursor == nullptr || written == nullptr || (out == nullptr && capacity)) {
    gtamd_set_error("invalid argument to %s", fn);
    return -1;
  }
  if (!sg->prepared) {
    gtamd_set_error("%s: nothing is prepared (gtamd_strgraph_prepare)", FEATURE);
    return -1;
  }
  return 0;
}

extern "C" int gtamd_strgraph_emit(gtamd_strgraph *sg, uint64_t *cursor, gtamd_strgraph_contig *out, uint64_t capacity,
                                   int out_on_device, uint64_t *written) {
  GTAMD_ABI_BEGIN
  TRY(refuse_emit(sg, cursor, written, out, capacity, "gtamd_strgraph_emit"));
  HIP_TRY(hipSetDevice(sg->device));
  return emit_contigs(sg, cursor, out, capacity, out_on_device, written);
  GTAMD_ABI_END(-1)
}

extern "C" int gtamd_strgraph_emit_symbols(gtamd_strgraph *sg, uint64_t *cursor, uint8_t *out, uint64_t capacity,
                                           int out_on_device, uint64_t *written) {
  GTAMD_ABI_BEGIN
  TRY(refuse_emit(sg, cursor, written, out, capacity, "gtamd_strgraph_emit_symbols"));
  HIP_TRY(hipSetDevice(sg->device));
  TRY(emit_symbols(sg, cursor, out, capacity, out_on_device, written));
  sg->info.device_bytes = held_bytes(sg);
  return 0;
  GTAMD_ABI_END(-1)
}

extern "C" int gtamd_strgraph_get_info(const gtamd_strgraph *sg, gtamd_strgraph_info *info) {
  GTAMD_ABI_BEGIN
  return consumer_info(sg, info, "gtamd_strgraph_get_info");
  GTAMD_ABI_END(-1)
}
