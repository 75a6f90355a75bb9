// esa_locali.hip -- local alignments of queries against .suf and the sequence in
// device memory: `gt dev idxlocali -th T -esa INDEX -q FILES` (C ABI, the
// semantics and the order: include/gtamd_locali.h).
//
//   0  k_lc_cuts          one lane per table entry, once per index: where the
//                         first CUT_MAX symbols of neighbours differ, and at
//                         which depth; a prepare takes the cuts above its depth q
//   a  k_lc_validate      one lane per query: what is refused; the longest query
//   b  k_lc_walk<false>   one WAVE per job (query, group), the waves of the grid
//                         taking jobs in turn: the depth-first walk over the
//                         intervals of the group, the column of every level of the
//                         path as a band of cells on a stack in global memory
//                         (esa_locali_core.h); the matches of the job are counted
//   c  JobOffsets::scan (esa_jobs) 64-bit exclusive scan of the counts
//   d  k_lc_walk<true>    the same walk for the jobs of a window of records,
//                         which writes those
//
// With a reader of the packed index as the index (gtamd_locali_set_index_pckidx,
// include/gtamd_pcklocali.h) there is no step 0, a job is (query,
// code of q letters), and steps b and d are k_lc_walk_pck: the same walk over
// intervals of rows of the decoded form (esa_pckidx_dec.h), all children of a level
// from one rank pair a letter, the column of each computed by the whole wave.
//
// Working memory: one entry per job, the cuts, and per wave of the grid a stack
// and two columns (three with a packed index).
#include <type_traits>
#include "esa_common.h"
#include "esa_jobs.h"
#include "esa_locali_core.h"
#include "../../include/gtamd_locali.h"
#include "../../include/gtamd_pcklocali.h"

namespace {

constexpr int LC_THREADS = SC_THREADS;
constexpr u32 LC_WAVES = LC_THREADS / 64;          // waves of one workgroup: each walks jobs of its own
constexpr u32 LC_WAVES_PER_CU = 8;                 // waves of the grid per compute unit
constexpr u32 LC_BATCH = IV_BATCH;
static_assert(LC_BATCH == DEC_BATCH, "suffixes of a table, rows of a packed index: as many at once");
constexpr u64 LC_MIN_CAPACITY = LC_BATCH;
constexpr u64 LC_MAX_QUERIES = 1ull << 24;
constexpr u64 LC_MAX_JOBS = 1ull << 31;
constexpr u32 LC_HEADER = 8;                       // words of a level on the stack
constexpr u32 LC_MAX_STACK = 1u << 28;             // words
constexpr u32 LC_CUT_GROUPS = 1u << 16;            // sigma ^ CUT_MAX stays below this ...
constexpr u32 LC_CUT_LIST = 1u << 18;              // ... so a suffix table has fewer cuts than this
constexpr u64 LC_TARGET_JOBS = 1u << 14;           // q is the smallest depth that gives as many jobs
constexpr u32 NO_LEVEL = 0xffffffffu;

enum { W_OTHER = W_WALK_WORDS, W_BAD, W_LONGEST, W_CUTS, W_ERROR, W_WORDS };
enum { BAD_LENGTH = 1, BAD_SCORE = 2, BAD_SYMBOL = 3 };

struct LcRecord { u64 query, dbstart, lenscore, qspan; };
static_assert(sizeof(LcRecord) == sizeof(gtamd_locali_record), "a record is four 64-bit numbers");

template <typename S> struct LcInput {
  IvText<S> text; u32 N;
  const u8 *queries; const u64 *qoff;
  const u32 *gstart; u32 groups;                   // group g: table entries [gstart[g], gstart[g + 1])
  LcScores sc; u32 T;
  u32 stack_words, col_words;                      // of one wave: its stack, then two columns of col_words
};

__device__ __forceinline__ LcRecord lc_record(u64 query, u64 p, u32 dblen, u32 score, u32 e, u32 qstart) {
  return LcRecord{ query, p, (u64) dblen | (u64) score << 32, (u64) qstart | (u64) (e - qstart) << 32 };
}

// the level on top of the stack, in registers; the others as LC_HEADER words each
struct LcLevel { u32 lo, end, cur, blo, bhi, cells, below, depth; };

__device__ __forceinline__ void lc_store(u32 *stack, u32 at, const LcLevel &L, u32 lane) {
  if (lane == 0) {
    stack[at] = L.lo; stack[at + 1] = L.end; stack[at + 2] = L.cur; stack[at + 3] = L.blo;
    stack[at + 4] = L.bhi; stack[at + 5] = L.cells; stack[at + 6] = L.below; stack[at + 7] = L.depth;
  }
  LC_WAVE_FENCE();
}

__device__ __forceinline__ LcLevel lc_load(const u32 *stack, u32 at) {
  return LcLevel{ uni(stack[at]), uni(stack[at + 1]), uni(stack[at + 2]), uni(stack[at + 3]),
                  uni(stack[at + 4]), uni(stack[at + 5]), uni(stack[at + 6]), uni(stack[at + 7]) };
}

// One job.  The stack holds, for every level of the path but the top one, its
// header, and for every level but the root the cells of its band; `at` is where
// the top level's header goes when a level is pushed above it, `free` the first
// word behind its cells.
template <typename S, bool EMIT>
__device__ void lc_job(const LcInput<S> &in, u64 j, u32 *stack, u32 *cola, u32 *colb, u32 *cnt, const u64 *off, u64 w0,
                       u64 w1, LcRecord *out, u64 *w, u32 lane) {
  const u64 query = j / in.groups;
  const u32 g = (u32) (j % in.groups);
  const IvText<S> &text = in.text;
  JobWindow<LcRecord> wk = { 0, 0, 0, nullptr };
  if (EMIT && !wk.open(off, j, w0, w1, out)) return;
  const u64 q0 = in.qoff[query];
  const u32 m = (u32) (in.qoff[query + 1] - q0);          // 1 .. LC_MAX_QUERY (k_lc_validate)
  const u8 *q = in.queries + q0;
  const u32 deepest = lc_max_depth(m, in.sc);
  const u32 glo = uni(in.gstart[g]), ghi = uni(in.gstart[g + 1]);

  LcLevel L = { glo, ghi, glo, 0, 0, 0, NO_LEVEL, 0 };
  u32 at = 0, free = LC_HEADER;
  u32 pushed = 0, children = 0, walks = 0;
  bool other = false;
  // Every round moves the cursor of the top level forward by at least one, pops
  // the level or pushes one of the next depth, which is at most `deepest`: it ends.
  for (;;) {
    if (EMIT && wk.full()) break;
    u32 s = IV_SEPARATOR;
    if (L.cur < L.end) s = uni(iv_symbol(text, L.cur, L.depth));
    if (s >= IV_WILDCARD) {
      // the level is done, or only specials are left in it, behind which no column is defined
      if (L.below == NO_LEVEL) break;
      free = at;
      at = L.below;
      L = lc_load(stack, at);
      continue;
    }
    const u32 cur = L.cur;
    const u32 e = iv_right_bound(text, cur, L.end, L.depth, s);
    L.cur = e;
    children += 1;
    if (L.depth >= deepest) continue;                 // (cannot be: a column that deep has no cell > 0)
    const bool first = L.depth == 0;
    const LcColumn above = { L.blo, L.bhi, 0, 0, 0 };
    const bool room = (u64) free + LC_HEADER + m <= in.stack_words;
    if (e - cur == 1 || !room) {
      // alone in the text, one suffix after the other, in the two columns of the wave
      if (e - cur > 1) other = true;
      for (u32 idx = cur; idx < e; idx++) {
        if (EMIT && wk.full()) break;
        const u64 raw = text.suf[idx];
        const u64 p = (u64) uni((u32) (raw >> 32)) << 32 | uni((u32) raw);
        LcMatch hit = { 0, 0, 0, 0 };
        if (p < text.n) hit = lc_walk(stack + L.cells, above, L.depth, text.enc, text.n, p, q, m, in.sc, in.T, cola, colb);
        wk.give<EMIT>(lane == 0 && hit.dblen != 0, lc_record(query, p, hit.dblen, hit.score, hit.e, hit.qstart));
      }
      walks += e - cur;
      continue;
    }
    u32 *dst = stack + free + LC_HEADER;
    const LcColumn col = lc_column(stack + L.cells, L.blo, L.bhi, first, s, q, m, in.sc, dst);
    if (col.M >= in.T) {
      // all suffixes of the child match with depth + 1 symbols
      for (u32 b = cur; b < e; b += LC_BATCH) {
        if (EMIT && wk.full()) break;
        const u32 idx = b + lane;                     // (e <= N <= 2^32 - 4096: no wrap)
        const u64 p = idx < e ? (u64) text.suf[idx] : text.n;
        wk.give<EMIT>(p < text.n, lc_record(query, p, L.depth + 1, col.M, col.e, col.qstart));
      }
      continue;
    }
    if (col.M == 0) continue;
    lc_store(stack, at, L, lane);
    const u32 cells = free + LC_HEADER + lc_band_offset(col, first, L.blo);
    L = LcLevel{ cur, e, cur, col.lo, col.hi, cells, at, L.depth + 1 };
    at = free;
    free = cells + (col.hi - col.lo);
    pushed += 1;
  }
  if (!EMIT && lane == 0) {
    report(w, cnt, j, wk.k, pushed, children, walks);
    if (other) atomicAdd((unsigned long long *) &w[W_OTHER], 1ull);
  }
}

// Jobs [j0, j1), taken in turn by the waves of the grid, each with its own part
// of `arena`.  EMIT false: cnt[job] = its matches.  EMIT true: records [w0, w1)
// of all are written to out, record w0 first.
template <typename S, bool EMIT>
__global__ __launch_bounds__(LC_THREADS) void k_lc_walk(LcInput<S> in, u64 j0, u64 j1, u32 *cnt, const u64 *off, u64 w0,
                                                        u64 w1, LcRecord *out, u32 *arena, u64 *w) {
  const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const u64 slot = (u64) blockIdx.x * LC_WAVES + wave, slots = (u64) gridDim.x * LC_WAVES;
  u32 *stack = arena + slot * ((u64) in.stack_words + 2ull * in.col_words);
  u32 *cola = stack + in.stack_words, *colb = cola + in.col_words;
  for (u64 j = j0 + slot; j < j1; j += slots)          // (the whole wave: the waves of a workgroup never wait for each other)
    lc_job<S, EMIT>(in, j, stack, cola, colb, cnt, off, w0, w1, out, w, lane);
}

// ---- the same walk over a packed index (include/gtamd_pcklocali.h) ----
// A level is an interval [lo, end) of rows of the decoded form: the rows whose
// suffixes, in the text of the index, begin with the letters taken so far, last
// letter first.  In LcLevel, cur is the set of letters whose children are still
// to be taken when the walk comes back to the level.  A job is (query, code of q
// letters): it walks the path of its code first, then the interval it reaches.
struct LcPkInput {
  PkxDec d;
  const u8 *queries; const u64 *qoff;
  u32 groups, q;                                   // sigma ^ q codes of q letters, the first letter the highest digit
  LcScores sc; u32 T;
  u32 stack_words, col_words;                      // of one wave: its stack, then three columns of col_words
};

// all rows [clo, chi) of a child whose column reached T after dblen letters
template <bool EMIT>
__device__ __forceinline__ void lc_pck_rows(const PkxDec &d, JobWindow<LcRecord> &wk, u64 query, u32 clo, u32 chi,
                                            u32 dblen, const LcColumn &col, u32 lane, u32 *err) {
  dec_rows<EMIT>(d, wk, clo, chi, dblen, lane, err,
                 [=](u64 p) { return lc_record(query, p, dblen, col.M, col.e, col.qstart); });
}

// Row `row` < N, reached by the letter s from a row whose `depth` letters gave the
// column `cur` in src (depth 0: none yet), goes on alone (lc_walk with the text
// read replaced): the next letter is the BWT symbol of the row, the next row its
// LF, both asked for before the column of s is computed.  A special ends it; so
// does the row of suffix 0, whose symbol is one, and lc_max_depth.  *at = the row
// the match was found at.  a and b: two buffers of m cells each, neither of them
// src.  The whole wave calls this with the same arguments.
__device__ __forceinline__ LcMatch lc_walk_pck(const PkxDec &d, const u32 *count, u32 sigma, const u32 *src,
                                               LcColumn cur, u32 depth, u32 s, u32 row, const u8 *q, u32 m,
                                               LcScores sc, u32 T, u32 *a, u32 *b, u32 *at, u32 *err) {
  const u32 deepest = lc_max_depth(m, sc);
  while (depth < deepest) {
    const u32 s2 = uni(dec_symbol(d, row));
    u64 next = d.N;
    if (s2 < sigma) next = (u64) count[s2] + uni(dec_rank(d, s2, row));
    const bool first = depth == 0;
    const LcColumn col = lc_column(src, cur.lo, cur.hi, first, s, q, m, sc, a);
    depth += 1;
    if (col.M >= T) { *at = row; return LcMatch{ depth, col.M, col.e, col.qstart }; }
    if (col.M == 0 || s2 >= sigma) break;
    if (next >= d.N) { dev_fail(err, PKX_E_WALK); break; }
    src = a + lc_band_offset(col, first, cur.lo);
    cur = col;
    u32 *t = a; a = b; b = t;
    s = s2;
    row = (u32) next;
  }
  return LcMatch{ 0, 0, 0, 0 };
}

// the record of a row that went on alone, if it has one: lane 0 locates it, in emit
// and where it falls into the window
template <bool EMIT>
__device__ __forceinline__ void lc_pck_one(const PkxDec &d, JobWindow<LcRecord> &wk, u64 query, const LcMatch &hit,
                                           u32 at, u32 lane, u32 *err) {
  u64 p = 0;
  if (EMIT && lane == 0 && hit.dblen != 0 && wk.k >= wk.first && wk.k < wk.stop) p = dec_dbstart(d, at, hit.dblen, err);
  wk.give<EMIT>(lane == 0 && hit.dblen != 0, lc_record(query, p, hit.dblen, hit.score, hit.e, hit.qstart));
}

// One job.  The columns of the path of the code go in turn to the third column
// of the wave and to its first, the last of them to the third, where it stays as
// the band of the root of the walk; the stack is that of lc_job, with the root's
// header at 0, and the first two columns are those of the rows that go on alone.
template <bool EMIT>
__device__ void lc_job_pck(const LcPkInput &in, const u32 *count, u32 sigma, u64 j, u32 *stack, u32 *cnt,
                           const u64 *off, u64 w0, u64 w1, LcRecord *out, u64 *w, u32 lane) {
  const PkxDec &d = in.d;
  u32 *err = reinterpret_cast<u32 *>(&w[W_ERROR]);
  const u64 query = j / in.groups;
  u32 code = (u32) (j % in.groups);
  JobWindow<LcRecord> wk = { 0, 0, 0, nullptr };
  if (EMIT && !wk.open(off, j, w0, w1, out)) return;
  const u64 q0 = in.qoff[query];
  const u32 m = (u32) (in.qoff[query + 1] - q0);          // 1 .. LC_MAX_QUERY (k_lc_validate)
  const u8 *q = in.queries + q0;
  const u32 deepest = lc_max_depth(m, in.sc);
  u32 *cola = stack + in.stack_words, *colb = cola + in.col_words, *colr = colb + in.col_words;
  const u32 all = dec_all_letters(sigma);
  u32 pushed = 0, children = 0, walks = 0;
  bool other = false;

  // the path of the code: one letter, one rank pair and one column a depth
  u32 lo = 0, hi = (u32) d.N, depth = 0, div = in.groups;
  LcColumn band = { 0, 0, 0, 0, 0 };
  const u32 *src = colr;
  bool live = true;
  for (u32 i = 0; i < in.q && live; i++) {
    div /= sigma;
    const u32 c = code / div;                           // (code < div * sigma: a letter)
    code -= c * div;                                    // the letters behind this one
    live = false;
    if (depth >= deepest) break;                        // (cannot be: a column that deep has no cell > 0)
    u32 ra, rb;
    dec_rank_pair(d, c, lo, hi, &ra, &rb);
    const u64 l = (u64) count[c] + uni(ra), h = (u64) count[c] + uni(rb);
    if (l > h || h > d.N) { dev_fail(err, PKX_E_WALK); break; }
    if (l == h) break;
    children += 1;
    u32 *dst = ((in.q - 1 - i) & 1u) ? cola : colr;
    const bool first = depth == 0;
    const LcColumn col = lc_column(src, band.lo, band.hi, first, c, q, m, in.sc, dst);
    lo = (u32) l; hi = (u32) h; depth += 1;
    if (col.M >= in.T) {
      // every job whose code begins with these letters finds this; the one whose other letters are 0 gives it
      if (code == 0) lc_pck_rows<EMIT>(d, wk, query, lo, hi, depth, col, lane, err);
      break;
    }
    if (col.M == 0) break;
    src = dst + lc_band_offset(col, first, band.lo);
    band = col;
    live = true;
  }

  // (a root of one row needs nothing of its own: the children step gives the one child its LF leads to)
  LcLevel L = { lo, hi, all, band.lo, band.hi, (u32) (src - stack), NO_LEVEL, depth };
  u32 at = 0, free = LC_HEADER;
  // Every round expands the top level for the letters left in it, which are fewer
  // each time, and ends with a push to the next depth, which is at most `deepest`,
  // or with a pop: the walk ends.
  while (live) {
    if (EMIT && wk.full()) break;
    u32 my_lo = 0, my_hi = 0;
    bool nonempty = false;
    if (L.cur != 0 && L.depth < deepest)
      nonempty = dec_children(d, count, L.lo, L.end, LC_LETTERS, L.cur, lane, &my_lo, &my_hi, err);
    u32 work = (u32) __ballot(nonempty);                   // (letters are lanes 0 .. 31)
    if (L.cur == all) children += (u32) __popc(work);
    const bool first = L.depth == 0;
    const LcColumn above = { L.blo, L.bhi, 0, 0, 0 };
    bool down = false;
    while (work && !(EMIT && wk.full())) {
      const u32 c = uni((u32) __builtin_ctz(work));
      work &= work - 1;
      const u32 clo = __builtin_amdgcn_readlane(my_lo, c), chi = __builtin_amdgcn_readlane(my_hi, c);
      const bool room = (u64) free + LC_HEADER + m <= in.stack_words;
      if (chi - clo == 1 || !room) {
        // alone, one row after the other, in the two columns of the wave
        if (chi - clo > 1) other = true;
        for (u32 row = clo; row < chi; row++) {
          if (EMIT && wk.full()) break;
          u32 found = 0;
          const LcMatch hit = lc_walk_pck(d, count, sigma, stack + L.cells, above, L.depth, c, row, q, m, in.sc, in.T, cola, colb, &found, err);
          lc_pck_one<EMIT>(d, wk, query, hit, found, lane, err);
        }
        walks += chi - clo;
        continue;
      }
      u32 *dst = stack + free + LC_HEADER;
      const LcColumn col = lc_column(stack + L.cells, L.blo, L.bhi, first, c, q, m, in.sc, dst);
      if (col.M >= in.T) {
        lc_pck_rows<EMIT>(d, wk, query, clo, chi, L.depth + 1, col, lane, err);
        continue;
      }
      if (col.M == 0) continue;
      L.cur = work;
      lc_store(stack, at, L, lane);
      const u32 cells = free + LC_HEADER + lc_band_offset(col, first, L.blo);
      L = LcLevel{ clo, chi, all, col.lo, col.hi, cells, at, L.depth + 1 };
      at = free;
      free = cells + (col.hi - col.lo);
      pushed += 1;
      down = true;
      break;
    }
    if (down) continue;
    if (L.below == NO_LEVEL) break;
    free = at;
    at = L.below;
    L = lc_load(stack, at);
  }
  if (!EMIT && lane == 0) {
    report(w, cnt, j, wk.k, pushed, children, walks);
    if (other) atomicAdd((unsigned long long *) &w[W_OTHER], 1ull);
  }
}

// k_lc_walk for a packed index: the same counts, windows and records
template <bool EMIT>
__global__ __launch_bounds__(LC_THREADS) void k_lc_walk_pck(LcPkInput in, u64 j0, u64 j1, u32 *cnt, const u64 *off, u64 w0,
                                                            u64 w1, LcRecord *out, u32 *arena, u64 *w) {
  __shared__ u32 s_count[LC_WAVES][LC_LETTERS + 1];
  const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const u64 slot = (u64) blockIdx.x * LC_WAVES + wave, slots = (u64) gridDim.x * LC_WAVES;
  u32 *stack = arena + slot * ((u64) in.stack_words + 3ull * in.col_words);
  u32 *count = s_count[wave];
  const u32 sigma = dec_count_to_lds(in.d, count, LC_LETTERS);
  for (u64 j = j0 + slot; j < j1; j += slots)          // (the whole wave: the waves of a workgroup never wait for each other)
    lc_job_pck<EMIT>(in, count, sigma, j, stack, cnt, off, w0, w1, out, w, lane);
}

// w[W_BAD] = the smallest (query << 2 | what is wrong with it); w[W_LONGEST]
__global__ __launch_bounds__(LC_THREADS) void k_lc_validate(const u8 *queries, const u64 *qoff, u64 Q, u32 match,
                                                            u32 sigma, u64 *w) {
  const u64 t = (u64) blockIdx.x * LC_THREADS + threadIdx.x;
  if (t >= Q) return;
  const u64 a = qoff[t], b = qoff[t + 1];
  u32 bad = 0;
  if ((t == 0 && a != 0) || b <= a || b - a > LC_MAX_QUERY || b > qoff[Q]) bad = BAD_LENGTH;
  else if ((b - a) * match > LC_MAX_SCORE) bad = BAD_SCORE;
  else {
    for (u64 x = a; x < b; x++)
      if (queries[x] >= sigma && queries[x] != IV_WILDCARD) bad = BAD_SYMBOL;
    atomicMax((unsigned long long *) &w[W_LONGEST], (unsigned long long) (b - a));
  }
  if (bad) atomicMin((unsigned long long *) &w[W_BAD], (unsigned long long) (t << 2 | bad));
}

// Table entry i in [1, N): the first depth k < depth_max at which the symbols of
// the suffixes i - 1 and i differ, two specials being equal and ending the
// comparison: cuts[..] = i | k << 32, in no order; w[W_CUTS] = how many there
// are.  Those beyond `room` are dropped, which joins two groups and loses none.
template <typename S>
__global__ __launch_bounds__(LC_THREADS) void k_lc_cuts(IvText<S> text, u32 N, u32 depth_max, u64 *cuts, u32 room,
                                                        u64 *w) {
  const u64 i = (u64) blockIdx.x * LC_THREADS + threadIdx.x + 1;
  if (i >= N) return;
  for (u32 k = 0; k < depth_max; k++) {
    const u32 a = iv_symbol(text, (u32) i - 1, k), b = iv_symbol(text, (u32) i, k);
    if (a >= IV_WILDCARD && b >= IV_WILDCARD) return;
    if (a != b) {
      const u64 place = atomicAdd((unsigned long long *) &w[W_CUTS], 1ull);
      if (place < room) cuts[place] = i | (u64) k << 32;
      return;
    }
  }
}

}  // namespace

struct gtamd_locali : ConsumerBase<> {
  IndexSlot index;
  u32 sigma = 0, cut_max = 0, compute_units = 0;
  std::vector<u64> cuts;          // of the index, ascending table index: i | depth << 32
  u32 forced_stack = 0, forced_cut = GTAMD_LOCALI_AUTO;
  bool prepared = false;
  // what a prepare leaves for the emit calls
  SequenceSet queries;
  u64 Q = 0, jobs = 0;
  LcScores sc = { 1, -1, 1 };
  u32 T = 1, groups = 0, q = 0, stack_words = 0, col_words = 0, blocks = 0;
  JobOffsets jo;
  Dev<u32> gstart, arena;
  Dev<u64> cutlist;
  Dev<u8> out;                    // records on their way to host memory
  gtamd_locali_info info = gtamd_locali_info();
};

namespace {

const char FEATURE[] = "local alignments";

// the cuts of a new index down to the largest depth q may take
template <typename S> int find_cuts(gtamd_locali *lc) {
  const IndexView &v = lc->index.tab;
  const u32 N = (u32) (v.n + 1);
  if (lc->cutlist.grow((u64) LC_CUT_LIST * 8) != hipSuccess) return out_of_memory(FEATURE, LC_CUT_LIST, "cuts");
  HIP_TRY(hipMemsetAsync(lc->words + W_CUTS, 0, sizeof(u64), lc->st));
  if (N > 1)
    k_lc_cuts<S><<<(u32) div_up(N - 1, LC_THREADS), LC_THREADS, 0, lc->st>>>(
        IvText<S>{ v.enc, v.n, (const S *) v.suf }, N, lc->cut_max, lc->cutlist, LC_CUT_LIST,
        lc->words);
  HIP_TRY(hipGetLastError());
  u64 found = 0;
  TRY(fetch(lc->st, { { lc->words + W_CUTS, &found, sizeof found } }));
  if (found > LC_CUT_LIST) found = LC_CUT_LIST;        // (no suffix table)
  lc->cuts.resize(found);
  TRY(fetch(lc->st, { { lc->cutlist, lc->cuts.data(), found * 8 } }));
  std::sort(lc->cuts.begin(), lc->cuts.end(),
            [](u64 a, u64 b) { return (a & 0xffffffffull) < (b & 0xffffffffull); });
  return 0;
}

// the letters and the largest depth q may take: at most 2^16 groups
void set_alphabet(gtamd_locali *lc, u32 sigma) {
  lc->sigma = sigma;
  lc->cut_max = 1;
  for (u64 groups = sigma; sigma > 1 && groups * sigma <= LC_CUT_GROUPS; groups *= sigma) lc->cut_max += 1;
}

// what an image must be like to be the index
int refuse_image(const PkxDec &d) {
  if (d.sigma == 0 || d.sigma > LC_LETTERS) {
    gtamd_set_error("local alignments: an alphabet of %u letters, 1 to %u expected", d.sigma, LC_LETTERS);
    return -1;
  }
  if (d.N == 0) { gtamd_set_error("local alignments: a packed index without a row"); return -1; }
  return refuse_sizes(FEATURE, d.N - 1, 0);               // rows <= 2^32 - 4096
}

// every way of setting an index: what is refused, before anything is touched
int set_index(gtamd_locali *lc, const IndexView &v, u32 sigma, bool from_host) {
  if (lc == nullptr || v.suf == nullptr || (v.enc == nullptr && v.n)) {
    gtamd_set_error("invalid argument to gtamd_locali_set_index");
    return -1;
  }
  TRY(refuse_suf_bytes(FEATURE, v.suf_bytes));
  TRY(refuse_sizes(FEATURE, v.n, 0));
  if (sigma == 0 || sigma > LC_LETTERS) {
    gtamd_set_error("local alignments: an alphabet of %u letters, 1 to %u expected", sigma, LC_LETTERS);
    return -1;
  }
  HIP_TRY(hipSetDevice(lc->device));
  lc->prepared = false;
  set_alphabet(lc, sigma);
  TRY(lc->index.set_tables(FEATURE, v, from_host));
  const int rc = v.suf_bytes == 4 ? find_cuts<u32>(lc) : find_cuts<u64>(lc);
  if (rc != 0) lc->index.tab.drop();
  return rc;
}

u64 held_bytes(const gtamd_locali *lc) {
  return lc->index.bytes() + lc->queries.bytes() + lc->jo.bytes() + lc->gstart.bytes + lc->arena.bytes +
         lc->cutlist.bytes + lc->words.bytes + lc->out.bytes;
}

template <typename S> LcInput<S> input(const gtamd_locali *lc) {
  const IndexView &v = lc->index.tab;
  return LcInput<S>{ { v.enc, v.n, (const S *) v.suf }, (u32) (v.n + 1),
                     lc->queries.sym, lc->queries.off, lc->gstart, lc->groups, lc->sc, lc->T, lc->stack_words, lc->col_words };
}

LcPkInput input_pck(const gtamd_locali *lc) {
  return LcPkInput{ pckidx_dec(lc->index.pck), lc->queries.sym, lc->queries.off, lc->groups, lc->q, lc->sc, lc->T,
                    lc->stack_words, lc->col_words };
}

// the message for what k_lc_validate found
int refuse_query(gtamd_locali *lc, u64 found) {
  const u64 t = found >> 2;
  u64 ab[2] = { 0, 0 };
  TRY(fetch(lc->st, { { lc->queries.off + t, ab, sizeof ab } }));
  const unsigned long long query = t, len = ab[1] - ab[0];
  switch (found & 3) {
    case BAD_LENGTH:
      if (ab[1] > ab[0] && len > LC_MAX_QUERY)
        gtamd_set_error("local alignments: query number %llu of length %llu; queries must not be longer than %u",
                        query, len, LC_MAX_QUERY);
      else
        gtamd_set_error("local alignments: query number %llu is empty, or the offsets do not ascend from 0 to "
                        "their last", query);
      break;
    case BAD_SCORE:
      gtamd_set_error("local alignments: query number %llu of length %llu with a match score of %d can reach a "
                      "score above %u, the largest a cell holds", query, len, lc->sc.match, LC_MAX_SCORE);
      break;
    default:
      gtamd_set_error("local alignments: query number %llu holds a symbol that is neither a letter of the "
                      "alphabet of %u letters nor the wildcard", query, lc->sigma);
  }
  return -1;
}

// the groups of this prepare: the cuts above depth q, between 0 and N
int set_groups(gtamd_locali *lc, u64 Q) {
  const u64 N = lc->index.tab.n + 1;
  u32 q = lc->forced_cut;
  if (q == GTAMD_LOCALI_AUTO) {
    std::vector<u64> upto(lc->cut_max + 1, 1);         // groups with the cuts above depth q
    for (u64 c : lc->cuts)
      for (u32 d = (u32) (c >> 32) + 1; d <= lc->cut_max; d++) upto[d] += 1;
    q = 0;
    while (q < lc->cut_max && Q * upto[q] < LC_TARGET_JOBS) q += 1;
  }
  std::vector<u32> start;
  start.push_back(0);
  for (u64 c : lc->cuts)
    if ((u32) (c >> 32) < q) start.push_back((u32) c);
  start.push_back((u32) N);
  lc->groups = (u32) start.size() - 1;
  lc->info.cut_depth = q < lc->cut_max ? q : lc->cut_max;
  lc->info.groups = lc->groups;
  if (lc->gstart.grow(start.size() * 4) != hipSuccess) return out_of_memory(FEATURE, start.size(), "groups");
  HIP_TRY(hipMemcpy(lc->gstart, start.data(), start.size() * 4, hipMemcpyHostToDevice));
  return 0;
}

// the codes of this prepare with a packed index: every string of q letters
void set_codes(gtamd_locali *lc, u64 Q) {
  u32 q = lc->forced_cut;
  u64 codes = 1;
  if (q == GTAMD_LOCALI_AUTO) {
    q = 0;
    while (q < lc->cut_max && Q * codes < LC_TARGET_JOBS) { q += 1; codes *= lc->sigma; }
  } else {
    if (q > lc->cut_max) q = lc->cut_max;
    for (u32 d = 0; d < q; d++) codes *= lc->sigma;
  }
  lc->q = q;
  lc->groups = (u32) codes;                          // (at most LC_CUT_GROUPS)
  lc->info.cut_depth = q;
  lc->info.groups = lc->groups;
}

// S: the entries of .suf; void: the index is a reader of the packed index
template <typename S> int prepare(gtamd_locali *lc) {
  constexpr bool PCK = std::is_void<S>::value;
  hipStream_t st = lc->st;
  const u64 Q = lc->Q;
  HIP_TRY(hipMemsetAsync(lc->words, 0, W_CUTS * sizeof(u64), st));
  HIP_TRY(hipMemsetAsync(lc->words + W_BAD, 0xff, sizeof(u64), st));
  HIP_TRY(hipMemsetAsync(lc->words + W_ERROR, 0, sizeof(u64), st));
  HIP_TRY(hipEventRecord(lc->ev[0], st));
  k_lc_validate<<<(u32) div_up(Q, LC_THREADS), LC_THREADS, 0, st>>>(lc->queries.sym, lc->queries.off, Q, (u32) lc->sc.match,
                                                                   lc->sigma, lc->words);
  HIP_TRY(hipGetLastError());
  u64 found[2] = { 0, 0 };
  TRY(fetch(st, { { lc->words + W_BAD, found, sizeof found } }));
  if (found[0] != ~0ull) return refuse_query(lc, found[0]);
  if constexpr (PCK) set_codes(lc, Q);
  else TRY(set_groups(lc, Q));
  const u64 jobs = Q * lc->groups;
  if (jobs > LC_MAX_JOBS) {
    gtamd_set_error("local alignments: %llu queries times %u groups of the table are more than %llu jobs",
                    (unsigned long long) Q, lc->groups, (unsigned long long) LC_MAX_JOBS);
    return -1;
  }
  lc->jobs = jobs;
  lc->info.jobs = jobs;
  if (lc->jo.grow(jobs) != hipSuccess) return out_of_memory(FEATURE, jobs, "jobs");
  // per wave of the grid: the stack, and two columns of the longest query for the suffixes that go on alone;
  // with a packed index a third, for the column the path of a code ends with
  const u32 longest = (u32) found[1];
  lc->col_words = (longest + 63) / 64 * 64;
  lc->stack_words = lc->forced_stack ? lc->forced_stack : 32 * lc->col_words + 4096;
  const u64 most = (u64) lc->compute_units * LC_WAVES_PER_CU / LC_WAVES;
  lc->blocks = (u32) std::min<u64>(div_up(jobs, LC_WAVES), most ? most : 1);
  const u64 words = (u64) lc->blocks * LC_WAVES * ((u64) lc->stack_words + (PCK ? 3ull : 2ull) * lc->col_words);
  if (lc->arena.grow(words * 4) != hipSuccess) {
    gtamd_set_error("local alignments: cannot allocate %llu bytes of device memory for the columns of %u waves "
                    "(%u words of stack each; gtamd_locali_set_limits)", (unsigned long long) (words * 4),
                    lc->blocks * LC_WAVES, lc->stack_words);
    return -1;
  }
  if constexpr (PCK)
    k_lc_walk_pck<false><<<lc->blocks, LC_THREADS, 0, st>>>(input_pck(lc), 0, jobs, lc->jo.cnt, nullptr, 0, 0, nullptr,
                                                           lc->arena, lc->words);
  else
    k_lc_walk<S, false><<<lc->blocks, LC_THREADS, 0, st>>>(input<S>(lc), 0, jobs, lc->jo.cnt, nullptr, 0, 0, nullptr,
                                                          lc->arena, lc->words);
  HIP_TRY(hipGetLastError());
  u64 h[W_WORDS];
  TRY(finish_count(lc, lc->jo, jobs, h, W_ERROR, &lc->info));       // (W_ERROR: 0 behind a walk over .suf)
  lc->info.jobs_finished_alone = h[W_OTHER];
  lc->info.stack_words = lc->stack_words;
  return 0;
}

// the walk of the jobs [j0, j1) that writes the records [cur, w1) to dst
void launch_emit(gtamd_locali *lc, u64 j0, u64 j1, u64 cur, u64 w1, LcRecord *dst) {
  const u32 blocks = (u32) std::min<u64>(div_up(j1 - j0, LC_WAVES), lc->blocks);      // (the arena has room for lc->blocks)
  if (lc->index.pck != nullptr)
    k_lc_walk_pck<true><<<blocks, LC_THREADS, 0, lc->st>>>(input_pck(lc), j0, j1, nullptr, lc->jo.off, cur, w1, dst,
                                                          lc->arena, lc->words);
  else if (lc->index.tab.suf_bytes == 4)
    k_lc_walk<u32, true><<<blocks, LC_THREADS, 0, lc->st>>>(input<u32>(lc), j0, j1, nullptr, lc->jo.off, cur, w1, dst,
                                                             lc->arena, lc->words);
  else
    k_lc_walk<u64, true><<<blocks, LC_THREADS, 0, lc->st>>>(input<u64>(lc), j0, j1, nullptr, lc->jo.off, cur, w1, dst,
                                                             lc->arena, lc->words);
}

}  // namespace

extern "C" gtamd_locali *gtamd_locali_create(int device) {
  GTAMD_ABI_BEGIN
  gtamd_locali *lc = create_consumer<gtamd_locali>(device, W_WORDS, "the local aligner");
  if (lc == nullptr) return nullptr;
  int units = 0;
  if (hipDeviceGetAttribute(&units, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || units <= 0) {
    gtamd_set_error("cannot read the number of compute units of device %d", device);
    destroy_consumer(lc);
    return nullptr;
  }
  lc->compute_units = (u32) units;
  return lc;
  GTAMD_ABI_END(nullptr)
}

extern "C" void gtamd_locali_destroy(gtamd_locali *lc) { destroy_consumer(lc); }

extern "C" void gtamd_locali_geometry(uint32_t *jobs_per_workgroup, uint64_t *min_capacity, uint32_t *max_query,
                                      uint32_t *min_stack_words) {
  if (jobs_per_workgroup != nullptr) *jobs_per_workgroup = LC_WAVES;
  if (min_capacity != nullptr) *min_capacity = LC_MIN_CAPACITY;
  if (max_query != nullptr) *max_query = LC_MAX_QUERY;
  if (min_stack_words != nullptr) *min_stack_words = LC_HEADER;
}

extern "C" int gtamd_locali_set_index(gtamd_locali *lc, const uint8_t *enc, uint64_t n, const void *suf,
                                      uint32_t suf_bytes, uint32_t numofchars) {
  GTAMD_ABI_BEGIN
  return set_index(lc, IndexView{ enc, n, suf, suf_bytes }, numofchars, false);
  GTAMD_ABI_END(-1)
}

extern "C" int gtamd_locali_set_index_host(gtamd_locali *lc, const uint8_t *enc, uint64_t n, const void *suf,
                                           uint32_t suf_bytes, uint32_t numofchars) {
  GTAMD_ABI_BEGIN
  return set_index(lc, IndexView{ enc, n, suf, suf_bytes }, numofchars, true);
  GTAMD_ABI_END(-1)
}

extern "C" int gtamd_locali_set_index_esa(gtamd_locali *lc, const gtamd_esa_ctx *esa, const uint8_t *enc, uint64_t n,
                                          uint32_t numofchars) {
  GTAMD_ABI_BEGIN
  if (lc == nullptr || esa == nullptr) { gtamd_set_error("invalid argument to gtamd_locali_set_index_esa"); return -1; }
  IndexView v;
  TRY(engine_tables(FEATURE, esa, enc, n, false, &v));
  return set_index(lc, v, numofchars, false);
  GTAMD_ABI_END(-1)
}

extern "C" int gtamd_locali_set_index_pckidx(gtamd_locali *lc, const gtamd_pckidx *px) {
  GTAMD_ABI_BEGIN
  TRY(IndexSlot::refuse_reader(FEATURE, "locali", "the aligner", lc, px));
  const PkxDec &d = pckidx_dec(px);
  TRY(refuse_image(d));
  HIP_TRY(hipSetDevice(lc->device));
  lc->prepared = false;
  lc->index.set_reader(px);
  lc->cuts.clear();
  set_alphabet(lc, d.sigma);
  return 0;
  GTAMD_ABI_END(-1)
}

extern "C" int gtamd_locali_set_limits(gtamd_locali *lc, uint32_t stack_words, uint32_t cut_depth) {
  GTAMD_ABI_BEGIN
  if (lc == nullptr) { gtamd_set_error("invalid argument to gtamd_locali_set_limits"); return -1; }
  if (stack_words != 0 && (stack_words < LC_HEADER || stack_words > LC_MAX_STACK)) {
    gtamd_set_error("local alignments: a stack of %u words, 0 (chosen from the longest query) or %u to %u expected",
                    stack_words, LC_HEADER, LC_MAX_STACK);
    return -1;
  }
  if (cut_depth != GTAMD_LOCALI_AUTO && cut_depth > 16) {
    gtamd_set_error("local alignments: a cut depth of %u, GTAMD_LOCALI_AUTO or 0 to 16 expected (a depth beyond "
                    "what the alphabet allows is taken as the largest it allows)", cut_depth);
    return -1;
  }
  lc->forced_stack = stack_words;
  lc->forced_cut = cut_depth;          // (what is prepared keeps the sizes it was prepared with)
  return 0;
  GTAMD_ABI_END(-1)
}

extern "C" int gtamd_locali_prepare(gtamd_locali *lc, const uint8_t *queries, const uint64_t *offsets, uint64_t Q,
                                    int is_device, int32_t match, int32_t mismatch, int32_t gapextend,
                                    uint32_t threshold, gtamd_locali_info *info) {
  GTAMD_ABI_BEGIN
  if (lc == nullptr || (Q != 0 && (queries == nullptr || offsets == nullptr))) {
    gtamd_set_error("invalid argument to gtamd_locali_prepare");
    return -1;
  }
  TRY(lc->index.refuse_unset(FEATURE, "locali"));
  if (lc->index.pck != nullptr) {
    // the reader may hold another image than when it was set: this prepare is of the one it holds now
    TRY(lc->index.refuse_lost_reader(FEATURE));
    TRY(refuse_image(pckidx_dec(lc->index.pck)));
  }
  if (match <= 0 || mismatch >= 0 || gapextend >= 0 || match > LC_MAX_WEIGHT || mismatch < -LC_MAX_WEIGHT ||
      gapextend < -LC_MAX_WEIGHT) {
    gtamd_set_error("local alignments: scores match %d, mismatch %d, gapextend %d; match must be in 1..%d, mismatch "
                    "and gapextend in -%d..-1 (with other signs the walk need not end)", match, mismatch, gapextend,
                    LC_MAX_WEIGHT, LC_MAX_WEIGHT);
    return -1;
  }
  if (threshold == 0) {
    gtamd_set_error("local alignments: a threshold of 0, at least 1 expected");
    return -1;
  }
  if (Q > LC_MAX_QUERIES) {
    gtamd_set_error("local alignments: %llu queries, at most %llu in one call", (unsigned long long) Q,
                    (unsigned long long) LC_MAX_QUERIES);
    return -1;
  }
  HIP_TRY(hipSetDevice(lc->device));
  lc->prepared = false;
  if (lc->index.pck != nullptr) {
    set_alphabet(lc, pckidx_dec(lc->index.pck).sigma);
    lc->index.stamp();
  }
  lc->info = gtamd_locali_info();
  lc->Q = Q;
  lc->jobs = 0;
  lc->sc = LcScores{ match, mismatch, -gapextend };
  lc->T = threshold;
  lc->jo.off_host.assign(1, 0);
  if (Q != 0) {
    TRY(lc->queries.set(FEATURE, "query symbols", queries, offsets, Q, is_device, lc->st));
    TRY(lc->index.pck != nullptr ? prepare<void>(lc) : lc->index.tab.suf_bytes == 4 ? prepare<u32>(lc) : prepare<u64>(lc));
  }
  lc->info.device_bytes = held_bytes(lc);
  lc->prepared = true;
  if (info != nullptr) *info = lc->info;
  return 0;
  GTAMD_ABI_END(-1)
}

extern "C" int gtamd_locali_emit(gtamd_locali *lc, uint64_t *cursor, gtamd_locali_record *out, uint64_t capacity,
                                 int out_on_device, uint64_t *written) {
  GTAMD_ABI_BEGIN
  if (lc == nullptr || cursor == nullptr || written == nullptr || (out == nullptr && capacity)) {
    gtamd_set_error("invalid argument to gtamd_locali_emit");
    return -1;
  }
  if (!lc->prepared) {
    gtamd_set_error("local alignments: nothing is prepared (gtamd_locali_prepare)");
    return -1;
  }
  HIP_TRY(hipSetDevice(lc->device));
  TRY(emit_jobs<LcRecord>(FEATURE, "gtamd_locali_prepare", lc->index, lc->jo, lc->info.matches, cursor, capacity,
                          LC_MIN_CAPACITY, out, out_on_device, lc->out, lc->st, lc->words + W_ERROR, written,
                          [lc](u64 j0, u64 j1, u64 cur, u64 w1, LcRecord *dst) { launch_emit(lc, j0, j1, cur, w1, dst); }));
  lc->info.emitted += *written;
  lc->info.device_bytes = held_bytes(lc);
  return 0;
  GTAMD_ABI_END(-1)
}

extern "C" int gtamd_locali_get_info(const gtamd_locali *lc, gtamd_locali_info *info) {
  GTAMD_ABI_BEGIN
  return consumer_info(lc, info, "gtamd_locali_get_info");
  GTAMD_ABI_END(-1)
}
