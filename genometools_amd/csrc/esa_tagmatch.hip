// esa_tagmatch.hip -- approximate matches of short tags against .suf and the
// sequence in device memory: `gt tagerator -e K -esa INDEX -q TAGS` (C ABI, the
// semantics and the order: include/gtamd_tagmatch.h).
//
//   a  k_tm_validate      one lane per tag: what is refused
//   b  k_tm_walk<false>   one WAVE per job (tag, strand): the depth-first walk
//                         over the intervals of the table, one level per depth in
//                         LDS; the matches of the job are counted
//      k_tm_settle        one lane per tag: K' of a tag with a match (with BEST
//                         step b runs for k = 0..K over the tags without one)
//   c  JobOffsets::scan (esa_jobs) 64-bit exclusive scan of the counts
//   d  k_tm_walk<true>    the same walk for the jobs of a window of records,
//                         which writes those
//
// Every working array has one entry per job or per tag, none has N.
//
// With a reader of the packed index as the index (gtamd_tagmatch_set_index_pckidx,
// include/gtamd_pcktag.h) steps b and d are k_tm_walk_pck: the same
// jobs, windows and records, the levels intervals of rows of the decoded form
// (esa_pckidx_dec.h), all children of a level from one rank pair a letter.
#include <type_traits>
#include "esa_common.h"
#include "esa_jobs.h"
#include "esa_tagmatch_core.h"
#include "../../include/gtamd_tagmatch.h"
#include "../../include/gtamd_pcktag.h"

namespace {

constexpr int TM_THREADS = SC_THREADS;
constexpr u32 TM_WAVES = TM_THREADS / 64;          // jobs of one workgroup: one a wave
constexpr u32 TM_LEVELS = 128;                     // depths 0 .. m + K - 1 <= 126 have a level
constexpr u32 TM_BATCH = IV_BATCH;                 // suffixes the lanes of a wave take at once
static_assert(TM_BATCH == DEC_BATCH, "and as many rows of a packed index");
constexpr u64 TM_MIN_CAPACITY = TM_BATCH;
constexpr u64 TM_MAX_TAGS = 1ull << 30;
constexpr u32 TM_STRANDS = GTAMD_TAGMATCH_FORWARD | GTAMD_TAGMATCH_REVCOMP;
constexpr u32 NO_K = GTAMD_TAGMATCH_NO_K;

enum { W_BAD = W_WALK_WORDS, W_ERROR, W_WORDS };   // W_ERROR: the error word of a walk over a packed index
enum { BAD_LENGTH = 1, BAD_SHORT = 2, BAD_SYMBOL = 3 };

struct TmRecord { u64 tag, dbstart, lendist; };

// one level of a walk: the suffixes [lo, end) share as many symbols as the level
// is deep; cur: the left bound of the next child; the column after those symbols
struct TmLevel { u32 lo, end, cur, rowval; u64 Pv, Mv; };
static_assert(sizeof(TmLevel) == 32, "a level is 32 bytes of LDS");

template <typename S> struct TmInput {
  IvText<S> text; u32 N;
  const u8 *tags; const u64 *toff; u64 T;
  u32 strands, wild;
};

// what job j is: its tag, its strand and its K; false if this pass has nothing to
// do for it (EMIT: its tag has no K'; else: its tag has one already)
struct TmJob { u64 tag, tagword; u32 K; bool rc; };
template <bool EMIT> __device__ __forceinline__ bool tm_job(u32 strands, u64 j, u32 k_pass, const u32 *kbest, TmJob *job) {
  const bool both = strands == TM_STRANDS;
  job->tag = both ? j >> 1 : j;
  job->rc = both ? (j & 1) != 0 : strands == GTAMD_TAGMATCH_REVCOMP;
  job->K = EMIT ? kbest[job->tag] : k_pass;
  job->tagword = 2 * job->tag + (job->rc ? 1 : 0);
  return EMIT ? job->K != NO_K : kbest[job->tag] == NO_K;
}

// the tag, one letter a lane, as the strand reads it; its Eq words by ballot; its length
__device__ __forceinline__ u32 tm_tag_eq(const u8 *tags, const u64 *toff, u64 tag, bool rc, u32 lane, u64 *eq) {
  const u64 t0 = toff[tag];
  const u32 m = (u32) (toff[tag + 1] - t0);             // 1 .. 64 (k_tm_validate)
  u32 letter = IV_SEPARATOR;
  if (lane < m) letter = rc ? 3u - tags[t0 + (m - 1 - lane)] : tags[t0 + lane];
  for (u32 c = 0; c < TM_LETTERS; c++) {
    const u64 word = __ballot(letter == c);
    eq[c] = word;                              // (every lane the same word)
  }
  return m;
}

// Jobs [j0, j1), one a wave.  EMIT false: cnt[job] = its matches for K = k_pass,
// for the jobs of the tags whose kbest is still none.  EMIT true: K of a job is
// kbest of its tag; records [w0, w1) of all are written to out, record w0 first.
template <typename S, bool EMIT>
__global__ __launch_bounds__(TM_THREADS) void k_tm_walk(TmInput<S> in, u64 j0, u64 j1, u32 k_pass, const u32 *kbest,
                                                        u32 *cnt, const u64 *off, u64 w0, u64 w1, TmRecord *out,
                                                        u64 *w) {
  __shared__ TmLevel s_level[TM_WAVES][TM_LEVELS];
  __shared__ u64 s_eq[TM_WAVES][TM_LETTERS];
  const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const u64 j = j0 + (u64) blockIdx.x * TM_WAVES + wave;
  if (j >= j1) return;                       // (the whole wave: the waves of a workgroup never wait for each other)
  TmJob job;
  if (!tm_job<EMIT>(in.strands, j, k_pass, kbest, &job)) return;
  const u32 K = job.K;

  const IvText<S> &text = in.text;
  const u64 tagword = job.tagword;
  JobWindow<TmRecord> wk = { 0, 0, 0, nullptr };
  if (EMIT && !wk.open(off, j, w0, w1, out)) return;

  u64 *eq = s_eq[wave];
  const u32 m = tm_tag_eq(in.tags, in.toff, job.tag, job.rc, lane, eq);

  TmLevel *level = s_level[wave];
  level[0] = TmLevel{ 0, in.N, 0, K | K << 16, ~0ull, 0 };
  u32 depth = 0;                               // of the top level, which is its index
  u32 pushed = 0, children = 0, walks = 0;
  // Every round moves the cursor of the top level forward by at least one, pops
  // the level or pushes one of the next depth, which is below m + K: it ends.
  for (;;) {
    if (EMIT && wk.full()) break;
    const u32 cur = uni(level[depth].cur), end = uni(level[depth].end);
    if (cur >= end) {
      if (depth == 0) break;
      depth -= 1;
      continue;
    }
    const u32 s = uni(iv_symbol(text, cur, depth));
    TmColumn col = { level[depth].Pv, level[depth].Mv, 0, 0 };
    const u32 rowval = uni(level[depth].rowval);
    col.row = rowval & 0xffff;
    col.val = rowval >> 16;
    if (s >= IV_WILDCARD) {
      // only specials from here to the end of the level: each goes on alone, if at all
      if (!in.wild) {
        if (depth == 0) break;
        depth -= 1;
        continue;
      }
      const u32 many = end - cur < TM_BATCH ? end - cur : TM_BATCH;
      level[depth].cur = cur + many;
      u32 len = 0, dist = 0;
      u64 p = 0;
      if (lane < many) {
        p = text.suf[cur + lane];
        if (p < text.n) len = tm_walk(col, eq, text.enc, text.n, p, depth, m, K, true, &dist);
      }
      walks += many;
      wk.give<EMIT>(len != 0, TmRecord{ tagword, p, (u64) len | (u64) dist << 32 });
      continue;
    }
    const u32 e = iv_right_bound(text, cur, end, depth, s);
    level[depth].cur = e;
    children += 1;
    tm_step(col, s < TM_LETTERS ? eq[s] : 0, K);
    if (tm_dead(col)) continue;
    if (tm_success(col, m)) {
      // all suffixes of the child match with depth + 1 symbols
      for (u32 b = cur; b < e; b += TM_BATCH) {
        if (EMIT && wk.full()) break;
        const u32 idx = b + lane;                   // (e <= N <= 2^32 - 4096: no wrap)
        const u64 p = idx < e ? (u64) text.suf[idx] : text.n;
        wk.give<EMIT>(p < text.n, TmRecord{ tagword, p, (u64) (depth + 1) | (u64) col.val << 32 });
      }
      continue;
    }
    if (e - cur <= TM_BATCH) {
      u32 len = 0, dist = 0;
      u64 p = 0;
      if (lane < e - cur) {
        p = text.suf[cur + lane];
        if (p < text.n) len = tm_walk(col, eq, text.enc, text.n, p, depth + 1, m, K, in.wild != 0, &dist);
      }
      walks += e - cur;
      wk.give<EMIT>(len != 0, TmRecord{ tagword, p, (u64) len | (u64) dist << 32 });
      continue;
    }
    if (depth + 1 >= TM_LEVELS) continue;          // (cannot be: a column alive at depth m + K has reached row m)
    depth += 1;
    level[depth] = TmLevel{ cur, e, cur, col.row | col.val << 16, col.Pv, col.Mv };
    pushed += 1;
  }
  if (!EMIT && lane == 0) report(w, cnt, j, wk.k, pushed, children, walks);
}

// ---- the same walk over a packed index (include/gtamd_pcktag.h) ----
// A level is an interval [lo, end) of rows of the decoded form: the rows whose
// suffixes, in the text of the index, begin with the letters taken so far, last
// letter first.  In TmLevel, cur is the set of letters whose children are still
// to be taken when the walk comes back to the level.
struct PkInput {
  PkxDec d;
  const u8 *tags; const u64 *toff; u64 T;
  u32 strands;
};

// The children step, one letter a lane: lane c of `todo` gets the rows [*clo, *chi)
// of the child of letter c of the interval [lo, hi) -- one rank pair, all lanes
// in the same one or two lines -- and, where the child is not empty, *ccol = col
// after letter c.  An empty child, and every other lane, has *clo == *chi.
// count: count[] of the index, eq: the Eq words of the tag.  Bounds that are none
// (the decoded form is inconsistent) leave the error word and an empty child.
__device__ __forceinline__ void pk_children(const PkxDec &d, const u32 *count, const u64 *eq, u32 lo, u32 hi,
                                            const TmColumn &col, u32 K, u32 todo, u32 lane, u32 *clo, u32 *chi,
                                            TmColumn *ccol, u32 *err) {
  *ccol = col;
  if (dec_children(d, count, lo, hi, TM_LETTERS, todo, lane, clo, chi, err)) tm_step(*ccol, eq[lane], K);
}

// Row `row`, whose `depth` letters gave column c (alive, no success yet), goes on
// alone: the next letter is the BWT symbol of the row, the next row its LF
// (pck_overcontext of the reference, one row a lane).  The length of its match,
// *dist = its distance, *at = the row the match was found at; 0 if it has none.  A
// special ends it: so does the row of suffix 0, whose symbol is one.  At most
// m + K letters are part of a match, and every row is checked against the rows.
__device__ __forceinline__ u32 pk_walk(const PkxDec &d, const u32 *count, const u64 *eq, TmColumn c, u32 row, u32 depth,
                                       u32 m, u32 K, u32 *dist, u32 *at, u32 *err) {
  while (depth < m + K) {
    const u32 s = dec_symbol(d, row);
    if (s >= d.sigma || s >= TM_LETTERS) return 0;
    tm_step(c, eq[s], K);
    depth += 1;
    if (tm_dead(c)) return 0;
    const u64 next = (u64) count[s] + dec_rank(d, s, row);
    if (next >= d.N) { dev_fail(err, PKX_E_WALK); return 0; }
    row = (u32) next;
    if (tm_success(c, m)) { *dist = c.val; *at = row; return depth; }
  }
  return 0;
}

// k_tm_walk for a packed index: the same jobs, counts, windows and records.
template <bool EMIT>
__global__ __launch_bounds__(TM_THREADS) void k_tm_walk_pck(PkInput in, u64 j0, u64 j1, u32 k_pass, const u32 *kbest,
                                                            u32 *cnt, const u64 *off, u64 w0, u64 w1, TmRecord *out,
                                                            u64 *w) {
  __shared__ TmLevel s_level[TM_WAVES][TM_LEVELS];
  __shared__ u64 s_eq[TM_WAVES][TM_LETTERS];
  __shared__ u32 s_count[TM_WAVES][TM_LETTERS + 1];
  const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const u64 j = j0 + (u64) blockIdx.x * TM_WAVES + wave;
  if (j >= j1) return;                       // (the whole wave: the waves of a workgroup never wait for each other)
  TmJob job;
  if (!tm_job<EMIT>(in.strands, j, k_pass, kbest, &job)) return;
  const u32 K = job.K;
  const u64 tagword = job.tagword;
  JobWindow<TmRecord> wk = { 0, 0, 0, nullptr };
  if (EMIT && !wk.open(off, j, w0, w1, out)) return;

  const PkxDec &d = in.d;
  u32 *err = reinterpret_cast<u32 *>(&w[W_ERROR]);
  u64 *eq = s_eq[wave];
  const u32 m = tm_tag_eq(in.tags, in.toff, job.tag, job.rc, lane, eq);
  u32 *count = s_count[wave];
  const u32 sigma = dec_count_to_lds(d, count, TM_LETTERS);

  TmLevel *level = s_level[wave];
  level[0] = TmLevel{ 0, (u32) d.N, 0, K | K << 16, ~0ull, 0 };
  u32 depth = 0;                               // of the top level, which is its index
  bool fresh = true;                           // the top level has not been expanded yet
  u32 pushed = 0, children = 0, walks = 0;
  // Every round expands the top level: for the first time, with all letters, or
  // again after a child of it has been walked, with the letters behind that
  // child, which are fewer each time.  A round ends with a push to the next
  // depth, which is below m + K, or with a pop: the walk ends.
  for (;;) {
    if (EMIT && wk.full()) break;
    const u32 lo = uni(level[depth].lo), hi = uni(level[depth].end);
    const u32 todo = fresh ? dec_all_letters(sigma) : uni(level[depth].cur);
    if (todo == 0) {
      if (depth == 0) break;
      depth -= 1;
      fresh = false;
      continue;
    }
    TmColumn col = { level[depth].Pv, level[depth].Mv, 0, 0 };
    const u32 rowval = uni(level[depth].rowval);
    col.row = rowval & 0xffff;
    col.val = rowval >> 16;
    u32 my_lo, my_hi;
    TmColumn my_col;
    pk_children(d, count, eq, lo, hi, col, K, todo, lane, &my_lo, &my_hi, &my_col, err);
    const bool nonempty = my_lo < my_hi;
    if (fresh) children += (u32) __popcll(__ballot(nonempty));
    u32 work = (u32) __ballot(nonempty && !tm_dead(my_col));          // (letters are lanes 0 .. 31)
    const u32 success = (u32) __ballot(nonempty && tm_success(my_col, m));
    bool down = false;
    while (work && !(EMIT && wk.full())) {
      const u32 c = uni((u32) __builtin_ctz(work));
      work &= work - 1;
      const u32 clo = __builtin_amdgcn_readlane(my_lo, c), chi = __builtin_amdgcn_readlane(my_hi, c);
      TmColumn ccol;
      ccol.Pv = (u64) __builtin_amdgcn_readlane((u32) my_col.Pv, c) | (u64) __builtin_amdgcn_readlane((u32) (my_col.Pv >> 32), c) << 32;
      ccol.Mv = (u64) __builtin_amdgcn_readlane((u32) my_col.Mv, c) | (u64) __builtin_amdgcn_readlane((u32) (my_col.Mv >> 32), c) << 32;
      ccol.row = __builtin_amdgcn_readlane(my_col.row, c);
      ccol.val = __builtin_amdgcn_readlane(my_col.val, c);
      if ((success >> c) & 1u) {
        // all rows of the child match with depth + 1 letters
        const u64 lendist = (u64) (depth + 1) | (u64) ccol.val << 32;
        dec_rows<EMIT>(d, wk, clo, chi, depth + 1, lane, err, [=](u64 p) { return TmRecord{ tagword, p, lendist }; });
        continue;
      }
      if (chi - clo <= TM_BATCH) {
        u32 len = 0, dist = 0, at = 0;
        if (lane < chi - clo) len = pk_walk(d, count, eq, ccol, clo + lane, depth + 1, m, K, &dist, &at, err);
        walks += chi - clo;
        u64 p = 0;
        if (EMIT) {
          const u64 place = wk.k + lanes_before(__ballot(len != 0));
          if (len != 0 && place >= wk.first && place < wk.stop) p = dec_dbstart(d, at, len, err);
        }
        wk.give<EMIT>(len != 0, TmRecord{ tagword, p, (u64) len | (u64) dist << 32 });
        continue;
      }
      if (depth + 1 >= TM_LEVELS) continue;          // (cannot be: a column alive at depth m + K has reached row m)
      level[depth].cur = work;
      depth += 1;
      level[depth] = TmLevel{ clo, chi, 0, ccol.row | ccol.val << 16, ccol.Pv, ccol.Mv };
      pushed += 1;
      down = true;
      break;
    }
    if (down) { fresh = true; continue; }
    if (depth == 0) break;
    depth -= 1;
    fresh = false;
  }
  if (!EMIT && lane == 0) report(w, cnt, j, wk.k, pushed, children, walks);
}

// kbest of a tag that had none and whose jobs have a match now: k
__global__ __launch_bounds__(TM_THREADS) void k_tm_settle(const u32 *cnt, u32 per_tag, u64 T, u32 k, u32 *kbest) {
  const u64 t = (u64) blockIdx.x * TM_THREADS + threadIdx.x;
  if (t >= T || kbest[t] != NO_K) return;
  u32 any = 0;
  for (u32 s = 0; s < per_tag; s++) any |= cnt[t * per_tag + s];
  if (any) kbest[t] = k;
}

// w[W_BAD] = the smallest (tag << 2 | what is wrong with it)
__global__ __launch_bounds__(TM_THREADS) void k_tm_validate(const u8 *tags, const u64 *toff, u64 T, u32 K, u32 sigma,
                                                            u64 *w) {
  const u64 t = (u64) blockIdx.x * TM_THREADS + threadIdx.x;
  if (t >= T) return;
  const u64 a = toff[t], b = toff[t + 1];
  u32 bad = 0;
  if ((t == 0 && a != 0) || b <= a || b - a > TM_MAX_TAG || b > toff[T]) bad = BAD_LENGTH;
  else if (b - a <= K) bad = BAD_SHORT;
  else
    for (u64 x = a; x < b; x++)
      if (tags[x] >= sigma) bad = BAD_SYMBOL;
  if (bad) atomicMin((unsigned long long *) &w[W_BAD], (unsigned long long) (t << 2 | bad));
}

}  // namespace

struct gtamd_tagmatch : ConsumerBase<> {
  IndexSlot index;
  u32 sigma = 0;
  bool prepared = false;
  // what a prepare leaves for the emit calls
  SequenceSet tags;
  u64 T = 0, jobs = 0;
  u32 flags = 0;
  JobOffsets jo;
  Dev<u32> kbest;
  Dev<u8> out;                    // records on their way to host memory
  gtamd_tagmatch_info info = gtamd_tagmatch_info();
};

namespace {

const char FEATURE[] = "tag matches";

// every way of setting an index: what is refused, before anything is touched
int set_index(gtamd_tagmatch *tm, const IndexView &v, u32 sigma, bool from_host) {
  if (tm == nullptr || v.suf == nullptr || (v.enc == nullptr && v.n)) {
    gtamd_set_error("invalid argument to gtamd_tagmatch_set_index");
    return -1;
  }
  TRY(refuse_suf_bytes(FEATURE, v.suf_bytes));
  TRY(refuse_sizes(FEATURE, v.n, 0));
  if (sigma == 0 || sigma > TM_LETTERS) {
    gtamd_set_error("tag matches: an alphabet of %u letters, 1 to %u expected", sigma, TM_LETTERS);
    return -1;
  }
  HIP_TRY(hipSetDevice(tm->device));
  tm->prepared = false;
  tm->sigma = sigma;
  return tm->index.set_tables(FEATURE, v, from_host);
}

u64 held_bytes(const gtamd_tagmatch *tm) {
  return tm->index.bytes() + tm->tags.bytes() + tm->jo.bytes() + tm->kbest.bytes + tm->words.bytes + tm->out.bytes;
}

template <typename S> TmInput<S> input(const gtamd_tagmatch *tm) {
  const IndexView &v = tm->index.tab;
  return TmInput<S>{ { v.enc, v.n, (const S *) v.suf }, (u32) (v.n + 1),
                     tm->tags.sym, tm->tags.off, tm->T, tm->flags & TM_STRANDS,
                     (tm->flags & GTAMD_TAGMATCH_WITH_WILDCARDS) ? 1u : 0u };
}

// the message for what k_tm_validate found
int refuse_tag(gtamd_tagmatch *tm, u64 found, u32 K) {
  const u64 t = found >> 2;
  u64 ab[2] = { 0, 0 };
  TRY(fetch(tm->st, { { tm->tags.off + t, ab, sizeof ab } }));
  const unsigned long long tag = t, len = ab[1] - ab[0];
  switch (found & 3) {
    case BAD_LENGTH:
      if (ab[1] > ab[0] && len > TM_MAX_TAG)
        gtamd_set_error("tag matches: tag number %llu of length %llu; tags must not be longer than %u", tag, len,
                        TM_MAX_TAG);
      else
        gtamd_set_error("tag matches: tag number %llu is empty, or the offsets do not ascend from 0 to their last", tag);
      break;
    case BAD_SHORT:
      gtamd_set_error("tag matches: tag number %llu of length %llu; tags must be longer than the allowed number "
                      "of errors (which is %u)", tag, len, K);
      break;
    default:
      gtamd_set_error("tag matches: tag number %llu holds a symbol that is no letter of the alphabet of %u "
                      "letters (a wildcard in a tag is refused)", tag, tm->sigma);
  }
  return -1;
}

PkInput input_pck(const gtamd_tagmatch *tm) {
  return PkInput{ pckidx_dec(tm->index.pck), tm->tags.sym, tm->tags.off, tm->T, tm->flags & TM_STRANDS };
}

// S: the entries of .suf; void: the index is a reader of the packed index
template <typename S> int prepare(gtamd_tagmatch *tm, u32 K) {
  hipStream_t st = tm->st;
  const u64 T = tm->T, jobs = tm->jobs;
  const u32 per_tag = (u32) (jobs / T);
  HIP_TRY(hipMemsetAsync(tm->words, 0, W_WORDS * sizeof(u64), st));
  HIP_TRY(hipMemsetAsync(tm->words + W_BAD, 0xff, sizeof(u64), st));
  HIP_TRY(hipEventRecord(tm->ev[0], st));
  k_tm_validate<<<(u32) div_up(T, TM_THREADS), TM_THREADS, 0, st>>>(tm->tags.sym, tm->tags.off, T, K, tm->sigma, tm->words);
  HIP_TRY(hipGetLastError());
  u64 found = 0;
  TRY(fetch(st, { { tm->words + W_BAD, &found, sizeof found } }));
  if (found != ~0ull) return refuse_tag(tm, found, K);
  HIP_TRY(hipMemsetAsync(tm->kbest, 0xff, T * sizeof(u32), st));
  for (u32 k = (tm->flags & GTAMD_TAGMATCH_BEST) ? 0 : K; k <= K; k++) {
    if constexpr (std::is_void<S>::value)
      k_tm_walk_pck<false><<<(u32) div_up(jobs, TM_WAVES), TM_THREADS, 0, st>>>(input_pck(tm), 0, jobs, k, tm->kbest, tm->jo.cnt,
                                                                              nullptr, 0, 0, nullptr, tm->words);
    else
      k_tm_walk<S, false><<<(u32) div_up(jobs, TM_WAVES), TM_THREADS, 0, st>>>(input<S>(tm), 0, jobs, k, tm->kbest, tm->jo.cnt,
                                                                             nullptr, 0, 0, nullptr, tm->words);
    HIP_TRY(hipGetLastError());
    k_tm_settle<<<(u32) div_up(T, TM_THREADS), TM_THREADS, 0, st>>>(tm->jo.cnt, per_tag, T, k, tm->kbest);
    HIP_TRY(hipGetLastError());
  }
  u64 h[W_WORDS];
  return finish_count(tm, tm->jo, jobs, h, W_ERROR, &tm->info);
}

// the walk of the jobs [j0, j1) that writes the records [cur, w1) to dst
void launch_emit(gtamd_tagmatch *tm, u64 j0, u64 j1, u64 cur, u64 w1, TmRecord *dst) {
  const u32 blocks = (u32) div_up(j1 - j0, TM_WAVES);
  if (tm->index.pck != nullptr)
    k_tm_walk_pck<true><<<blocks, TM_THREADS, 0, tm->st>>>(input_pck(tm), j0, j1, 0, tm->kbest, nullptr, tm->jo.off, cur, w1,
                                                           dst, tm->words);
  else if (tm->index.tab.suf_bytes == 4)
    k_tm_walk<u32, true><<<blocks, TM_THREADS, 0, tm->st>>>(input<u32>(tm), j0, j1, 0, tm->kbest, nullptr, tm->jo.off, cur,
                                                             w1, dst, tm->words);
  else
    k_tm_walk<u64, true><<<blocks, TM_THREADS, 0, tm->st>>>(input<u64>(tm), j0, j1, 0, tm->kbest, nullptr, tm->jo.off, cur,
                                                             w1, dst, tm->words);
}

}  // namespace

extern "C" gtamd_tagmatch *gtamd_tagmatch_create(int device) {
  GTAMD_ABI_BEGIN
  return create_consumer<gtamd_tagmatch>(device, W_WORDS, "the tag matcher");
  GTAMD_ABI_END(nullptr)
}

extern "C" void gtamd_tagmatch_destroy(gtamd_tagmatch *tm) { destroy_consumer(tm); }

extern "C" void gtamd_tagmatch_geometry(uint32_t *jobs_per_workgroup, uint64_t *min_capacity, uint32_t *max_levels) {
  if (jobs_per_workgroup != nullptr) *jobs_per_workgroup = TM_WAVES;
  if (min_capacity != nullptr) *min_capacity = TM_MIN_CAPACITY;
  if (max_levels != nullptr) *max_levels = TM_LEVELS;
}

extern "C" int gtamd_tagmatch_set_index(gtamd_tagmatch *tm, const uint8_t *enc, uint64_t n, const void *suf,
                                        uint32_t suf_bytes, uint32_t numofchars) {
  GTAMD_ABI_BEGIN
  return set_index(tm, IndexView{ enc, n, suf, suf_bytes }, numofchars, false);
  GTAMD_ABI_END(-1)
}

extern "C" int gtamd_tagmatch_set_index_host(gtamd_tagmatch *tm, const uint8_t *enc, uint64_t n, const void *suf,
                                             uint32_t suf_bytes, uint32_t numofchars) {
  GTAMD_ABI_BEGIN
  return set_index(tm, IndexView{ enc, n, suf, suf_bytes }, numofchars, true);
  GTAMD_ABI_END(-1)
}

extern "C" int gtamd_tagmatch_set_index_esa(gtamd_tagmatch *tm, const gtamd_esa_ctx *esa, const uint8_t *enc,
                                            uint64_t n, uint32_t numofchars) {
  GTAMD_ABI_BEGIN
  if (tm == nullptr || esa == nullptr) { gtamd_set_error("invalid argument to gtamd_tagmatch_set_index_esa"); return -1; }
  IndexView v;
  TRY(engine_tables(FEATURE, esa, enc, n, false, &v));
  return set_index(tm, v, numofchars, false);
  GTAMD_ABI_END(-1)
}

extern "C" int gtamd_tagmatch_set_index_pckidx(gtamd_tagmatch *tm, const gtamd_pckidx *px) {
  GTAMD_ABI_BEGIN
  TRY(IndexSlot::refuse_reader(FEATURE, "tagmatch", "the matcher", tm, px));
  const u32 sigma = pckidx_dec(px).sigma;
  if (sigma == 0 || sigma > TM_LETTERS) {
    gtamd_set_error("tag matches: an alphabet of %u letters, 1 to %u expected", sigma, TM_LETTERS);
    return -1;
  }
  HIP_TRY(hipSetDevice(tm->device));
  tm->prepared = false;
  tm->index.set_reader(px);
  tm->sigma = sigma;
  return 0;
  GTAMD_ABI_END(-1)
}

extern "C" int gtamd_tagmatch_prepare(gtamd_tagmatch *tm, const uint8_t *tags, const uint64_t *offsets, uint64_t T,
                                      int is_device, uint32_t K, uint32_t flags, gtamd_tagmatch_info *info) {
  GTAMD_ABI_BEGIN
  if (tm == nullptr || (T != 0 && (tags == nullptr || offsets == nullptr))) {
    gtamd_set_error("invalid argument to gtamd_tagmatch_prepare");
    return -1;
  }
  TRY(tm->index.refuse_unset(FEATURE, "tagmatch"));
  if (tm->index.pck != nullptr) {
    TRY(tm->index.refuse_lost_reader(FEATURE));
    if (flags & GTAMD_TAGMATCH_WITH_WILDCARDS) {
      gtamd_set_error("tag matches: GTAMD_TAGMATCH_WITH_WILDCARDS is not taken with a packed index as the index "
                      "(include/gtamd_pcktag.h)");
      return -1;
    }
  }
  const u32 known = TM_STRANDS | GTAMD_TAGMATCH_BEST | GTAMD_TAGMATCH_WITH_WILDCARDS;
  if ((flags & ~known) != 0 || (flags & TM_STRANDS) == 0) {
    gtamd_set_error("tag matches: flags 0x%x, an OR of GTAMD_TAGMATCH_* with at least one strand expected", flags);
    return -1;
  }
  if ((flags & GTAMD_TAGMATCH_REVCOMP) && tm->sigma != 4) {
    gtamd_set_error("tag matches: the reverse-complement strand (GTAMD_TAGMATCH_REVCOMP) is defined for an "
                    "alphabet of 4 letters only, this index has %u", tm->sigma);
    return -1;
  }
  if ((flags & GTAMD_TAGMATCH_WITH_WILDCARDS) && K == 0) {
    gtamd_set_error("tag matches: GTAMD_TAGMATCH_WITH_WILDCARDS is taken only with K > 0");
    return -1;
  }
  if (K >= TM_MAX_TAG) {
    gtamd_set_error("tag matches: %u differences, at most %u (tags have at most %u letters)", K, TM_MAX_TAG - 1,
                    TM_MAX_TAG);
    return -1;
  }
  if (T > TM_MAX_TAGS) {
    gtamd_set_error("tag matches: %llu tags, at most %llu in one call", (unsigned long long) T,
                    (unsigned long long) TM_MAX_TAGS);
    return -1;
  }
  HIP_TRY(hipSetDevice(tm->device));
  tm->prepared = false;
  if (tm->index.pck != nullptr) tm->index.stamp();
  tm->info = gtamd_tagmatch_info();
  tm->T = T;
  tm->flags = flags;
  tm->jobs = T * ((flags & TM_STRANDS) == TM_STRANDS ? 2 : 1);
  tm->info.jobs = tm->jobs;
  tm->jo.off_host.assign(1, 0);
  if (T != 0) {
    if (tm->jo.grow(tm->jobs) != hipSuccess || tm->kbest.grow(T * 4) != hipSuccess)
      return out_of_memory(FEATURE, tm->jobs, "jobs");
    TRY(tm->tags.set(FEATURE, "tag symbols", tags, offsets, T, is_device, tm->st));
    TRY(tm->index.pck != nullptr ? prepare<void>(tm, K) : tm->index.tab.suf_bytes == 4 ? prepare<u32>(tm, K) : prepare<u64>(tm, K));
  }
  tm->info.device_bytes = held_bytes(tm);
  tm->prepared = true;
  if (info != nullptr) *info = tm->info;
  return 0;
  GTAMD_ABI_END(-1)
}

extern "C" int gtamd_tagmatch_emit(gtamd_tagmatch *tm, uint64_t *cursor, gtamd_tagmatch_record *out, uint64_t capacity,
                                   int out_on_device, uint64_t *written) {
  GTAMD_ABI_BEGIN
  if (tm == nullptr || cursor == nullptr || written == nullptr || (out == nullptr && capacity)) {
    gtamd_set_error("invalid argument to gtamd_tagmatch_emit");
    return -1;
  }
  if (!tm->prepared) {
    gtamd_set_error("tag matches: nothing is prepared (gtamd_tagmatch_prepare)");
    return -1;
  }
  HIP_TRY(hipSetDevice(tm->device));
  TRY(emit_jobs<TmRecord>(FEATURE, "gtamd_tagmatch_prepare", tm->index, tm->jo, tm->info.matches, cursor, capacity,
                          TM_MIN_CAPACITY, out, out_on_device, tm->out, tm->st, tm->words + W_ERROR, written,
                          [tm](u64 j0, u64 j1, u64 cur, u64 w1, TmRecord *dst) { launch_emit(tm, j0, j1, cur, w1, dst); }));
  tm->info.emitted += *written;
  tm->info.device_bytes = held_bytes(tm);
  return 0;
  GTAMD_ABI_END(-1)
}

extern "C" int gtamd_tagmatch_best_k(gtamd_tagmatch *tm, uint32_t *k_host, uint64_t T) {
  GTAMD_ABI_BEGIN
  if (tm == nullptr || (k_host == nullptr && T)) { gtamd_set_error("invalid argument to gtamd_tagmatch_best_k"); return -1; }
  if (!tm->prepared || T != tm->T) {
    gtamd_set_error("tag matches: K' of %llu tags asked for, %llu are prepared", (unsigned long long) T,
                    (unsigned long long) (tm->prepared ? tm->T : 0));
    return -1;
  }
  HIP_TRY(hipSetDevice(tm->device));
  return fetch(tm->st, { { tm->kbest, k_host, T * sizeof(u32) } });
  GTAMD_ABI_END(-1)
}

extern "C" int gtamd_tagmatch_get_info(const gtamd_tagmatch *tm, gtamd_tagmatch_info *info) {
  GTAMD_ABI_BEGIN
  return consumer_info(tm, info, "gtamd_tagmatch_get_info");
  GTAMD_ABI_END(-1)
}
