// esa_jobs.h -- what the consumers share that walk an index job by job, one wave
// a job (esa_tagmatch.hip, esa_locali.hip): what a counting walk
// reports and the tail of its pass, the 64-bit places of the jobs' records, the
// window of records of an emit pass and the pass itself, the sequences the jobs
// are made of.  The lane code of the walk over the intervals of .suf is
// esa_ivwalk.h, that of the walk over intervals of rows of a packed index
// esa_pckidx_dec.h, with the step that needs the window here.  Beside esa_index.h,
// which is host code for every consumer: this has device code, for those with
// jobs.  Only .hip files include it.
#pragma once
#include <algorithm>
#include <vector>
#include "esa_index.h"
#include "esa_prims.h"
#include "esa_devutil.h"
#include "esa_pckidx_dec.h"

// ---- the kernels' side ---------------------------------------------------------
// the words every walk reports through; a consumer's own words follow, one of
// them the error word of a walk over a packed index (esa_pckidx_core.h)
enum { W_MATCHES = 0, W_MAXJOB, W_LEVELS, W_CHILDREN, W_WALKS, W_WALK_WORDS };

// lane 0 of a counting walk: the k matches of job j, and what the walk took
__device__ __forceinline__ void report(u64 *w, u32 *cnt, u64 j, u64 k, u32 pushed, u32 children, u32 walks) {
  cnt[j] = (u32) k;                               // (at most one match per table entry: below 2^32)
  if (k) atomicMax((unsigned long long *) &w[W_MAXJOB], (unsigned long long) k);
  if (pushed) atomicAdd((unsigned long long *) &w[W_LEVELS], (unsigned long long) pushed);
  if (children) atomicAdd((unsigned long long *) &w[W_CHILDREN], (unsigned long long) children);
  if (walks) atomicAdd((unsigned long long *) &w[W_WALKS], (unsigned long long) walks);
}

// the records of type R a wave has found for its job, and where they go
template <typename R> struct JobWindow {
  u64 k;                 // records of the job so far
  u64 first, stop;       // EMIT: the records [first, stop) of the job are written ...
  R *dst;                // ... record `first` here

  // EMIT: records [w0, w1) of all jobs go to out, record w0 first; false: job j has none of them
  __device__ __forceinline__ bool open(const u64 *off, u64 j, u64 w0, u64 w1, R *out) {
    const u64 base = off[j], after = off[j + 1];
    if (after <= w0 || base >= w1 || after == base) return false;
    first = w0 > base ? w0 - base : 0;
    stop = (w1 < after ? w1 : after) - base;
    dst = out + (base + first - w0);
    return true;
  }
  __device__ __forceinline__ bool full() const { return k >= stop; }
  // `keep` lanes have a record each, in table order: counted, and written where
  // they fall into the window
  template <bool EMIT> __device__ __forceinline__ void give(bool keep, const R &record) {
    const u64 mask = __ballot(keep);
    if (EMIT && keep) {
      const u64 place = k + lanes_before(mask);
      if (place >= first && place < stop) dst[place - first] = record;
    }
    k += (u64) __popcll(mask);
  }
};

// rows of a packed index a wave locates at once, one a lane
constexpr u32 DEC_BATCH = 64;

// All rows [clo, chi) of a child match with `len` letters: counted, and in emit
// located DEC_BATCH at a time, those whose records lie in front of the window
// skipped by arithmetic.  make(p): the record of a row with dbstart p.
template <bool EMIT, typename R, typename Make>
__device__ __forceinline__ void dec_rows(const PkxDec &d, JobWindow<R> &wk, u32 clo, u32 chi, u32 len, u32 lane,
                                         u32 *err, Make make) {
  if (!EMIT) { wk.k += chi - clo; return; }
  u32 b = clo;
  if (wk.k < wk.first) {
    const u64 skip = wk.first - wk.k < chi - clo ? wk.first - wk.k : chi - clo;
    b += (u32) skip;
    wk.k += skip;
  }
  for (; b < chi; b += DEC_BATCH) {
    if (wk.full()) break;
    const u32 row = b + lane;                         // (chi <= N <= 2^32 - 4096: no wrap)
    const u64 place = wk.k + lane;
    u64 p = 0;
    if (row < chi && place >= wk.first && place < wk.stop) p = dec_dbstart(d, row, len, err);
    wk.template give<EMIT>(row < chi, make(p));
  }
}

// ---- the host side -------------------------------------------------------------
// the counts of the jobs and the places of their first records
struct JobOffsets {
  Dev<u32> cnt; Dev<u64> tsum, off;
  std::vector<u64> off_host;      // off, on the host: which jobs a window needs

  hipError_t grow(u64 jobs) {
    if (cnt.grow(jobs * 4) != hipSuccess || off.grow((jobs + 1) * 8) != hipSuccess) return hipErrorOutOfMemory;
    return tsum.grow(div_up(jobs, SC_THREADS) * 8);
  }
  // off[j] = the counts in front of job j, *total_dev = off[jobs]; no wait
  int scan(u64 jobs, u64 *total_dev, hipStream_t st) { return offsets_u64_counted(cnt, jobs, tsum, off, total_dev, st); }
  // an item of fetch(): off_host = off
  Fetch fetch(u64 jobs) {
    off_host.resize(jobs + 1);
    return Fetch{ off, off_host.data(), (jobs + 1) * sizeof(u64) };
  }
  // the jobs [*j0, *j1) with a record in [cur, w1): from the last whose first record
  // is not behind cur up to the first whose first record is not in front of w1
  void jobs_of(u64 cur, u64 w1, u64 *j0, u64 *j1) const {
    *j0 = (u64) (std::upper_bound(off_host.begin(), off_host.end(), cur) - off_host.begin()) - 1;
    *j1 = (u64) (std::lower_bound(off_host.begin(), off_host.end(), w1) - off_host.begin());
  }
  u64 bytes() const { return cnt.bytes + tsum.bytes + off.bytes; }
};

// T sequences, number t the symbols [off[t], off[t + 1]): the caller's device
// memory, or buffers of its own filled from host memory on the stream
struct SequenceSet {
  Dev<u8> own_sym; Dev<u64> own_off;
  const u8 *sym = nullptr; const u64 *off = nullptr;

  // what: "tag symbols", for the message
  int set(const char *feature, const char *what, const u8 *symbols, const u64 *offsets, u64 T, int is_device,
          hipStream_t st) {
    sym = symbols; off = offsets;
    if (is_device) return 0;
    const u64 count = offsets[T];
    if (own_sym.grow(count ? count : 1) != hipSuccess || own_off.grow((T + 1) * 8) != hipSuccess)
      return out_of_memory(feature, count, what);
    if (count) HIP_TRY(hipMemcpyAsync(own_sym, symbols, count, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(own_off, offsets, (T + 1) * 8, hipMemcpyHostToDevice, st));
    sym = own_sym; off = own_off;
    return 0;
  }
  u64 bytes() const { return own_sym.bytes + own_off.bytes; }
};

// The tail of a counting pass over `jobs` jobs of consumer c, whose walks have been
// launched behind ev[0]: the places of the jobs' records, h = the words, with one
// wait, and what every walk reports to the fields every job walker's info has.
// w_error: which word is the error word of a walk over a packed index.
template <typename C, size_t WORDS, typename I>
int finish_count(C *c, JobOffsets &jo, u64 jobs, u64 (&h)[WORDS], u32 w_error, I *info) {
  TRY(jo.scan(jobs, c->words + W_MATCHES, c->st));
  HIP_TRY(hipEventRecord(c->ev[1], c->st));
  TRY(fetch(c->st, { { c->words, h, sizeof h }, jo.fetch(jobs) }));
  if (h[w_error]) { pckidx_set_search_error(h[w_error]); return -1; }
  HIP_TRY(hipEventElapsedTime(&info->device_ms, c->ev[0], c->ev[1]));
  info->matches = h[W_MATCHES];
  info->max_matches_of_one_job = h[W_MAXJOB];
  info->levels_pushed = h[W_LEVELS];
  info->children_examined = h[W_CHILDREN];
  info->single_walks = h[W_WALKS];
  return 0;
}

// One emit call of a job walker: the records [*cursor, *cursor + *written) of the
// `total` that `prepare_fn` (its name, for the messages) counted, at most
// `capacity`, which is at least `least`, to `out` -- through `buf` where that is
// host memory.  launch(j0, j1, cur, w1, dst) launches the walk of the jobs
// [j0, j1) that writes the records [cur, w1) to dst.  `error`: the error word of a
// walk over a packed index, device memory.
template <typename R, typename Launch>
int emit_jobs(const char *feature, const char *prepare_fn, const IndexSlot &index, const JobOffsets &jo, u64 total,
              u64 *cursor, u64 capacity, u64 least, void *out, int out_on_device, Dev<u8> &buf, hipStream_t st,
              u64 *error, u64 *written, Launch launch) {
  *written = 0;
  const u64 cur = *cursor;
  if (index.pck != nullptr) {
    TRY(index.refuse_lost_reader(feature));
    TRY(index.refuse_other_image(feature, prepare_fn));
    TRY(index.refuse_no_locate(feature, "positions cannot be had from it, only the counts of ", prepare_fn));
  }
  TRY(refuse_window(feature, "records", cur, total, capacity, least));
  if (cur == total) return 0;
  const u64 w1 = capacity < total - cur ? cur + capacity : total;
  u64 j0, j1;
  jo.jobs_of(cur, w1, &j0, &j1);
  RecordStage<R> stage(out, out_on_device);
  if (stage.begin(buf, w1 - cur) != hipSuccess) return out_of_memory(feature, w1 - cur, "records");
  if (index.pck != nullptr) HIP_TRY(hipMemsetAsync(error, 0, sizeof(u64), st));
  launch(j0, j1, cur, w1, stage.dst);
  HIP_TRY(hipGetLastError());
  TRY(stage.finish(w1 - cur, st));
  if (index.pck != nullptr) {
    u64 found = 0;
    TRY(fetch(st, { { error, &found, sizeof found } }));
    if (found) { pckidx_set_search_error(found); return -1; }
  }
  *cursor = w1;
  *written = w1 - cur;
  return 0;
}
