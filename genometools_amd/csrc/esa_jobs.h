// esa_jobs.h -- what the consumers share that walk the intervals of .suf job by
// job, one wave a job (esa_tagmatch.hip, esa_locali.hip): what a
// counting walk reports, the 64-bit places of the jobs' records, the window of
// records of an emit pass, the sequences the jobs are made of.  The lane code of
// the walk is esa_ivwalk.h.  Beside esa_index.h, which is host code for every
// consumer: this has device code, for those with jobs.  Only .hip files include it.
#pragma once
#include <algorithm>
#include <vector>
#include "esa_index.h"
#include "esa_prims.h"
#include "esa_devutil.h"

// ---- the kernels' side ---------------------------------------------------------
// the words every walk reports through; a consumer's own words follow
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
      const u32 before = __builtin_amdgcn_mbcnt_hi((u32) (mask >> 32), __builtin_amdgcn_mbcnt_lo((u32) mask, 0u));
      const u64 place = k + before;
      if (place >= first && place < stop) dst[place - first] = record;
    }
    k += (u64) __popcll(mask);
  }
};

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
