// esa_spm.hip -- all suffix-prefix matches of a sequence set from .suf and .lcp
// in device memory: `gt encseq2spm -l L -spm show|count` (C ABI, the semantics
// and the algorithm: include/gtamd_spm.h).
//
//   1, 2  k_sp_select<false>   one lane per table entry and position: terminal
//                              suffix, read start, separator; counted per tile;
//                              scans (esa_prims)
//         k_sp_select<true>    the same lanes write the three lists, in order
//   3     k_sp_intervals       one lane per terminal suffix: its interval
//                              (esa_spm_core.h) and the read starts inside it
//   4     offsets_u64 (esa_prims)     64-bit exclusive scan of those numbers
//   5     k_sp_emit            one lane per (terminal suffix, read start) pair
//                              of a chunk: every one is a record
//
// Every working array has one entry per terminal suffix, per read start, per
// separator or per tile; none has N.
#include "esa_common.h"
#include "esa_index.h"
#include "esa_prims.h"
#include "esa_devutil.h"
#include "esa_spm_core.h"
#include "esa_spm_state.h"

namespace {

constexpr int SP_THREADS = SC_THREADS;
constexpr u32 SP_WAVES = SP_THREADS / 64;
constexpr u32 SP_PER = 4;                         // items of one lane in a select pass, SP_THREADS apart
constexpr u32 SP_SEL_TILE = SP_THREADS * SP_PER;  // items of one workgroup there
constexpr u32 SP_TILE = SP_THREADS;               // terminal suffixes, or candidates, of one workgroup: one a lane
constexpr u64 SP_MIN_CAPACITY = SP_TILE;          // the smallest capacity of an emit call
constexpr u64 SP_MAX_CHUNK = 1ull << 24;          // candidates of one launch: 65536 workgroups

enum { K_TERMINAL = 0, K_START, K_SEPARATOR, K_KINDS };
enum { W_MATCHES = 0, W_MAXWIDTH, W_MAXCOUNT, W_SEARCH, W_WORDS };

// ---- steps 1 and 2 -------------------------------------------------------------
// Item blockIdx.x * SP_SEL_TILE + e * SP_THREADS + threadIdx.x, e < SP_PER, is a
// table entry (below N) and a position (below n).  WRITE false: tiles[kind *
// stride + b] = the selected items of a kind in workgroup b.  WRITE true: that
// word is where they go in their list; they are written in item order, the place
// of each from the ballots of its wave and the counts of the groups in front.
template <typename S, bool WRITE>
__global__ __launch_bounds__(SP_THREADS) void k_sp_select(SpIndex<S> x, u32 L, u32 *tiles, u64 stride, SpLists out) {
  __shared__ u32 groups[K_KINDS][SP_PER * SP_WAVES];
  const u32 wave = threadIdx.x >> 6;
  const u64 base = (u64) blockIdx.x * SP_SEL_TILE + threadIdx.x, N = x.n + 1;
  u32 h[SP_PER], before[K_KINDS][SP_PER];
  bool sel[K_KINDS][SP_PER];
#pragma unroll
  for (u32 e = 0; e < SP_PER; e++) {
    const u64 i = base + (u64) e * SP_THREADS;
    h[e] = 0;
    sel[K_TERMINAL][e] = i < N && sp_terminal(x, i, L, &h[e]);
    sel[K_START][e] = i < N && sp_read_start(x, i);
    sel[K_SEPARATOR][e] = i < x.n && x.enc[i] == 255;
#pragma unroll
    for (u32 k = 0; k < K_KINDS; k++) {
      const u64 mask = __ballot(sel[k][e]);
      before[k][e] = lanes_before(mask);
      if ((threadIdx.x & 63) == 0) groups[k][e * SP_WAVES + wave] = (u32) __popcll(mask);
    }
  }
  __syncthreads();
  if (threadIdx.x < K_KINDS) {
    // WRITE: every group's count becomes the place of its first item
    u32 run = WRITE ? tiles[threadIdx.x * stride + blockIdx.x] : 0;
    for (u32 g = 0; g < SP_PER * SP_WAVES; g++) {
      const u32 v = groups[threadIdx.x][g];
      groups[threadIdx.x][g] = run;
      run += v;
    }
    if (!WRITE) tiles[threadIdx.x * stride + blockIdx.x] = run;
  }
  if (!WRITE) return;
  __syncthreads();
#pragma unroll
  for (u32 e = 0; e < SP_PER; e++) {
    const u64 i = base + (u64) e * SP_THREADS;
    const u32 g = e * SP_WAVES + wave;
    if (sel[K_TERMINAL][e]) {
      const u32 at = groups[K_TERMINAL][g] + before[K_TERMINAL][e];
      out.idx[at] = (u32) i;
      out.len[at] = h[e];
    }
    if (sel[K_START][e]) out.starts[groups[K_START][g] + before[K_START][e]] = (u32) i;
    if (sel[K_SEPARATOR][e]) out.seps[groups[K_SEPARATOR][g] + before[K_SEPARATOR][e]] = (u32) i;
  }
}

// ---- step 3 ----------------------------------------------------------------------
template <typename S>
__global__ __launch_bounds__(SP_THREADS) void k_sp_intervals(SpIndex<S> x, const u32 *idx, const u32 *len, u32 M,
                                                             const u32 *starts, u32 R, u32 *first, u32 *cnt,
                                                             u64 *tsum, u64 *w) {
  __shared__ unsigned long long ssum, ssearch;
  __shared__ u32 swidth, scount;
  if (threadIdx.x == 0) { ssum = 0; ssearch = 0; swidth = 0; scount = 0; }
  __syncthreads();
  const u64 k = (u64) blockIdx.x * SP_TILE + threadIdx.x;
  if (k < M) {
    u32 lo, width, f;
    u64 compared = 0;
    sp_interval(x, (u64) idx[k], len[k], &lo, &width, &compared);
    const u32 c = sp_starts_inside(starts, R, lo, width, &f);
    first[k] = f;
    cnt[k] = c;
    atomicMax(&swidth, width);
    if (c) { atomicAdd(&ssum, (unsigned long long) c); atomicMax(&scount, c); }
    if (compared) atomicAdd(&ssearch, (unsigned long long) compared);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    tsum[blockIdx.x] = ssum;
    atomicMax((unsigned long long *) &w[W_MAXWIDTH], (unsigned long long) swidth);
    if (scount) atomicMax((unsigned long long *) &w[W_MAXCOUNT], (unsigned long long) scount);
    if (ssearch) atomicAdd((unsigned long long *) &w[W_SEARCH], ssearch);
  }
}

// ---- step 5 ----------------------------------------------------------------------
// records [c0, c1) of all off[M] to out, SP_TILE a workgroup
template <typename S>
__global__ __launch_bounds__(SP_THREADS) void k_sp_emit(SpIndex<S> x, SpLists l, const u32 *first, const u64 *off, u32 M,
                                                        u32 nseps, u64 c0, u64 c1, SpRecord *out) {
  __shared__ u64 span[2];                 // the terminal suffixes of the workgroup's first and last record
  const u64 g0 = c0 + (u64) blockIdx.x * SP_TILE;
  const u64 last = (c1 - g0 < SP_TILE ? c1 : g0 + SP_TILE) - 1;
  if (threadIdx.x < 2) span[threadIdx.x] = entry_of(off, 0, M, threadIdx.x == 0 ? g0 : last);
  __syncthreads();
  const u64 g = g0 + threadIdx.x;
  if (g > last) return;
  const u64 k = entry_of(off, span[0], span[1] + 1, g);
  SpRecord rec;
  sp_record(x, l.starts, l.seps, nseps, l.idx[k], l.len[k], first[k], g - off[k], &rec);
  out[g - c0] = rec;
}

}  // namespace

namespace {

const char FEATURE[] = "suffix-prefix matches";

// every way of setting an index: what is refused, before anything is touched
int set_index(gtamd_spm *sp, const IndexView &v, bool from_host) {
  if (sp == nullptr || v.suf == nullptr || (v.enc == nullptr && v.n) || (v.llv == nullptr && v.llv_pairs)) {
    gtamd_set_error("invalid argument to gtamd_spm_set_index");
    return -1;
  }
  if (v.lcp == nullptr) {
    gtamd_set_error("suffix-prefix matches: no .lcp table is given: the matches are found from .suf and .lcp together");
    return -1;
  }
  TRY(refuse_suf_bytes(FEATURE, v.suf_bytes));
  TRY(refuse_sizes(FEATURE, v.n, v.llv_pairs));
  HIP_TRY(hipSetDevice(sp->device));
  sp->prepared = false;
  if (from_host) return sp->index.upload_from_host(FEATURE, v);
  sp->index.borrow(v);
  return 0;
}

u64 held_bytes(const gtamd_spm *sp) {
  return sp->index.bytes() + sp->tiles.bytes + sp->scanws.bytes + sp->idx.bytes + sp->len.bytes + sp->starts.bytes +
         sp->seps.bytes + sp->first.bytes + sp->cnt.bytes + sp->tsum.bytes + sp->off.bytes + sp->words.bytes +
         sp->out.bytes;
}

template <typename S> SpIndex<S> view(const gtamd_spm *sp) {
  const ResidentIndex &x = sp->index;
  return SpIndex<S>{ x.enc, x.n, (const S *) x.suf, x.lcp, x.llv, x.llv_pairs };
}

SpLists lists(const gtamd_spm *sp) { return SpLists{ sp->idx, sp->len, sp->starts, sp->seps }; }

template <typename S> int prepare(gtamd_spm *sp, u32 L) {
  hipStream_t st = sp->st;
  const u64 N = sp->index.n + 1, T = div_up(N, SP_SEL_TILE), stride = T + 1;
  if (sp->tiles.grow(K_KINDS * stride * sizeof(u32)) != hipSuccess ||
      sp->scanws.grow(scan_workspace_words(stride) * sizeof(u32)) != hipSuccess)
    return out_of_memory(FEATURE, stride, "tiles");
  HIP_TRY(hipMemsetAsync(sp->words, 0, W_WORDS * sizeof(u64), st));
  HIP_TRY(hipMemsetAsync(sp->tiles, 0, K_KINDS * stride * sizeof(u32), st));
  HIP_TRY(hipEventRecord(sp->ev[0], st));

  // 1, 2: the terminal suffixes, the read starts, the separators
  k_sp_select<S, false><<<(u32) T, SP_THREADS, 0, st>>>(view<S>(sp), L, sp->tiles, stride, SpLists());
  HIP_TRY(hipGetLastError());
  for (u32 k = 0; k < K_KINDS; k++)
    TRY(scan_u32(SCAN_SUM, sp->tiles + k * stride, sp->tiles + k * stride, stride, false, sp->scanws, st));
  u32 M, R, nseps;
  TRY(fetch(st, { { sp->tiles + K_TERMINAL * stride + T, &M, sizeof M }, { sp->tiles + K_START * stride + T, &R, sizeof R },
                  { sp->tiles + K_SEPARATOR * stride + T, &nseps, sizeof nseps } }));
  const u32 tiles = (u32) div_up(M, SP_TILE);
  if (sp->idx.grow((M ? (u64) M : 1) * 4) != hipSuccess || sp->len.grow((M ? (u64) M : 1) * 4) != hipSuccess ||
      sp->first.grow((M ? (u64) M : 1) * 4) != hipSuccess || sp->cnt.grow((M ? (u64) M : 1) * 4) != hipSuccess ||
      sp->off.grow(((u64) M + 1) * 8) != hipSuccess || sp->tsum.grow((tiles ? (u64) tiles : 1) * 8) != hipSuccess)
    return out_of_memory(FEATURE, M, "terminal suffixes");
  if (sp->starts.grow((R ? (u64) R : 1) * 4) != hipSuccess || sp->seps.grow((nseps ? (u64) nseps : 1) * 4) != hipSuccess)
    return out_of_memory(FEATURE, (u64) R + nseps, "read starts and separators");
  sp->M = M; sp->R = R; sp->nseps = nseps;
  k_sp_select<S, true><<<(u32) T, SP_THREADS, 0, st>>>(view<S>(sp), L, sp->tiles, stride, lists(sp));
  HIP_TRY(hipGetLastError());

  if (M != 0) {
    // 3, 4: the read starts inside every interval, and their places
    k_sp_intervals<S><<<tiles, SP_THREADS, 0, st>>>(view<S>(sp), sp->idx, sp->len, M, sp->starts, R, sp->first, sp->cnt,
                                                   sp->tsum, sp->words);
    HIP_TRY(hipGetLastError());
    TRY(offsets_u64(sp->cnt, M, sp->tsum, sp->off, sp->words + W_MATCHES, st));
  }
  HIP_TRY(hipEventRecord(sp->ev[1], st));
  u64 h[W_WORDS];
  TRY(fetch(st, { { sp->words, h, sizeof h } }));
  HIP_TRY(hipEventElapsedTime(&sp->info.device_ms, sp->ev[0], sp->ev[1]));
  sp->info.table_entries = N;
  sp->info.terminal_suffixes = M;
  sp->info.read_starts = R;
  sp->info.matches = h[W_MATCHES];
  sp->info.max_width = h[W_MAXWIDTH];
  sp->info.max_matches_of_one_suffix = h[W_MAXCOUNT];
  sp->info.search_symbols = h[W_SEARCH];
  return 0;
}

template <typename S> int emit_records(gtamd_spm *sp, u64 c0, u64 count, SpRecord *dst) {
  for (u64 done = 0; done < count; done += SP_MAX_CHUNK) {
    const u64 chunk = count - done < SP_MAX_CHUNK ? count - done : SP_MAX_CHUNK;
    k_sp_emit<S><<<(u32) div_up(chunk, SP_TILE), SP_THREADS, 0, sp->st>>>(view<S>(sp), lists(sp), sp->first, sp->off,
                                                                         sp->M, sp->nseps, c0 + done,
                                                                         c0 + done + chunk, dst + done);
    HIP_TRY(hipGetLastError());
  }
  return 0;
}

int emit(gtamd_spm *sp, u64 *cursor, gtamd_spm_record *out, u64 capacity, int out_on_device, u64 *written) {
  *written = 0;
  const u64 Z = sp->info.matches, cur = *cursor;
  TRY(refuse_window(FEATURE, "matches", cur, Z, capacity, SP_MIN_CAPACITY));
  if (cur == Z) return 0;
  const u64 count = capacity < Z - cur ? capacity : Z - cur;
  RecordStage<SpRecord> stage(out, out_on_device);
  if (stage.begin(sp->out, count) != hipSuccess) return out_of_memory(FEATURE, count, "records");
  TRY(sp->index.suf_bytes == 4 ? emit_records<u32>(sp, cur, count, stage.dst)
                               : emit_records<u64>(sp, cur, count, stage.dst));
  TRY(stage.finish(count, sp->st));
  *cursor = cur + count;
  *written = count;
  return 0;
}

}  // namespace

extern "C" gtamd_spm *gtamd_spm_create(int device) {
  GTAMD_ABI_BEGIN
  return create_consumer<gtamd_spm>(device, W_WORDS, "the suffix-prefix matcher");
  GTAMD_ABI_END(nullptr)
}

extern "C" void gtamd_spm_destroy(gtamd_spm *sp) { destroy_consumer(sp); }

extern "C" void gtamd_spm_geometry(uint32_t *tile_suffixes, uint64_t *min_capacity) {
  if (tile_suffixes != nullptr) *tile_suffixes = SP_TILE;
  if (min_capacity != nullptr) *min_capacity = SP_MIN_CAPACITY;
}

extern "C" int gtamd_spm_set_index(gtamd_spm *sp, const uint8_t *enc, uint64_t n, const void *suf, uint32_t suf_bytes,
                                   const uint8_t *lcp, const uint64_t *llv, uint64_t llv_pairs) {
  GTAMD_ABI_BEGIN
  return set_index(sp, IndexView{ enc, n, suf, suf_bytes, lcp, llv, llv_pairs }, false);
  GTAMD_ABI_END(-1)
}

extern "C" int gtamd_spm_set_index_host(gtamd_spm *sp, const uint8_t *enc, uint64_t n, const void *suf,
                                        uint32_t suf_bytes, const uint8_t *lcp, const uint64_t *llv,
                                        uint64_t llv_pairs) {
  GTAMD_ABI_BEGIN
  return set_index(sp, IndexView{ enc, n, suf, suf_bytes, lcp, llv, llv_pairs }, true);
  GTAMD_ABI_END(-1)
}

extern "C" int gtamd_spm_set_index_esa(gtamd_spm *sp, const gtamd_esa_ctx *esa, const uint8_t *enc, uint64_t n) {
  GTAMD_ABI_BEGIN
  if (sp == nullptr || esa == nullptr) { gtamd_set_error("invalid argument to gtamd_spm_set_index_esa"); return -1; }
  IndexView v;
  TRY(engine_tables(FEATURE, esa, enc, n, true, &v));
  return set_index(sp, v, false);
  GTAMD_ABI_END(-1)
}

extern "C" int gtamd_spm_prepare(gtamd_spm *sp, uint32_t min_len, gtamd_spm_info *info) {
  GTAMD_ABI_BEGIN
  if (sp == nullptr) { gtamd_set_error("invalid argument to gtamd_spm_prepare"); return -1; }
  if (!sp->index.set) {
    gtamd_set_error("suffix-prefix matches: no index is set (gtamd_spm_set_index)");
    return -1;
  }
  if (min_len == 0) {
    gtamd_set_error("suffix-prefix matches: a minimum length of 0 is refused, 1 or more expected");
    return -1;
  }
  HIP_TRY(hipSetDevice(sp->device));
  sp->prepared = false;
  sp->info = gtamd_spm_info();
  sp->M = sp->R = sp->nseps = 0;
  TRY(sp->index.suf_bytes == 4 ? prepare<u32>(sp, min_len) : prepare<u64>(sp, min_len));
  sp->info.device_bytes = held_bytes(sp);
  sp->prepared = true;
  if (info != nullptr) *info = sp->info;
  return 0;
  GTAMD_ABI_END(-1)
}

extern "C" int gtamd_spm_emit(gtamd_spm *sp, uint64_t *cursor, gtamd_spm_record *out, uint64_t capacity,
                              int out_on_device, uint64_t *written) {
  GTAMD_ABI_BEGIN
  if (sp == nullptr || cursor == nullptr || written == nullptr || (out == nullptr && capacity)) {
    gtamd_set_error("invalid argument to gtamd_spm_emit");
    return -1;
  }
  if (!sp->prepared) {
    gtamd_set_error("suffix-prefix matches: nothing is prepared (gtamd_spm_prepare)");
    return -1;
  }
  HIP_TRY(hipSetDevice(sp->device));
  TRY(emit(sp, cursor, out, capacity, out_on_device, written));
  sp->info.device_bytes = held_bytes(sp);
  return 0;
  GTAMD_ABI_END(-1)
}

extern "C" int gtamd_spm_get_info(const gtamd_spm *sp, gtamd_spm_info *info) {
  GTAMD_ABI_BEGIN
  return consumer_info(sp, info, "gtamd_spm_get_info");
  GTAMD_ABI_END(-1)
}
