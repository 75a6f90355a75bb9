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
//   4     k_sp_scan64, k_sp_offsets   64-bit exclusive scan of those numbers
//   5     k_sp_emit            one lane per (terminal suffix, read start) pair
//                              of a chunk: every one is a record
//
// Every working array has one entry per terminal suffix, per read start, per
// separator or per tile; none has N.
#include "esa_common.h"
#include "esa_own.h"
#include "esa_prims.h"
#include "esa_devutil.h"
#include "esa_spm_core.h"
#include "../../include/gtamd_spm.h"

namespace {

constexpr int SP_THREADS = SC_THREADS;
constexpr u32 SP_WAVES = SP_THREADS / 64;
constexpr u32 SP_PER = 4;                         // items of one lane in a select pass, SP_THREADS apart
constexpr u32 SP_SEL_TILE = SP_THREADS * SP_PER;  // items of one workgroup there
constexpr u32 SP_TILE = SP_THREADS;               // terminal suffixes, or candidates, of one workgroup: one a lane
constexpr u64 SP_MIN_CAPACITY = SP_TILE;          // the smallest capacity of an emit call
constexpr u64 SP_MAX_CHUNK = 1ull << 24;          // candidates of one launch: 65536 workgroups
constexpr u64 SP_MAX_ENTRIES = (1ull << 32) - 4096;   // single-build limit of esa_engine.hip
constexpr u64 UPLOAD_PIECE = 64ull << 20;

enum { K_TERMINAL = 0, K_START, K_SEPARATOR, K_KINDS };
enum { W_MATCHES = 0, W_MAXWIDTH, W_MAXCOUNT, W_SEARCH, W_WORDS };

// the three lists of steps 1 and 2
struct SpLists {
  u32 *idx, *len;        // terminal suffixes: table index, letters
  u32 *starts;           // read starts: table index
  u32 *seps;             // separators: position
};

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
      before[k][e] = __builtin_amdgcn_mbcnt_hi((u32) (mask >> 32), __builtin_amdgcn_mbcnt_lo((u32) mask, 0u));
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

// ---- step 4 ----------------------------------------------------------------------
// one workgroup: a[i] = sum of a[0..i), *total = the sum of all
__global__ __launch_bounds__(SP_THREADS) void k_sp_scan64(u64 *a, u64 count, u64 *total) {
  __shared__ u64 s[SP_THREADS];
  block_scan_excl_array_u64(a, count, total, s);
}

// off[k] = the records in front of terminal suffix k; off[M] = all
__global__ __launch_bounds__(SP_THREADS) void k_sp_offsets(const u32 *cnt, const u64 *tsum, u32 M, u64 *off) {
  __shared__ u64 s[SP_THREADS];
  const u64 k = (u64) blockIdx.x * SP_TILE + threadIdx.x;
  const u64 v = k < M ? cnt[k] : 0;
  const u64 incl = block_scan_incl_u64(v, s) + tsum[blockIdx.x];
  if (k < M) {
    off[k] = incl - v;
    if (k + 1 == M) off[M] = incl;
  }
}

// ---- step 5 ----------------------------------------------------------------------
// the last terminal suffix of [a, b) whose first record is not behind record g;
// off[a] <= g, and off[b] is not read
__device__ __forceinline__ u64 suffix_of(const u64 *off, u64 a, u64 b, u64 g) {
  while (b - a > 1) {
    const u64 mid = a + (b - a) / 2;
    if (off[mid] <= g) a = mid; else b = mid;
  }
  return a;
}

// records [c0, c1) of all off[M] to out, SP_TILE a workgroup
template <typename S>
__global__ __launch_bounds__(SP_THREADS) void k_sp_emit(SpIndex<S> x, SpLists l, const u32 *first, const u64 *off, u32 M,
                                                        u32 nseps, u64 c0, u64 c1, SpRecord *out) {
  __shared__ u64 span[2];                 // the terminal suffixes of the workgroup's first and last record
  const u64 g0 = c0 + (u64) blockIdx.x * SP_TILE;
  const u64 last = (c1 - g0 < SP_TILE ? c1 : g0 + SP_TILE) - 1;
  if (threadIdx.x < 2) span[threadIdx.x] = suffix_of(off, 0, M, threadIdx.x == 0 ? g0 : last);
  __syncthreads();
  const u64 g = g0 + threadIdx.x;
  if (g > last) return;
  const u64 k = suffix_of(off, span[0], span[1] + 1, g);
  SpRecord rec;
  sp_record(x, l.starts, l.seps, nseps, l.idx[k], l.len[k], first[k], g - off[k], &rec);
  out[g - c0] = rec;
}

}  // namespace

struct gtamd_spm {
  int device = 0;
  Stream st;             // (before the buffers: they go first)
  Event ev[2];
  Dev<u8> own_enc, own_suf, own_lcp;   // an index set from host memory
  Dev<u64> own_llv;
  const u8 *enc = nullptr;             // the index: the caller's, an engine's or the four above
  const void *suf = nullptr;
  const u8 *lcp = nullptr;
  const u64 *llv = nullptr;
  u64 n = 0, llv_pairs = 0;
  u32 suf_bytes = 0;
  bool have_index = false, prepared = false;
  // what a prepare leaves for the emit calls
  Dev<u32> tiles, scanws, idx, len, starts, seps, first, cnt;
  Dev<u64> tsum, off, words;
  Dev<u8> out;                         // records on their way to host memory
  u32 M = 0, R = 0, nseps = 0;
  gtamd_spm_info info = gtamd_spm_info();
};

namespace {

void drop_index(gtamd_spm *sp) {
  sp->have_index = sp->prepared = false;
  sp->own_enc.reset(); sp->own_suf.reset(); sp->own_lcp.reset(); sp->own_llv.reset();
  sp->enc = nullptr; sp->suf = nullptr; sp->lcp = nullptr; sp->llv = nullptr;
}

// what every way of setting an index refuses, before anything is touched
int index_arguments(const gtamd_spm *sp, const void *enc, u64 n, const void *suf, u32 suf_bytes, const void *lcp,
                    const void *llv, u64 llv_pairs) {
  if (sp == nullptr || suf == nullptr || (enc == nullptr && n) || (llv == nullptr && llv_pairs)) {
    gtamd_set_error("invalid argument to gtamd_spm_set_index");
    return -1;
  }
  if (lcp == nullptr) {
    gtamd_set_error("suffix-prefix matches: no .lcp table is given: the matches are found from .suf and .lcp together");
    return -1;
  }
  if (suf_bytes != 4 && suf_bytes != 8) {
    gtamd_set_error("suffix-prefix matches: .suf entries of %u bytes, 4 or 8 expected", suf_bytes);
    return -1;
  }
  if (n >= SP_MAX_ENTRIES) {
    gtamd_set_error("suffix-prefix matches: sequence of %llu symbols is beyond the limit of a single build "
                    "(%llu table entries); the slices of a build in parts are not searched",
                    (unsigned long long) n, (unsigned long long) SP_MAX_ENTRIES);
    return -1;
  }
  if (llv_pairs > n) {
    gtamd_set_error("suffix-prefix matches: %llu .llv pairs for %llu symbols", (unsigned long long) llv_pairs,
                    (unsigned long long) n);
    return -1;
  }
  return 0;
}

void take_index(gtamd_spm *sp, const u8 *enc, u64 n, const void *suf, u32 suf_bytes, const u8 *lcp, const u64 *llv,
                u64 llv_pairs) {
  sp->enc = enc; sp->n = n; sp->suf = suf; sp->suf_bytes = suf_bytes;
  sp->lcp = lcp; sp->llv = llv; sp->llv_pairs = llv_pairs;
  sp->have_index = true;
  sp->prepared = false;
}

// host memory -> a device buffer of its own, piece by piece
template <typename T> int upload(Dev<T> &d, const void *src, u64 bytes, const char *what) {
  if (d.alloc(bytes ? bytes : 1) != hipSuccess) {
    gtamd_set_error("suffix-prefix matches: cannot allocate %llu bytes of device memory for %s",
                    (unsigned long long) bytes, what);
    return -1;
  }
  for (u64 off = 0; off < bytes; off += UPLOAD_PIECE) {
    const u64 cnt = bytes - off < UPLOAD_PIECE ? bytes - off : UPLOAD_PIECE;
    HIP_TRY(hipMemcpy((u8 *) d.p + off, (const u8 *) src + off, cnt, hipMemcpyHostToDevice));
  }
  return 0;
}

u64 held_bytes(const gtamd_spm *sp) {
  return sp->own_enc.bytes + sp->own_suf.bytes + sp->own_lcp.bytes + sp->own_llv.bytes + sp->tiles.bytes +
         sp->scanws.bytes + sp->idx.bytes + sp->len.bytes + sp->starts.bytes + sp->seps.bytes + sp->first.bytes +
         sp->cnt.bytes + sp->tsum.bytes + sp->off.bytes + sp->words.bytes + sp->out.bytes;
}

int out_of_memory(u64 entries, const char *of) {
  gtamd_set_error("suffix-prefix matches: cannot allocate device memory for %llu %s", (unsigned long long) entries, of);
  return -1;
}

template <typename S> SpIndex<S> view(const gtamd_spm *sp) {
  return SpIndex<S>{ sp->enc, sp->n, (const S *) sp->suf, sp->lcp, sp->llv, sp->llv_pairs };
}

SpLists lists(const gtamd_spm *sp) { return SpLists{ sp->idx, sp->len, sp->starts, sp->seps }; }

template <typename S> int prepare(gtamd_spm *sp, u32 L) {
  hipStream_t st = sp->st;
  const u64 N = sp->n + 1, T = div_up(N, SP_SEL_TILE), stride = T + 1;
  if (sp->tiles.grow(K_KINDS * stride * sizeof(u32)) != hipSuccess ||
      sp->scanws.grow(scan_workspace_words(stride) * sizeof(u32)) != hipSuccess)
    return out_of_memory(stride, "tiles");
  HIP_TRY(hipMemsetAsync(sp->words, 0, W_WORDS * sizeof(u64), st));
  HIP_TRY(hipMemsetAsync(sp->tiles, 0, K_KINDS * stride * sizeof(u32), st));
  HIP_TRY(hipEventRecord(sp->ev[0], st));

  // 1, 2: the terminal suffixes, the read starts, the separators
  k_sp_select<S, false><<<(u32) T, SP_THREADS, 0, st>>>(view<S>(sp), L, sp->tiles, stride, SpLists());
  HIP_TRY(hipGetLastError());
  u32 total[K_KINDS];
  for (u32 k = 0; k < K_KINDS; k++) {
    TRY(scan_u32(SCAN_SUM, sp->tiles + k * stride, sp->tiles + k * stride, stride, false, sp->scanws, st));
    HIP_TRY(hipMemcpyAsync(&total[k], sp->tiles + k * stride + T, sizeof(u32), hipMemcpyDeviceToHost, st));
  }
  HIP_TRY(hipStreamSynchronize(st));
  const u32 M = total[K_TERMINAL], R = total[K_START], nseps = total[K_SEPARATOR];
  const u32 tiles = (u32) div_up(M, SP_TILE);
  if (sp->idx.grow((M ? (u64) M : 1) * 4) != hipSuccess || sp->len.grow((M ? (u64) M : 1) * 4) != hipSuccess ||
      sp->first.grow((M ? (u64) M : 1) * 4) != hipSuccess || sp->cnt.grow((M ? (u64) M : 1) * 4) != hipSuccess ||
      sp->off.grow(((u64) M + 1) * 8) != hipSuccess || sp->tsum.grow((tiles ? (u64) tiles : 1) * 8) != hipSuccess)
    return out_of_memory(M, "terminal suffixes");
  if (sp->starts.grow((R ? (u64) R : 1) * 4) != hipSuccess || sp->seps.grow((nseps ? (u64) nseps : 1) * 4) != hipSuccess)
    return out_of_memory((u64) R + nseps, "read starts and separators");
  sp->M = M; sp->R = R; sp->nseps = nseps;
  k_sp_select<S, true><<<(u32) T, SP_THREADS, 0, st>>>(view<S>(sp), L, sp->tiles, stride, lists(sp));
  HIP_TRY(hipGetLastError());

  if (M != 0) {
    // 3, 4: the read starts inside every interval, and their places
    k_sp_intervals<S><<<tiles, SP_THREADS, 0, st>>>(view<S>(sp), sp->idx, sp->len, M, sp->starts, R, sp->first, sp->cnt,
                                                   sp->tsum, sp->words);
    HIP_TRY(hipGetLastError());
    k_sp_scan64<<<1, SP_THREADS, 0, st>>>(sp->tsum, tiles, sp->words + W_MATCHES);
    HIP_TRY(hipGetLastError());
    k_sp_offsets<<<tiles, SP_THREADS, 0, st>>>(sp->cnt, sp->tsum, M, sp->off);
    HIP_TRY(hipGetLastError());
  }
  HIP_TRY(hipEventRecord(sp->ev[1], st));
  u64 h[W_WORDS];
  HIP_TRY(hipMemcpyAsync(h, sp->words, sizeof h, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
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
  if (cur > Z) {
    gtamd_set_error("suffix-prefix matches: cursor %llu is not one of this enumeration (%llu matches)",
                    (unsigned long long) cur, (unsigned long long) Z);
    return -1;
  }
  if (capacity < SP_MIN_CAPACITY) {
    gtamd_set_error("suffix-prefix matches: a capacity of %llu records is too small: a capacity of at least %llu "
                    "is needed", (unsigned long long) capacity, (unsigned long long) SP_MIN_CAPACITY);
    return -1;
  }
  if (cur == Z) return 0;
  const u64 count = capacity < Z - cur ? capacity : Z - cur;
  SpRecord *dst = (SpRecord *) out;
  if (!out_on_device) {
    if (sp->out.grow(count * sizeof(SpRecord)) != hipSuccess) return out_of_memory(count, "records");
    dst = (SpRecord *) sp->out.p;
  }
  TRY(sp->suf_bytes == 4 ? emit_records<u32>(sp, cur, count, dst) : emit_records<u64>(sp, cur, count, dst));
  if (!out_on_device) HIP_TRY(hipMemcpyAsync(out, dst, count * sizeof(SpRecord), hipMemcpyDeviceToHost, sp->st));
  HIP_TRY(hipStreamSynchronize(sp->st));
  *cursor = cur + count;
  *written = count;
  return 0;
}

}  // namespace

extern "C" gtamd_spm *gtamd_spm_create(int device) {
  GTAMD_ABI_BEGIN
  if (gtamd_device_count() <= device || device < 0) {
    gtamd_set_error("no HIP device %d available (this library has no CPU fallback)", device);
    return nullptr;
  }
  if (hipSetDevice(device) != hipSuccess) { gtamd_set_error("hipSetDevice(%d) failed", device); return nullptr; }
  gtamd_spm *sp = new gtamd_spm();
  sp->device = device;
  if (create(sp->st) != hipSuccess || create(sp->ev[0]) != hipSuccess || create(sp->ev[1]) != hipSuccess ||
      sp->words.alloc(W_WORDS * sizeof(u64)) != hipSuccess) {
    gtamd_set_error("cannot create the suffix-prefix matcher on device %d", device);
    delete sp;
    return nullptr;
  }
  return sp;
  GTAMD_ABI_END(nullptr)
}

extern "C" void gtamd_spm_destroy(gtamd_spm *sp) {
  if (sp == nullptr) return;
  (void) hipSetDevice(sp->device);
  (void) hipStreamSynchronize(sp->st);
  delete sp;
}

extern "C" void gtamd_spm_geometry(uint32_t *tile_suffixes, uint64_t *min_capacity) {
  if (tile_suffixes != nullptr) *tile_suffixes = SP_TILE;
  if (min_capacity != nullptr) *min_capacity = SP_MIN_CAPACITY;
}

extern "C" int gtamd_spm_set_index(gtamd_spm *sp, const uint8_t *enc, uint64_t n, const void *suf, uint32_t suf_bytes,
                                   const uint8_t *lcp, const uint64_t *llv, uint64_t llv_pairs) {
  GTAMD_ABI_BEGIN
  TRY(index_arguments(sp, enc, n, suf, suf_bytes, lcp, llv, llv_pairs));
  HIP_TRY(hipSetDevice(sp->device));
  drop_index(sp);
  take_index(sp, enc, n, suf, suf_bytes, lcp, llv, llv_pairs);
  return 0;
  GTAMD_ABI_END(-1)
}

extern "C" int gtamd_spm_set_index_host(gtamd_spm *sp, const uint8_t *enc, uint64_t n, const void *suf,
                                        uint32_t suf_bytes, const uint8_t *lcp, const uint64_t *llv,
                                        uint64_t llv_pairs) {
  GTAMD_ABI_BEGIN
  TRY(index_arguments(sp, enc, n, suf, suf_bytes, lcp, llv, llv_pairs));
  HIP_TRY(hipSetDevice(sp->device));
  drop_index(sp);
  TRY(upload(sp->own_enc, enc, n, "the sequence"));
  TRY(upload(sp->own_suf, suf, (n + 1) * suf_bytes, "the .suf table"));
  TRY(upload(sp->own_lcp, lcp, n + 1, "the .lcp table"));
  TRY(upload(sp->own_llv, llv, llv_pairs * 16, "the .llv table"));
  take_index(sp, sp->own_enc, n, sp->own_suf.p, suf_bytes, sp->own_lcp, sp->own_llv, llv_pairs);
  return 0;
  GTAMD_ABI_END(-1)
}

extern "C" int gtamd_spm_set_index_esa(gtamd_spm *sp, const gtamd_esa_ctx *esa, const uint8_t *enc, uint64_t n) {
  GTAMD_ABI_BEGIN
  if (sp == nullptr || esa == nullptr) { gtamd_set_error("invalid argument to gtamd_spm_set_index_esa"); return -1; }
  const void *suf = gtamd_esa_table_device(esa, GTAMD_TAB_SUF);
  const u8 *lcp = (const u8 *) gtamd_esa_table_device(esa, GTAMD_TAB_LCP);
  const u64 pairs = gtamd_esa_table_entries(esa, GTAMD_TAB_LLV);
  const u64 *llv = pairs ? (const u64 *) gtamd_esa_table_device(esa, GTAMD_TAB_LLV) : nullptr;
  if (suf == nullptr || lcp == nullptr || (pairs && llv == nullptr)) {
    gtamd_set_error("suffix-prefix matches: the last run did not produce the .suf and .lcp tables");
    return -1;
  }
  if (gtamd_esa_table_offset(esa) != 0 || gtamd_esa_table_entries(esa, GTAMD_TAB_SUF) != n + 1) {
    gtamd_set_error("suffix-prefix matches: the context holds %llu entries from table index %llu on, not the "
                    "whole table of %llu symbols; the slices of a build in parts are not searched",
                    (unsigned long long) gtamd_esa_table_entries(esa, GTAMD_TAB_SUF),
                    (unsigned long long) gtamd_esa_table_offset(esa), (unsigned long long) n);
    return -1;
  }
  TRY(index_arguments(sp, enc, n, suf, 8, lcp, llv, pairs));
  HIP_TRY(hipSetDevice(sp->device));
  drop_index(sp);
  take_index(sp, enc, n, suf, 8, lcp, llv, pairs);
  return 0;
  GTAMD_ABI_END(-1)
}

extern "C" int gtamd_spm_prepare(gtamd_spm *sp, uint32_t min_len, gtamd_spm_info *info) {
  GTAMD_ABI_BEGIN
  if (sp == nullptr) { gtamd_set_error("invalid argument to gtamd_spm_prepare"); return -1; }
  if (!sp->have_index) {
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
  TRY(sp->suf_bytes == 4 ? prepare<u32>(sp, min_len) : prepare<u64>(sp, min_len));
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
  if (sp == nullptr || info == nullptr) { gtamd_set_error("invalid argument to gtamd_spm_get_info"); return -1; }
  *info = sp->info;
  return 0;
  GTAMD_ABI_END(-1)
}
