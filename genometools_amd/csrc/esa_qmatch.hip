// esa_qmatch.hip -- maximal exact matches of a query against .suf and the
// sequence in device memory: `gt repfind -q`, `-r`, `-p` (C ABI, the semantics
// and the algorithm: include/gtamd_qmatch.h).
//
//   a  k_qm_intervals     one lane per query position: the interval of the
//                         suffixes that start with its L symbols
//                         (esa_qmatch_core.h), the sum of the widths per tile
//   b  offsets_u64 (esa_prims)     64-bit exclusive scan of the widths
//   c  k_qm_emit<false>   one lane per candidate of a chunk: the left-maximal
//                         ones, counted per workgroup; scan (esa_prims)
//      k_qm_emit<true>    the same lanes extend theirs to the right and write
//                         the records, compacted in candidate order
//
// Every working array has m entries (or one per tile of positions or of
// candidates of a chunk), none has N.
#include "esa_common.h"
#include "esa_index.h"
#include "esa_prims.h"
#include "esa_devutil.h"
#include "esa_qmatch_core.h"
#include "../../include/gtamd_qmatch.h"

namespace {

constexpr int QM_THREADS = SC_THREADS;
constexpr u32 QM_TILE = QM_THREADS;               // query positions, or candidates, of one workgroup: one a lane
constexpr u64 QM_MIN_CHUNK = 4 * QM_TILE;         // the smallest chunk of candidates, and capacity
constexpr u64 QM_MAX_CHUNK = 1ull << 24;          // the largest: 65536 workgroups a launch
constexpr u64 QM_MAX_QUERY = (1ull << 32) - 1;

enum { W_CANDIDATES = 0, W_SEEDS, W_MAXWIDTH, W_SEARCH, W_EXTENSION, W_WORDS };

// what the lanes of steps a and c are given
template <typename S> struct QmInput {
  const u8 *enc; u64 n; const S *suf;
  const u8 *q; u64 m;
  u32 L;
};

// ---- step a ----------------------------------------------------------------------
template <typename S>
__global__ __launch_bounds__(QM_THREADS) void k_qm_intervals(QmInput<S> in, u32 *lo, u32 *width, u64 *tsum, u64 *w) {
  __shared__ unsigned long long ssum, ssearch;
  __shared__ u32 sseeds, smax;
  if (threadIdx.x == 0) { ssum = 0; ssearch = 0; sseeds = 0; smax = 0; }
  __syncthreads();
  const u64 i = (u64) blockIdx.x * QM_TILE + threadIdx.x;
  if (i < in.m) {
    Lane c = { in.q, in.m, i, in.enc, in.n, 0 };
    u32 l, wd;
    qm_interval(c, in.suf, in.n + 1, in.L, &l, &wd);
    lo[i] = l;
    width[i] = wd;
    if (wd) { atomicAdd(&ssum, (unsigned long long) wd); atomicAdd(&sseeds, 1u); atomicMax(&smax, wd); }
    if (c.compared) atomicAdd(&ssearch, (unsigned long long) c.compared);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    tsum[blockIdx.x] = ssum;
    if (sseeds) {
      atomicAdd((unsigned long long *) &w[W_SEEDS], (unsigned long long) sseeds);
      atomicMax((unsigned long long *) &w[W_MAXWIDTH], (unsigned long long) smax);
    }
    if (ssearch) atomicAdd((unsigned long long *) &w[W_SEARCH], ssearch);
  }
}

// ---- step c ----------------------------------------------------------------------
// Candidates [c0, c1) of all off[m], QM_TILE a workgroup.  WRITE false:
// tiles[b] = the number of left-maximal candidates of workgroup b.  WRITE true:
// tiles[b] is where their records go in out, in candidate order.
template <typename S, bool WRITE>
__global__ __launch_bounds__(QM_THREADS) void k_qm_emit(QmInput<S> in, const u32 *lo, const u64 *off, u64 c0, u64 c1,
                                                        u32 *tiles, QmRecord *out, u64 *w) {
  __shared__ u64 span[2];                 // the positions of the workgroup's first and last candidate
  __shared__ u32 wave_kept[QM_THREADS / 64];
  __shared__ unsigned long long sext;
  const u64 first = c0 + (u64) blockIdx.x * QM_TILE;
  const u64 last = (c1 - first < QM_TILE ? c1 : first + QM_TILE) - 1;
  if (threadIdx.x < 2) span[threadIdx.x] = entry_of(off, 0, in.m, threadIdx.x == 0 ? first : last);
  if (threadIdx.x == 0) sext = 0;
  __syncthreads();
  const u64 g = first + threadIdx.x;
  bool keep = false;
  QmRecord rec = { 0, 0, 0 };
  if (g <= last) {
    const u64 i = entry_of(off, span[0], span[1] + 1, g);
    Lane c = { in.q, in.m, i, in.enc, in.n, 0 };
    u64 p;
    keep = qm_kept(c, in.suf, lo[i], (u32) (g - off[i]), &p);
    if (WRITE && keep) {
      qm_extend(c, p, in.L, &rec);
      atomicAdd(&sext, (unsigned long long) c.compared);
    }
  }
  // the kept candidates in front of this one: in its wave, in the waves before
  const u64 mask = __ballot(keep);
  const u32 before = lanes_before(mask);
  const u32 wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) wave_kept[wave] = (u32) __popcll(mask);
  __syncthreads();
  u32 base = 0, total = 0;
#pragma unroll
  for (u32 k = 0; k < QM_THREADS / 64; k++) {
    const u32 v = wave_kept[k];
    if (k < wave) base += v;
    total += v;
  }
  if (!WRITE) {
    if (threadIdx.x == 0) tiles[blockIdx.x] = total;
    return;
  }
  if (keep) out[(u64) tiles[blockIdx.x] + base + before] = rec;
  if (threadIdx.x == 0 && sext) atomicAdd((unsigned long long *) &w[W_EXTENSION], sext);
}

}  // namespace

struct gtamd_qmatch : ConsumerBase<> {
  ResidentIndex index;
  bool prepared = false;
  // what a prepare leaves for the emit calls
  Dev<u8> own_query;
  const u8 *q = nullptr;
  u64 m = 0;
  u32 L = 0;
  Dev<u32> lo, width, tiles, scanws;
  Dev<u64> tsum, off;
  Dev<u8> out;                    // records on their way to host memory
  gtamd_qmatch_info info = gtamd_qmatch_info();
};

namespace {

const char FEATURE[] = "query matches";

// every way of setting an index: what is refused, before anything is touched
int set_index(gtamd_qmatch *qm, const IndexView &v, bool from_host) {
  if (qm == nullptr || v.suf == nullptr || (v.enc == nullptr && v.n)) {
    gtamd_set_error("invalid argument to gtamd_qmatch_set_index");
    return -1;
  }
  TRY(refuse_suf_bytes(FEATURE, v.suf_bytes));
  TRY(refuse_sizes(FEATURE, v.n, 0));
  HIP_TRY(hipSetDevice(qm->device));
  qm->prepared = false;
  if (from_host) return qm->index.upload_from_host(FEATURE, v);
  qm->index.borrow(v);
  return 0;
}

u64 held_bytes(const gtamd_qmatch *qm) {
  return qm->index.bytes() + qm->own_query.bytes + qm->lo.bytes + qm->width.bytes + qm->tiles.bytes +
         qm->scanws.bytes + qm->tsum.bytes + qm->off.bytes + qm->words.bytes + qm->out.bytes;
}

template <typename S> QmInput<S> input(const gtamd_qmatch *qm) {
  return QmInput<S>{ qm->index.enc, qm->index.n, (const S *) qm->index.suf, qm->q, qm->m, qm->L };
}

template <typename S> int prepare(gtamd_qmatch *qm) {
  hipStream_t st = qm->st;
  const u64 m = qm->m;
  HIP_TRY(hipMemsetAsync(qm->words, 0, W_WORDS * sizeof(u64), st));
  HIP_TRY(hipEventRecord(qm->ev[0], st));
  if (m != 0) {
    k_qm_intervals<S><<<(u32) div_up(m, QM_TILE), QM_THREADS, 0, st>>>(input<S>(qm), qm->lo, qm->width, qm->tsum, qm->words);
    HIP_TRY(hipGetLastError());
    TRY(offsets_u64(qm->width, m, qm->tsum, qm->off, qm->words + W_CANDIDATES, st));
  }
  HIP_TRY(hipEventRecord(qm->ev[1], st));
  u64 h[W_WORDS];
  TRY(fetch(st, { { qm->words, h, sizeof h } }));
  HIP_TRY(hipEventElapsedTime(&qm->info.device_ms, qm->ev[0], qm->ev[1]));
  qm->info.positions = m;
  qm->info.seeds = h[W_SEEDS];
  qm->info.candidates = h[W_CANDIDATES];
  qm->info.max_width = h[W_MAXWIDTH];
  qm->info.search_symbols = h[W_SEARCH];
  return 0;
}

// one chunk: candidates [c0, c1) -> *kept records at dst
template <typename S> int emit_chunk(gtamd_qmatch *qm, u64 c0, u64 c1, QmRecord *dst, u64 *kept, u64 *extension) {
  hipStream_t st = qm->st;
  const u64 blocks = div_up(c1 - c0, QM_TILE);
  if (qm->tiles.grow((blocks + 1) * sizeof(u32)) != hipSuccess ||
      qm->scanws.grow(scan_workspace_words(blocks + 1) * sizeof(u32)) != hipSuccess)
    return out_of_memory(FEATURE, blocks + 1, "tiles of candidates");
  HIP_TRY(hipMemsetAsync(qm->tiles, 0, (blocks + 1) * sizeof(u32), st));
  k_qm_emit<S, false><<<(u32) blocks, QM_THREADS, 0, st>>>(input<S>(qm), qm->lo, qm->off, c0, c1, qm->tiles, nullptr,
                                                           qm->words);
  HIP_TRY(hipGetLastError());
  TRY(scan_u32(SCAN_SUM, qm->tiles, qm->tiles, blocks + 1, false, qm->scanws, st));
  k_qm_emit<S, true><<<(u32) blocks, QM_THREADS, 0, st>>>(input<S>(qm), qm->lo, qm->off, c0, c1, qm->tiles, dst,
                                                          qm->words);
  HIP_TRY(hipGetLastError());
  u32 total = 0;
  TRY(fetch(st, { { qm->tiles + blocks, &total, sizeof total }, { qm->words + W_EXTENSION, extension, sizeof(u64) } }));
  *kept = total;
  return 0;
}

int emit(gtamd_qmatch *qm, u64 *cursor, gtamd_qmatch_record *out, u64 capacity, int out_on_device, u64 *written) {
  *written = 0;
  const u64 C = qm->info.candidates;
  u64 cur = *cursor, total = 0;
  TRY(refuse_window(FEATURE, "candidates", cur, C, capacity, QM_MIN_CHUNK));
  if (cur == C) return 0;
  RecordStage<QmRecord> stage(out, out_on_device);
  const u64 most = capacity < C - cur ? capacity : C - cur;
  if (stage.begin(qm->out, most) != hipSuccess) return out_of_memory(FEATURE, most, "records");
  QmRecord *dst = stage.dst;
  // a chunk of `room` candidates gives at most `room` records
  while (cur < C && capacity - total >= QM_MIN_CHUNK) {
    u64 chunk = capacity - total, kept = 0;
    if (chunk > C - cur) chunk = C - cur;
    if (chunk > QM_MAX_CHUNK) chunk = QM_MAX_CHUNK;
    TRY(qm->index.suf_bytes == 4 ? emit_chunk<u32>(qm, cur, cur + chunk, dst + total, &kept, &qm->info.extension_symbols)
                           : emit_chunk<u64>(qm, cur, cur + chunk, dst + total, &kept, &qm->info.extension_symbols));
    total += kept;
    cur += chunk;
  }
  if (!out_on_device && total) TRY(stage.finish(total, qm->st));      // (every chunk has waited for its own)
  qm->info.matches += total;
  *cursor = cur;
  *written = total;
  return 0;
}

}  // namespace

extern "C" gtamd_qmatch *gtamd_qmatch_create(int device) {
  GTAMD_ABI_BEGIN
  return create_consumer<gtamd_qmatch>(device, W_WORDS, "the query matcher");
  GTAMD_ABI_END(nullptr)
}

extern "C" void gtamd_qmatch_destroy(gtamd_qmatch *qm) { destroy_consumer(qm); }

extern "C" void gtamd_qmatch_geometry(uint32_t *tile_positions, uint64_t *min_capacity) {
  if (tile_positions != nullptr) *tile_positions = QM_TILE;
  if (min_capacity != nullptr) *min_capacity = QM_MIN_CHUNK;
}

extern "C" int gtamd_qmatch_set_index(gtamd_qmatch *qm, const uint8_t *enc, uint64_t n, const void *suf,
                                      uint32_t suf_bytes) {
  GTAMD_ABI_BEGIN
  return set_index(qm, IndexView{ enc, n, suf, suf_bytes }, false);
  GTAMD_ABI_END(-1)
}

extern "C" int gtamd_qmatch_set_index_host(gtamd_qmatch *qm, const uint8_t *enc, uint64_t n, const void *suf,
                                           uint32_t suf_bytes) {
  GTAMD_ABI_BEGIN
  return set_index(qm, IndexView{ enc, n, suf, suf_bytes }, true);
  GTAMD_ABI_END(-1)
}

extern "C" int gtamd_qmatch_set_index_esa(gtamd_qmatch *qm, const gtamd_esa_ctx *esa, const uint8_t *enc,
                                          uint64_t n) {
  GTAMD_ABI_BEGIN
  if (qm == nullptr || esa == nullptr) { gtamd_set_error("invalid argument to gtamd_qmatch_set_index_esa"); return -1; }
  IndexView v;
  TRY(engine_tables(FEATURE, esa, enc, n, false, &v));
  return set_index(qm, v, false);
  GTAMD_ABI_END(-1)
}

extern "C" int gtamd_qmatch_prepare(gtamd_qmatch *qm, const uint8_t *query, uint64_t m, int is_device,
                                    uint32_t min_len, gtamd_qmatch_info *info) {
  GTAMD_ABI_BEGIN
  if (qm == nullptr || (query == nullptr && m)) { gtamd_set_error("invalid argument to gtamd_qmatch_prepare"); return -1; }
  if (!qm->index.set) {
    gtamd_set_error("query matches: no index is set (gtamd_qmatch_set_index)");
    return -1;
  }
  if (min_len == 0) {
    gtamd_set_error("query matches: a minimum length of 0 is refused, 1 or more expected");
    return -1;
  }
  if (m > QM_MAX_QUERY) {
    gtamd_set_error("query matches: query of %llu symbols, at most %llu in one call", (unsigned long long) m,
                    (unsigned long long) QM_MAX_QUERY);
    return -1;
  }
  HIP_TRY(hipSetDevice(qm->device));
  qm->prepared = false;
  qm->info = gtamd_qmatch_info();
  const u64 T = div_up(m, QM_TILE);
  if ((!is_device && qm->own_query.grow(m ? m : 1) != hipSuccess) || qm->lo.grow((m ? m : 1) * 4) != hipSuccess ||
      qm->width.grow((m ? m : 1) * 4) != hipSuccess || qm->off.grow((m + 1) * 8) != hipSuccess ||
      qm->tsum.grow((T ? T : 1) * 8) != hipSuccess)
    return out_of_memory(FEATURE, m, "query positions");
  qm->q = query;
  if (!is_device) {
    if (m) HIP_TRY(hipMemcpyAsync(qm->own_query, query, m, hipMemcpyHostToDevice, qm->st));
    qm->q = qm->own_query;
  }
  qm->m = m;
  qm->L = min_len;
  TRY(qm->index.suf_bytes == 4 ? prepare<u32>(qm) : prepare<u64>(qm));
  qm->info.device_bytes = held_bytes(qm);
  qm->prepared = true;
  if (info != nullptr) *info = qm->info;
  return 0;
  GTAMD_ABI_END(-1)
}

extern "C" int gtamd_qmatch_emit(gtamd_qmatch *qm, uint64_t *cursor, gtamd_qmatch_record *out, uint64_t capacity,
                                 int out_on_device, uint64_t *written) {
  GTAMD_ABI_BEGIN
  if (qm == nullptr || cursor == nullptr || written == nullptr || (out == nullptr && capacity)) {
    gtamd_set_error("invalid argument to gtamd_qmatch_emit");
    return -1;
  }
  if (!qm->prepared) {
    gtamd_set_error("query matches: nothing is prepared (gtamd_qmatch_prepare)");
    return -1;
  }
  HIP_TRY(hipSetDevice(qm->device));
  TRY(emit(qm, cursor, out, capacity, out_on_device, written));
  qm->info.device_bytes = held_bytes(qm);
  return 0;
  GTAMD_ABI_END(-1)
}

extern "C" int gtamd_qmatch_get_info(const gtamd_qmatch *qm, gtamd_qmatch_info *info) {
  GTAMD_ABI_BEGIN
  return consumer_info(qm, info, "gtamd_qmatch_get_info");
  GTAMD_ABI_END(-1)
}
