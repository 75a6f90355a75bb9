// esa_mstat.hip -- matching statistics and minimum unique prefixes of a query
// against a suffix array in device memory: `gt matstat -esa` and `gt uniquesub
// -esa` (C ABI, the semantics and the algorithm: include/gtamd_mstat.h).
//
// One kernel, one lane per query position (workgroups of MST_TILE lanes): a
// binary search over the whole table for the place of the query suffix, which
// carries the letters shared with both borders, then at most one more search
// (the witness) or one more comparison (the second neighbour, for uniqueness):
// esa_mstat_search.h.  Letters are compared MST_WORD at a time through 4-byte words.
//
// With a reader of the packed index as the index (gtamd_mstat_set_index_pckidx,
// include/gtamd_pckidx.h) the same two calls run the backward search of
// esa_pckidx.hip instead.
#include "esa_common.h"
#include "esa_index.h"
#include "esa_mstat_search.h"
#include "../../include/gtamd_mstat.h"
#include "../../include/gtamd_pckidx.h"

namespace {

constexpr int MST_THREADS = 256;
constexpr u32 MST_TILE = 256;            // query positions per workgroup, one a lane
constexpr u64 MST_MAX_QUERY = (1ull << 32) - 1;

enum { W_COMPARED = 0, W_RERUNS, W_ERROR, W_WORDS };   // W_ERROR: the error word of a packed-index search

// one lane per query position: mst_position of esa_mstat_search.h
template <typename S, bool MATSTAT>
__global__ __launch_bounds__(MST_THREADS) void k_mstat(const u8 *enc, u64 n, const S *suf, const u8 *q, u64 m,
                                                       u32 limit, u32 *len_out, u64 *pos_out, u64 *w) {
  __shared__ unsigned long long scompared;
  __shared__ u32 sreruns;
  if (threadIdx.x == 0) { scompared = 0; sreruns = 0; }
  __syncthreads();
  const u64 N = n + 1, i = (u64) blockIdx.x * MST_TILE + threadIdx.x;
  Lane c = { q, m, i, enc, n, 0 };
  u32 reruns = 0;
  if (i < m) {
    u32 len;
    u64 pos;
    reruns = mst_position<S, MATSTAT>(c, suf, N, limit, pos_out != nullptr, &len, &pos);
    len_out[i] = len;
    if (MATSTAT && pos_out != nullptr) pos_out[i] = pos;
  }
  if (c.compared) atomicAdd(&scompared, (unsigned long long) c.compared);
  if (reruns) atomicAdd(&sreruns, reruns);
  __syncthreads();
  if (threadIdx.x == 0) {
    if (scompared) atomicAdd((unsigned long long *) &w[W_COMPARED], scompared);
    if (sreruns) atomicAdd((unsigned long long *) &w[W_RERUNS], (unsigned long long) sreruns);
  }
}

}  // namespace

struct gtamd_mstat : ConsumerBase<> {
  IndexSlot index;
  u32 numofchars = 0;
  Dev<u8> query;
  Dev<u32> len;
  Dev<u64> pos;
  gtamd_mstat_info info = gtamd_mstat_info();
};

namespace {

const char FEATURE[] = "matching statistics";

// every way of setting an index: what is refused, before anything is touched
int set_index(gtamd_mstat *ms, const IndexView &v, u32 numofchars, bool from_host) {
  if (ms == nullptr || v.suf == nullptr || (v.enc == nullptr && v.n)) {
    gtamd_set_error("invalid argument to gtamd_mstat_set_index");
    return -1;
  }
  TRY(refuse_suf_bytes(FEATURE, v.suf_bytes));
  if (numofchars < 1 || numofchars > 253) {
    gtamd_set_error("matching statistics: an alphabet of %u letters, 1 to 253 expected", numofchars);
    return -1;
  }
  TRY(refuse_sizes(FEATURE, v.n, 0));
  HIP_TRY(hipSetDevice(ms->device));
  ms->numofchars = numofchars;
  return ms->index.set_tables(FEATURE, v, from_host);
}

u64 held_bytes(const gtamd_mstat *ms) {
  return ms->index.bytes() + ms->query.bytes + ms->len.bytes + ms->pos.bytes + ms->words.bytes;
}

template <typename S, bool MATSTAT>
void launch(gtamd_mstat *ms, const u8 *q, u64 m, u32 limit, u32 *len, u64 *pos) {
  k_mstat<S, MATSTAT><<<(u32) div_up(m, MST_TILE), MST_THREADS, 0, ms->st>>>(
      ms->index.tab.enc, ms->index.tab.n, (const S *) ms->index.tab.suf, q, m, limit, len, pos, ms->words);
}

int run_query(gtamd_mstat *ms, bool matstat, const u8 *query, u64 m, int is_device, u32 max_len,
              u32 *length_out, u64 *subjectpos_out, int out_is_device) {
  if (ms == nullptr || (m && (query == nullptr || length_out == nullptr))) {
    gtamd_set_error("invalid argument to gtamd_mstat_%s", matstat ? "matstat" : "uniquesub");
    return -1;
  }
  TRY(ms->index.refuse_unset(FEATURE, "mstat"));
  if (ms->index.pck != nullptr) TRY(ms->index.refuse_lost_reader(FEATURE));
  if (m > MST_MAX_QUERY) {
    gtamd_set_error("matching statistics: query of %llu symbols, at most %llu in one call",
                    (unsigned long long) m, (unsigned long long) MST_MAX_QUERY);
    return -1;
  }
  ms->info = gtamd_mstat_info();
  ms->info.positions = m;
  ms->info.device_bytes = held_bytes(ms);
  if (m == 0) return 0;
  HIP_TRY(hipSetDevice(ms->device));
  const bool want_pos = matstat && subjectpos_out != nullptr;
  if (ms->index.pck != nullptr && want_pos) TRY(ms->index.refuse_no_locate(FEATURE, "subject positions cannot be had from it"));
  if ((!is_device && ms->query.grow(m) != hipSuccess) ||
      (!out_is_device && (ms->len.grow(m * sizeof(u32)) != hipSuccess ||
                          (want_pos && ms->pos.grow(m * sizeof(u64)) != hipSuccess)))) {
    gtamd_set_error("matching statistics: cannot allocate device memory for a query of %llu symbols",
                    (unsigned long long) m);
    return -1;
  }
  hipStream_t st = ms->st;
  const u8 *q = query;
  if (!is_device) {
    HIP_TRY(hipMemcpyAsync(ms->query, query, m, hipMemcpyHostToDevice, st));
    q = ms->query;
  }
  u32 *len = out_is_device ? length_out : (u32 *) ms->len;
  u64 *pos = !want_pos ? nullptr : out_is_device ? subjectpos_out : (u64 *) ms->pos;
  const u32 limit = max_len == 0 || max_len >= MST_MAX_QUERY ? (u32) MST_MAX_QUERY : max_len + 1;
  HIP_TRY(hipMemsetAsync(ms->words, 0, W_WORDS * sizeof(u64), st));
  HIP_TRY(hipEventRecord(ms->ev[0], st));
  if (ms->index.pck != nullptr) {
    TRY(pckidx_search(ms->index.pck, st, matstat, q, m, limit, len, pos, &ms->words[W_COMPARED], &ms->words[W_ERROR]));
  } else if (ms->index.tab.suf_bytes == 4) {
    if (matstat) launch<u32, true>(ms, q, m, limit, len, pos); else launch<u32, false>(ms, q, m, limit, len, pos);
  } else {
    if (matstat) launch<u64, true>(ms, q, m, limit, len, pos); else launch<u64, false>(ms, q, m, limit, len, pos);
  }
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(ms->ev[1], st));
  u64 h[W_WORDS];
  TRY(fetch(st, { { len, length_out, out_is_device ? 0 : m * sizeof(u32) },
                  { pos, subjectpos_out, out_is_device || !want_pos ? 0 : m * sizeof(u64) },
                  { ms->words, h, sizeof h } }));
  if (h[W_ERROR]) { pckidx_set_search_error(h[W_ERROR]); return -1; }
  HIP_TRY(hipEventElapsedTime(&ms->info.device_ms, ms->ev[0], ms->ev[1]));
  ms->info.symbols_compared = h[W_COMPARED];
  ms->info.reruns = (u32) h[W_RERUNS];
  ms->info.device_bytes = held_bytes(ms);
  return 0;
}

}  // namespace

extern "C" gtamd_mstat *gtamd_mstat_create(int device) {
  GTAMD_ABI_BEGIN
  return create_consumer<gtamd_mstat>(device, W_WORDS, "the matching statistics searcher");
  GTAMD_ABI_END(nullptr)
}

extern "C" void gtamd_mstat_destroy(gtamd_mstat *ms) { destroy_consumer(ms); }

extern "C" void gtamd_mstat_geometry(uint32_t *tile_positions, uint32_t *word_symbols, uint32_t *word_min) {
  if (tile_positions != nullptr) *tile_positions = MST_TILE;
  if (word_symbols != nullptr) *word_symbols = MST_WORD;
  if (word_min != nullptr) *word_min = MST_WORD_MIN;
}

extern "C" int gtamd_mstat_set_index(gtamd_mstat *ms, const uint8_t *enc, uint64_t n, const void *suf,
                                     uint32_t suf_bytes, uint32_t numofchars) {
  GTAMD_ABI_BEGIN
  return set_index(ms, IndexView{ enc, n, suf, suf_bytes }, numofchars, false);
  GTAMD_ABI_END(-1)
}

extern "C" int gtamd_mstat_set_index_host(gtamd_mstat *ms, const uint8_t *enc, uint64_t n, const void *suf,
                                          uint32_t suf_bytes, uint32_t numofchars) {
  GTAMD_ABI_BEGIN
  return set_index(ms, IndexView{ enc, n, suf, suf_bytes }, numofchars, true);
  GTAMD_ABI_END(-1)
}

extern "C" int gtamd_mstat_set_index_esa(gtamd_mstat *ms, const gtamd_esa_ctx *esa, const uint8_t *enc,
                                         uint64_t n, uint32_t numofchars) {
  GTAMD_ABI_BEGIN
  if (ms == nullptr || esa == nullptr) { gtamd_set_error("invalid argument to gtamd_mstat_set_index_esa"); return -1; }
  IndexView v;
  TRY(engine_tables(FEATURE, esa, enc, n, false, &v));
  return set_index(ms, v, numofchars, false);
  GTAMD_ABI_END(-1)
}

extern "C" int gtamd_mstat_set_index_pckidx(gtamd_mstat *ms, const gtamd_pckidx *px) {
  GTAMD_ABI_BEGIN
  TRY(IndexSlot::refuse_reader(FEATURE, "mstat", "the searcher", ms, px));
  HIP_TRY(hipSetDevice(ms->device));
  ms->index.set_reader(px);
  return 0;
  GTAMD_ABI_END(-1)
}

extern "C" int gtamd_mstat_matstat(gtamd_mstat *ms, const uint8_t *query, uint64_t m, int is_device,
                                   uint32_t max_len, uint32_t *length_out, uint64_t *subjectpos_out,
                                   int out_is_device) {
  GTAMD_ABI_BEGIN
  return run_query(ms, true, query, m, is_device, max_len, length_out, subjectpos_out, out_is_device);
  GTAMD_ABI_END(-1)
}

extern "C" int gtamd_mstat_uniquesub(gtamd_mstat *ms, const uint8_t *query, uint64_t m, int is_device,
                                     uint32_t max_len, uint32_t *length_out, int out_is_device) {
  GTAMD_ABI_BEGIN
  return run_query(ms, false, query, m, is_device, max_len, length_out, nullptr, out_is_device);
  GTAMD_ABI_END(-1)
}

extern "C" int gtamd_mstat_get_info(const gtamd_mstat *ms, gtamd_mstat_info *info) {
  GTAMD_ABI_BEGIN
  return consumer_info(ms, info, "gtamd_mstat_get_info");
  GTAMD_ABI_END(-1)
}
