// esa_contained.hip -- the contained reads of a read set from .suf and .lcp of its
// mirrored set in device memory, and the set without them: the decision of `gt
// readjoiner prefilter` (C ABI, the definition, the tie rule and the algorithm:
// include/gtamd_contained.h).
//
//   1, 2  gtamd_spm_prepare (esa_spm.hip)   the object owns a gtamd_spm: read
//                              starts and separators (no terminal suffix is asked for)
//   3     k_ct_starts          one lane per read start: position and length of its sequence
//   4     k_ct_images          one lane per sequence: what it finds out about
//                              itself (esa_contained_core.h)
//   5     k_ct_verdicts        one lane per read: the verdict from its two images;
//                              a wave's verdicts of a class are one ballot
//   compact  k_ct_kept         one lane per read: the symbols it gives
//            offsets_u64_counted (esa_prims)   64-bit exclusive scan of those
//            k_ct_compact      one lane per symbol of the result
//   k_ct_wildcards, k_ct_tally the first filter: a flag per read, and the same compaction
//   k_ct_mirror                one lane per symbol of the mirrored set
#include <vector>
#include "esa_common.h"
#include "esa_index.h"
#include "esa_prims.h"
#include "esa_devutil.h"
#include "esa_contained_core.h"
#include "esa_spm_state.h"
#include "../../include/gtamd_contained.h"

static_assert(CT_KEPT == GTAMD_CONTAINED_KEPT && CT_DUPLICATE == GTAMD_CONTAINED_DUPLICATE &&
              CT_AFFIX == GTAMD_CONTAINED_AFFIX && CT_INTERNAL == GTAMD_CONTAINED_INTERNAL &&
              CT_SELF_COMPLEMENTARY == GTAMD_CONTAINED_SELF_COMPLEMENTARY && CT_VERDICTS == GTAMD_CONTAINED_VERDICTS,
              "the verdicts of the lane header are those of the C ABI");

namespace {

constexpr int CT_THREADS = SC_THREADS;
constexpr u32 CT_TILE = CT_THREADS;               // reads, sequences or symbols of one workgroup: one a lane
constexpr u64 CT_MAX_CHUNK = 1ull << 24;          // symbols of one launch of the compaction: 65536 workgroups
constexpr u32 CT_NO_TERMINALS = 0xFFFFFFFFu;      // a minimum length no suffix has: steps 1 and 2 list none

enum { W_COUNT = 0, W_TOTAL = W_COUNT + CT_VERDICTS, W_WORDS };

// ---- step 3 ----------------------------------------------------------------------
template <typename S>
__global__ __launch_bounds__(CT_THREADS) void k_ct_starts(SpIndex<S> x, const u32 *starts, u32 K, const u32 *seps,
                                                          u32 nseps, u32 *spos, u32 *slen) {
  const u64 j = (u64) blockIdx.x * CT_TILE + threadIdx.x;
  if (j >= K) return;
  u32 pos, len;
  sr_start(x, starts, seps, nseps, j, &pos, &len);
  spos[j] = pos;
  slen[j] = len;
}

// ---- step 4 ----------------------------------------------------------------------
template <typename S> __global__ __launch_bounds__(CT_THREADS) void k_ct_images(SpIndex<S> x, CtLists a, u8 *image) {
  const u64 j = (u64) blockIdx.x * CT_TILE + threadIdx.x;
  if (j >= a.R) return;
  u64 s;
  const u8 f = ct_image(x, a, j, &s);
  image[s] = f;                                    // (s <= nseps: one of the R sequences)
}

// ---- step 5 ----------------------------------------------------------------------
// every lane of the wave comes here; one without a read has valid false
__device__ __forceinline__ void tally(u8 v, bool valid, u64 *w) {
#pragma unroll
  for (u32 c = 0; c < CT_VERDICTS; c++) {
    const u64 mask = __ballot(valid && v == c);
    if ((threadIdx.x & 63) == 0 && mask) atomicAdd((unsigned long long *) &w[W_COUNT + c], (unsigned long long) __popcll(mask));
  }
}

__global__ __launch_bounds__(CT_THREADS) void k_ct_verdicts(const u8 *image, u32 R, u8 *verdict, u64 *w) {
  const u64 r = (u64) blockIdx.x * CT_TILE + threadIdx.x;
  u8 v = CT_KEPT;
  if (r < R) {
    v = ct_verdict(image[r], image[2 * (u64) R - 1 - r]);
    verdict[r] = v;
  }
  tally(v, r < R, w);
}

__global__ __launch_bounds__(CT_THREADS) void k_ct_tally(const u8 *verdict, u32 R, u64 *w) {
  const u64 r = (u64) blockIdx.x * CT_TILE + threadIdx.x;
  tally(r < R ? verdict[r] : CT_KEPT, r < R, w);
}

// ---- the compaction ----------------------------------------------------------------
__global__ __launch_bounds__(CT_THREADS) void k_ct_kept(const u8 *verdict, u32 mask, const u32 *seps, u32 nseps, u64 n,
                                                        u32 R, u32 *klen) {
  const u64 r = (u64) blockIdx.x * CT_TILE + threadIdx.x;
  if (r < R) klen[r] = ct_kept_symbols(verdict, mask, seps, nseps, n, r);
}

// symbols [e0, e1) of the result to out, CT_TILE a workgroup; off[R] is beyond all of them
__global__ __launch_bounds__(CT_THREADS) void k_ct_compact(const u8 *enc, const u32 *seps, u32 nseps, u64 n,
                                                           const u64 *off, u32 R, u64 e0, u64 e1, u8 *out) {
  __shared__ u64 span[2];                 // the reads of the workgroup's first and last symbol
  const u64 b0 = e0 + (u64) blockIdx.x * CT_TILE;
  const u64 last = (e1 - b0 < CT_TILE ? e1 : b0 + CT_TILE) - 1;
  if (threadIdx.x < 2) span[threadIdx.x] = entry_of(off, 0, R, threadIdx.x == 0 ? b0 : last);
  __syncthreads();
  const u64 e = b0 + threadIdx.x;
  if (e > last) return;
  const u64 r = entry_of(off, span[0], span[1] + 1, e);
  out[e] = ct_symbol(enc, seps, nseps, n, off, r, e);
}

// flag[r] = 1 for a read with a wildcard; flag is 0 before
__global__ __launch_bounds__(CT_THREADS) void k_ct_wildcards(const u8 *enc, u64 n, const u32 *seps, u32 nseps, u8 *flag) {
  const u64 p = (u64) blockIdx.x * CT_TILE + threadIdx.x;
  if (p < n && enc[p] == 254) flag[sp_sequence_of(seps, nseps, p)] = 1;
}

__global__ __launch_bounds__(CT_THREADS) void k_ct_mirror(const u8 *enc, u64 n, u8 *out) {
  const u64 e = (u64) blockIdx.x * CT_TILE + threadIdx.x;
  if (e <= 2 * n) out[e] = ct_mirror_symbol(enc, n, e);
}

}  // namespace

struct gtamd_contained : ConsumerBase<2> {
  gtamd_spm *sp = nullptr;             // steps 1 and 2, and the index
  bool decided = false;
  u32 R = 0;                           // reads of the last decide
  u64 result = 0;                      // symbols of the last compaction, in out
  u32 flagged = 0;                     // reads of the last drop_wildcards, a flag each
  Dev<u32> spos, slen, klen, seps;     // (seps: those of a set without an index, drop_wildcards)
  Dev<u8> image, verdict, flag, out, both;
  Dev<u64> tsum, off;
  gtamd_contained_info info = gtamd_contained_info();
  ~gtamd_contained() { gtamd_spm_destroy(sp); }
};

namespace {

const char FEATURE[] = "contained reads";

u64 held_bytes(const gtamd_contained *ct) {
  return ct->sp->info.device_bytes + ct->spos.bytes + ct->slen.bytes + ct->klen.bytes + ct->seps.bytes +
         ct->image.bytes + ct->verdict.bytes + ct->flag.bytes + ct->out.bytes + ct->both.bytes + ct->tsum.bytes + ct->off.bytes +
         ct->words.bytes;
}

template <typename S> SpIndex<S> view(const gtamd_contained *ct) {
  const ResidentIndex &x = ct->sp->index;
  return SpIndex<S>{ x.enc, x.n, (const S *) x.suf, x.lcp, x.llv, x.llv_pairs };
}

template <typename S> int decide(gtamd_contained *ct, u32 K) {
  hipStream_t st = ct->st;
  const gtamd_spm *sp = ct->sp;
  const u32 R = K / 2, tiles = (u32) div_up(K, CT_TILE);
  if (ct->spos.grow((u64) K * 4) != hipSuccess || ct->slen.grow((u64) K * 4) != hipSuccess ||
      ct->image.grow(K) != hipSuccess || ct->verdict.grow(R) != hipSuccess)
    return out_of_memory(FEATURE, K, "sequences");
  HIP_TRY(hipMemsetAsync(ct->words, 0, W_WORDS * sizeof(u64), st));
  HIP_TRY(hipEventRecord(ct->ev[0], st));
  k_ct_starts<S><<<tiles, CT_THREADS, 0, st>>>(view<S>(ct), sp->starts, K, sp->seps, sp->nseps, ct->spos, ct->slen);
  HIP_TRY(hipGetLastError());
  const CtLists a = { sp->starts, ct->spos, ct->slen, K, sp->seps, sp->nseps };
  k_ct_images<S><<<tiles, CT_THREADS, 0, st>>>(view<S>(ct), a, ct->image);
  HIP_TRY(hipGetLastError());
  k_ct_verdicts<<<(u32) div_up(R, CT_TILE), CT_THREADS, 0, st>>>(ct->image, R, ct->verdict, ct->words);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(ct->ev[1], st));
  u64 h[W_WORDS];
  TRY(fetch(st, { { ct->words, h, sizeof h } }));
  float own = 0;
  HIP_TRY(hipEventElapsedTime(&own, ct->ev[0], ct->ev[1]));
  for (u32 c = 0; c < CT_VERDICTS; c++) ct->info.count[c] = h[W_COUNT + c];
  ct->info.lists_ms = sp->info.device_ms;
  ct->info.device_ms = sp->info.device_ms + own;
  return 0;
}

// The R reads among the n symbols at enc without those whose byte in `verdict` is a
// bit of mask; seps: nseps separators, R - 1 at least.  The result is ct->out.
int compact(gtamd_contained *ct, const u8 *verdict, u32 mask, const u8 *enc, u64 n, const u32 *seps, u32 nseps, u32 R,
            u8 **out_device, u64 *out_n) {
  hipStream_t st = ct->st;
  *out_device = nullptr;
  *out_n = 0;
  ct->result = 0;
  if (R == 0) return 0;
  if (ct->klen.grow((u64) R * 4) != hipSuccess || ct->off.grow(((u64) R + 1) * 8) != hipSuccess ||
      ct->tsum.grow(div_up(R, SC_THREADS) * 8) != hipSuccess)
    return out_of_memory(FEATURE, R, "kept lengths");
  k_ct_kept<<<(u32) div_up(R, CT_TILE), CT_THREADS, 0, st>>>(verdict, mask, seps, nseps, n, R, ct->klen);
  HIP_TRY(hipGetLastError());
  TRY(offsets_u64_counted(ct->klen, R, ct->tsum, ct->off, ct->words + W_TOTAL, st));
  u64 total = 0;
  TRY(fetch(st, { { ct->words + W_TOTAL, &total, sizeof total } }));
  if (total == 0) return 0;
  total--;                                         // no separator behind the last read
  if (total > n) {                                 // (lengths that are none: a set and separators that do not belong together)
    gtamd_set_error("%s: %llu symbols would be kept of %llu", FEATURE, (unsigned long long) total, (unsigned long long) n);
    return -1;
  }
  if (ct->out.grow(total) != hipSuccess) return out_of_memory(FEATURE, total, "kept symbols");
  for (u64 e0 = 0; e0 < total; e0 += CT_MAX_CHUNK) {
    const u64 e1 = total - e0 < CT_MAX_CHUNK ? total : e0 + CT_MAX_CHUNK;
    k_ct_compact<<<(u32) div_up(e1 - e0, CT_TILE), CT_THREADS, 0, st>>>(enc, seps, nseps, n, ct->off, R, e0, e1, ct->out);
    HIP_TRY(hipGetLastError());
  }
  HIP_TRY(hipStreamSynchronize(st));
  *out_device = ct->out;
  *out_n = ct->result = total;
  return 0;
}

// a new index: what was decided is none
int index_set(gtamd_contained *ct, int rc) {
  ct->decided = false;
  return rc;
}

}  // namespace

extern "C" gtamd_contained *gtamd_contained_create(int device) {
  GTAMD_ABI_BEGIN
  gtamd_contained *ct = create_consumer<gtamd_contained>(device, W_WORDS, "the finder of contained reads");
  if (ct != nullptr && (ct->sp = gtamd_spm_create(device)) == nullptr) {
    destroy_consumer(ct);
    return nullptr;
  }
  return ct;
  GTAMD_ABI_END(nullptr)
}

extern "C" void gtamd_contained_destroy(gtamd_contained *ct) { destroy_consumer(ct); }

extern "C" void gtamd_contained_geometry(uint32_t *tile_reads) {
  if (tile_reads != nullptr) *tile_reads = CT_TILE;
}

extern "C" int gtamd_contained_set_index(gtamd_contained *ct, const uint8_t *enc, uint64_t n, const void *suf,
                                         uint32_t suf_bytes, const uint8_t *lcp, const uint64_t *llv,
                                         uint64_t llv_pairs) {
  GTAMD_ABI_BEGIN
  if (ct == nullptr) { gtamd_set_error("invalid argument to gtamd_contained_set_index"); return -1; }
  return index_set(ct, gtamd_spm_set_index(ct->sp, enc, n, suf, suf_bytes, lcp, llv, llv_pairs));
  GTAMD_ABI_END(-1)
}

extern "C" int gtamd_contained_set_index_host(gtamd_contained *ct, const uint8_t *enc, uint64_t n, const void *suf,
                                              uint32_t suf_bytes, const uint8_t *lcp, const uint64_t *llv,
                                              uint64_t llv_pairs) {
  GTAMD_ABI_BEGIN
  if (ct == nullptr) { gtamd_set_error("invalid argument to gtamd_contained_set_index_host"); return -1; }
  return index_set(ct, gtamd_spm_set_index_host(ct->sp, enc, n, suf, suf_bytes, lcp, llv, llv_pairs));
  GTAMD_ABI_END(-1)
}

extern "C" int gtamd_contained_set_index_esa(gtamd_contained *ct, const gtamd_esa_ctx *esa, const uint8_t *enc,
                                             uint64_t n) {
  GTAMD_ABI_BEGIN
  if (ct == nullptr) { gtamd_set_error("invalid argument to gtamd_contained_set_index_esa"); return -1; }
  return index_set(ct, gtamd_spm_set_index_esa(ct->sp, esa, enc, n));
  GTAMD_ABI_END(-1)
}

extern "C" int gtamd_contained_decide(gtamd_contained *ct, gtamd_contained_info *info) {
  GTAMD_ABI_BEGIN
  if (ct == nullptr) { gtamd_set_error("invalid argument to gtamd_contained_decide"); return -1; }
  if (!ct->sp->index.set) {
    gtamd_set_error("%s: no index is set (gtamd_contained_set_index)", FEATURE);
    return -1;
  }
  ct->decided = false;
  ct->R = 0;
  ct->info = gtamd_contained_info();
  TRY(gtamd_spm_prepare(ct->sp, CT_NO_TERMINALS, nullptr));
  const gtamd_spm *sp = ct->sp;
  const u64 K = sp->index.n ? (u64) sp->nseps + 1 : 0;
  if (K % 2) {
    gtamd_set_error("%s: %llu sequences are no mirrored set: an even number is expected, the reads and their "
                    "reverse complements", FEATURE, (unsigned long long) K);
    return -1;
  }
  if (sp->R != K) {
    gtamd_set_error("%s: %llu of %llu sequences are empty or start with a wildcard: a set of reads of letters is "
                    "expected (gtamd_contained_drop_wildcards)", FEATURE, (unsigned long long) (K - sp->R),
                    (unsigned long long) K);
    return -1;
  }
  if (K / 2 > 0xFFFFFFFFull) {
    gtamd_set_error("%s: %llu reads, 4294967295 at most expected", FEATURE, (unsigned long long) (K / 2));
    return -1;
  }
  HIP_TRY(hipSetDevice(ct->device));
  if (K != 0) {
    // the separator in the middle: the reads are the first half, of (n - 1) / 2 symbols
    u32 middle = 0;
    TRY(fetch(ct->st, { { sp->seps + (K / 2 - 1), &middle, sizeof middle } }));
    if (sp->index.n % 2 == 0 || middle != (sp->index.n - 1) / 2) {
      gtamd_set_error("%s: %llu symbols with separator %llu at position %u are no mirrored set: that separator is "
                      "expected in the middle", FEATURE, (unsigned long long) sp->index.n,
                      (unsigned long long) (K / 2 - 1), middle);
      return -1;
    }
    TRY(sp->index.suf_bytes == 4 ? decide<u32>(ct, (u32) K) : decide<u64>(ct, (u32) K));
  }
  ct->R = (u32) (K / 2);
  ct->info.table_entries = sp->index.n + 1;
  ct->info.sequences = K;
  ct->info.reads = K / 2;
  ct->info.device_bytes = held_bytes(ct);
  ct->decided = true;
  if (info != nullptr) *info = ct->info;
  return 0;
  GTAMD_ABI_END(-1)
}

extern "C" int gtamd_contained_verdicts(const gtamd_contained *ct, uint8_t *out, int out_on_device) {
  GTAMD_ABI_BEGIN
  if (ct == nullptr || (out == nullptr && ct->R)) { gtamd_set_error("invalid argument to gtamd_contained_verdicts"); return -1; }
  if (!ct->decided) {
    gtamd_set_error("%s: nothing is decided (gtamd_contained_decide)", FEATURE);
    return -1;
  }
  if (ct->R == 0) return 0;
  HIP_TRY(hipSetDevice(ct->device));
  HIP_TRY(hipMemcpyAsync(out, ct->verdict, ct->R, out_on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, ct->st));
  HIP_TRY(hipStreamSynchronize(ct->st));
  return 0;
  GTAMD_ABI_END(-1)
}

extern "C" int gtamd_contained_compact(gtamd_contained *ct, uint32_t mask, const uint8_t *enc, uint64_t n,
                                       uint8_t **out_device, uint64_t *out_n) {
  GTAMD_ABI_BEGIN
  if (ct == nullptr || out_device == nullptr || out_n == nullptr) {
    gtamd_set_error("invalid argument to gtamd_contained_compact");
    return -1;
  }
  if (!ct->decided) {
    gtamd_set_error("%s: nothing is decided (gtamd_contained_decide)", FEATURE);
    return -1;
  }
  if (mask >> CT_VERDICTS) {
    gtamd_set_error("%s: mask %u names a verdict that is none (%u verdicts)", FEATURE, mask, CT_VERDICTS);
    return -1;
  }
  const gtamd_spm *sp = ct->sp;
  const u64 half = sp->index.n ? (sp->index.n - 1) / 2 : 0;
  if (n != half) {
    gtamd_set_error("%s: %llu symbols given, the reads of the index are %llu", FEATURE, (unsigned long long) n,
                    (unsigned long long) half);
    return -1;
  }
  HIP_TRY(hipSetDevice(ct->device));
  TRY(compact(ct, ct->verdict, mask, enc != nullptr ? enc : sp->index.enc, n, sp->seps, sp->nseps, ct->R, out_device,
              out_n));
  ct->info.device_bytes = held_bytes(ct);
  return 0;
  GTAMD_ABI_END(-1)
}

extern "C" int gtamd_contained_result(const gtamd_contained *ct, uint8_t *out, int out_on_device) {
  GTAMD_ABI_BEGIN
  if (ct == nullptr || (out == nullptr && ct->result)) { gtamd_set_error("invalid argument to gtamd_contained_result"); return -1; }
  if (ct->result == 0) return 0;
  HIP_TRY(hipSetDevice(ct->device));
  HIP_TRY(hipMemcpyAsync(out, ct->out, ct->result, out_on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost,
                         ct->st));
  HIP_TRY(hipStreamSynchronize(ct->st));
  return 0;
  GTAMD_ABI_END(-1)
}

extern "C" int gtamd_contained_get_info(const gtamd_contained *ct, gtamd_contained_info *info) {
  GTAMD_ABI_BEGIN
  return consumer_info(ct, info, "gtamd_contained_get_info");
  GTAMD_ABI_END(-1)
}

extern "C" int gtamd_contained_mirror(gtamd_contained *ct, const uint8_t *enc, uint64_t n, uint8_t *out) {
  GTAMD_ABI_BEGIN
  if (ct == nullptr || out == nullptr || (enc == nullptr && n)) {
    gtamd_set_error("invalid argument to gtamd_contained_mirror");
    return -1;
  }
  TRY(refuse_sizes(FEATURE, 2 * n + 1, 0, "mirrored"));
  HIP_TRY(hipSetDevice(ct->device));
  k_ct_mirror<<<(u32) div_up(2 * n + 1, CT_TILE), CT_THREADS, 0, ct->st>>>(enc, n, out);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(ct->st));
  return 0;
  GTAMD_ABI_END(-1)
}

extern "C" int gtamd_contained_drop_wildcards(gtamd_contained *ct, const uint8_t *enc, uint64_t n,
                                              const uint64_t *separators, uint64_t count, uint8_t **out_device,
                                              uint64_t *out_n, uint64_t *dropped) {
  GTAMD_ABI_BEGIN
  if (ct == nullptr || out_device == nullptr || out_n == nullptr || (enc == nullptr && n) ||
      (separators == nullptr && count)) {
    gtamd_set_error("invalid argument to gtamd_contained_drop_wildcards");
    return -1;
  }
  *out_device = nullptr;
  *out_n = 0;
  if (dropped != nullptr) *dropped = 0;
  ct->result = 0;
  ct->flagged = 0;
  if (n == 0) return 0;
  TRY(refuse_sizes(FEATURE, n, 0, "filtered"));
  std::vector<u32> seps(count);
  for (u64 k = 0; k < count; k++) {
    if (separators[k] >= n || (k && separators[k] <= separators[k - 1])) {
      gtamd_set_error("%s: separator %llu at position %llu: ascending positions below %llu expected", FEATURE,
                      (unsigned long long) k, (unsigned long long) separators[k], (unsigned long long) n);
      return -1;
    }
    seps[k] = (u32) separators[k];
  }
  HIP_TRY(hipSetDevice(ct->device));
  hipStream_t st = ct->st;
  const u32 R = (u32) count + 1;
  if (ct->seps.grow((count ? count : 1) * 4) != hipSuccess || ct->flag.grow(R) != hipSuccess)
    return out_of_memory(FEATURE, R, "reads");
  if (count) HIP_TRY(hipMemcpyAsync(ct->seps, seps.data(), count * 4, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemsetAsync(ct->flag, 0, R, st));
  HIP_TRY(hipMemsetAsync(ct->words, 0, W_WORDS * sizeof(u64), st));
  k_ct_wildcards<<<(u32) div_up(n, CT_TILE), CT_THREADS, 0, st>>>(enc, n, ct->seps, (u32) count, ct->flag);
  HIP_TRY(hipGetLastError());
  k_ct_tally<<<(u32) div_up(R, CT_TILE), CT_THREADS, 0, st>>>(ct->flag, R, ct->words);
  HIP_TRY(hipGetLastError());
  u64 flagged = 0;
  TRY(fetch(st, { { ct->words + W_COUNT + 1, &flagged, sizeof flagged } }));    // (seps is read by the copy: idle now)
  if (dropped != nullptr) *dropped = flagged;
  ct->flagged = R;
  TRY(compact(ct, ct->flag, 1u << 1, enc, n, ct->seps, (u32) count, R, out_device, out_n));
  ct->info.device_bytes = held_bytes(ct);
  return 0;
  GTAMD_ABI_END(-1)
}

extern "C" int gtamd_contained_wildcard_flags(const gtamd_contained *ct, uint8_t *out, int out_on_device) {
  GTAMD_ABI_BEGIN
  if (ct == nullptr || (out == nullptr && ct->flagged)) {
    gtamd_set_error("invalid argument to gtamd_contained_wildcard_flags");
    return -1;
  }
  if (ct->flagged == 0) return 0;
  HIP_TRY(hipSetDevice(ct->device));
  HIP_TRY(hipMemcpyAsync(out, ct->flag, ct->flagged, out_on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost,
                         ct->st));
  HIP_TRY(hipStreamSynchronize(ct->st));
  return 0;
  GTAMD_ABI_END(-1)
}

extern "C" int gtamd_contained_mirror_result(gtamd_contained *ct, uint8_t **out_device, uint64_t *out_n) {
  GTAMD_ABI_BEGIN
  if (ct == nullptr || out_device == nullptr || out_n == nullptr) {
    gtamd_set_error("invalid argument to gtamd_contained_mirror_result");
    return -1;
  }
  *out_device = nullptr;
  *out_n = 0;
  const u64 n = ct->result;
  TRY(refuse_sizes(FEATURE, 2 * n + 1, 0, "mirrored"));
  HIP_TRY(hipSetDevice(ct->device));
  if (ct->both.grow(2 * n + 1) != hipSuccess) return out_of_memory(FEATURE, 2 * n + 1, "mirrored symbols");
  k_ct_mirror<<<(u32) div_up(2 * n + 1, CT_TILE), CT_THREADS, 0, ct->st>>>(ct->out, n, ct->both);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(ct->st));
  ct->info.device_bytes = held_bytes(ct);
  *out_device = ct->both;
  *out_n = 2 * n + 1;
  return 0;
  GTAMD_ABI_END(-1)
}
