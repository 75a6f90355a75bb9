// esa_spmred.hip -- the irreducible suffix-prefix matches of a read set from .suf
// and .lcp in device memory: `gt readjoiner overlap -l L` (C ABI, the semantics
// and the algorithm: include/gtamd_spmred.h).
//
//   1-4   gtamd_spm_prepare (esa_spm.hip)   the object owns a gtamd_spm: terminal
//                              suffixes, read starts, intervals, the places of
//                              the Z pairs
//   5     k_sr_starts          one lane per read start: position and length of
//                              its sequence; the contained sequences counted
//         k_sr_positions       one lane per terminal suffix: its text position;
//         radix_sort_pairs (esa_prims)      sorted, with the way back
//   6     k_sr_decide          one lane per pair of a chunk: transitive or not
//                              (esa_spmred_core.h), the mirror filter; a wave's
//                              64 verdicts are one ballot, one word of the bitmap
//   7     offsets_u64_counted (esa_prims)   64-bit exclusive scan of the words' counts
//   8     k_sr_emit            one lane per kept record of a chunk
#include "esa_common.h"
#include "esa_index.h"
#include "esa_prims.h"
#include "esa_devutil.h"
#include "esa_spmred_core.h"
#include "esa_spm_state.h"
#include "../../include/gtamd_spmred.h"

static_assert(SR_ELIMTRANS == GTAMD_SPMRED_ELIMTRANS && SR_MIRRORED == GTAMD_SPMRED_MIRRORED &&
              SR_PREFIX_DIRECT == GTAMD_SPMRED_PREFIX_DIRECT && SR_SUFFIX_DIRECT == GTAMD_SPMRED_SUFFIX_DIRECT,
              "the flags of the lane header are those of the C ABI");
static_assert(sizeof(SrRecord) == sizeof(gtamd_spmred_record), "one record");

namespace {

constexpr int SR_THREADS = SC_THREADS;
constexpr u32 SR_TILE = SR_THREADS;               // pairs, or records, of one workgroup: one a lane
constexpr u64 SR_MIN_CAPACITY = SR_TILE;          // the smallest capacity of an emit call
constexpr u64 SR_CHUNK = 1ull << 20;              // pairs of one launch of step 6: 4096 workgroups
constexpr u64 SR_MAX_EMIT = 1ull << 24;           // records of one launch of step 8
constexpr u64 SR_MAX_PAIRS = 64 * ((1ull << 32) - 256);   // the words of the bitmap are counts of one scan
static_assert(SR_CHUNK % 64 == 0 && SR_TILE % 64 == 0, "a wave's ballot is one whole word of the bitmap");

enum { W_KEPT = 0, W_SAME, W_OTHER, W_CONTAINED, W_CANDIDATES, W_MAXCAND, W_LETTERS, W_WORDS };

// ---- step 5 ----------------------------------------------------------------------
template <typename S>
__global__ __launch_bounds__(SR_THREADS) void k_sr_starts(SpIndex<S> x, const u32 *starts, u32 R, const u32 *seps,
                                                          u32 nseps, u32 L, u32 *spos, u32 *slen, u64 *w) {
  const u64 j = (u64) blockIdx.x * SR_TILE + threadIdx.x;
  bool contained = false;
  if (j < R) {
    u32 pos, len;
    sr_start(x, starts, seps, nseps, j, &pos, &len);
    spos[j] = pos;
    slen[j] = len;
    contained = sr_contained(x, starts, j, L);
  }
  const u64 mask = __ballot(contained);
  if ((threadIdx.x & 63) == 0 && mask) atomicAdd((unsigned long long *) &w[W_CONTAINED], (unsigned long long) __popcll(mask));
}

template <typename S>
__global__ __launch_bounds__(SR_THREADS) void k_sr_positions(SpIndex<S> x, const u32 *idx, u32 M, u32 *pos, u32 *place) {
  const u64 k = (u64) blockIdx.x * SR_TILE + threadIdx.x;
  if (k >= M) return;
  const u64 p = x.suf[idx[k]];
  pos[k] = (u32) (p < x.n ? p : x.n);
  place[k] = (u32) k;
}

// ---- step 6 ----------------------------------------------------------------------
// pairs [c0, c1) of all off[M], c0 a multiple of 64, SR_TILE a workgroup: bit g &
// 63 of bitmap[g / 64] = pair g is kept, wcnt[g / 64] = the set bits of that word
template <typename S>
__global__ __launch_bounds__(SR_THREADS) void k_sr_decide(SpIndex<S> x, SrLists a, u32 L, u32 flags, const u64 *off,
                                                          u64 c0, u64 c1, u64 *bitmap, u32 *wcnt, u64 *w) {
  __shared__ u64 span[2];                 // the terminal suffixes of the workgroup's first and last pair
  __shared__ unsigned long long fig[W_WORDS];
  const u64 g0 = c0 + (u64) blockIdx.x * SR_TILE;
  const u64 last = (c1 - g0 < SR_TILE ? c1 : g0 + SR_TILE) - 1;
  if (threadIdx.x < 2) span[threadIdx.x] = entry_of(off, 0, a.M, threadIdx.x == 0 ? g0 : last);
  if (threadIdx.x < W_WORDS) fig[threadIdx.x] = 0;
  __syncthreads();
  const u64 g = g0 + threadIdx.x;
  bool kept = false, same = false, other = false;
  if (g <= last) {
    const u64 k = entry_of(off, span[0], span[1] + 1, g), j = g - off[k];
    kept = true;
    if (flags & SR_ELIMTRANS) {
      SrWalk walk = { 0, 0 };
      if (sr_transitive(x, a, L, k, j, &walk)) {
        SpRecord rec;
        sp_record(x, a.starts, a.seps, a.nseps, a.idx[k], a.len[k], a.first[k], j, &rec);
        bool d;
        const u64 K = a.nseps + 1;
        same = (flags & SR_MIRRORED) ? sr_read_of(rec.suffix_seq, K, &d) == sr_read_of(rec.prefix_seq, K, &d)
                                     : rec.suffix_seq == rec.prefix_seq;
        other = !same;
        kept = false;
      }
      if (walk.candidates) {
        atomicAdd(&fig[W_CANDIDATES], (unsigned long long) walk.candidates);
        atomicMax(&fig[W_MAXCAND], (unsigned long long) walk.candidates);
      }
      if (walk.letters) atomicAdd(&fig[W_LETTERS], (unsigned long long) walk.letters);
    }
    if (kept && (flags & SR_MIRRORED)) kept = sr_pair_kept(x, a, k, j);
  }
  // (all lanes of the wave are here: those without a pair vote 0)
  const u64 mk = __ballot(kept), ms = __ballot(same), mo = __ballot(other);
  if ((threadIdx.x & 63) == 0) {
    if (g <= last) {
      bitmap[g >> 6] = mk;
      wcnt[g >> 6] = (u32) __popcll(mk);
    }
    if (ms) atomicAdd(&fig[W_SAME], (unsigned long long) __popcll(ms));
    if (mo) atomicAdd(&fig[W_OTHER], (unsigned long long) __popcll(mo));
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    if (fig[W_SAME]) atomicAdd((unsigned long long *) &w[W_SAME], fig[W_SAME]);
    if (fig[W_OTHER]) atomicAdd((unsigned long long *) &w[W_OTHER], fig[W_OTHER]);
    if (fig[W_CANDIDATES]) atomicAdd((unsigned long long *) &w[W_CANDIDATES], fig[W_CANDIDATES]);
    if (fig[W_MAXCAND]) atomicMax((unsigned long long *) &w[W_MAXCAND], fig[W_MAXCAND]);
    if (fig[W_LETTERS]) atomicAdd((unsigned long long *) &w[W_LETTERS], fig[W_LETTERS]);
  }
}

// ---- step 8 ----------------------------------------------------------------------
// the pair behind kept record e: woff[v] = kept records of the words in front of word v
__device__ __forceinline__ u64 pair_of(const u64 *bitmap, const u64 *woff, u64 va, u64 vb, u64 e) {
  const u64 v = entry_of(woff, va, vb, e);
  return v * 64 + sr_select(bitmap[v], (u32) (e - woff[v]));
}

// kept records [e0, e1) of all woff[W] to out, SR_TILE a workgroup
template <typename S>
__global__ __launch_bounds__(SR_THREADS) void k_sr_emit(SpIndex<S> x, SrLists a, u32 flags, const u64 *off,
                                                        const u64 *bitmap, const u64 *woff, u64 W, u64 e0, u64 e1,
                                                        SrRecord *out) {
  __shared__ u64 word[2], span[2];        // the words and the terminal suffixes of the first and last record
  const u64 b0 = e0 + (u64) blockIdx.x * SR_TILE;
  const u64 last = (e1 - b0 < SR_TILE ? e1 : b0 + SR_TILE) - 1;
  if (threadIdx.x < 2) {
    const u64 e = threadIdx.x == 0 ? b0 : last;
    const u64 v = entry_of(woff, 0, W, e);
    word[threadIdx.x] = v;
    span[threadIdx.x] = entry_of(off, 0, a.M, v * 64 + sr_select(bitmap[v], (u32) (e - woff[v])));
  }
  __syncthreads();
  const u64 e = b0 + threadIdx.x;
  if (e > last) return;
  const u64 g = pair_of(bitmap, woff, word[0], word[1] + 1, e);
  const u64 k = entry_of(off, span[0], span[1] + 1, g);
  SrRecord rec;
  sr_record(x, a, flags, k, g - off[k], &rec);
  out[e - e0] = rec;
}

}  // namespace

struct gtamd_spmred : ConsumerBase<4> {
  gtamd_spm *sp = nullptr;             // steps 1 to 4, and the index
  bool prepared = false;
  u32 L = 0, flags = 0;
  // what a prepare leaves for the emit calls
  Dev<u32> spos, slen, pos_a, pos_b, place_a, place_b, sortws, wcnt;
  Dev<u64> bitmap, woff, tsum;
  Dev<u8> out;                         // records on their way to host memory
  const u32 *tpos = nullptr, *tperm = nullptr;
  u64 W = 0;
  gtamd_spmred_info info = gtamd_spmred_info();
  ~gtamd_spmred() { gtamd_spm_destroy(sp); }
};

namespace {

const char FEATURE[] = "irreducible suffix-prefix matches";

u64 held_bytes(const gtamd_spmred *sr) {
  return sr->sp->info.device_bytes + sr->spos.bytes + sr->slen.bytes + sr->pos_a.bytes + sr->pos_b.bytes +
         sr->place_a.bytes + sr->place_b.bytes + sr->sortws.bytes + sr->wcnt.bytes + sr->bitmap.bytes +
         sr->woff.bytes + sr->tsum.bytes + sr->words.bytes + sr->out.bytes;
}

template <typename S> SpIndex<S> view(const gtamd_spmred *sr) {
  const ResidentIndex &x = sr->sp->index;
  return SpIndex<S>{ x.enc, x.n, (const S *) x.suf, x.lcp, x.llv, x.llv_pairs };
}

SrLists lists(const gtamd_spmred *sr) {
  const gtamd_spm *sp = sr->sp;
  return SrLists{ sp->idx, sp->len, sp->first, sp->cnt, sp->M, sp->starts, sr->spos, sr->slen, sp->R,
                  sp->seps, sp->nseps, sr->tpos, sr->tperm };
}

template <typename S> int prepare(gtamd_spmred *sr, u32 L, u32 flags) {
  hipStream_t st = sr->st;
  gtamd_spm *sp = sr->sp;
  const u32 M = sp->M, R = sp->R;
  const u64 Z = sp->info.matches, W = div_up(Z, 64);
  HIP_TRY(hipMemsetAsync(sr->words, 0, W_WORDS * sizeof(u64), st));
  HIP_TRY(hipEventRecord(sr->ev[0], st));

  // 5: the sequences of the read starts; the terminal suffixes by text position
  if (sr->spos.grow((R ? (u64) R : 1) * 4) != hipSuccess || sr->slen.grow((R ? (u64) R : 1) * 4) != hipSuccess)
    return out_of_memory(FEATURE, R, "read starts");
  if (R != 0) {
    k_sr_starts<S><<<(u32) div_up(R, SR_TILE), SR_THREADS, 0, st>>>(view<S>(sr), sp->starts, R, sp->seps, sp->nseps, L,
                                                                    sr->spos, sr->slen, sr->words);
    HIP_TRY(hipGetLastError());
  }
  if (Z != 0) {
    const u64 m4 = (u64) M * 4;
    if (sr->pos_a.grow(m4) != hipSuccess || sr->pos_b.grow(m4) != hipSuccess || sr->place_a.grow(m4) != hipSuccess ||
        sr->place_b.grow(m4) != hipSuccess || sr->sortws.grow(radix_workspace_words(M) * sizeof(u32)) != hipSuccess)
      return out_of_memory(FEATURE, M, "terminal suffixes by position");
    k_sr_positions<S><<<(u32) div_up(M, SR_TILE), SR_THREADS, 0, st>>>(view<S>(sr), sp->idx, M, sr->pos_a, sr->place_a);
    HIP_TRY(hipGetLastError());
    int shifts[4], widths[4], passes = 0;
    for (u64 top = sp->index.n; top != 0 && passes < 4; top >>= 8, passes++) {
      shifts[passes] = 8 * passes;
      widths[passes] = 8;
    }
    TRY(radix_sort_pairs<u32, u32>(sr->pos_a, sr->place_a, sr->pos_b, sr->place_b, M, shifts, widths, passes,
                                   sr->sortws, st, nullptr, nullptr));
    sr->tpos = (passes & 1) ? sr->pos_b : sr->pos_a;
    sr->tperm = (passes & 1) ? sr->place_b : sr->place_a;

    // 6: the verdicts, chunk by chunk
    const u64 bytes = W * 8 + W * 4 + (W + 1) * 8 + div_up(W, 256) * 8;
    if (Z > SR_MAX_PAIRS || sr->bitmap.grow(W * 8) != hipSuccess || sr->wcnt.grow(W * 4) != hipSuccess ||
        sr->woff.grow((W + 1) * 8) != hipSuccess || sr->tsum.grow(div_up(W, 256) * 8) != hipSuccess) {
      gtamd_set_error("%s: %llu pairs need %llu bytes of device memory for their verdicts and places, which %s",
                      FEATURE, (unsigned long long) Z, (unsigned long long) bytes,
                      Z > SR_MAX_PAIRS ? "is beyond the limit of one scan" : "cannot be allocated");
      return -1;
    }
    HIP_TRY(hipEventRecord(sr->ev[1], st));
    for (u64 c0 = 0; c0 < Z; c0 += SR_CHUNK) {
      const u64 c1 = Z - c0 < SR_CHUNK ? Z : c0 + SR_CHUNK;
      k_sr_decide<S><<<(u32) div_up(c1 - c0, SR_TILE), SR_THREADS, 0, st>>>(view<S>(sr), lists(sr), L, flags, sp->off,
                                                                           c0, c1, sr->bitmap, sr->wcnt, sr->words);
      HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipEventRecord(sr->ev[2], st));
    // 7: the places
    TRY(offsets_u64_counted(sr->wcnt, W, sr->tsum, sr->woff, sr->words + W_KEPT, st));
  }
  HIP_TRY(hipEventRecord(sr->ev[3], st));
  u64 h[W_WORDS];
  TRY(fetch(st, { { sr->words, h, sizeof h } }));
  float own = 0, decide = 0;
  HIP_TRY(hipEventElapsedTime(&own, sr->ev[0], sr->ev[3]));
  if (Z != 0) HIP_TRY(hipEventElapsedTime(&decide, sr->ev[1], sr->ev[2]));
  sr->W = W;
  gtamd_spmred_info &o = sr->info;
  const gtamd_spm_info &i = sp->info;
  o.table_entries = i.table_entries;
  o.terminal_suffixes = i.terminal_suffixes;
  o.read_starts = i.read_starts;
  o.matches = i.matches;
  o.max_width = i.max_width;
  o.max_matches_of_one_suffix = i.max_matches_of_one_suffix;
  o.search_symbols = i.search_symbols;
  o.kept = h[W_KEPT];
  o.transitive_same_read = h[W_SAME];
  o.transitive_other = h[W_OTHER];
  o.contained_sequences = h[W_CONTAINED];
  o.candidates_examined = h[W_CANDIDATES];
  o.max_candidates_of_one_pair = h[W_MAXCAND];
  o.letters_compared = h[W_LETTERS];
  o.spm_ms = i.device_ms;
  o.decide_ms = decide;
  o.device_ms = i.device_ms + own;
  return 0;
}

template <typename S> int emit_records(gtamd_spmred *sr, u64 e0, u64 count, SrRecord *dst) {
  for (u64 done = 0; done < count; done += SR_MAX_EMIT) {
    const u64 chunk = count - done < SR_MAX_EMIT ? count - done : SR_MAX_EMIT;
    k_sr_emit<S><<<(u32) div_up(chunk, SR_TILE), SR_THREADS, 0, sr->st>>>(view<S>(sr), lists(sr), sr->flags, sr->sp->off,
                                                                         sr->bitmap, sr->woff, sr->W, e0 + done,
                                                                         e0 + done + chunk, dst + done);
    HIP_TRY(hipGetLastError());
  }
  return 0;
}

int emit(gtamd_spmred *sr, u64 *cursor, gtamd_spmred_record *out, u64 capacity, int out_on_device, u64 *written) {
  *written = 0;
  const u64 total = sr->info.kept, cur = *cursor;
  TRY(refuse_window(FEATURE, "kept matches", cur, total, capacity, SR_MIN_CAPACITY));
  if (cur == total) return 0;
  const u64 count = capacity < total - cur ? capacity : total - cur;
  RecordStage<SrRecord> stage(out, out_on_device);
  if (stage.begin(sr->out, count) != hipSuccess) return out_of_memory(FEATURE, count, "records");
  TRY(sr->sp->index.suf_bytes == 4 ? emit_records<u32>(sr, cur, count, stage.dst)
                                   : emit_records<u64>(sr, cur, count, stage.dst));
  TRY(stage.finish(count, sr->st));
  *cursor = cur + count;
  *written = count;
  return 0;
}

// a new index: what was prepared is none
int index_set(gtamd_spmred *sr, int rc) {
  sr->prepared = false;
  return rc;
}

}  // namespace

extern "C" gtamd_spmred *gtamd_spmred_create(int device) {
  GTAMD_ABI_BEGIN
  gtamd_spmred *sr = create_consumer<gtamd_spmred>(device, W_WORDS, "the matcher of irreducible suffix-prefix matches");
  if (sr != nullptr && (sr->sp = gtamd_spm_create(device)) == nullptr) {
    destroy_consumer(sr);
    return nullptr;
  }
  return sr;
  GTAMD_ABI_END(nullptr)
}

extern "C" void gtamd_spmred_destroy(gtamd_spmred *sr) { destroy_consumer(sr); }

extern "C" void gtamd_spmred_geometry(uint64_t *chunk_pairs, uint64_t *min_capacity) {
  if (chunk_pairs != nullptr) *chunk_pairs = SR_CHUNK;
  if (min_capacity != nullptr) *min_capacity = SR_MIN_CAPACITY;
}

extern "C" int gtamd_spmred_set_index(gtamd_spmred *sr, const uint8_t *enc, uint64_t n, const void *suf,
                                      uint32_t suf_bytes, const uint8_t *lcp, const uint64_t *llv, uint64_t llv_pairs) {
  GTAMD_ABI_BEGIN
  if (sr == nullptr) { gtamd_set_error("invalid argument to gtamd_spmred_set_index"); return -1; }
  return index_set(sr, gtamd_spm_set_index(sr->sp, enc, n, suf, suf_bytes, lcp, llv, llv_pairs));
  GTAMD_ABI_END(-1)
}

extern "C" int gtamd_spmred_set_index_host(gtamd_spmred *sr, const uint8_t *enc, uint64_t n, const void *suf,
                                           uint32_t suf_bytes, const uint8_t *lcp, const uint64_t *llv,
                                           uint64_t llv_pairs) {
  GTAMD_ABI_BEGIN
  if (sr == nullptr) { gtamd_set_error("invalid argument to gtamd_spmred_set_index_host"); return -1; }
  return index_set(sr, gtamd_spm_set_index_host(sr->sp, enc, n, suf, suf_bytes, lcp, llv, llv_pairs));
  GTAMD_ABI_END(-1)
}

extern "C" int gtamd_spmred_set_index_esa(gtamd_spmred *sr, const gtamd_esa_ctx *esa, const uint8_t *enc, uint64_t n) {
  GTAMD_ABI_BEGIN
  if (sr == nullptr) { gtamd_set_error("invalid argument to gtamd_spmred_set_index_esa"); return -1; }
  return index_set(sr, gtamd_spm_set_index_esa(sr->sp, esa, enc, n));
  GTAMD_ABI_END(-1)
}

extern "C" int gtamd_spmred_prepare(gtamd_spmred *sr, uint32_t min_len, uint32_t flags, gtamd_spmred_info *info) {
  GTAMD_ABI_BEGIN
  if (sr == nullptr) { gtamd_set_error("invalid argument to gtamd_spmred_prepare"); return -1; }
  if (flags & ~(GTAMD_SPMRED_ELIMTRANS | GTAMD_SPMRED_MIRRORED)) {
    gtamd_set_error("%s: flags %u, GTAMD_SPMRED_ELIMTRANS | GTAMD_SPMRED_MIRRORED at most expected", FEATURE, flags);
    return -1;
  }
  sr->prepared = false;
  sr->info = gtamd_spmred_info();
  // (no index, a minimum length of 0: refused there, in its words)
  TRY(gtamd_spm_prepare(sr->sp, min_len, nullptr));
  const u64 K = sr->sp->index.n ? (u64) sr->sp->nseps + 1 : 0;
  if ((flags & GTAMD_SPMRED_MIRRORED) && K % 2) {
    gtamd_set_error("%s: %llu sequences are no mirrored set: an even number is expected, the reads and their "
                    "reverse complements", FEATURE, (unsigned long long) K);
    return -1;
  }
  HIP_TRY(hipSetDevice(sr->device));
  TRY(sr->sp->index.suf_bytes == 4 ? prepare<u32>(sr, min_len, flags) : prepare<u64>(sr, min_len, flags));
  sr->L = min_len;
  sr->flags = flags;
  sr->info.device_bytes = held_bytes(sr);
  sr->prepared = true;
  if (info != nullptr) *info = sr->info;
  return 0;
  GTAMD_ABI_END(-1)
}

extern "C" int gtamd_spmred_emit(gtamd_spmred *sr, uint64_t *cursor, gtamd_spmred_record *out, uint64_t capacity,
                                 int out_on_device, uint64_t *written) {
  GTAMD_ABI_BEGIN
  if (sr == nullptr || cursor == nullptr || written == nullptr || (out == nullptr && capacity)) {
    gtamd_set_error("invalid argument to gtamd_spmred_emit");
    return -1;
  }
  if (!sr->prepared) {
    gtamd_set_error("%s: nothing is prepared (gtamd_spmred_prepare)", FEATURE);
    return -1;
  }
  HIP_TRY(hipSetDevice(sr->device));
  TRY(emit(sr, cursor, out, capacity, out_on_device, written));
  sr->info.device_bytes = held_bytes(sr);
  return 0;
  GTAMD_ABI_END(-1)
}

extern "C" int gtamd_spmred_get_info(const gtamd_spmred *sr, gtamd_spmred_info *info) {
  GTAMD_ABI_BEGIN
  return consumer_info(sr, info, "gtamd_spmred_get_info");
  GTAMD_ABI_END(-1)
}
