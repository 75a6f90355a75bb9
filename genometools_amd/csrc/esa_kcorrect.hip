// esa_kcorrect.hip -- the letters `gt readjoiner correct -k K -c C` rewrites in a
// read set, from .suf and .lcp of its (mirrored) text in device memory, and the
// set with them rewritten (C ABI, the definition and the algorithm:
// include/gtamd_kcorrect.h).
//
//   k_kc_letters   one lane per symbol: the non-special suffixes, counted by ballot
//   1  k_kc_heads      one lane per table entry: a flag per child head, the flags of a tile summed by ballot
//      offsets_u64 (esa_prims)   their places
//   2  k_kc_children   one lane per table entry: the heads compacted
//   3  k_kc_groups     one lane per child: the records it gives (esa_kcorrect_core.h)
//      offsets_u64_counted       their places
//   4  k_kc_emit       one lane per child: its records
//   5  radix_sort_pairs          the records by (target, order)
//      k_kc_first, k_kc_round    the letter of every record: the record it depends on, pointer doubling
//      k_kc_finals     one lane per sorted record: the last of a target, the tallies
//   6  k_kc_apply      one lane per sorted record: a final letter into the copy
#include "esa_common.h"
#include "esa_index.h"
#include "esa_prims.h"
#include "esa_devutil.h"
#include "esa_kcorrect_core.h"
#include "../../include/gtamd_kcorrect.h"

namespace {

constexpr int KC_THREADS = SC_THREADS;
constexpr u32 KC_TILE = KC_THREADS;               // entries, children or records of one workgroup: one a lane
constexpr u8 KC_NOT_FINAL = 255;

enum { W_LETTERS = 0, W_CHILDREN, W_RECORDS, W_GROUPS, W_UNTRUSTED, W_DEPENDENT, W_OPEN, W_CHANGED, W_DELTA,
       W_WORDS = W_DELTA + 4 };

// every lane of the wave comes here: the lanes with `flag` counted into *w by the first
__device__ __forceinline__ void wave_count(bool flag, u64 *w) {
  const u64 mask = __ballot(flag);
  if ((threadIdx.x & 63) == 0 && mask) atomicAdd((unsigned long long *) w, (unsigned long long) __popcll(mask));
}

__global__ __launch_bounds__(KC_THREADS) void k_kc_letters(const u8 *enc, u64 n, u64 *w) {
  const u64 p = (u64) blockIdx.x * KC_TILE + threadIdx.x;
  wave_count(p < n && enc[p] < 254, w + W_LETTERS);
}

// ---- step 1 ----------------------------------------------------------------------
__global__ __launch_bounds__(KC_THREADS) void k_kc_heads(const u8 *lcp, u64 N, u32 k, u32 *flag, u64 *tsum) {
  __shared__ u32 wsum[KC_THREADS / 64];
  const u64 i = (u64) blockIdx.x * KC_TILE + threadIdx.x;
  const bool head = i < N && kc_is_head(lcp, i, k);
  if (i < N) flag[i] = head;
  const u64 mask = __ballot(head);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = (u32) __popcll(mask);
  __syncthreads();
  if (threadIdx.x == 0) {
    u32 s = 0;
    for (u32 v = 0; v < KC_THREADS / 64; v++) s += wsum[v];
    tsum[blockIdx.x] = s;
  }
}

// ---- step 2 ----------------------------------------------------------------------
__global__ __launch_bounds__(KC_THREADS) void k_kc_children(const u32 *flag, const u64 *off, u64 N, u32 *heads) {
  const u64 i = (u64) blockIdx.x * KC_TILE + threadIdx.x;
  if (i >= N) return;
  if (flag[i]) heads[off[i]] = (u32) i;
  if (i + 1 == N) heads[off[N]] = (u32) N;            // (off[N] = C: heads has room for C + 1)
}

// ---- step 3 ----------------------------------------------------------------------
template <typename S>
__global__ __launch_bounds__(KC_THREADS) void k_kc_groups(KcIndex<S> x, const u32 *heads, u64 C, u32 k, u32 c, u32 *rcount,
                                                          u32 *src, u32 *first, u64 *w) {
  const u64 j = (u64) blockIdx.x * KC_TILE + threadIdx.x;
  bool examined = false, emits = false;
  if (j < C) {
    rcount[j] = kc_child(x, heads, C, k, c, j, &src[j], &first[j]);
    if (kc_group_start(x, heads, j, k)) {
      const KcGroup g = kc_group(x, heads, C, k, c, j);
      examined = g.examined;
      emits = g.emits;
    }
  }
  wave_count(examined, w + W_GROUPS);
  wave_count(emits, w + W_UNTRUSTED);
}

// ---- step 4 ----------------------------------------------------------------------
// the records of a child: fewer than c
template <typename S>
__global__ __launch_bounds__(KC_THREADS) void k_kc_emit(KcIndex<S> x, const u32 *heads, u64 C, u32 k, const u32 *rcount,
                                                        const u32 *src, const u32 *first, const u64 *roff, u32 rbits,
                                                        u32 *entry, u64 *target, u64 *source, u32 *group_first, u64 *keys,
                                                        u32 *order) {
  const u64 j = (u64) blockIdx.x * KC_TILE + threadIdx.x;
  if (j >= C || rcount[j] == 0) return;
  const u64 s = kc_normalised(x, (u64) x.suf[src[j]] + k - 1), g = roff[first[j]];
  for (u32 t = 0; t < rcount[j]; t++) {
    const u64 r = roff[j] + t, e = (u64) heads[j] + t;
    const u64 tg = kc_normalised(x, (u64) x.suf[e] + k - 1);
    entry[r] = (u32) e;
    target[r] = tg;
    source[r] = s;
    group_first[r] = (u32) g;
    keys[r] = (tg >> 1) << rbits | r;
    order[r] = (u32) r;
  }
}

// ---- step 5 ----------------------------------------------------------------------
__global__ __launch_bounds__(KC_THREADS) void k_kc_first(const u8 *enc, const u64 *keys, u64 R, u32 rbits, const u64 *target,
                                                         const u64 *source, const u32 *group_first, u64 *state, u64 *w) {
  const u64 r = (u64) blockIdx.x * KC_TILE + threadIdx.x;
  bool open = false;
  if (r < R) {
    const u64 s = kc_first_state(enc, keys, R, rbits, target[r], source[r], group_first[r]);
    state[r] = s;
    open = !(s & KC_DONE);
  }
  wave_count(open, w + W_DEPENDENT);
}

// one round: the states at `before` to `after`; *open counts those still not done
__global__ __launch_bounds__(KC_THREADS) void k_kc_round(const u64 *before, u64 R, u64 *after, u64 *open_count) {
  const u64 r = (u64) blockIdx.x * KC_TILE + threadIdx.x;
  bool open = false;
  if (r < R) {
    u64 s = before[r];
    if (!(s & KC_DONE)) s = kc_next_state(before, s);
    after[r] = s;
    open = !(s & KC_DONE);
  }
  wave_count(open, open_count);
}

// The final letters: flet[s] for the last sorted record of a target, else
// KC_NOT_FINAL; fpos[s] its position.  The positions whose letter changes and
// the change of the letter counts, one atomic per wave and figure.
__global__ __launch_bounds__(KC_THREADS) void k_kc_finals(const u8 *enc, u64 n, const u64 *keys, u64 R, u32 rbits,
                                                          const u64 *state, u32 *fpos, u8 *flet, u64 *w) {
  const u64 s = (u64) blockIdx.x * KC_TILE + threadIdx.x;
  u8 was = 255, now = 255;
  if (s < R) {
    const u64 pos = keys[s] >> rbits;
    u8 f = KC_NOT_FINAL;
    if (pos < n && kc_is_final(keys, R, rbits, s)) {       // (pos >= n: a table that is none)
      f = (u8) (state[keys[s] & ((1ull << rbits) - 1)] & 3);
      if (enc[pos] != f) { was = enc[pos]; now = f; }
    }
    fpos[s] = (u32) pos;
    flet[s] = f;
  }
  wave_count(now != 255, w + W_CHANGED);
#pragma unroll
  for (u32 a = 0; a < 4; a++) {
    const u64 plus = __ballot(now == a), minus = __ballot(was == a);
    const long long d = (long long) __popcll(plus) - (long long) __popcll(minus);
    if ((threadIdx.x & 63) == 0 && d != 0) atomicAdd((unsigned long long *) &w[W_DELTA + a], (unsigned long long) d);
  }
}

// (entry, normalised position, letter) of every record, in record order
__global__ __launch_bounds__(KC_THREADS) void k_kc_triples(const u32 *entry, const u64 *target, const u64 *state, u64 R,
                                                           u64 *out) {
  const u64 r = (u64) blockIdx.x * KC_TILE + threadIdx.x;
  if (r >= R) return;
  out[3 * r] = entry[r];
  out[3 * r + 1] = target[r] >> 1;
  out[3 * r + 2] = state[r] & 3;
}

// ---- step 6 ----------------------------------------------------------------------
__global__ __launch_bounds__(KC_THREADS) void k_kc_apply(const u32 *fpos, const u8 *flet, u64 R, u64 n, u8 *out) {
  const u64 s = (u64) blockIdx.x * KC_TILE + threadIdx.x;
  if (s < R && flet[s] != KC_NOT_FINAL && fpos[s] < n) out[fpos[s]] = flet[s];
}

}  // namespace

struct gtamd_kcorrect : ConsumerBase<2> {
  ResidentIndex index;
  bool mirrored = false;
  bool decided = false;
  u64 R = 0;                           // records of the last decide
  u64 result = 0;                      // symbols of the last apply, in out
  Dev<u32> flag, heads, rcount, src, first, entry, group_first, order, order_b, fpos, sortws;
  Dev<u64> tsum, off, roff, target, source, keys, keys_b, state, state_b;
  Dev<u8> flet, out, stage;
  u64 *sorted = nullptr, *letters = nullptr;      // keys or keys_b, state or state_b: where the results are
  gtamd_kcorrect_info info = gtamd_kcorrect_info();
};

namespace {

const char FEATURE[] = "k-mer correction";

u64 held_bytes(const gtamd_kcorrect *kc) {
  return kc->index.bytes() + kc->words.bytes + kc->flag.bytes + kc->heads.bytes + kc->rcount.bytes + kc->src.bytes +
         kc->first.bytes + kc->entry.bytes + kc->group_first.bytes + kc->order.bytes + kc->order_b.bytes + kc->fpos.bytes +
         kc->sortws.bytes + kc->tsum.bytes + kc->off.bytes + kc->roff.bytes + kc->target.bytes + kc->source.bytes +
         kc->keys.bytes + kc->keys_b.bytes + kc->state.bytes + kc->state_b.bytes + kc->flet.bytes + kc->out.bytes +
         kc->stage.bytes;
}

u32 bits_of(u64 v) {                   // bits that hold every value up to v, one at least
  u32 b = 1;
  while (b < 64 && v >> b) b++;
  return b;
}

// the symbols the correction rewrites: the first half of a mirrored text
u64 unmirrored_symbols(const gtamd_kcorrect *kc) { return kc->mirrored ? kc->index.n >> 1 : kc->index.n; }

template <typename S> int decide(gtamd_kcorrect *kc, u32 k, u32 c) {
  hipStream_t st = kc->st;
  const ResidentIndex &ix = kc->index;
  KcIndex<S> x = { ix.enc, ix.n, (const S *) ix.suf, ix.lcp, 0, kc->mirrored ? ix.n >> 1 : ix.n };
  u64 h[W_WORDS];
  k_kc_letters<<<(u32) div_up(ix.n, KC_TILE), KC_THREADS, 0, st>>>(ix.enc, ix.n, kc->words);
  HIP_TRY(hipGetLastError());
  TRY(fetch(st, { { kc->words, h, sizeof h } }));
  const u64 N = x.N = h[W_LETTERS];
  kc->info.suffixes = N;
  if (N == 0 || k < 2) return 0;
  // 1, 2: the children
  const u64 tiles = div_up(N, KC_TILE);
  if (kc->flag.grow(N * 4) != hipSuccess || kc->off.grow((N + 1) * 8) != hipSuccess || kc->tsum.grow(tiles * 8) != hipSuccess)
    return out_of_memory(FEATURE, N, "table entries");
  k_kc_heads<<<(u32) tiles, KC_THREADS, 0, st>>>(ix.lcp, N, k, kc->flag, kc->tsum);
  HIP_TRY(hipGetLastError());
  TRY(offsets_u64(kc->flag, N, kc->tsum, kc->off, kc->words + W_CHILDREN, st));
  TRY(fetch(st, { { kc->words, h, sizeof h } }));
  const u64 C = h[W_CHILDREN];                          // (entry 0 is a head: one at least)
  if (kc->heads.grow((C + 1) * 4) != hipSuccess || kc->rcount.grow(C * 4) != hipSuccess || kc->src.grow(C * 4) != hipSuccess ||
      kc->first.grow(C * 4) != hipSuccess || kc->roff.grow((C + 1) * 8) != hipSuccess ||
      kc->tsum.grow(div_up(C, SC_THREADS) * 8) != hipSuccess)
    return out_of_memory(FEATURE, C, "k-mers");
  k_kc_children<<<(u32) tiles, KC_THREADS, 0, st>>>(kc->flag, kc->off, N, kc->heads);
  HIP_TRY(hipGetLastError());
  // 3: the groups
  k_kc_groups<S><<<(u32) div_up(C, KC_TILE), KC_THREADS, 0, st>>>(x, kc->heads, C, k, c, kc->rcount, kc->src, kc->first,
                                                                 kc->words);
  HIP_TRY(hipGetLastError());
  TRY(offsets_u64_counted(kc->rcount, C, kc->tsum, kc->roff, kc->words + W_RECORDS, st));
  TRY(fetch(st, { { kc->words, h, sizeof h } }));
  const u64 R = h[W_RECORDS];
  kc->info.groups = h[W_GROUPS];
  kc->info.untrusted_groups = h[W_UNTRUSTED];
  kc->info.records = R;
  if (R == 0) return 0;
  // 4: the records
  const u32 rbits = bits_of(R - 1), pbits = bits_of(ix.n);
  const u64 rtiles = div_up(R, KC_TILE);
  if (kc->entry.grow(R * 4) != hipSuccess || kc->group_first.grow(R * 4) != hipSuccess || kc->order.grow(R * 4) != hipSuccess ||
      kc->order_b.grow(R * 4) != hipSuccess || kc->fpos.grow(R * 4) != hipSuccess || kc->target.grow(R * 8) != hipSuccess ||
      kc->source.grow(R * 8) != hipSuccess || kc->keys.grow(R * 8) != hipSuccess || kc->keys_b.grow(R * 8) != hipSuccess ||
      kc->state.grow(R * 8) != hipSuccess || kc->state_b.grow(R * 8) != hipSuccess || kc->flet.grow(R) != hipSuccess ||
      kc->sortws.grow(radix_workspace_words(R) * 4) != hipSuccess)
    return out_of_memory(FEATURE, R, "records");
  k_kc_emit<S><<<(u32) div_up(C, KC_TILE), KC_THREADS, 0, st>>>(x, kc->heads, C, k, kc->rcount, kc->src, kc->first, kc->roff,
                                                               rbits, kc->entry, kc->target, kc->source, kc->group_first,
                                                               kc->keys, kc->order);
  HIP_TRY(hipGetLastError());
  // 5: by (target, order).  The records are in order already: only the digits of the target are sorted on.
  int shifts[8], widths[8], passes = 0;
  for (u32 b = 0; b < pbits; b += 8, passes++) {
    shifts[passes] = (int) (rbits + b);
    widths[passes] = (int) (pbits - b < 8 ? pbits - b : 8);
  }
  TRY(radix_sort_pairs<u64, u32>(kc->keys, kc->order, kc->keys_b, kc->order_b, R, shifts, widths, passes, kc->sortws, st,
                                 nullptr, nullptr));
  kc->sorted = passes % 2 ? kc->keys_b : kc->keys;
  k_kc_first<<<(u32) rtiles, KC_THREADS, 0, st>>>(ix.enc, kc->sorted, R, rbits, kc->target, kc->source, kc->group_first,
                                                  kc->state, kc->words);
  HIP_TRY(hipGetLastError());
  TRY(fetch(st, { { kc->words, h, sizeof h } }));
  kc->info.dependent = h[W_DEPENDENT];
  u64 *before = kc->state, *after = kc->state_b;
  for (u64 open = h[W_DEPENDENT]; open != 0; kc->info.rounds++) {
    HIP_TRY(hipMemsetAsync(kc->words + W_OPEN, 0, sizeof(u64), st));
    k_kc_round<<<(u32) rtiles, KC_THREADS, 0, st>>>(before, R, after, kc->words + W_OPEN);
    HIP_TRY(hipGetLastError());
    TRY(fetch(st, { { kc->words + W_OPEN, &open, sizeof open } }));
    u64 *t = before; before = after; after = t;
    if (kc->info.rounds > 64) {                          // (a chain halves every round)
      gtamd_set_error("%s: the records' dependencies do not resolve: the tables are not those of the text", FEATURE);
      return -1;
    }
  }
  kc->letters = before;
  k_kc_finals<<<(u32) rtiles, KC_THREADS, 0, st>>>(ix.enc, ix.n, kc->sorted, R, rbits, kc->letters, kc->fpos, kc->flet, kc->words);
  HIP_TRY(hipGetLastError());
  TRY(fetch(st, { { kc->words, h, sizeof h } }));
  kc->info.changed = h[W_CHANGED];
  for (u32 a = 0; a < 4; a++) kc->info.delta[a] = (int64_t) h[W_DELTA + a];
  return 0;
}

int refuse_mirror(gtamd_kcorrect *kc, int mirrored) {
  kc->decided = false;
  kc->mirrored = mirrored != 0;
  if (!mirrored || kc->index.n == 0) return 0;
  u8 middle = 0;
  if (kc->index.n % 2) {
    HIP_TRY(hipSetDevice(kc->device));
    TRY(fetch(kc->st, { { kc->index.enc + (kc->index.n >> 1), &middle, 1 } }));
  }
  if (middle != 255) {
    gtamd_set_error("%s: %llu symbols are no mirrored set: an odd number with a separator in the middle is expected",
                    FEATURE, (unsigned long long) kc->index.n);
    kc->index.drop();
    return -1;
  }
  return 0;
}

int refuse_index(const char *fn, const gtamd_kcorrect *kc, const void *enc, u64 n, const void *suf, u32 suf_bytes,
                 const void *lcp) {
  if (kc == nullptr || suf == nullptr || lcp == nullptr || (enc == nullptr && n)) {
    gtamd_set_error("invalid argument to %s", fn);
    return -1;
  }
  TRY(refuse_suf_bytes(FEATURE, suf_bytes));
  return refuse_sizes(FEATURE, n, 0, "corrected");
}

}  // namespace

extern "C" gtamd_kcorrect *gtamd_kcorrect_create(int device) {
  GTAMD_ABI_BEGIN
  return create_consumer<gtamd_kcorrect>(device, W_WORDS, "the k-mer corrector");
  GTAMD_ABI_END(nullptr)
}

extern "C" void gtamd_kcorrect_destroy(gtamd_kcorrect *kc) { destroy_consumer(kc); }

extern "C" void gtamd_kcorrect_geometry(uint32_t *tile_entries) {
  if (tile_entries != nullptr) *tile_entries = KC_TILE;
}

extern "C" int gtamd_kcorrect_set_index(gtamd_kcorrect *kc, const uint8_t *enc, uint64_t n, const void *suf,
                                        uint32_t suf_bytes, const uint8_t *lcp, int mirrored) {
  GTAMD_ABI_BEGIN
  TRY(refuse_index("gtamd_kcorrect_set_index", kc, enc, n, suf, suf_bytes, lcp));
  IndexView v;
  v.enc = enc; v.n = n; v.suf = suf; v.suf_bytes = suf_bytes; v.lcp = lcp;
  kc->index.borrow(v);
  return refuse_mirror(kc, mirrored);
  GTAMD_ABI_END(-1)
}

extern "C" int gtamd_kcorrect_set_index_host(gtamd_kcorrect *kc, const uint8_t *enc, uint64_t n, const void *suf,
                                             uint32_t suf_bytes, const uint8_t *lcp, int mirrored) {
  GTAMD_ABI_BEGIN
  TRY(refuse_index("gtamd_kcorrect_set_index_host", kc, enc, n, suf, suf_bytes, lcp));
  IndexView v;
  v.enc = enc; v.n = n; v.suf = suf; v.suf_bytes = suf_bytes; v.lcp = lcp;
  kc->decided = false;
  HIP_TRY(hipSetDevice(kc->device));
  TRY(kc->index.upload_from_host(FEATURE, v));
  return refuse_mirror(kc, mirrored);
  GTAMD_ABI_END(-1)
}

extern "C" int gtamd_kcorrect_set_index_esa(gtamd_kcorrect *kc, const gtamd_esa_ctx *esa, const uint8_t *enc, uint64_t n,
                                            int mirrored) {
  GTAMD_ABI_BEGIN
  if (kc == nullptr || esa == nullptr || (enc == nullptr && n)) {
    gtamd_set_error("invalid argument to gtamd_kcorrect_set_index_esa");
    return -1;
  }
  TRY(refuse_sizes(FEATURE, n, 0, "corrected"));
  IndexView v;
  kc->decided = false;
  TRY(engine_tables(FEATURE, esa, enc, n, true, &v, "corrected"));
  kc->index.borrow(v);
  return refuse_mirror(kc, mirrored);
  GTAMD_ABI_END(-1)
}

extern "C" int gtamd_kcorrect_decide(gtamd_kcorrect *kc, uint32_t k, uint32_t c, gtamd_kcorrect_info *info) {
  GTAMD_ABI_BEGIN
  if (kc == nullptr) { gtamd_set_error("invalid argument to gtamd_kcorrect_decide"); return -1; }
  if (!kc->index.set) {
    gtamd_set_error("%s: no index is set (gtamd_kcorrect_set_index)", FEATURE);
    return -1;
  }
  if (k < 1 || k > GTAMD_KCORRECT_MAX_K) {
    gtamd_set_error("%s: k = %u: a k-mer length from 1 to %u is expected (the byte table .lcp alone is read, and a byte "
                    "of 255 says no more than that)", FEATURE, k, GTAMD_KCORRECT_MAX_K);
    return -1;
  }
  if (c < 1) {
    gtamd_set_error("%s: c = 0: a trusted count of 1 at least is expected", FEATURE);
    return -1;
  }
  kc->decided = false;
  kc->R = 0;
  kc->info = gtamd_kcorrect_info();
  kc->info.k = k;
  kc->info.c = c;
  kc->info.table_entries = kc->index.n + 1;
  HIP_TRY(hipSetDevice(kc->device));
  if (kc->index.n != 0) {
    HIP_TRY(hipMemsetAsync(kc->words, 0, W_WORDS * sizeof(u64), kc->st));
    HIP_TRY(hipEventRecord(kc->ev[0], kc->st));
    TRY(kc->index.suf_bytes == 4 ? decide<u32>(kc, k, c) : decide<u64>(kc, k, c));
    HIP_TRY(hipEventRecord(kc->ev[1], kc->st));
    HIP_TRY(hipEventSynchronize(kc->ev[1]));
    HIP_TRY(hipEventElapsedTime(&kc->info.device_ms, kc->ev[0], kc->ev[1]));
  }
  kc->R = kc->info.records;
  kc->info.device_bytes = held_bytes(kc);
  kc->decided = true;
  if (info != nullptr) *info = kc->info;
  return 0;
  GTAMD_ABI_END(-1)
}

extern "C" int gtamd_kcorrect_records(const gtamd_kcorrect *kc, uint64_t *out, int out_on_device) {
  GTAMD_ABI_BEGIN
  if (kc == nullptr || (out == nullptr && kc->R)) { gtamd_set_error("invalid argument to gtamd_kcorrect_records"); return -1; }
  if (!kc->decided) {
    gtamd_set_error("%s: nothing is decided (gtamd_kcorrect_decide)", FEATURE);
    return -1;
  }
  if (kc->R == 0) return 0;
  struct Triple { u64 entry, position, letter; };
  HIP_TRY(hipSetDevice(kc->device));
  gtamd_kcorrect *own = const_cast<gtamd_kcorrect *>(kc);      // (its staging buffer)
  RecordStage<Triple> stage(out, out_on_device);
  if (stage.begin(own->stage, kc->R) != hipSuccess) return out_of_memory(FEATURE, kc->R, "records");
  k_kc_triples<<<(u32) div_up(kc->R, KC_TILE), KC_THREADS, 0, kc->st>>>(kc->entry, kc->target, kc->letters, kc->R,
                                                                       (u64 *) stage.dst);
  HIP_TRY(hipGetLastError());
  return stage.finish(kc->R, kc->st);
  GTAMD_ABI_END(-1)
}

extern "C" int gtamd_kcorrect_apply(gtamd_kcorrect *kc, const uint8_t *enc, uint64_t n, uint8_t **out_device,
                                    uint64_t *out_n) {
  GTAMD_ABI_BEGIN
  if (kc == nullptr || out_device == nullptr || out_n == nullptr) {
    gtamd_set_error("invalid argument to gtamd_kcorrect_apply");
    return -1;
  }
  *out_device = nullptr;
  *out_n = 0;
  kc->result = 0;
  if (!kc->decided) {
    gtamd_set_error("%s: nothing is decided (gtamd_kcorrect_decide)", FEATURE);
    return -1;
  }
  const u64 m = unmirrored_symbols(kc);
  if (enc != nullptr && n != m) {
    gtamd_set_error("%s: %llu symbols given, the reads of the index are %llu", FEATURE, (unsigned long long) n,
                    (unsigned long long) m);
    return -1;
  }
  if (m == 0) return 0;
  HIP_TRY(hipSetDevice(kc->device));
  if (kc->out.grow(m) != hipSuccess) return out_of_memory(FEATURE, m, "corrected symbols");
  HIP_TRY(hipMemcpyAsync(kc->out, enc != nullptr ? enc : kc->index.enc, m, hipMemcpyDeviceToDevice, kc->st));
  if (kc->R != 0) {
    k_kc_apply<<<(u32) div_up(kc->R, KC_TILE), KC_THREADS, 0, kc->st>>>(kc->fpos, kc->flet, kc->R, m, kc->out);
    HIP_TRY(hipGetLastError());
  }
  HIP_TRY(hipStreamSynchronize(kc->st));
  kc->info.device_bytes = held_bytes(kc);
  *out_device = kc->out;
  *out_n = kc->result = m;
  return 0;
  GTAMD_ABI_END(-1)
}

extern "C" int gtamd_kcorrect_result(const gtamd_kcorrect *kc, uint8_t *out, int out_on_device) {
  GTAMD_ABI_BEGIN
  if (kc == nullptr || (out == nullptr && kc->result)) { gtamd_set_error("invalid argument to gtamd_kcorrect_result"); return -1; }
  if (kc->result == 0) return 0;
  HIP_TRY(hipSetDevice(kc->device));
  HIP_TRY(hipMemcpyAsync(out, kc->out, kc->result, out_on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, kc->st));
  HIP_TRY(hipStreamSynchronize(kc->st));
  return 0;
  GTAMD_ABI_END(-1)
}

extern "C" int gtamd_kcorrect_get_info(const gtamd_kcorrect *kc, gtamd_kcorrect_info *info) {
  GTAMD_ABI_BEGIN
  return consumer_info(kc, info, "gtamd_kcorrect_get_info");
  GTAMD_ABI_END(-1)
}
