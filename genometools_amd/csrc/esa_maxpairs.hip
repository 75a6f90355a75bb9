// esa_maxpairs.hip -- maximal exact repeats from .suf and .lcp in device memory:
// `gt repfind -l L -ii INDEX` (C ABI, the semantics and the algorithm:
// include/gtamd_maxpairs.h).
//
//   1  k_mp_select<InRun>      flag the table entries that lie in a run, count
//                              them per tile, scan (esa_prims), compact: table
//                              index, LCP value, left class of the M suffixes
//   2  k_mp_select<SegStart>   the same two passes over the M entries: where a
//                              segment starts, the segment of every entry
//      k_mp_segments           one lane per segment: esa_maxpairs_walk.h
//   3  k_mp_count              one lane per entry: the walk that counts
//      offsets_u64 (esa_prims)     64-bit exclusive scan of the counts
//   4  k_mp_emit               one lane per entry: the walk that writes
//
// Every working array has M entries (or one per tile), none has N.
#include "esa_common.h"
#include "esa_index.h"
#include "esa_prims.h"
#include "esa_devutil.h"
#include "esa_maxpairs_walk.h"
#include "../../include/gtamd_maxpairs.h"

namespace {

constexpr int MP_THREADS = SC_THREADS;          // (the block scans of esa_devutil.h)
constexpr u32 MP_PER = 4;                         // consecutive items of one lane in a select pass
constexpr u32 MP_TILE = MP_THREADS * MP_PER;      // items of one workgroup there
constexpr u32 MP_WALK_TILE = MP_THREADS;          // entries of one workgroup in a walk: one a lane

enum { W_RUNS = 0, W_PAIRS, W_MAXCNT, W_MAXLEN, W_STEPS, W_WORDS };

// ---- steps 1 and 2: select ---------------------------------------------------
// table index i lies in a run: lcp[i] >= L or lcp[i + 1] >= L
template <typename S> struct InRun {
  const u8 *enc; u64 n; const S *suf; const u8 *lcp; const u64 *llv; u64 m; u32 L;
  u32 *idx, *val; u8 *cls;

  // the LCP value of table index i in [1, n]
  __device__ u32 value(u64 i) const {
    const u32 b = lcp[i];
    if (b != 255) return b;
    const u64 j = llv_lower_bound(llv, m, i);
    return j < m && llv[2 * j] == i ? (u32) llv[2 * j + 1] : 255u;
  }
  __device__ bool flag(u64 i) const {
    if (i == 0 || i > n) return false;
    if (L <= 255) return lcp[i] >= L;
    return lcp[i] == 255 && value(i) >= L;
  }
  // sel[e]: item first + e is selected; returns the number of runs that start here
  __device__ u32 load(u64 first, u64 N, bool *sel) const {
    u32 starts = 0;
    bool f = flag(first);
#pragma unroll
    for (u32 e = 0; e < MP_PER; e++) {
      const bool g = flag(first + e + 1);
      sel[e] = first + e < N && (f || g);
      starts += sel[e] && !f;
      f = g;
    }
    return starts;
  }
  __device__ void write(u64 i, u32 k) const {
    idx[k] = (u32) i;
    val[k] = flag(i) ? value(i) : 0;            // (0: the first of its run)
    const u64 p = suf[i];
    const u32 c = p == 0 || p > n ? MP_UNIQUE : enc[p - 1];
    cls[k] = (u8) (c >= 254 ? MP_UNIQUE : c);
  }
  __device__ void every(u64, u32) const {}
};

// entry k starts a segment: first of a run, unique, or another class than k - 1
struct SegStart {
  const u32 *val; const u8 *cls; u32 *seg_first, *seg_of;

  __device__ u32 load(u64 first, u64 M, bool *sel) const {
#pragma unroll
    for (u32 e = 0; e < MP_PER; e++) {
      const u64 k = first + e;
      sel[e] = k < M && (k == 0 || val[k] == 0 || cls[k] == MP_UNIQUE || cls[k] != cls[k - 1]);
    }
    return 0;
  }
  __device__ void write(u64 k, u32 s) const { seg_first[s] = (u32) k; }
  __device__ void every(u64 k, u32 upto) const { seg_of[k] = upto - 1; }   // (entry 0 is selected: upto >= 1)
};

// WRITE false: tiles[t] = the number of selected items of tile t, *tally += what
// the loads return.  WRITE true: tiles[t] is where the selected items of tile t
// go; p.write(item, place) for them and p.every(item, selected up to and
// including it) for all.
template <typename P, bool WRITE>
__global__ __launch_bounds__(MP_THREADS) void k_mp_select(P p, u64 count, u32 *tiles, u64 *tally) {
  __shared__ u32 lds4[MP_THREADS / 64];
  __shared__ u32 stally;
  if (!WRITE && threadIdx.x == 0) stally = 0;
  const u64 first = (u64) blockIdx.x * MP_TILE + (u64) threadIdx.x * MP_PER;
  bool sel[MP_PER];
  const u32 extra = p.load(first, count, sel);
  u32 c = 0, total;
#pragma unroll
  for (u32 e = 0; e < MP_PER; e++) c += sel[e];
  const u32 before = block_scan_excl_sum(c, &total, lds4);     // (syncs)
  if (!WRITE) {
    if (extra) atomicAdd(&stally, extra);
    __syncthreads();
    if (threadIdx.x == 0) {
      tiles[blockIdx.x] = total;
      if (stally) atomicAdd((unsigned long long *) tally, (unsigned long long) stally);
    }
    return;
  }
  u32 k = tiles[blockIdx.x] + before;
#pragma unroll
  for (u32 e = 0; e < MP_PER; e++) {
    const u64 i = first + e;
    if (i >= count) break;
    if (sel[e]) p.write(i, k++);
    p.every(i, k);
  }
}

__global__ __launch_bounds__(MP_THREADS) void k_mp_segments(const u32 *val, const u8 *cls, const u32 *seg_first,
                                                            u32 nseg, u32 *tmin, u32 *seg_min, u16 *seg_info) {
  const u64 s = (u64) blockIdx.x * MP_THREADS + threadIdx.x;
  if (s < nseg) mp_segment_fill(val, cls, seg_first, (u32) s, tmin, seg_min, seg_info);
}

// ---- step 3 --------------------------------------------------------------------
__global__ __launch_bounds__(MP_THREADS) void k_mp_count(MpSegments g, const u8 *cls, u32 M, u32 *cnt, u64 *tsum,
                                                         u64 *w) {
  __shared__ unsigned long long ssum, ssteps;
  __shared__ u32 smaxc, smaxl;
  if (threadIdx.x == 0) { ssum = 0; ssteps = 0; smaxc = 0; smaxl = 0; }
  __syncthreads();
  const u64 k = (u64) blockIdx.x * MP_WALK_TILE + threadIdx.x;
  if (k < M) {
    u32 longest, steps;
    const u32 c = mp_walk_count(g, (u32) k, cls[k], &longest, &steps);
    cnt[k] = c;
    if (c) { atomicAdd(&ssum, (unsigned long long) c); atomicMax(&smaxc, c); atomicMax(&smaxl, longest); }
    if (steps) atomicAdd(&ssteps, (unsigned long long) steps);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    tsum[blockIdx.x] = ssum;
    if (smaxc) {
      atomicMax((unsigned long long *) &w[W_MAXCNT], (unsigned long long) smaxc);
      atomicMax((unsigned long long *) &w[W_MAXLEN], (unsigned long long) smaxl);
    }
    if (ssteps) atomicAdd((unsigned long long *) &w[W_STEPS], ssteps);
  }
}

// ---- step 4 --------------------------------------------------------------------
// entries [k0, k1): their records to out, the record at off[k0] first
template <typename S>
__global__ __launch_bounds__(MP_THREADS) void k_mp_emit(MpSegments g, const u8 *cls, const u32 *idx, const S *suf,
                                                        const u64 *off, u32 k0, u32 k1, u64 base, MpRecord *out) {
  const u64 k = (u64) k0 + (u64) blockIdx.x * MP_WALK_TILE + threadIdx.x;
  if (k < k1) mp_walk_emit<S>(g, (u32) k, cls[k], idx[k], suf, out + (off[k] - base));
}

}  // namespace

struct gtamd_maxpairs : ConsumerBase<> {
  ResidentIndex index;
  bool prepared = false;
  // what a prepare leaves for the emit calls
  Dev<u32> tiles, scanws, idx, val, tmin, seg_of, cnt, seg_first, seg_min;
  Dev<u16> seg_info;
  Dev<u8> cls;
  Dev<u64> tsum, off;
  Dev<u8> out;                         // records on their way to host memory
  u32 M = 0, nseg = 0;
  gtamd_maxpairs_info info = gtamd_maxpairs_info();
};

namespace {

const char FEATURE[] = "maximal pairs";

// every way of setting an index: what is refused, before anything is touched
int set_index(gtamd_maxpairs *mp, const IndexView &v, bool from_host) {
  if (mp == nullptr || v.suf == nullptr || v.lcp == nullptr || (v.enc == nullptr && v.n) ||
      (v.llv == nullptr && v.llv_pairs)) {
    gtamd_set_error("invalid argument to gtamd_maxpairs_set_index");
    return -1;
  }
  TRY(refuse_suf_bytes(FEATURE, v.suf_bytes));
  TRY(refuse_sizes(FEATURE, v.n, v.llv_pairs));
  HIP_TRY(hipSetDevice(mp->device));
  mp->prepared = false;
  if (from_host) return mp->index.upload_from_host(FEATURE, v);
  mp->index.borrow(v);
  return 0;
}

u64 held_bytes(const gtamd_maxpairs *mp) {
  return mp->index.bytes() + mp->tiles.bytes + mp->scanws.bytes + mp->idx.bytes + mp->val.bytes + mp->tmin.bytes +
         mp->seg_of.bytes + mp->cnt.bytes + mp->seg_first.bytes + mp->seg_min.bytes + mp->seg_info.bytes +
         mp->cls.bytes + mp->tsum.bytes + mp->off.bytes + mp->words.bytes + mp->out.bytes;
}

MpSegments view(const gtamd_maxpairs *mp) {
  return MpSegments{ mp->val, mp->tmin, mp->seg_of, mp->seg_first, mp->seg_min, mp->seg_info, mp->nseg };
}

// both passes of a selection over `count` items: *selected = their number
template <typename P>
int select(gtamd_maxpairs *mp, const P &p, u64 count, u64 *tally, u32 *selected, bool write) {
  hipStream_t st = mp->st;
  const u64 T = div_up(count, MP_TILE);
  if (!write) {
    HIP_TRY(hipMemsetAsync(mp->tiles, 0, (T + 1) * sizeof(u32), st));
    k_mp_select<P, false><<<(u32) T, MP_THREADS, 0, st>>>(p, count, mp->tiles, tally);
    HIP_TRY(hipGetLastError());
    TRY(scan_u32(SCAN_SUM, mp->tiles, mp->tiles, T + 1, false, mp->scanws, st));
    TRY(fetch(st, { { mp->tiles + T, selected, sizeof(u32) } }));
  } else {
    k_mp_select<P, true><<<(u32) T, MP_THREADS, 0, st>>>(p, count, mp->tiles, tally);
    HIP_TRY(hipGetLastError());
  }
  return 0;
}

template <typename S> int prepare(gtamd_maxpairs *mp, u32 L) {
  hipStream_t st = mp->st;
  const ResidentIndex &x = mp->index;
  const u64 N = x.n + 1, T = div_up(N, MP_TILE);
  if (mp->tiles.grow((T + 1) * sizeof(u32)) != hipSuccess ||
      mp->scanws.grow(scan_workspace_words(T + 1) * sizeof(u32)) != hipSuccess)
    return out_of_memory(FEATURE, T + 1, "tiles");
  HIP_TRY(hipMemsetAsync(mp->words, 0, W_WORDS * sizeof(u64), st));
  HIP_TRY(hipEventRecord(mp->ev[0], st));

  // 1: the suffixes in runs
  InRun<S> in = { x.enc, x.n, (const S *) x.suf, x.lcp, x.llv, x.llv_pairs, L,
                  nullptr, nullptr, nullptr };
  u32 M = 0, nseg = 0;
  TRY(select(mp, in, N, mp->words + W_RUNS, &M, false));
  mp->M = M;
  if (M != 0) {
    if (mp->idx.grow((u64) M * 4) != hipSuccess || mp->val.grow((u64) M * 4) != hipSuccess ||
        mp->tmin.grow((u64) M * 4) != hipSuccess || mp->seg_of.grow((u64) M * 4) != hipSuccess ||
        mp->cnt.grow((u64) M * 4) != hipSuccess || mp->cls.grow(M) != hipSuccess ||
        mp->off.grow(((u64) M + 1) * 8) != hipSuccess ||
        mp->tsum.grow(div_up(M, MP_WALK_TILE) * 8) != hipSuccess)
      return out_of_memory(FEATURE, M, "suffixes in runs");
    in.idx = mp->idx; in.val = mp->val; in.cls = mp->cls;
    TRY(select(mp, in, N, nullptr, nullptr, true));

    // 2: the segments
    SegStart seg = { mp->val, mp->cls, nullptr, mp->seg_of };
    TRY(select(mp, seg, M, nullptr, &nseg, false));
    if (mp->seg_first.grow(((u64) nseg + 1) * 4) != hipSuccess || mp->seg_min.grow((u64) nseg * 4) != hipSuccess ||
        mp->seg_info.grow((u64) nseg * 2) != hipSuccess)
      return out_of_memory(FEATURE, nseg, "segments");
    seg.seg_first = mp->seg_first;
    TRY(select(mp, seg, M, nullptr, nullptr, true));
    HIP_TRY(hipMemcpyAsync(mp->seg_first + nseg, &mp->M, sizeof(u32), hipMemcpyHostToDevice, st));
    mp->nseg = nseg;
    k_mp_segments<<<(u32) div_up(nseg, MP_THREADS), MP_THREADS, 0, st>>>(mp->val, mp->cls, mp->seg_first, nseg,
                                                                        mp->tmin, mp->seg_min, mp->seg_info);
    HIP_TRY(hipGetLastError());

    // 3: the counts and their places
    const u32 tiles = (u32) div_up(M, MP_WALK_TILE);
    k_mp_count<<<tiles, MP_THREADS, 0, st>>>(view(mp), mp->cls, M, mp->cnt, mp->tsum, mp->words);
    HIP_TRY(hipGetLastError());
    TRY(offsets_u64(mp->cnt, M, mp->tsum, mp->off, mp->words + W_PAIRS, st));
  }
  HIP_TRY(hipEventRecord(mp->ev[1], st));
  u64 h[W_WORDS];
  TRY(fetch(st, { { mp->words, h, sizeof h } }));
  HIP_TRY(hipEventElapsedTime(&mp->info.device_ms, mp->ev[0], mp->ev[1]));
  mp->info.pairs = h[W_PAIRS];
  mp->info.run_suffixes = M;
  mp->info.runs = h[W_RUNS];
  mp->info.segments = nseg;
  mp->info.max_pairs_of_one_suffix = h[W_MAXCNT];
  mp->info.max_len = h[W_MAXLEN];
  mp->info.walk_steps = h[W_STEPS];
  return 0;
}

// off[k] of the prepared object, k <= M
int offset_at(gtamd_maxpairs *mp, u64 k, u64 *v) { return fetch(mp->st, { { mp->off + k, v, sizeof(u64) } }); }

int emit(gtamd_maxpairs *mp, u64 *cursor, gtamd_maxpairs_record *out, u64 capacity, int out_on_device,
         u64 *written) {
  *written = 0;
  const u64 M = mp->M, z = mp->info.pairs, k0 = *cursor;
  TRY(refuse_window(FEATURE, "suffixes in runs", k0, M, capacity, 0));      // (its least capacity: below, once known)
  if (k0 == M || z == 0) { *cursor = M; return 0; }
  u64 base;
  TRY(offset_at(mp, k0, &base));
  if (base == z) { *cursor = M; return 0; }
  if (capacity < mp->info.max_pairs_of_one_suffix) {
    gtamd_set_error("maximal pairs: a capacity of %llu records is too small, one suffix alone has %llu: "
                    "a capacity of at least %llu is needed", (unsigned long long) capacity,
                    (unsigned long long) mp->info.max_pairs_of_one_suffix,
                    (unsigned long long) mp->info.max_pairs_of_one_suffix);
    return -1;
  }
  // the largest k1 with off[k1] - base <= capacity
  u64 k1 = M, count = z - base;
  if (count > capacity) {
    u64 lo = k0, hi = M;                 // off[lo] fits, off[hi] does not
    while (hi - lo > 1) {
      const u64 mid = lo + (hi - lo) / 2;
      u64 v;
      TRY(offset_at(mp, mid, &v));
      if (v - base <= capacity) lo = mid; else hi = mid;
    }
    k1 = lo;
    TRY(offset_at(mp, k1, &count));
    count -= base;
  }
  // (capacity >= the pairs of any one suffix: k1 > k0)
  if (count) {
    RecordStage<MpRecord> stage(out, out_on_device);
    if (stage.begin(mp->out, count) != hipSuccess) return out_of_memory(FEATURE, count, "records");
    const u32 blocks = (u32) div_up(k1 - k0, MP_WALK_TILE);
    if (mp->index.suf_bytes == 4)
      k_mp_emit<u32><<<blocks, MP_THREADS, 0, mp->st>>>(view(mp), mp->cls, mp->idx, (const u32 *) mp->index.suf,
                                                       mp->off, (u32) k0, (u32) k1, base, stage.dst);
    else
      k_mp_emit<u64><<<blocks, MP_THREADS, 0, mp->st>>>(view(mp), mp->cls, mp->idx, (const u64 *) mp->index.suf,
                                                       mp->off, (u32) k0, (u32) k1, base, stage.dst);
    HIP_TRY(hipGetLastError());
    TRY(stage.finish(count, mp->st));
  }
  *cursor = k1;
  *written = count;
  return 0;
}

}  // namespace

extern "C" gtamd_maxpairs *gtamd_maxpairs_create(int device) {
  GTAMD_ABI_BEGIN
  return create_consumer<gtamd_maxpairs>(device, W_WORDS, "the maximal pairs enumerator");
  GTAMD_ABI_END(nullptr)
}

extern "C" void gtamd_maxpairs_destroy(gtamd_maxpairs *mp) { destroy_consumer(mp); }

extern "C" int gtamd_maxpairs_set_index(gtamd_maxpairs *mp, const uint8_t *enc, uint64_t n, const void *suf,
                                        uint32_t suf_bytes, const uint8_t *lcp, const uint64_t *llv,
                                        uint64_t llv_pairs) {
  GTAMD_ABI_BEGIN
  return set_index(mp, IndexView{ enc, n, suf, suf_bytes, lcp, llv, llv_pairs }, false);
  GTAMD_ABI_END(-1)
}

extern "C" int gtamd_maxpairs_set_index_host(gtamd_maxpairs *mp, const uint8_t *enc, uint64_t n, const void *suf,
                                             uint32_t suf_bytes, const uint8_t *lcp, const uint64_t *llv,
                                             uint64_t llv_pairs) {
  GTAMD_ABI_BEGIN
  return set_index(mp, IndexView{ enc, n, suf, suf_bytes, lcp, llv, llv_pairs }, true);
  GTAMD_ABI_END(-1)
}

extern "C" int gtamd_maxpairs_set_index_esa(gtamd_maxpairs *mp, const gtamd_esa_ctx *esa, const uint8_t *enc,
                                            uint64_t n) {
  GTAMD_ABI_BEGIN
  if (mp == nullptr || esa == nullptr) { gtamd_set_error("invalid argument to gtamd_maxpairs_set_index_esa"); return -1; }
  IndexView v;
  TRY(engine_tables(FEATURE, esa, enc, n, true, &v));
  return set_index(mp, v, false);
  GTAMD_ABI_END(-1)
}

extern "C" int gtamd_maxpairs_prepare(gtamd_maxpairs *mp, uint32_t min_len, gtamd_maxpairs_info *info) {
  GTAMD_ABI_BEGIN
  if (mp == nullptr) { gtamd_set_error("invalid argument to gtamd_maxpairs_prepare"); return -1; }
  if (!mp->index.set) {
    gtamd_set_error("maximal pairs: no index is set (gtamd_maxpairs_set_index)");
    return -1;
  }
  if (min_len == 0) {
    gtamd_set_error("maximal pairs: a minimum length of 0 is refused, 1 or more expected");
    return -1;
  }
  HIP_TRY(hipSetDevice(mp->device));
  mp->prepared = false;
  mp->info = gtamd_maxpairs_info();
  mp->M = mp->nseg = 0;
  TRY(mp->index.suf_bytes == 4 ? prepare<u32>(mp, min_len) : prepare<u64>(mp, min_len));
  mp->info.device_bytes = held_bytes(mp);
  mp->prepared = true;
  if (info != nullptr) *info = mp->info;
  return 0;
  GTAMD_ABI_END(-1)
}

extern "C" int gtamd_maxpairs_emit(gtamd_maxpairs *mp, uint64_t *cursor, gtamd_maxpairs_record *out,
                                   uint64_t capacity, int out_on_device, uint64_t *written) {
  GTAMD_ABI_BEGIN
  if (mp == nullptr || cursor == nullptr || written == nullptr || (out == nullptr && capacity)) {
    gtamd_set_error("invalid argument to gtamd_maxpairs_emit");
    return -1;
  }
  if (!mp->prepared) {
    gtamd_set_error("maximal pairs: nothing is prepared (gtamd_maxpairs_prepare)");
    return -1;
  }
  HIP_TRY(hipSetDevice(mp->device));
  TRY(emit(mp, cursor, out, capacity, out_on_device, written));
  mp->info.device_bytes = held_bytes(mp);
  return 0;
  GTAMD_ABI_END(-1)
}

extern "C" int gtamd_maxpairs_get_info(const gtamd_maxpairs *mp, gtamd_maxpairs_info *info) {
  GTAMD_ABI_BEGIN
  return consumer_info(mp, info, "gtamd_maxpairs_get_info");
  GTAMD_ABI_END(-1)
}
