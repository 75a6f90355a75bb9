// esa_check.hip -- the index checker of `gt dev sfxmap -suf -lcp -bwt` on the
// device (C ABI and the criteria, with their citations: include/gtamd_check.h).
//
// Five phases over tables in device memory, each a few kernels of one lane per
// table entry (workgroups of 256 lanes take CHK_TILE entries); a phase runs
// only when the ones before it accepted the tables, because from phase 2 on
// the suffix table and its inverse are used as indices:
//   1  range of every .suf entry while the inverse is scattered, then the
//      permutation test through the inverse
//   2  order of every pair of neighbours
//   3  every .bwt byte
//   4  lcp[0], every .llv pair, the number of bytes 255
//   5  every .lcp / .llv value (Kasai's inheritance argument); a position with
//      more than CHK_LONG_CLAIM symbols to compare goes to a work list that
//      whole workgroups compare 4 KiB per step, leaving at the first difference
// A kernel reports the smallest index that fails: the minimum of a workgroup
// in LDS, one atomicMin per workgroup on a 64-bit slot.  What a report says
// beyond that index the host reads from the tables afterwards.
#include "esa_common.h"
#include "esa_index.h"
#include "esa_devutil.h"
#include "../../include/gtamd_check.h"

namespace {

constexpr int CHK_THREADS = 256;
constexpr u32 CHK_TILE = 2048;           // table entries per workgroup
constexpr u32 CHK_LONG_CLAIM = 512;      // longer ranges of (b) go to the work list
constexpr u32 CHK_LONG_BLOCKS = 2048;    // workgroups that share the work list
constexpr u32 RANK_UNSET = 0xffffffffu;
constexpr u64 NONE = ~0ull;

// the words the kernels report through
enum { W_FAIL = 0, W_LONGEST, W_COUNT255, W_DEPTH, W_LISTED, W_TRUE_LCP, W_WORDS };

// smallest key of the workgroup -> *slot; NONE: this lane has nothing to report
__device__ __forceinline__ void block_min_to(u64 key, u64 *slot) {
  __shared__ unsigned long long smin;
  if (threadIdx.x == 0) smin = NONE;
  __syncthreads();
  if (key != NONE) atomicMin(&smin, (unsigned long long) key);
  __syncthreads();
  if (threadIdx.x == 0 && smin != NONE) atomicMin((unsigned long long *) slot, smin);
}

__device__ __forceinline__ u32 sym_at(const u8 *enc, u64 n, u64 p) {
  return p < n ? enc[p] : 255u;
}

// ---- phase 1 --------------------------------------------------------------
template <typename S>
__global__ __launch_bounds__(CHK_THREADS) void k_chk_range(const S *suf, u64 N, u32 *rank, u64 *w) {
  const u64 base = (u64) blockIdx.x * CHK_TILE;
  u64 bad = NONE;
  for (u32 t = threadIdx.x; t < CHK_TILE; t += CHK_THREADS) {
    const u64 i = base + t;
    if (i >= N) break;
    const u64 v = suf[i];
    if (v >= N) { if (bad == NONE) bad = i; continue; }
    rank[v] = (u32) i;
    if (v == 0) atomicMin((unsigned long long *) &w[W_LONGEST], (unsigned long long) i);
  }
  block_min_to(bad, &w[W_FAIL]);
}

template <typename S>
__global__ __launch_bounds__(CHK_THREADS) void k_chk_perm(const S *suf, u64 N, const u32 *rank, u64 *w) {
  const u64 base = (u64) blockIdx.x * CHK_TILE;
  u64 bad = NONE;
  for (u32 t = threadIdx.x; t < CHK_TILE; t += CHK_THREADS) {
    const u64 p = base + t;
    if (p >= N) break;
    const u32 r = rank[p];                  // a row that was written: < N
    if ((r == RANK_UNSET || (u64) suf[r] != p) && bad == NONE) bad = p;
  }
  block_min_to(bad, &w[W_FAIL]);
}

// ---- phase 2 --------------------------------------------------------------
template <typename S>
__global__ __launch_bounds__(CHK_THREADS) void k_chk_order(const u8 *enc, u64 n, const S *suf,
                                                           const u32 *rank, u64 *w) {
  const u64 N = n + 1, base = (u64) blockIdx.x * CHK_TILE;
  u64 bad = NONE;
  for (u32 t = threadIdx.x; t < CHK_TILE; t += CHK_THREADS) {
    const u64 i = base + t;
    if (i >= N) break;
    if (i == 0) continue;
    const u64 a = suf[i - 1], b = suf[i];
    const u32 sa = sym_at(enc, n, a), sb = sym_at(enc, n, b);
    const u64 ca = sa >= 254 ? 256 + a : sa, cb = sb >= 254 ? 256 + b : sb;
    // (equal letters: neither is the end, a + 1 and b + 1 are positions)
    const bool ok = ca < cb || (ca == cb && sa < 254 && rank[a + 1] < rank[b + 1]);
    if (!ok && bad == NONE) bad = i;
  }
  block_min_to(bad, &w[W_FAIL]);
}

// ---- phase 3 --------------------------------------------------------------
template <typename S>
__global__ __launch_bounds__(CHK_THREADS) void k_chk_bwt(const u8 *enc, const S *suf, const u8 *bwt,
                                                         u64 N, u64 *w) {
  const u64 base = (u64) blockIdx.x * CHK_TILE;
  u64 bad = NONE;
  for (u32 t = threadIdx.x; t < CHK_TILE; t += CHK_THREADS) {
    const u64 i = base + t;
    if (i >= N) break;
    const u64 p = suf[i];
    const u32 want = p ? enc[p - 1] : 254u;
    if (bwt[i] != want && bad == NONE) bad = i;
  }
  block_min_to(bad, &w[W_FAIL]);
}

// ---- phase 4 --------------------------------------------------------------
__global__ __launch_bounds__(CHK_THREADS) void k_chk_llv_pairs(const u8 *lcp, const u64 *llv, u64 m,
                                                               u64 n, u64 *w) {
  const u64 base = (u64) blockIdx.x * CHK_TILE;
  u64 bad = NONE;
  for (u32 t = threadIdx.x; t < CHK_TILE; t += CHK_THREADS) {
    const u64 j = base + t;
    if (j >= m) break;
    const u64 idx = llv[2 * j], val = llv[2 * j + 1];
    bool ok = idx >= 1 && idx <= n && val >= 255 && val <= n;
    if (ok && j > 0) ok = llv[2 * j - 2] < idx;
    if (ok) ok = lcp[idx] == 255;
    if (!ok && bad == NONE) bad = j;
  }
  block_min_to(bad, &w[W_FAIL]);
}

__global__ __launch_bounds__(CHK_THREADS) void k_chk_count255(const u8 *lcp, u64 N, u64 *w) {
  __shared__ u32 scount;
  if (threadIdx.x == 0) scount = 0;
  __syncthreads();
  const u64 base = (u64) blockIdx.x * CHK_TILE;
  u32 cnt = 0;
  for (u32 t = threadIdx.x; t < CHK_TILE; t += CHK_THREADS) {
    const u64 i = base + t;
    if (i >= N) break;
    cnt += lcp[i] == 255;
  }
  if (cnt) atomicAdd(&scount, cnt);
  __syncthreads();
  if (threadIdx.x == 0 && scount) atomicAdd((unsigned long long *) &w[W_COUNT255], (unsigned long long) scount);
}

// the first byte 255 without a pair (the pairs have passed: they ascend)
__global__ __launch_bounds__(CHK_THREADS) void k_chk_unlisted(const u8 *lcp, u64 N, const u64 *llv,
                                                              u64 m, u64 *w) {
  const u64 base = (u64) blockIdx.x * CHK_TILE;
  u64 bad = NONE;
  for (u32 t = threadIdx.x; t < CHK_TILE; t += CHK_THREADS) {
    const u64 i = base + t;
    if (i >= N) break;
    if (lcp[i] != 255) continue;
    const u64 j = llv_lower_bound(llv, m, i);
    if ((j >= m || llv[2 * j] != i) && bad == NONE) bad = i;
  }
  block_min_to(bad, &w[W_FAIL]);
}

// ---- phase 5 --------------------------------------------------------------
__device__ __forceinline__ u32 claim_of(const u8 *lcp, const u64 *llv, u64 m, u32 r) {
  const u32 b = lcp[r];
  if (b != 255) return b;
  const u64 j = llv_lower_bound(llv, m, r);
  // (phase 4 has passed: the pair is there and its value is at most n < 2^32)
  return j < m && llv[2 * j] == r ? (u32) llv[2 * j + 1] : 255u;
}

// 0x80 in every byte of x that is zero
__device__ __forceinline__ u32 zero_bytes(u32 x) {
  return ~(((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x | 0x7f7f7f7fu);
}

// the first of cnt <= 16 offsets at which the symbols at xa + k and xb + k are
// not equal letters, or cnt.  Whole words where all 20 bytes around each side
// lie inside the sequence, single bytes at its borders and for a short count.
__device__ __forceinline__ u32 first_bad16(const u8 *enc, u64 n, u64 xa, u64 xb, u32 cnt) {
  if (cnt >= 8 && xa >= 3 && xb >= 3 && xa + 20 <= n && xb + 20 <= n) {
    const uintptr_t pa = (uintptr_t) enc + xa, pb = (uintptr_t) enc + xb;
    const u32 ma = pa & 3, mb = pb & 3;
    const u32 *wa = (const u32 *) (pa - ma), *wb = (const u32 *) (pb - mb);
    u32 a[5], b[5];
#pragma unroll
    for (int k = 0; k < 5; k++) { a[k] = wa[k]; b[k] = wb[k]; }
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const u32 x = __builtin_amdgcn_alignbyte(a[k + 1], a[k], ma);
      const u32 y = __builtin_amdgcn_alignbyte(b[k + 1], b[k], mb);
      // a byte differs, or is a special (>= 254: all of its upper seven bits set)
      const u32 d = x ^ y, sp = zero_bytes((x & 0xfefefefeu) ^ 0xfefefefeu);
      if (d | sp) {
        const u32 at = 4 * k + (min(__ffs((int) d) - 1u, __ffs((int) sp) - 1u) >> 3);
        return at < cnt ? at : cnt;
      }
    }
    return cnt;
  }
  for (u32 k = 0; k < cnt; k++) {
    const u32 va = sym_at(enc, n, xa + k), vb = sym_at(enc, n, xb + k);
    if (va != vb || va >= 254) return k;
  }
  return cnt;
}

// the same over [from, to) by the whole workgroup, 16 symbols a lane and step;
// the same value in every lane: the first such offset, or `to`
__device__ __forceinline__ u64 block_first_bad(const u8 *enc, u64 n, u64 p, u64 q, u64 from, u64 to) {
  __shared__ unsigned long long sbad;
  for (u64 base = from; base < to; base += 16 * CHK_THREADS) {
    if (threadIdx.x == 0) sbad = NONE;
    __syncthreads();
    const u64 o = base + 16 * threadIdx.x;
    if (o < to) {
      const u32 cnt = (u32) (to - o < 16 ? to - o : 16);
      const u32 k = first_bad16(enc, n, p + o, q + o, cnt);
      if (k < cnt) atomicMin(&sbad, (unsigned long long) (o + k));
    }
    __syncthreads();
    const u64 v = sbad;
    __syncthreads();
    if (v != NONE) return v;
  }
  return to;
}

// what position p has to compare: row r = rank[p] >= 1, the suffix q in front
// of it in the table, the claim C of the row and the start s of range (b)
template <typename S> struct LcpTask { u32 r, C, s; u64 q; };

template <typename S>
__global__ __launch_bounds__(CHK_THREADS) void k_chk_lcp(const u8 *enc, u64 n, const S *suf, const u32 *rank,
                                                         const u8 *lcp, const u64 *llv, u64 m,
                                                         u32 *list, u64 list_cap, u64 *w) {
  __shared__ u32 sdepth;
  if (threadIdx.x == 0) sdepth = 0;
  __syncthreads();
  const u64 N = n + 1, base = (u64) blockIdx.x * CHK_TILE;
  u64 bad = NONE;
  u32 depth = 0;
  // (every lane of a wave takes every step: the claim of p - 1 comes from the lane below)
  for (u32 t = threadIdx.x; t < CHK_TILE; t += CHK_THREADS) {
    const u64 p = base + t;
    const bool live = p < N;
    const u32 r = live ? rank[p] : 0;
    const bool has = r >= 1;
    const u32 C = has ? claim_of(lcp, llv, m, r) : 0;
    u32 prevC = __shfl_up(C, 1);
    if ((threadIdx.x & 63) == 0) {
      prevC = 0;
      if (live && p > 0) {
        const u32 rp = rank[p - 1];
        if (rp >= 1) prevC = claim_of(lcp, llv, m, rp);
      }
    }
    if (!has) continue;
    depth = max(depth, C);
    const u32 s = prevC ? prevC - 1 : 0;
    const u64 q = suf[r - 1];
    // (a) p + C <= 2n: no wrap in 64 bits
    const u32 va = sym_at(enc, n, p + C), vb = sym_at(enc, n, q + C);
    bool fails = va == vb && va < 254;
    // (b)
    if (!fails && C > s) {
      bool listed = false;
      if (C - s > CHK_LONG_CLAIM) {
        const u64 at = atomicAdd((unsigned long long *) &w[W_LISTED], 1ull);
        listed = at < list_cap;          // (a damaged table can claim more than 2N symbols)
        if (listed) list[at] = (u32) p;
      }
      if (!listed)
        for (u64 o = s; o < C && !fails; o += 16) {
          const u32 cnt = (u32) (C - o < 16 ? C - o : 16);
          fails = first_bad16(enc, n, p + o, q + o, cnt) < cnt;
        }
    }
    if (fails && (bad == NONE || r < bad)) bad = r;
  }
  block_min_to(bad, &w[W_FAIL]);
  if (depth) atomicMax(&sdepth, depth);
  __syncthreads();
  if (threadIdx.x == 0 && sdepth) atomicMax((unsigned long long *) &w[W_DEPTH], (unsigned long long) sdepth);
}

template <typename S>
__global__ __launch_bounds__(CHK_THREADS) void k_chk_lcp_long(const u8 *enc, u64 n, const S *suf,
                                                              const u32 *rank, const u8 *lcp,
                                                              const u64 *llv, u64 m, const u32 *list,
                                                              u64 list_cap, u64 *w) {
  const u64 listed = w[W_LISTED] < list_cap ? w[W_LISTED] : list_cap;
  for (u64 k = blockIdx.x; k < listed; k += gridDim.x) {
    const u64 p = list[k];
    const u32 r = rank[p], C = claim_of(lcp, llv, m, r);
    u32 s = 0;
    if (p > 0) {
      const u32 rp = rank[p - 1];
      if (rp >= 1) s = max(claim_of(lcp, llv, m, rp), 1u) - 1;
    }
    const u64 q = suf[r - 1];
    const u64 at = block_first_bad(enc, n, p, q, s, C);
    if (at < C && threadIdx.x == 0) atomicMin((unsigned long long *) &w[W_FAIL], (unsigned long long) r);
  }
}

// for the report: the common prefix of letters of suffixes p and q
__global__ __launch_bounds__(CHK_THREADS) void k_chk_true_lcp(const u8 *enc, u64 n, u64 p, u64 q, u64 *w) {
  const u64 at = block_first_bad(enc, n, p, q, 0, n + 1);
  if (threadIdx.x == 0) w[W_TRUE_LCP] = at;
}

}  // namespace

struct gtamd_check : ConsumerBase<GTAMD_CHECK_PHASES + 1> {
  Dev<u32> rank;         // the inverse of the suffix table
  Dev<u32> list;         // positions with a long range (b)
};

namespace {

const char FEATURE[] = "index check";

struct Tables {
  const u8 *enc; u64 n;
  const void *suf; u32 suf_bytes;
  const u8 *lcp; const u64 *llv; u64 m;
  const u8 *bwt;
};

Tables tables(const IndexView &v, const u8 *bwt) {
  return Tables{ v.enc, v.n, v.suf, v.suf_bytes, v.lcp, v.llv, v.llv_pairs, bwt };
}

int read_words(gtamd_check *c, u64 *h) { return fetch(c->st, { { c->words, h, W_WORDS * sizeof(u64) } }); }

int reset_fail(gtamd_check *c) {
  HIP_TRY(hipMemsetAsync(c->words, 0xff, sizeof(u64), c->st));    // W_FAIL = NONE
  return 0;
}

int fetch(gtamd_check *c, const void *src, u64 bytes, void *dst) { return ::fetch(c->st, { { src, dst, bytes } }); }

template <typename S> int fetch_suf(gtamd_check *c, const S *suf, u64 i, u64 *out) {
  S v;
  TRY(fetch(c, suf + i, sizeof(S), &v));
  *out = v;
  return 0;
}

void fail(gtamd_check_report *rep, u32 table, u32 criterion, u64 index) {
  rep->ok = 0;
  rep->table = table;
  rep->criterion = criterion;
  rep->index = index;
}

// the phases; *rep is filled as far as they get
template <typename S> int run_phases(gtamd_check *c, const Tables &tb, gtamd_check_report *rep) {
  const S *suf = (const S *) tb.suf;
  const u64 n = tb.n, N = n + 1;
  const u32 blocks = (u32) div_up(N, CHK_TILE);
  u64 h[W_WORDS];
  u64 *w = c->words;
  hipStream_t st = c->st;
  int phase = 0;
  HIP_TRY(hipMemsetAsync(w, 0, W_WORDS * sizeof(u64), st));
  HIP_TRY(hipMemsetAsync(w + W_LONGEST, 0xff, sizeof(u64), st));
  HIP_TRY(hipEventRecord(c->ev[0], st));

  // ---- 1
  TRY(reset_fail(c));
  HIP_TRY(hipMemsetAsync(c->rank, 0xff, N * sizeof(u32), st));
  k_chk_range<S><<<blocks, CHK_THREADS, 0, st>>>(suf, N, c->rank, w);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(c->ev[++phase], st));     // (recorded again behind the second pass)
  TRY(read_words(c, h));
  if (h[W_FAIL] != NONE) {
    fail(rep, GTAMD_CHECK_SUF, GTAMD_CHECK_CRIT_RANGE, h[W_FAIL]);
    TRY(fetch_suf(c, suf, h[W_FAIL], &rep->claimed));
    return phase;
  }
  k_chk_perm<S><<<blocks, CHK_THREADS, 0, st>>>(suf, N, c->rank, w);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(c->ev[phase], st));
  TRY(read_words(c, h));
  if (h[W_FAIL] != NONE) {
    u32 r;
    fail(rep, GTAMD_CHECK_SUF, GTAMD_CHECK_CRIT_PERM, h[W_FAIL]);
    TRY(fetch(c, c->rank + h[W_FAIL], sizeof r, &r));
    rep->pos_a = h[W_FAIL];
    rep->claimed = r;
    if (r != RANK_UNSET) TRY(fetch_suf(c, suf, r, &rep->found));
    return phase;
  }
  rep->longest = h[W_LONGEST];

  // ---- 2
  TRY(reset_fail(c));
  k_chk_order<S><<<blocks, CHK_THREADS, 0, st>>>(tb.enc, n, suf, c->rank, w);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(c->ev[++phase], st));
  TRY(read_words(c, h));
  if (h[W_FAIL] != NONE) {
    fail(rep, GTAMD_CHECK_SUF, GTAMD_CHECK_CRIT_ORDER, h[W_FAIL]);
    TRY(fetch_suf(c, suf, h[W_FAIL] - 1, &rep->pos_a));
    TRY(fetch_suf(c, suf, h[W_FAIL], &rep->pos_b));
    return phase;
  }

  // ---- 3
  if (tb.bwt != nullptr) {
    TRY(reset_fail(c));
    k_chk_bwt<S><<<blocks, CHK_THREADS, 0, st>>>(tb.enc, suf, tb.bwt, N, w);
    HIP_TRY(hipGetLastError());
  }
  HIP_TRY(hipEventRecord(c->ev[++phase], st));
  if (tb.bwt != nullptr) {
    TRY(read_words(c, h));
    if (h[W_FAIL] != NONE) {
      u8 got, want = 254;
      fail(rep, GTAMD_CHECK_BWT, GTAMD_CHECK_CRIT_BWT, h[W_FAIL]);
      TRY(fetch_suf(c, suf, h[W_FAIL], &rep->pos_b));
      TRY(fetch(c, tb.bwt + h[W_FAIL], 1, &got));
      if (rep->pos_b) TRY(fetch(c, tb.enc + rep->pos_b - 1, 1, &want));
      rep->claimed = got;
      rep->found = want;
      return phase;
    }
  }
  if (tb.lcp == nullptr) {
    HIP_TRY(hipEventRecord(c->ev[++phase], st));
    HIP_TRY(hipEventRecord(c->ev[++phase], st));
    return phase;
  }

  // ---- 4
  TRY(reset_fail(c));
  if (tb.m) {
    k_chk_llv_pairs<<<(u32) div_up(tb.m, CHK_TILE), CHK_THREADS, 0, st>>>(tb.lcp, tb.llv, tb.m, n, w);
    HIP_TRY(hipGetLastError());
  }
  k_chk_count255<<<blocks, CHK_THREADS, 0, st>>>(tb.lcp, N, w);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(c->ev[++phase], st));
  TRY(read_words(c, h));
  {
    u8 first;
    TRY(fetch(c, tb.lcp, 1, &first));
    if (first != 0) {
      fail(rep, GTAMD_CHECK_LCP, GTAMD_CHECK_CRIT_LCP0, 0);
      rep->claimed = first;
      rep->found = 0;
      return phase;
    }
  }
  if (h[W_FAIL] != NONE) {
    u64 pair[2];
    TRY(fetch(c, tb.llv + 2 * h[W_FAIL], sizeof pair, pair));
    fail(rep, GTAMD_CHECK_LLV, GTAMD_CHECK_CRIT_LLV_ENTRY, pair[0]);
    rep->llv_entry = h[W_FAIL];
    rep->claimed = pair[1];
    return phase;
  }
  rep->largelcpvalues = h[W_COUNT255];
  if (h[W_COUNT255] != tb.m) {
    // every pair names a byte 255 of its own: there are more bytes than pairs
    k_chk_unlisted<<<blocks, CHK_THREADS, 0, st>>>(tb.lcp, N, tb.llv, tb.m, w);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(c->ev[phase], st));
    TRY(read_words(c, h));
    fail(rep, GTAMD_CHECK_LLV, GTAMD_CHECK_CRIT_LLV_MISSING, h[W_FAIL]);
    rep->claimed = tb.m;
    rep->found = h[W_COUNT255];
    for (u64 lo = 0, hi = tb.m;;) {          // where the pair would stand
      if (lo >= hi) { rep->llv_entry = lo; break; }
      const u64 mid = (lo + hi) >> 1;
      u64 idx;
      TRY(fetch(c, tb.llv + 2 * mid, sizeof idx, &idx));
      if (idx < h[W_FAIL]) lo = mid + 1; else hi = mid;
    }
    return phase;
  }

  // ---- 5
  const u64 list_cap = 2 * N / CHK_LONG_CLAIM + 1;
  TRY(reset_fail(c));
  k_chk_lcp<S><<<blocks, CHK_THREADS, 0, st>>>(tb.enc, n, suf, c->rank, tb.lcp, tb.llv, tb.m,
                                              c->list, list_cap, w);
  HIP_TRY(hipGetLastError());
  k_chk_lcp_long<S><<<(u32) (list_cap < CHK_LONG_BLOCKS ? list_cap : CHK_LONG_BLOCKS), CHK_THREADS, 0, st>>>(
      tb.enc, n, suf, c->rank, tb.lcp, tb.llv, tb.m, c->list, list_cap, w);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(c->ev[++phase], st));
  TRY(read_words(c, h));
  rep->maxbranchdepth = h[W_DEPTH];
  rep->long_claims = h[W_LISTED];
  if (h[W_FAIL] != NONE) {
    const u64 r = h[W_FAIL];
    u8 byte;
    TRY(fetch(c, tb.lcp + r, 1, &byte));
    TRY(fetch_suf(c, suf, r - 1, &rep->pos_a));
    TRY(fetch_suf(c, suf, r, &rep->pos_b));
    rep->claimed = byte;
    if (byte == 255)
      for (u64 lo = 0, hi = tb.m; lo < hi;) {
        const u64 mid = (lo + hi) >> 1;
        u64 pair[2];
        TRY(fetch(c, tb.llv + 2 * mid, sizeof pair, pair));
        if (pair[0] == r) { rep->llv_entry = mid; rep->claimed = pair[1]; break; }
        if (pair[0] < r) lo = mid + 1; else hi = mid;
      }
    k_chk_true_lcp<<<1, CHK_THREADS, 0, st>>>(tb.enc, n, rep->pos_b, rep->pos_a, w);
    HIP_TRY(hipGetLastError());
    TRY(read_words(c, h));
    rep->found = h[W_TRUE_LCP];
    fail(rep, byte == 255 ? GTAMD_CHECK_LLV : GTAMD_CHECK_LCP,
         rep->claimed < rep->found ? GTAMD_CHECK_CRIT_LCP_SMALL : GTAMD_CHECK_CRIT_LCP_LARGE, r);
  }
  return phase;
}

int run_check(gtamd_check *c, const Tables &tb, gtamd_check_report *rep) {
  if (c == nullptr || rep == nullptr || tb.suf == nullptr || (tb.enc == nullptr && tb.n) ||
      (tb.llv == nullptr && tb.m) || (tb.lcp == nullptr && tb.m)) {
    gtamd_set_error("invalid argument to gtamd_check_tables");
    return -1;
  }
  TRY(refuse_suf_bytes(FEATURE, tb.suf_bytes));
  TRY(refuse_sizes(FEATURE, tb.n, 0, "checked"));
  const u64 N = tb.n + 1;
  HIP_TRY(hipSetDevice(c->device));
  *rep = gtamd_check_report();
  rep->ok = 1;
  rep->checked = GTAMD_CHECK_SUF | (tb.lcp ? GTAMD_CHECK_LCP | GTAMD_CHECK_LLV : 0) |
                 (tb.bwt ? GTAMD_CHECK_BWT : 0);
  rep->index = rep->llv_entry = rep->pos_a = rep->pos_b = rep->claimed = rep->found = GTAMD_CHECK_NONE;
  rep->longest = GTAMD_CHECK_NONE;
  if (c->rank.grow(N * sizeof(u32)) != hipSuccess ||
      (tb.lcp && c->list.grow((2 * N / CHK_LONG_CLAIM + 1) * sizeof(u32)) != hipSuccess)) {
    gtamd_set_error("index check: cannot allocate %llu bytes of device memory for the inverse of "
                    "the suffix table", (unsigned long long) (N * sizeof(u32)));
    return -1;
  }
  const int phases = tb.suf_bytes == 4 ? run_phases<u32>(c, tb, rep) : run_phases<u64>(c, tb, rep);
  if (phases < 0) return -1;
  HIP_TRY(hipStreamSynchronize(c->st));
  for (int k = 0; k < phases; k++) HIP_TRY(hipEventElapsedTime(&rep->phase_ms[k], c->ev[k], c->ev[k + 1]));
  HIP_TRY(hipEventElapsedTime(&rep->check_ms, c->ev[0], c->ev[phases]));
  return 0;
}

}  // namespace

extern "C" gtamd_check *gtamd_check_create(int device) {
  GTAMD_ABI_BEGIN
  return create_consumer<gtamd_check>(device, W_WORDS, "the index checker");
  GTAMD_ABI_END(nullptr)
}

extern "C" void gtamd_check_destroy(gtamd_check *c) { destroy_consumer(c); }

extern "C" void gtamd_check_geometry(uint32_t *tile_entries, uint32_t *long_claim) {
  if (tile_entries != nullptr) *tile_entries = CHK_TILE;
  if (long_claim != nullptr) *long_claim = CHK_LONG_CLAIM;
}

extern "C" int gtamd_check_tables(gtamd_check *c, const uint8_t *enc, uint64_t n, const void *suf,
                                  uint32_t suf_bytes, const uint8_t *lcp, const uint64_t *llv,
                                  uint64_t llv_pairs, const uint8_t *bwt, gtamd_check_report *rep) {
  GTAMD_ABI_BEGIN
  const Tables tb = { enc, n, suf, suf_bytes, lcp, llv, llv_pairs, bwt };
  return run_check(c, tb, rep);
  GTAMD_ABI_END(-1)
}

extern "C" int gtamd_check_tables_host(gtamd_check *c, const uint8_t *enc, uint64_t n, const void *suf,
                                       uint32_t suf_bytes, const uint8_t *lcp, const uint64_t *llv,
                                       uint64_t llv_pairs, const uint8_t *bwt, gtamd_check_report *rep) {
  GTAMD_ABI_BEGIN
  if (c == nullptr || suf == nullptr || (suf_bytes != 4 && suf_bytes != 8) || n >= SINGLE_LIMIT ||
      (llv_pairs && (llv == nullptr || lcp == nullptr))) {
    const Tables tb = { enc, n, suf, suf_bytes, lcp, llv, llv_pairs, bwt };
    return run_check(c, tb, rep);        // (words the refusal)
  }
  HIP_TRY(hipSetDevice(c->device));
  Dev<u8> d_enc, d_suf, d_lcp, d_bwt;
  Dev<u64> d_llv;
  // (a table that is not given stays a null pointer: it is not checked)
  TRY(upload(d_enc, enc != nullptr ? (const void *) enc : (const void *) "", n, FEATURE, "the sequence"));
  TRY(upload(d_suf, suf, (n + 1) * suf_bytes, FEATURE, "the .suf table"));
  if (lcp != nullptr) TRY(upload(d_lcp, lcp, n + 1, FEATURE, "the .lcp table"));
  if (llv_pairs) TRY(upload(d_llv, llv, llv_pairs * 16, FEATURE, "the .llv table"));
  if (bwt != nullptr) TRY(upload(d_bwt, bwt, n + 1, FEATURE, "the .bwt table"));
  const Tables tb = { d_enc, n, d_suf.p, suf_bytes, d_lcp, d_llv, llv_pairs, d_bwt };
  return run_check(c, tb, rep);
  GTAMD_ABI_END(-1)
}

extern "C" int gtamd_check_esa(gtamd_check *c, const gtamd_esa_ctx *esa, const uint8_t *enc, uint64_t n,
                               uint32_t want, gtamd_check_report *rep) {
  GTAMD_ABI_BEGIN
  if (c == nullptr || esa == nullptr || rep == nullptr) { gtamd_set_error("invalid argument to gtamd_check_esa"); return -1; }
  if (!(want & GTAMD_WANT_SUF)) { gtamd_set_error("index check: the .lcp and .bwt tables are checked through the .suf table"); return -1; }
  IndexView v;
  TRY(engine_tables(FEATURE, esa, enc, n, false, &v, "checked"));
  Tables tb = tables(v, nullptr);
  if (want & GTAMD_WANT_LCP) {
    tb.lcp = (const u8 *) gtamd_esa_table_device(esa, GTAMD_TAB_LCP);
    tb.m = gtamd_esa_table_entries(esa, GTAMD_TAB_LLV);
    tb.llv = tb.m ? (const u64 *) gtamd_esa_table_device(esa, GTAMD_TAB_LLV) : nullptr;
    if (tb.lcp == nullptr || (tb.m && tb.llv == nullptr)) { gtamd_set_error("index check: the last run did not produce the .lcp table"); return -1; }
  }
  if (want & GTAMD_WANT_BWT) {
    tb.bwt = (const u8 *) gtamd_esa_table_device(esa, GTAMD_TAB_BWT);
    if (tb.bwt == nullptr) { gtamd_set_error("index check: the last run did not produce the .bwt table"); return -1; }
  }
  return run_check(c, tb, rep);
  GTAMD_ABI_END(-1)
}

extern "C" int gtamd_check_message(const gtamd_check_report *r, char *buf, size_t buflen) {
  GTAMD_ABI_BEGIN
  if (r == nullptr || (buf == nullptr && buflen)) { gtamd_set_error("invalid argument to gtamd_check_message"); return -1; }
  typedef unsigned long long ull;
  switch (r->ok ? GTAMD_CHECK_CRIT_NONE : r->criterion) {
    case GTAMD_CHECK_CRIT_NONE:
      return snprintf(buf, buflen, "%s", "");
    case GTAMD_CHECK_CRIT_RANGE:
      return snprintf(buf, buflen, "suf: entry %llu at table index %llu lies outside [0, n]",
                      (ull) r->claimed, (ull) r->index);
    case GTAMD_CHECK_CRIT_PERM:
      if (r->claimed == RANK_UNSET)
        return snprintf(buf, buflen, "suf: not a permutation, position %llu is missing", (ull) r->index);
      return snprintf(buf, buflen, "suf: not a permutation, position %llu occurs more than once "
                      "(not at table index %llu)", (ull) r->index, (ull) r->claimed);
    case GTAMD_CHECK_CRIT_ORDER:
      return snprintf(buf, buflen, "suf: suffixes out of order at table index %llu (suffixes %llu, %llu)",
                      (ull) r->index, (ull) r->pos_a, (ull) r->pos_b);
    case GTAMD_CHECK_CRIT_BWT:
      return snprintf(buf, buflen, "bwt: symbol %llu at table index %llu (suffix %llu), the sequence gives %llu",
                      (ull) r->claimed, (ull) r->index, (ull) r->pos_b, (ull) r->found);
    case GTAMD_CHECK_CRIT_LCP0:
      return snprintf(buf, buflen, "lcp: byte at table index 0 is %llu", (ull) r->claimed);
    case GTAMD_CHECK_CRIT_LLV_ENTRY:
      return snprintf(buf, buflen, "llv: entry %llu (table index %llu, value %llu) does not ascend, lies "
                      "outside the table, names no byte 255 of .lcp or has a value outside [255, n]",
                      (ull) r->llv_entry, (ull) r->index, (ull) r->claimed);
    case GTAMD_CHECK_CRIT_LLV_MISSING:
      return snprintf(buf, buflen, "llv: %llu lcp bytes of 255, %llu .llv entries: none for table index %llu",
                      (ull) r->found, (ull) r->claimed, (ull) r->index);
    case GTAMD_CHECK_CRIT_LCP_SMALL:
    case GTAMD_CHECK_CRIT_LCP_LARGE:
      return snprintf(buf, buflen, "%s: value at table index %llu (suffixes %llu, %llu) is %llu, too %s: "
                      "the suffixes share %llu symbols", r->table == GTAMD_CHECK_LLV ? "llv" : "lcp",
                      (ull) r->index, (ull) r->pos_a, (ull) r->pos_b, (ull) r->claimed,
                      r->criterion == GTAMD_CHECK_CRIT_LCP_SMALL ? "small" : "large", (ull) r->found);
  }
  return snprintf(buf, buflen, "unknown criterion %u", r->criterion);
  GTAMD_ABI_END(-1)
}
