// esa_pckidx.hip -- the reader of the packed index (INDEX.bdx) on the device: C ABI,
// the decoded form and the semantics: include/gtamd_pckidx.h.
//
// Opening an image: the host reads the headers and the region list
// (esa_pckidx_core.h: every field the kernels index with is checked there), then
//   k_pkx_decode     one thread per bucket: pkx_decode_bucket into the lines (or
//                    the rows and the counter table), pkx_bucket_marks into the
//                    bitmap of the marked rows
//   popcount + scan  the marks before every word of the bitmap
//   k_pkx_marks      one thread per bucket: the stored numbers to their places in
//                    row order, the stored ranks of the special rows
// and the host checks what the decode counted against the regions.
// Searching: dec_rank / dec_rank_pair / dec_symbol / dec_locate on the decoded
// form (esa_pckidx_dec.h, shared with the walk of esa_tagmatch.hip); k_pkx_mstat
// is the backward search of matstat and uniquesub, one lane per query position.
#include <vector>
#include "esa_common.h"
#include "esa_own.h"
#include "esa_prims.h"
#include "esa_index.h"
#include "esa_pckidx_core.h"
#include "esa_pckidx.h"
#include "esa_pckidx_dec.h"
#include "../../include/gtamd_pckidx.h"

namespace {

constexpr int PKX_THREADS = 256;
constexpr u32 PKX_E_ARG = 100;           // a batch call with a row or a letter outside the index
enum { PART_ROWS = 0, PART_AUX, PART_MARKS, PART_MARKPRE, PART_MARKPOS, PART_SPRANK, PART_REGIONS, PART_COUNT, PARTS };

// ---- decode ----------------------------------------------------------------------
struct DecodeSink {
  PkxDec d;
  u64 word;      // two_bit: the word of the lines being put together
  u32 acc;
  __device__ __forceinline__ void flush() {
    if (acc) atomicOr(&d.lines[word], acc);
    acc = 0;
  }
  __device__ __forceinline__ void counters(u64 line, const u32 *run) {
    for (u32 s = 0; s < 4; s++) d.lines[line * LINE_WORDS + s] = s < d.sigma ? run[s] : 0u;
  }
  __device__ __forceinline__ void row(u64 row, u32 code, const u32 *run) {
    if (d.two_bit) {
      const u64 line = row / LINE_ROWS;
      const u32 i = (u32) (row % LINE_ROWS);
      if (i == 0) counters(line, run);
      const u64 wd = line * LINE_WORDS + 4 + i / 16;
      if (wd != word) { flush(); word = wd; }
      if (code >= 254) atomicOr(&d.flags[line >> 5], 1u << (line & 31));
      else acc |= code << (2 * (i % 16));
    } else {
      d.sym[row] = (u8) code;
      if (row % CP_ROWS == 0)
        for (u32 s = 0; s < d.sigma; s++) d.cp[(row / CP_ROWS) * d.sigma + s] = run[s];
    }
  }
  // behind the last row: the totals, and the counters a rank at row N reads
  __device__ __forceinline__ void end(const u32 *run) {
    for (u32 s = 0; s < d.sigma; s++) d.totals[s] = run[s];
    if (d.two_bit) { if (d.N % LINE_ROWS == 0) counters(d.N / LINE_ROWS, run); }
    else if (d.N % CP_ROWS == 0)
      for (u32 s = 0; s < d.sigma; s++) d.cp[(d.N / CP_ROWS) * d.sigma + s] = run[s];
  }
  __device__ __forceinline__ void mark(u64 row, u64) { atomicOr((unsigned long long *) &d.mk[row >> 6], 1ull << (row & 63)); }
  __device__ __forceinline__ void sprank(u32, u64, u64) {}
};

// 1 for every bucket whose var offset field is smaller than the one before: pkx_var_offset
__global__ void k_pkx_wrap_flags(PkxGeom g, PkxImage im, u32 *wraps, u32 *err) {
  const u64 bucket = (u64) blockIdx.x * blockDim.x + threadIdx.x;
  if (bucket >= g.nb) return;
  u32 e = PKX_OK;
  wraps[bucket] = pkx_wrap_flag(g, im, bucket, &e);
  dev_fail(err, e);
}

__global__ __launch_bounds__(PKX_THREADS) void k_pkx_decode(PkxGeom g, PkxImage im, const u8 *comp_tab, const u32 *wraps,
                                                            PkxDec d, u32 *err) {
  const u64 bucket = (u64) blockIdx.x * PKX_THREADS + threadIdx.x;
  if (bucket >= g.nb) return;
  DecodeSink sink = { d, ~0ull, 0 };
  u32 e = PKX_OK;
  pkx_decode_bucket(g, im, comp_tab, d.rg, wraps, bucket, sink, &e);
  sink.flush();
  if (e == PKX_OK) pkx_bucket_marks(g, im, d.rg, wraps, bucket, sink, &e);
  dev_fail(err, e);
}

struct MarkSink {
  PkxDec d;
  __device__ __forceinline__ void mark(u64 row, u64 val) {
    const u64 w = d.mk[row >> 6];
    d.mkpos[d.mkpre[row >> 6] + (u32) __popcll(w & ((1ull << (row & 63)) - 1))] = (u32) val;
  }
  __device__ __forceinline__ void sprank(u32 ri, u64 row, u64 rank) {
    d.sprank[d.rg.pre[ri] + (u32) (row - d.rg.start[ri])] = (u32) rank;
  }
};

__global__ __launch_bounds__(PKX_THREADS) void k_pkx_marks(PkxGeom g, PkxImage im, const u32 *wraps, PkxDec d, u32 *err) {
  const u64 bucket = (u64) blockIdx.x * PKX_THREADS + threadIdx.x;
  if (bucket >= g.nb) return;
  MarkSink sink = { d };
  u32 e = PKX_OK;
  pkx_bucket_marks(g, im, d.rg, wraps, bucket, sink, &e);
  dev_fail(err, e);
}

__global__ void k_pkx_popc(const u64 *__restrict__ mk, u64 nwords, u32 *__restrict__ cnt) {
  const u64 i = (u64) blockIdx.x * blockDim.x + threadIdx.x;
  if (i <= nwords) cnt[i] = i < nwords ? (u32) __popcll(mk[i]) : 0u;
}

// ---- batch entry points ------------------------------------------------------------
__global__ void k_pkx_bwt(PkxDec d, u64 row0, u64 count, u8 *out) {
  const u64 i = (u64) blockIdx.x * blockDim.x + threadIdx.x;
  if (i < count) out[i] = (u8) dec_symbol(d, row0 + i);
}
__global__ void k_pkx_rank(PkxDec d, const u8 *sym, const u64 *rows, u64 count, u64 *out, u32 *err) {
  const u64 i = (u64) blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  const u32 s = sym[i];
  const u64 r = rows[i];
  if (s >= d.sigma || r > d.N) { dev_fail(err, PKX_E_ARG); out[i] = 0; return; }
  out[i] = dec_rank(d, s, r);
}
__global__ void k_pkx_locate(PkxDec d, const u64 *rows, u64 count, u64 *out, u32 *err) {
  const u64 i = (u64) blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  const u64 r = rows[i];
  if (r >= d.N) { dev_fail(err, PKX_E_ARG); out[i] = 0; return; }
  out[i] = dec_locate(d, r, err);
}

// ---- matstat and uniquesub -----------------------------------------------------------
// gt_packedindexmstatsforward / gt_packedindexuniqueforward, src/match/eis-bwtseq.c:
// 225-364, and gt_voidpackedfindfirstmatchconvert, eis-voiditf.c:428-438
template <bool MATSTAT>
__global__ __launch_bounds__(PKX_THREADS) void k_pkx_mstat(PkxDec d, const u8 *__restrict__ q, u64 m, u32 limit,
                                                           u32 *len_out, u64 *pos_out, u64 *pairs, u64 *error) {
  __shared__ u32 s_count[PKX_MAX_SIGMA + 2];
  __shared__ u32 s_pairs, s_err;
  if (threadIdx.x <= d.sigma) s_count[threadIdx.x] = d.count[threadIdx.x];
  if (threadIdx.x == 0) { s_pairs = 0; s_err = 0; }
  __syncthreads();
  const u64 i = (u64) blockIdx.x * PKX_THREADS + threadIdx.x;
  u32 steps = 0;
  if (i < m) {
    const u64 rest = m - i;
    u32 len = 0, c = q[i];
    u64 pos = 0;
    if (c < d.sigma && s_count[c] < s_count[c + 1]) {
      u32 lo = s_count[c], hi = s_count[c + 1];
      if (MATSTAT) {
        u32 prev = lo;
        for (len = 1; len < limit && len < rest; len++) {
          c = q[i + len];
          if (c >= d.sigma) break;
          u32 a, b;
          dec_rank_pair(d, c, lo, hi, &a, &b);
          steps++;
          lo = s_count[c] + a; hi = s_count[c] + b;
          if (lo >= hi) break;
          prev = lo;
        }
        if (pos_out != nullptr) {
          const u64 located = dec_locate(d, prev, &s_err) + len;
          pos = located <= d.N - 1 ? d.N - 1 - located : 0;
        }
      } else {
        u64 k = 1;
        while (k < rest && lo + 1 < hi) {
          c = q[i + k];
          if (c >= d.sigma) { lo = hi; break; }
          u32 a, b;
          dec_rank_pair(d, c, lo, hi, &a, &b);
          steps++;
          lo = s_count[c] + a; hi = s_count[c] + b;
          k++;
        }
        len = lo + 1 == hi ? (k < limit ? (u32) k : limit) : 0;
      }
    }
    len_out[i] = len;
    if (MATSTAT && pos_out != nullptr) pos_out[i] = pos;
  }
  if (steps) atomicAdd(&s_pairs, steps);
  __syncthreads();
  if (threadIdx.x == 0) {
    if (s_pairs) atomicAdd((unsigned long long *) pairs, (unsigned long long) s_pairs);
    if (s_err) atomicMax((unsigned long long *) error, (unsigned long long) s_err);
  }
}

const char FEATURE[] = "packed index reader";

}  // namespace

struct gtamd_pckidx : ConsumerBase<> {
  PkxGeom g = PkxGeom();
  PkxDec d = PkxDec();
  bool open = false;
  u64 opens = 0;                // open calls so far: which image a consumer saw
  Dev<u8> image;               // a host image on its way through the decode
  Dev<u8> comp_tab; u32 tab_sigma = 0, tab_B = 0;
  Dev<u32> rows, aux, count, mkpre, mkpos, sprank, rg_start, rg_pre, totals, ws;
  Dev<u64> mk;
  Dev<u8> rg_sym;
  Dev<u8> in, out;             // staging of the batch calls
  u64 part_bytes[PARTS] = {};
  gtamd_pckidx_info info = gtamd_pckidx_info();
};

namespace {

int refuse(const char *msg) { gtamd_set_error("%s", msg); return -1; }

// headers and region list of an image whose bytes are read through `read`
template <typename Read>
int parse_image(Read read, u64 bytes, PkxGeom *g, std::vector<u32> &start, std::vector<u32> &pre, std::vector<u8> &sym) {
  char msg[512];
  std::vector<u8> head((size_t) (bytes < 8192 ? bytes : 8192));
  TRY(read(0, head.size(), head.data()));
  if (pkx_parse_header(head.data(), head.size(), bytes, g, msg, sizeof msg) != 0) return refuse(msg);
  std::vector<u8> list((size_t) (bytes - g->range_enc_pos));
  TRY(read(g->range_enc_pos, list.size(), list.data()));
  if (pkx_parse_regions(list.data(), list.size(), g, start, pre, sym, msg, sizeof msg) != 0) return refuse(msg);
  return 0;
}

template <typename T> int put(Dev<T> &dst, const void *src, u64 bytes, const char *what) {
  if (dst.alloc(bytes ? bytes : 8) != hipSuccess) {
    gtamd_set_error("%s: cannot allocate %llu bytes of device memory for %s", FEATURE, (unsigned long long) bytes, what);
    return -1;
  }
  if (bytes) HIP_TRY(hipMemcpy(dst.p, src, bytes, hipMemcpyHostToDevice));
  return 0;
}
template <typename T> int zeroed(Dev<T> &dst, u64 bytes, const char *what, hipStream_t st) {
  if (dst.alloc(bytes ? bytes : 8) != hipSuccess) {
    gtamd_set_error("%s: cannot allocate %llu bytes of device memory for %s", FEATURE, (unsigned long long) bytes, what);
    return -1;
  }
  HIP_TRY(hipMemsetAsync(dst.p, 0, bytes ? bytes : 8, st));
  return 0;
}

// host: non-null for an image in host memory; dev: the same bytes on the device
int open_image(gtamd_pckidx *px, const u8 *host, const u8 *dev, u64 bytes) {
  // (a searcher may still point here: whatever happens below, it finds no image
  // and no pointer of the one before)
  px->open = false;
  px->opens += 1;
  px->d = PkxDec();
  px->g = PkxGeom();
  HIP_TRY(hipSetDevice(px->device));
  PkxGeom g;
  std::vector<u32> start, pre;
  std::vector<u8> sym;
  if (host != nullptr) {
    TRY(parse_image([&](u64 off, u64 cnt, u8 *dst) { memcpy(dst, host + off, cnt); return 0; }, bytes, &g, start, pre, sym));
    TRY(upload(px->image, host, bytes, FEATURE, "the image"));
    dev = px->image;
  } else
    TRY(parse_image([&](u64 off, u64 cnt, u8 *dst) {
      if (cnt) HIP_TRY(hipMemcpy(dst, dev + off, cnt, hipMemcpyDeviceToHost));
      return 0;
    }, bytes, &g, start, pre, sym));

  hipStream_t st = px->st;
  if (px->comp_tab.p == nullptr || px->tab_sigma != g.sigma || px->tab_B != g.B) {
    std::vector<u8> tab((size_t) (g.ncomp * g.sigma));
    pkx_comp_table(g.sigma, g.B, tab.data());
    TRY(put(px->comp_tab, tab.data(), tab.size(), "the composition table"));
    px->tab_sigma = g.sigma; px->tab_B = g.B;
  }
  TRY(put(px->rg_start, start.data(), start.size() * 4, "the regions"));
  TRY(put(px->rg_pre, pre.data(), pre.size() * 4, "the regions"));
  TRY(put(px->rg_sym, sym.data(), sym.size(), "the regions"));

  PkxDec d = PkxDec();
  d.N = g.N; d.rot0 = g.rot0; d.first_special_row = g.first_special_row;
  d.sigma = g.sigma; d.two_bit = g.sigma <= 4; d.locint = g.locint; d.reversible = g.reversible;
  d.rg = PkxRegions{ px->rg_start, px->rg_pre, px->rg_sym, (u32) g.nregions };
  u64 *pb = px->part_bytes;
  memset(pb, 0, sizeof px->part_bytes);
  const u64 nlines = g.N / LINE_ROWS + 1, ncp = g.N / CP_ROWS + 1, nwords = g.N / 64 + 1;
  if (d.two_bit) {
    pb[PART_ROWS] = nlines * LINE_WORDS * 4;
    pb[PART_AUX] = (nlines / 32 + 1) * 4;
  } else {
    pb[PART_ROWS] = ncp * CP_ROWS;
    pb[PART_AUX] = ncp * g.sigma * 4;
  }
  TRY(zeroed(px->rows, pb[PART_ROWS], "the decoded rows", st));
  TRY(zeroed(px->aux, pb[PART_AUX], d.two_bit ? "the line flags" : "the counter table", st));
  TRY(zeroed(px->totals, (PKX_MAX_SIGMA + 2) * 4, "the totals", st));
  HIP_TRY(hipMemsetAsync(px->words, 0, 8, st));
  if (d.two_bit) { d.lines = px->rows; d.flags = px->aux; } else { d.sym = (u8 *) px->rows.p; d.cp = px->aux; }
  d.totals = px->totals;
  pb[PART_REGIONS] = start.size() * 4;
  pb[PART_COUNT] = (g.sigma + 1) * 4;
  if (g.locint) {
    pb[PART_MARKS] = nwords * 8;
    pb[PART_MARKPRE] = (nwords + 1) * 4;
    TRY(zeroed(px->mk, pb[PART_MARKS], "the mark bitmap", st));
    TRY(zeroed(px->mkpre, pb[PART_MARKPRE], "the mark directory", st));
    if (px->ws.grow(scan_workspace_words(nwords + 1) * 4 + 64) != hipSuccess) return out_of_memory(FEATURE, nwords, "words of scan workspace");
    if (g.reversible) {
      pb[PART_SPRANK] = (g.total_specials + 1) * 4;
      TRY(zeroed(px->sprank, pb[PART_SPRANK], "the ranks of the specials", st));
    }
    d.mk = px->mk; d.mkpre = px->mkpre; d.sprank = px->sprank;
  }
  u32 *err = (u32 *) px->words.p;
  const PkxImage im = { dev, bytes };
  const u32 grid = (u32) div_up(g.nb, PKX_THREADS);
  HIP_TRY(hipEventRecord(px->ev[0], st));
  Dev<u32> wraps;        // only for an image whose var offset fields wrap
  if (pkx_offsets_wrap(g)) {
    if (wraps.alloc(g.nb * 4) != hipSuccess || px->ws.grow(scan_workspace_words(g.nb) * 4 + 64) != hipSuccess)
      return out_of_memory(FEATURE, g.nb, "var offsets");
    k_pkx_wrap_flags<<<grid, PKX_THREADS, 0, st>>>(g, im, wraps, err);
    HIP_TRY(hipGetLastError());
    TRY(scan_u32(SCAN_SUM, wraps, wraps, g.nb, true, px->ws, st));
  }
  k_pkx_decode<<<grid, PKX_THREADS, 0, st>>>(g, im, px->comp_tab, wraps, d, err);
  HIP_TRY(hipGetLastError());
  u32 h_err = 0, h_totals[PKX_MAX_SIGMA + 2];
  if (g.locint) {
    k_pkx_popc<<<(u32) div_up(nwords + 1, 256), 256, 0, st>>>(px->mk, nwords, px->mkpre);
    HIP_TRY(hipGetLastError());
    TRY(scan_u32(SCAN_SUM, px->mkpre, px->mkpre, nwords + 1, false, px->ws, st));
    u32 nmarks = 0;
    u64 rot0_word = 0;
    TRY(fetch(st, { { err, &h_err, 4 }, { px->mkpre + nwords, &nmarks, 4 }, { px->mk + (g.rot0 >> 6), &rot0_word, 8 } }));
    if (h_err == PKX_OK && !((rot0_word >> (g.rot0 & 63)) & 1)) {
      gtamd_set_error("%s: row %llu of suffix 0 is not marked", FEATURE, (unsigned long long) g.rot0);
      return -1;
    }
    if (h_err == PKX_OK) {
      d.nmarks = nmarks;
      pb[PART_MARKPOS] = (u64) nmarks * 4;
      TRY(zeroed(px->mkpos, pb[PART_MARKPOS], "the stored positions", st));
      d.mkpos = px->mkpos;
      k_pkx_marks<<<grid, PKX_THREADS, 0, st>>>(g, im, wraps, d, err);
      HIP_TRY(hipGetLastError());
    }
  }
  HIP_TRY(hipEventRecord(px->ev[1], st));
  TRY(fetch(st, { { err, &h_err, 4 }, { px->totals, h_totals, g.sigma * 4 } }));
  px->image.reset();
  if (h_err != PKX_OK) {
    gtamd_set_error("%s: the image does not decode: %s", FEATURE, pkx_error_text(h_err));
    return -1;
  }
  // count[], and what the decode counted against the regions
  u32 count[PKX_MAX_SIGMA + 2];
  u64 letters = 0;
  for (u32 s = 0; s < g.sigma; s++) { count[s] = (u32) letters; letters += h_totals[s]; }
  count[g.sigma] = (u32) letters;
  if (letters != g.first_special_row) {
    gtamd_set_error("%s: the image does not decode: %s (%llu letters, %llu special rows, %llu rows)", FEATURE,
                    pkx_error_text(PKX_E_TOTALS), (unsigned long long) letters,
                    (unsigned long long) (g.N - g.first_special_row), (unsigned long long) g.N);
    return -1;
  }
  TRY(put(px->count, count, (g.sigma + 1) * 4, "count[]"));
  d.count = px->count;
  px->g = g;
  px->d = d;
  gtamd_pckidx_info &f = px->info;
  f = gtamd_pckidx_info();
  f.rows = g.N; f.buckets = g.nb; f.regions = g.nregions; f.special_rows = g.N - g.first_special_row;
  f.marks = d.nmarks; f.rot0_row = g.rot0; f.image_bytes = bytes;
  for (int k = 0; k < PARTS; k++) f.decoded_bytes += pb[k];
  f.decoded_bytes += pre.size() * 4 + sym.size();
  f.numofchars = g.sigma; f.block_size = g.B; f.bucket_blocks = g.K; f.locate_interval = g.locint;
  f.feature_toggles = (g.loc_bitmap ? 1u : 0u) | (g.loc_count ? 2u : 0u) | (g.reversible ? 4u : 0u);
  f.two_bit = d.two_bit; f.line_rows = d.two_bit ? LINE_ROWS : CP_ROWS;
  HIP_TRY(hipEventElapsedTime(&f.decode_ms, px->ev[0], px->ev[1]));
  px->open = true;
  return 0;
}

int need_open(const gtamd_pckidx *px, const char *fn) {
  if (px == nullptr) { gtamd_set_error("invalid argument to %s", fn); return -1; }
  if (!px->open) { gtamd_set_error("%s: no image is open (gtamd_pckidx_open_*)", FEATURE); return -1; }
  return 0;
}

// a batch call: in_bytes of input at in0 / in1 (host unless is_device), out_bytes of output
struct Staged { const u8 *in0; const u8 *in1; u8 *out; };
int stage(gtamd_pckidx *px, const void *in0, u64 b0, const void *in1, u64 b1, void *out, u64 out_bytes, int is_device,
          Staged *s) {
  if (is_device) { *s = Staged{ (const u8 *) in0, (const u8 *) in1, (u8 *) out }; return 0; }
  const u64 a0 = (b0 + 15) & ~15ull;
  if (px->in.grow(a0 + b1 + 16) != hipSuccess || px->out.grow(out_bytes + 16) != hipSuccess)
    return out_of_memory(FEATURE, a0 + b1 + out_bytes, "bytes of a batch call");
  if (b0) HIP_TRY(hipMemcpyAsync(px->in.p, in0, b0, hipMemcpyHostToDevice, px->st));
  if (b1) HIP_TRY(hipMemcpyAsync((u8 *) px->in.p + a0, in1, b1, hipMemcpyHostToDevice, px->st));
  *s = Staged{ px->in, (const u8 *) px->in.p + a0, px->out };
  return 0;
}
int finish(gtamd_pckidx *px, const Staged &s, void *out, u64 out_bytes, int is_device, const char *what) {
  u32 h_err = 0;
  TRY(fetch(px->st, { { px->words.p, &h_err, 4 }, { s.out, out, is_device ? 0 : out_bytes } }));
  if (h_err == PKX_E_ARG) { gtamd_set_error("%s: %s outside the index of %llu rows over %u letters", FEATURE, what, (unsigned long long) px->g.N, px->g.sigma); return -1; }
  if (h_err != PKX_OK) { pckidx_set_search_error(h_err); return -1; }
  return 0;
}

}  // namespace

int pckidx_device(const gtamd_pckidx *px) { return px->device; }
bool pckidx_is_open(const gtamd_pckidx *px) { return px->open; }
u64 pckidx_opens(const gtamd_pckidx *px) { return px->opens; }
bool pckidx_can_locate(const gtamd_pckidx *px) { return px->g.locint != 0; }
u64 pckidx_decoded_bytes(const gtamd_pckidx *px) { return px->info.decoded_bytes; }
const PkxDec &pckidx_dec(const gtamd_pckidx *px) { return px->d; }
void pckidx_set_search_error(u64 error) {
  gtamd_set_error("%s: the decoded index is inconsistent: %s", FEATURE, pkx_error_text((u32) error));
}
int pckidx_search(const gtamd_pckidx *px, hipStream_t st, bool matstat, const u8 *q, u64 m, u32 limit, u32 *len,
                  u64 *pos, u64 *pairs, u64 *error) {
  const u32 grid = (u32) div_up(m, PKX_THREADS);
  if (matstat) k_pkx_mstat<true><<<grid, PKX_THREADS, 0, st>>>(px->d, q, m, limit, len, pos, pairs, error);
  else k_pkx_mstat<false><<<grid, PKX_THREADS, 0, st>>>(px->d, q, m, limit, len, pos, pairs, error);
  HIP_TRY(hipGetLastError());
  return 0;
}

extern "C" int gtamd_pckidx_check_image(const void *image, uint64_t bytes) {
  GTAMD_ABI_BEGIN
  if (image == nullptr) { gtamd_set_error("invalid argument to gtamd_pckidx_check_image"); return -1; }
  PkxGeom g;
  std::vector<u32> start, pre;
  std::vector<u8> sym;
  const u8 *host = (const u8 *) image;
  return parse_image([&](u64 off, u64 cnt, u8 *dst) { memcpy(dst, host + off, cnt); return 0; }, bytes, &g, start, pre, sym);
  GTAMD_ABI_END(-1)
}

extern "C" gtamd_pckidx *gtamd_pckidx_create(int device) {
  GTAMD_ABI_BEGIN
  return create_consumer<gtamd_pckidx>(device, 1, "the packed index reader");
  GTAMD_ABI_END(nullptr)
}

extern "C" void gtamd_pckidx_destroy(gtamd_pckidx *px) { destroy_consumer(px); }

extern "C" int gtamd_pckidx_open_host(gtamd_pckidx *px, const void *image, uint64_t bytes) {
  GTAMD_ABI_BEGIN
  if (px == nullptr || image == nullptr) { gtamd_set_error("invalid argument to gtamd_pckidx_open_host"); return -1; }
  return open_image(px, (const u8 *) image, nullptr, bytes);
  GTAMD_ABI_END(-1)
}

extern "C" int gtamd_pckidx_open_device(gtamd_pckidx *px, const void *image, uint64_t bytes) {
  GTAMD_ABI_BEGIN
  if (px == nullptr || image == nullptr) { gtamd_set_error("invalid argument to gtamd_pckidx_open_device"); return -1; }
  return open_image(px, nullptr, (const u8 *) image, bytes);
  GTAMD_ABI_END(-1)
}

extern "C" int gtamd_pckidx_open_builder(gtamd_pckidx *px, const gtamd_pck *builder) {
  GTAMD_ABI_BEGIN
  if (px == nullptr || builder == nullptr) { gtamd_set_error("invalid argument to gtamd_pckidx_open_builder"); return -1; }
  gtamd_pck_info bi;
  TRY(gtamd_pck_get_info(builder, &bi));
  return open_image(px, nullptr, (const u8 *) gtamd_pck_image_device(builder), bi.file_bytes);
  GTAMD_ABI_END(-1)
}

extern "C" int gtamd_pckidx_get_info(const gtamd_pckidx *px, gtamd_pckidx_info *info) {
  GTAMD_ABI_BEGIN
  TRY(need_open(px, "gtamd_pckidx_get_info"));
  return consumer_info(px, info, "gtamd_pckidx_get_info");
  GTAMD_ABI_END(-1)
}

extern "C" int gtamd_pckidx_decoded_copy(gtamd_pckidx *px, uint32_t part, void *dst, uint64_t capacity, uint64_t *bytes) {
  GTAMD_ABI_BEGIN
  TRY(need_open(px, "gtamd_pckidx_decoded_copy"));
  if (part >= PARTS || bytes == nullptr) { gtamd_set_error("invalid argument to gtamd_pckidx_decoded_copy"); return -1; }
  const void *src[PARTS] = { px->rows.p, px->aux.p, px->mk.p, px->mkpre.p, px->mkpos.p, px->sprank.p, px->rg_start.p, px->count.p };
  *bytes = px->part_bytes[part];
  const u64 cnt = *bytes < capacity ? *bytes : capacity;
  HIP_TRY(hipSetDevice(px->device));
  if (dst != nullptr && cnt) HIP_TRY(hipMemcpy(dst, src[part], cnt, hipMemcpyDeviceToHost));
  return 0;
  GTAMD_ABI_END(-1)
}

extern "C" int gtamd_pckidx_bwt(gtamd_pckidx *px, uint64_t row0, uint64_t count, uint8_t *out, int is_device) {
  GTAMD_ABI_BEGIN
  TRY(need_open(px, "gtamd_pckidx_bwt"));
  if (row0 > px->g.N || count > px->g.N - row0) {
    gtamd_set_error("%s: rows [%llu,+%llu) outside the %llu rows of the index", FEATURE, (unsigned long long) row0,
                    (unsigned long long) count, (unsigned long long) px->g.N);
    return -1;
  }
  if (count == 0) return 0;
  if (out == nullptr) { gtamd_set_error("invalid argument to gtamd_pckidx_bwt"); return -1; }
  HIP_TRY(hipSetDevice(px->device));
  Staged s;
  TRY(stage(px, nullptr, 0, nullptr, 0, out, count, is_device, &s));
  HIP_TRY(hipMemsetAsync(px->words, 0, 8, px->st));
  k_pkx_bwt<<<(u32) div_up(count, 256), 256, 0, px->st>>>(px->d, row0, count, s.out);
  HIP_TRY(hipGetLastError());
  return finish(px, s, out, count, is_device, "a row");
  GTAMD_ABI_END(-1)
}

extern "C" int gtamd_pckidx_rank(gtamd_pckidx *px, const uint8_t *symbols, const uint64_t *rows, uint64_t count,
                                 uint64_t *out, int is_device) {
  GTAMD_ABI_BEGIN
  TRY(need_open(px, "gtamd_pckidx_rank"));
  if (count == 0) return 0;
  if (symbols == nullptr || rows == nullptr || out == nullptr || count >= (1ull << 32)) { gtamd_set_error("invalid argument to gtamd_pckidx_rank"); return -1; }
  HIP_TRY(hipSetDevice(px->device));
  Staged s;
  TRY(stage(px, symbols, count, rows, count * 8, out, count * 8, is_device, &s));
  HIP_TRY(hipMemsetAsync(px->words, 0, 8, px->st));
  k_pkx_rank<<<(u32) div_up(count, 256), 256, 0, px->st>>>(px->d, s.in0, (const u64 *) s.in1, count, (u64 *) s.out, (u32 *) px->words.p);
  HIP_TRY(hipGetLastError());
  return finish(px, s, out, count * 8, is_device, "a (letter, row) pair");
  GTAMD_ABI_END(-1)
}

extern "C" int gtamd_pckidx_locate(gtamd_pckidx *px, const uint64_t *rows, uint64_t count, uint64_t *out, int is_device) {
  GTAMD_ABI_BEGIN
  TRY(need_open(px, "gtamd_pckidx_locate"));
  if (!px->g.locint) {
    gtamd_set_error("%s: the index holds no locate information (locate interval 0): positions cannot be had from it", FEATURE);
    return -1;
  }
  if (count == 0) return 0;
  if (rows == nullptr || out == nullptr || count >= (1ull << 32)) { gtamd_set_error("invalid argument to gtamd_pckidx_locate"); return -1; }
  HIP_TRY(hipSetDevice(px->device));
  Staged s;
  TRY(stage(px, rows, count * 8, nullptr, 0, out, count * 8, is_device, &s));
  HIP_TRY(hipMemsetAsync(px->words, 0, 8, px->st));
  k_pkx_locate<<<(u32) div_up(count, 256), 256, 0, px->st>>>(px->d, (const u64 *) s.in0, count, (u64 *) s.out, (u32 *) px->words.p);
  HIP_TRY(hipGetLastError());
  return finish(px, s, out, count * 8, is_device, "a row");
  GTAMD_ABI_END(-1)
}
