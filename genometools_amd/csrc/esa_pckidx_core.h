// esa_pckidx_core.h -- the reader of an INDEX.bdx image (esa_pckidx.hip, C ABI and
// semantics: include/gtamd_pckidx.h), apart from the kernels so that a test can
// compile it with g++ alone (tests/pckidx_core_shim.cpp) and run the very code
// the lanes run on images of the oracle without a device.
//
// Two halves.  The host half reads the headers of an image into a PkxGeom and
// refuses whatever the lanes would index with unchecked (pkx_parse_header,
// pkx_parse_regions).  The lane half decodes one bucket: the occurrence counters
// and the composition indices from its constant-width record, the permutation
// indices from its var part, both unrankings, the specials put back from the
// region list (pkx_decode_bucket), and its locate records of both flavours with
// the ranks of its specials (pkx_bucket_marks).  Every read of the image goes
// through pkx_take, which knows where the section it reads ends: a lying var
// offset, mark count or mark position ends in an error word, not in a read
// beyond the image.  The layout is the one esa_pck.hip writes.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <vector>

typedef uint64_t u64;
typedef uint32_t u32;
typedef uint8_t u8;

#if defined(__HIPCC__)
#define PKX_HD __host__ __device__ inline
#else
#define PKX_HD inline
#endif

constexpr u32 PKX_MAX_SIGMA = 30;        // what the builder accepts
constexpr u32 PKX_MAX_BLOCK = 16;
constexpr u32 PKX_MAX_BUCKET = 16384;    // positions of a bucket
constexpr u32 PKX_MAX_COMP_BITS = 18, PKX_MAX_PERM_BITS = 40;
constexpr u64 PKX_MAX_ROWS = (1ull << 32) - 4096;   // SINGLE_LIMIT of esa_common.h

// the error word of a decode or a search: the first thing that went wrong
enum {
  PKX_OK = 0,
  PKX_E_READ,        // a field beyond the end of its section
  PKX_E_COUNTER,     // an occurrence counter beyond the rows
  PKX_E_VAROFF,      // a var offset behind the var part
  PKX_E_COMP,        // a composition index that is none
  PKX_E_PERM,        // a permutation index that is none of its composition
  PKX_E_PERMBITS,    // the bits of the permutation indices are not what the record says
  PKX_E_MARKCOUNT,   // more marks than rows
  PKX_E_MARKROW,     // mark rows that do not increase, or lie behind the bucket
  PKX_E_MARKVALUE,   // a stored text position beyond the text
  PKX_E_SPRANK,      // a stored rank beyond the specials
  PKX_E_WALK,        // a locate walk that does not end
  PKX_E_TOTALS,      // the decoded letters and the regions do not add up to the rows
  PKX_E_VARCHAIN     // the var part of a bucket does not end where the next one begins
};

static inline const char *pkx_error_text(u32 e) {
  static const char *const text[] = {
    "no error", "a field lies beyond the end of its section", "an occurrence counter exceeds the number of rows",
    "a var offset points behind the var part", "a composition index is none of its geometry",
    "a permutation index is none of its composition",
    "the permutation indices of a bucket do not have the bits its record states",
    "a bucket states more locate marks than it has rows",
    "the rows of the locate marks of a bucket do not increase or lie behind it",
    "a stored text position lies beyond the text", "a stored rank lies beyond the specials",
    "a locate walk does not reach a mark", "the decoded letters and the regions do not add up to the rows",
    "the var part of a bucket does not end where the next one begins" };
  return e < sizeof text / sizeof text[0] ? text[e] : "unknown error";
}

// gt_requiredUInt64Bits, src/core/bitpackstringop.c:60-79
PKX_HD u32 pkx_reqbits(u64 v) {
  u32 r = 1;
  while (v >>= 1) r++;
  return r;
}
PKX_HD u64 pkx_binom(u32 n, u32 k) {
  if (k > n) return 0;
  if (k > n - k) k = n - k;
  u64 r = 1;
  for (u32 i = 1; i <= k; i++) r = r * (n - k + i) / i;
  return r;
}
PKX_HD u64 pkx_factorial(u32 n) {
  u64 r = 1;
  while (n > 1) r *= n--;
  return r;
}
// arrangements of a block with cnt[s] letters s, B <= 16 in all
PKX_HD u64 pkx_arrangements(const u8 *cnt, u32 sigma, u32 B) {
  u64 r = pkx_factorial(B);
  for (u32 s = 0; s < sigma; s++)
    if (cnt[s] > 1) r /= pkx_factorial(cnt[s]);
  return r;
}

// everything the lanes need to know about an image, all of it from its headers
struct PkxGeom {
  u64 N, nb;                 // rows (n + 1), buckets
  u64 bytes;                 // of the image
  u64 cw_base_bit, cw_end_bit, var_base_bit, var_end_bit;   // the two bit strings
  u64 range_enc_pos, nregions;      // region list: position, records without the closing one
  u64 rot0;                  // row of suffix 0
  u64 ncomp;                 // compositions of a block
  u64 first_special_row, total_specials;   // (known once the regions are read)
  u32 sigma, B, K, L;
  u32 locint, loc_bitmap, loc_count, reversible;
  u32 comp_idx_bits, var_off_bits, cb_off_bits, bits_orig_pos, bits_orig_rank;
  u32 cw_bits, pre_var_idx, pre_cb_off, pre_comp_idx, pre_cw_ext;
  u32 sym_bits[PKX_MAX_SIGMA + 2], sym_off[PKX_MAX_SIGMA + 2];
};

struct PkxImage { const u8 *p; u64 bytes; };

PKX_HD void pkx_fail(u32 *err, u32 code) { if (*err == PKX_OK) *err = code; }

// THE accessor: w <= 64 bits at bit position `bit`, most significant first
// (gt_bsGetUInt64), of a section that ends at end_bit; anything else is PKX_E_READ
PKX_HD u64 pkx_take(const PkxImage &im, u64 end_bit, u64 bit, u32 w, u32 *err) {
  if (w == 0) return 0;
  if (w > 64 || end_bit > im.bytes * 8 || bit > end_bit || end_bit - bit < w) { pkx_fail(err, PKX_E_READ); return 0; }
  const u64 byte = bit >> 3;
  const u32 o = (u32) (bit & 7), nbytes = (o + w + 7) >> 3;     // <= 9
  u64 acc = 0;
  const u32 first = nbytes < 8 ? nbytes : 8;
  for (u32 k = 0; k < first; k++) acc = (acc << 8) | im.p[byte + k];
  if (nbytes <= 8) {
    const u64 v = acc >> (8 * nbytes - o - w);
    return w == 64 ? v : v & ((1ull << w) - 1);
  }
  const u32 r = o + w - 64;                                     // 1..7 bits of the ninth byte
  const u64 hi = acc & (~0ull >> o);
  return (hi << r) | (u64) (im.p[byte + 8] >> (8 - r));
}

// the regions of specials as the host read them from the list: rows
// [start[i], start[i] + pre[i + 1] - pre[i]) hold special sym[i] (0 wildcard, 1
// separator); increasing, apart, inside the rows; pre[n] = all special rows
struct PkxRegions { const u32 *start; const u32 *pre; const u8 *sym; u32 n; };

PKX_HD u64 pkx_region_end(const PkxRegions &rg, u32 i) { return (u64) rg.start[i] + (rg.pre[i + 1] - rg.pre[i]); }
// the first region that ends behind row, n for none
PKX_HD u32 pkx_region_from(const PkxRegions &rg, u64 row) {
  u32 lo = 0, hi = rg.n;
  while (lo < hi) {
    const u32 mid = lo + (hi - lo) / 2;
    if (pkx_region_end(rg, mid) > row) hi = mid; else lo = mid + 1;
  }
  return lo;
}

// ---- composition index -> letter counts: the table, built once per geometry --
// The compositions in ascending order of (count of letter 0, count of letter 1,
// ...), from (0, ..., 0, B): src/match/eis-seqblocktranslate.c:156-246.
// tab: ncomp x sigma counts.
static inline void pkx_comp_table(u32 sigma, u32 B, u8 *tab) {
  u8 c[PKX_MAX_SIGMA + 2];
  memset(c, 0, sizeof c);
  c[sigma - 1] = (u8) B;
  for (u64 idx = 0;; idx++) {
    memcpy(tab + idx * sigma, c, sigma);
    int j;
    u32 rest;
    if (c[sigma - 1] > 0) { j = (int) sigma - 2; rest = c[sigma - 1]; }
    else {
      int k = (int) sigma - 2;
      while (k >= 0 && c[k] == 0) k--;
      j = k - 1;
      rest = k >= 0 ? c[k] : 0;
      if (k >= 0) c[k] = 0;
    }
    if (j < 0) return;
    c[j]++;
    c[sigma - 1] = (u8) (rest - 1);
  }
}

// ---- permutation index -> the letters of a block -------------------------------
// inverse of gt_block2IndexPair, src/match/eis-seqblocktranslate.c:436-540: of
// the m arrangements of what is left, m * cnt[s] / left start with letter s
PKX_HD bool pkx_unrank(const u8 *cnt_in, u32 sigma, u32 B, u64 perm, u64 m, u8 *out) {
  u8 cnt[PKX_MAX_SIGMA + 2];
  for (u32 s = 0; s < sigma; s++) cnt[s] = cnt_in[s];
  u32 left = B;
  for (u32 i = 0; i < B; i++, left--) {
    u32 s = 0;
    for (; s < sigma; s++) {
      if (cnt[s] == 0) continue;
      const u64 ways = m * cnt[s] / left;
      if (perm < ways) { m = ways; break; }
      perm -= ways;
    }
    if (s == sigma) return false;
    cnt[s]--;
    out[i] = (u8) s;
  }
  return true;
}

PKX_HD u32 pkx_bucket_len(const PkxGeom &g, u64 bucket) {
  const u64 bpos = bucket * g.L;
  return g.N > bpos ? (u32) (g.N - bpos < g.L ? g.N - bpos : g.L) : 0;
}

// The var offset of a bucket.  The reference's bound for the size of the var
// parts can be too small (locBitsUpperBounds counts one mark per special where a
// special between letters makes two), and gt_bsStoreUInt64 then keeps the low
// var_off_bits bits of an offset: the fields wrap.  The offsets increase and a
// var part is shorter than 2^var_off_bits, so the lost upper bits of a bucket
// are the number of times the field decreases up to it: wraps[bucket], from a
// scan over pkx_wrap_flag, or nullptr when the var parts are shorter than that.
PKX_HD u64 pkx_var_field(const PkxGeom &g, const PkxImage &im, u64 bucket, u32 *err) {
  return pkx_take(im, g.cw_end_bit, g.cw_base_bit + bucket * g.cw_bits + g.pre_var_idx, g.var_off_bits, err);
}
PKX_HD u32 pkx_wrap_flag(const PkxGeom &g, const PkxImage &im, u64 bucket, u32 *err) {
  return bucket > 0 && pkx_var_field(g, im, bucket, err) < pkx_var_field(g, im, bucket - 1, err);
}
PKX_HD bool pkx_offsets_wrap(const PkxGeom &g) {
  return g.var_off_bits < 64 && ((g.var_end_bit - g.var_base_bit) >> g.var_off_bits) != 0;
}
PKX_HD u64 pkx_var_offset(const PkxGeom &g, const PkxImage &im, const u32 *wraps, u64 bucket, u32 *err) {
  const u64 v = pkx_var_field(g, im, bucket, err);
  return wraps != nullptr ? v + ((u64) wraps[bucket] << g.var_off_bits) : v;
}

// The var part of `bucket` ends at bit `end`: there the one of the next bucket
// begins, or, behind the last bucket with rows, the var parts end within a byte
// (a last bucket without rows holds at most the one bit of its mark count).
// This is what pins a var offset and a mark count: whoever lies about one
// moves the end of a var part.
PKX_HD void pkx_check_var_end(const PkxGeom &g, const PkxImage &im, const u32 *wraps, u64 bucket, u64 end, u32 *err) {
  if (*err) return;
  if (bucket + 1 < g.nb) {
    const u64 next = pkx_var_offset(g, im, wraps, bucket + 1, err);
    if (*err == PKX_OK && (next > g.var_end_bit - g.var_base_bit || g.var_base_bit + next != end))
      pkx_fail(err, PKX_E_VARCHAIN);
  } else if (end > g.var_end_bit || g.var_end_bit - end >= 8)
    pkx_fail(err, PKX_E_VARCHAIN);
}

// ---- one bucket: its rows ------------------------------------------------------
// sink.row(row, code, run): code 0..sigma-1 / 254 / 255 of the row and run[s],
// the letters s in the rows before it; sink.end(run) behind the last row of all.
template <class Sink>
PKX_HD void pkx_decode_bucket(const PkxGeom &g, const PkxImage &im, const u8 *comp_tab, const PkxRegions &rg,
                              const u32 *wraps, u64 bucket, Sink &sink, u32 *err) {
  const u64 bpos = bucket * g.L;
  const u32 len = pkx_bucket_len(g, bucket);
  if (len == 0) return;
  const u32 nblk = (len + g.B - 1) / g.B;
  const u64 cwbit = g.cw_base_bit + bucket * g.cw_bits;
  u32 run[PKX_MAX_SIGMA + 2];
  for (u32 s = 0; s < g.sigma; s++) {
    const u64 v = pkx_take(im, g.cw_end_bit, cwbit + g.sym_off[s], g.sym_bits[s], err);
    if (v > bpos) { pkx_fail(err, PKX_E_COUNTER); return; }
    run[s] = (u32) v;
  }
  const u64 var_off = pkx_var_offset(g, im, wraps, bucket, err);
  if (*err) return;
  if (var_off > g.var_end_bit - g.var_base_bit) { pkx_fail(err, PKX_E_VAROFF); return; }
  u64 vbit = g.var_base_bit + var_off;
  u32 ri = pkx_region_from(rg, bpos);
  u32 pb_sum = 0;
  for (u32 b = 0; b < nblk; b++) {
    const u64 comp = pkx_take(im, g.cw_end_bit, cwbit + g.pre_comp_idx + b * g.comp_idx_bits, g.comp_idx_bits, err);
    if (*err) return;
    if (comp >= g.ncomp) { pkx_fail(err, PKX_E_COMP); return; }
    const u8 *cnt = comp_tab + comp * g.sigma;
    const u64 m = pkx_arrangements(cnt, g.sigma, g.B);
    const u32 pb = m > 1 ? pkx_reqbits(m - 1) : 0;
    const u64 perm = pkx_take(im, g.var_end_bit, vbit, pb, err);
    if (*err) return;
    vbit += pb;
    pb_sum += pb;
    u8 blk[PKX_MAX_BLOCK];
    if (perm >= m || !pkx_unrank(cnt, g.sigma, g.B, perm, m, blk)) { pkx_fail(err, PKX_E_PERM); return; }
    for (u32 i = 0; i < g.B && b * g.B + i < len; i++) {
      const u64 row = bpos + b * g.B + i;
      u32 code = blk[i];
      while (ri < rg.n && pkx_region_end(rg, ri) <= row) ri++;
      if (ri < rg.n && row >= rg.start[ri]) code = 254u + rg.sym[ri];   // stored as letter 0
      sink.row(row, code, run);
      if (code < 254) run[code]++;
    }
  }
  if (g.locint && pb_sum != pkx_take(im, g.cw_end_bit, cwbit + g.pre_cb_off, g.cb_off_bits, err)) {
    pkx_fail(err, PKX_E_PERMBITS);
    return;
  }
  if (!g.locint) pkx_check_var_end(g, im, wraps, bucket, vbit, err);    // (else pkx_bucket_marks does, behind the marks)
  if (*err) return;
  if (bpos + len == g.N) sink.end(run);
}

// ---- one bucket: its locate records --------------------------------------------
// addLocateInfo, src/match/eis-bwtseq-extinfo.c:384-541.  sink.mark(row, value):
// a marked row and the number stored for it; sink.sprank(region, row, rank):
// -sprank, the stored rank of the special in `row` of region `region`.
template <class Sink>
PKX_HD void pkx_bucket_marks(const PkxGeom &g, const PkxImage &im, const PkxRegions &rg, const u32 *wraps, u64 bucket,
                             Sink &sink, u32 *err) {
  if (!g.locint) return;
  const u64 bpos = bucket * g.L;
  const u32 len = pkx_bucket_len(g, bucket);
  if (len == 0) return;
  const u64 cwbit = g.cw_base_bit + bucket * g.cw_bits;
  const u64 var_off = pkx_var_offset(g, im, wraps, bucket, err);
  const u64 cb = pkx_take(im, g.cw_end_bit, cwbit + g.pre_cb_off, g.cb_off_bits, err);
  if (*err) return;
  const u64 var_bits = g.var_end_bit - g.var_base_bit;
  if (var_off > var_bits || cb > var_bits - var_off) { pkx_fail(err, PKX_E_VAROFF); return; }
  u64 at = g.var_base_bit + var_off + cb;
  const u64 scale = g.reversible ? g.locint : 1;
  if (g.loc_count) {
    const u32 bc = pkx_reqbits(len), bw = pkx_reqbits((u64) len - 1);
    const u64 nm = pkx_take(im, g.var_end_bit, at, bc, err);
    if (*err) return;
    at += bc;
    if (nm > len) { pkx_fail(err, PKX_E_MARKCOUNT); return; }
    u64 next = 0;                                   // the least row the next mark may have
    for (u64 k = 0; k < nm; k++) {
      const u64 off = pkx_take(im, g.var_end_bit, at, bw, err);
      const u64 val = pkx_take(im, g.var_end_bit, at + bw, g.bits_orig_pos, err);
      if (*err) return;
      at += bw + g.bits_orig_pos;
      if (off < next || off >= len) { pkx_fail(err, PKX_E_MARKROW); return; }
      if (val > (g.N - 1) / scale) { pkx_fail(err, PKX_E_MARKVALUE); return; }
      next = off + 1;
      sink.mark(bpos + off, val);
    }
  } else {
    for (u32 o0 = 0; o0 < len; o0 += 64) {
      const u32 cnt = len - o0 < 64 ? len - o0 : 64;
      u64 bits = pkx_take(im, g.cw_end_bit, cwbit + g.pre_cw_ext + o0, cnt, err) << (64 - cnt);
      if (*err) return;
      for (u32 i = 0; bits; i++, bits <<= 1)
        if (bits >> 63) {
          const u64 val = pkx_take(im, g.var_end_bit, at, g.bits_orig_pos, err);
          if (*err) return;
          at += g.bits_orig_pos;
          if (val > (g.N - 1) / scale) { pkx_fail(err, PKX_E_MARKVALUE); return; }
          sink.mark(bpos + o0 + i, val);
        }
    }
  }
  if (g.bits_orig_rank)
    for (u32 ri = pkx_region_from(rg, bpos); ri < rg.n && rg.start[ri] < bpos + len; ri++) {
      const u64 a = rg.start[ri] > bpos ? rg.start[ri] : bpos;
      const u64 e = pkx_region_end(rg, ri) < bpos + len ? pkx_region_end(rg, ri) : bpos + len;
      for (u64 row = a; row < e; row++) {
        const u64 rank = pkx_take(im, g.var_end_bit, at, g.bits_orig_rank, err);
        if (*err) return;
        at += g.bits_orig_rank;
        if (rank > g.total_specials) { pkx_fail(err, PKX_E_SPRANK); return; }
        sink.sprank(ri, row, rank);
      }
    }
  pkx_check_var_end(g, im, wraps, bucket, at, err);
}

// ================================================================================
// the host half: headers and region list
// ================================================================================
#define PKX_REFUSE(...)                                  \
  do {                                                   \
    snprintf(msg, msg_len, __VA_ARGS__);                 \
    return -1;                                           \
  } while (0)

static inline u32 pkx_le32(const u8 *p) { u32 v; memcpy(&v, p, 4); return v; }
static inline u64 pkx_le64(const u8 *p) { u64 v; memcpy(&v, p, 8); return v; }

// The headers of an image of `bytes` bytes, of which the first head_bytes are at
// head (all of them up to the first record are wanted: 8192 do for every
// alphabet the builder accepts).  writeIdxHeader src/match/eis-blockcomp.c:
// 1984-2094, writeLocateInfoHeader / writeRankSortHeader eis-bwtseq-extinfo.c:
// 59-122.  0, or -1 and a message.
static inline int pkx_parse_header(const u8 *head, u64 head_bytes, u64 bytes, PkxGeom *g, char *msg, size_t msg_len) {
  memset(g, 0, sizeof *g);
  g->bytes = bytes;
  u64 o = 0;
  const u64 avail = head_bytes < bytes ? head_bytes : bytes;
#define PKX_NEED(n) \
  if (avail - o < (n)) PKX_REFUSE("packed index reader: the image of %llu bytes ends inside its header", (unsigned long long) bytes)
#define PKX_TAG(tag, name)                                                                                   \
  do {                                                                                                       \
    PKX_NEED(4);                                                                                             \
    if (pkx_le32(head + o) != (tag))                                                                         \
      PKX_REFUSE("packed index reader: header field %s expected at byte %llu, tag 0x%08x found", name,       \
                 (unsigned long long) o, pkx_le32(head + o));                                                \
    o += 4;                                                                                                  \
  } while (0)
  if (avail < 8) PKX_REFUSE("packed index reader: the image of %llu bytes ends inside its header", (unsigned long long) bytes);
  if (memcmp(head, "BDX", 4) != 0) PKX_REFUSE("packed index reader: not a packed index (no BDX magic)");
  const u32 header_size = pkx_le32(head + 4);
  o = 8;
  u64 var_data_pos, header_len;
  u32 spbt;
  PKX_TAG(0x424b535a, "BKSZ"); PKX_NEED(4); g->B = pkx_le32(head + o); o += 4;
  PKX_TAG(0x42424c4b, "BBLK"); PKX_NEED(4); g->K = pkx_le32(head + o); o += 4;
  PKX_TAG(0x564f4646, "VOFF"); PKX_NEED(8); var_data_pos = pkx_le64(head + o); o += 8;
  PKX_TAG(0x524f4646, "ROFF"); PKX_NEED(8); g->range_enc_pos = pkx_le64(head + o); o += 8;
  PKX_TAG(0x53454c45, "SELE"); PKX_NEED(8); g->N = pkx_le64(head + o); o += 8;
  PKX_TAG(0x53504254, "SPBT"); PKX_NEED(4); spbt = pkx_le32(head + o); o += 4;
  PKX_TAG(0x56444f42, "VDOB"); PKX_NEED(4); g->var_off_bits = pkx_le32(head + o); o += 4;
  PKX_TAG(0x53534254, "SSBT"); PKX_NEED(4); g->sigma = pkx_le32(head + o); o += 4;
  if (g->B < 1 || g->B > PKX_MAX_BLOCK)
    PKX_REFUSE("packed index reader: block size %u, 1 to %u expected", g->B, PKX_MAX_BLOCK);
  if (g->K < 1 || g->K > PKX_MAX_BUCKET / g->B)
    PKX_REFUSE("packed index reader: %u blocks of %u positions in a bucket, at most %u positions expected", g->K, g->B,
               PKX_MAX_BUCKET);
  g->L = g->B * g->K;
  if (g->N < 2 || g->N > PKX_MAX_ROWS)
    PKX_REFUSE("packed index reader: sequence of %llu rows, 2 to %llu expected (an index beyond the limit of a "
               "single build is not read)", (unsigned long long) g->N, (unsigned long long) PKX_MAX_ROWS);
  if (g->sigma < 2 || g->sigma > PKX_MAX_SIGMA)
    PKX_REFUSE("packed index reader: an alphabet of %u letters, 2 to %u expected", g->sigma, PKX_MAX_SIGMA);
  if (spbt != pkx_reqbits(g->N - 1))
    PKX_REFUSE("packed index reader: %u bits per position stated, %llu rows need %u", spbt,
               (unsigned long long) g->N, pkx_reqbits(g->N - 1));
  if (g->var_off_bits < 1 || g->var_off_bits > 64)
    PKX_REFUSE("packed index reader: var offsets of %u bits, 1 to 64 expected", g->var_off_bits);
  u32 off = 0;
  for (u32 s = 0; s < g->sigma; s++) {
    PKX_NEED(4);
    g->sym_bits[s] = pkx_le32(head + o); o += 4;
    if (g->sym_bits[s] < 1 || g->sym_bits[s] > spbt)
      PKX_REFUSE("packed index reader: occurrence counter of letter %u has %u bits, 1 to %u expected", s,
                 g->sym_bits[s], spbt);
    g->sym_off[s] = off;
    off += g->sym_bits[s];
  }
  PKX_TAG(0x42454642, "BEFB"); PKX_NEED(4);
  if (pkx_le32(head + o) != 0) PKX_REFUSE("packed index reader: block-encoded ranges (BEFB %u) are not read", pkx_le32(head + o));
  o += 4;
  PKX_TAG(0x52454642, "REFB"); PKX_NEED(4);
  if (pkx_le32(head + o) != 0) PKX_REFUSE("packed index reader: region-encoded ranges (REFB %u) are not read", pkx_le32(head + o));
  o += 4;
  PKX_TAG(0x4e4d524e, "NMRN"); PKX_NEED(12);
  if (pkx_le32(head + o) != 2 || pkx_le32(head + o + 4) != 1 || pkx_le32(head + o + 8) != 2)
    PKX_REFUSE("packed index reader: range modes (%u: %u, %u), letters in blocks and specials in regions (2: 1, 2) expected",
               pkx_le32(head + o), pkx_le32(head + o + 4), pkx_le32(head + o + 8));
  o += 12;
  // widths the geometry implies: gt_newGenBlockEncIdxSeq eis-blockcomp.c:336-339, 477-501
  g->ncomp = pkx_binom(g->B + g->sigma - 1, g->sigma - 1);
  g->comp_idx_bits = pkx_reqbits(g->ncomp - 1);
  u8 even[PKX_MAX_SIGMA + 2];
  for (u32 s = 0; s < g->sigma; s++) even[s] = (u8) (g->B / g->sigma + (s < g->B % g->sigma ? 1u : 0u));
  const u32 max_perm_bits = pkx_reqbits(pkx_arrangements(even, g->sigma, g->B) - 1);
  if (g->comp_idx_bits > PKX_MAX_COMP_BITS || max_perm_bits > PKX_MAX_PERM_BITS)
    PKX_REFUSE("packed index reader: block size %u over %u letters needs wider indices than the device builder packs",
               g->B, g->sigma);
  u64 cw_ext_bits = 0;
  const bool has_ext = avail - o >= 4 && pkx_le32(head + o) == 0x43424d42;
  if (has_ext) {
    o += 4; PKX_NEED(4); g->cb_off_bits = pkx_le32(head + o); o += 4;
    PKX_TAG(0x43455842, "CEXB"); PKX_NEED(8); cw_ext_bits = pkx_le64(head + o); o += 8;
    PKX_TAG(0x4d455842, "MEXB"); PKX_NEED(8); o += 8;
    if (g->cb_off_bits != pkx_reqbits((u64) max_perm_bits * g->K))
      PKX_REFUSE("packed index reader: %u bits for the bits of a bucket's permutation indices, the geometry implies %u",
                 g->cb_off_bits, pkx_reqbits((u64) max_perm_bits * g->K));
  }
  header_len = o;
  if (header_size != (header_len + 8191) / 8192 * 8192)
    PKX_REFUSE("packed index reader: header size %u stated, its %llu bytes imply %llu", header_size,
               (unsigned long long) header_len, (unsigned long long) ((header_len + 8191) / 8192 * 8192));
  // extension headers: locate, sort modes
  bool have_loc = false;
  while (avail - o >= 8 && (pkx_le32(head + o) >> 16) == 0x4548) {
    const u32 id = pkx_le32(head + o) & 0xffff, size = pkx_le32(head + o + 4);
    o += 8;
    if (id == 1111 && !have_loc) {
      if (size != 16) PKX_REFUSE("packed index reader: locate header of %u bytes, 16 expected", size);
      PKX_NEED(16);
      g->rot0 = pkx_le64(head + o);
      g->locint = pkx_le32(head + o + 8);
      const u32 toggles = pkx_le32(head + o + 12);
      o += 16;
      have_loc = true;
      if (g->rot0 >= g->N)
        PKX_REFUSE("packed index reader: row %llu of suffix 0 is none of the %llu rows", (unsigned long long) g->rot0,
                   (unsigned long long) g->N);
      if (g->locint < 1)
        PKX_REFUSE("packed index reader: locate interval 0 in a locate header (an index without locate information has no such header)");
      g->loc_bitmap = (toggles & 1) != 0;
      g->loc_count = (toggles & 2) != 0;
      g->reversible = (toggles & 4) != 0;
      if ((toggles & ~7u) || g->loc_bitmap == g->loc_count)
        PKX_REFUSE("packed index reader: feature toggles %u, a locate bitmap (1) or locate counts (2), with or "
                   "without reversibly sorted specials (4), expected", toggles);
    } else if (id == 1112 && have_loc && !g->bits_orig_rank) {
      if (size != 8) PKX_REFUSE("packed index reader: sort-mode header of %u bytes, 8 expected", size);
      PKX_NEED(8);
      g->bits_orig_rank = pkx_le32(head + o);
      uint16_t m0, m1;
      memcpy(&m0, head + o + 4, 2);
      memcpy(&m1, head + o + 6, 2);
      o += 8;
      if (g->bits_orig_rank < 1 || g->bits_orig_rank > 32)
        PKX_REFUSE("packed index reader: ranks of specials of %u bits, 1 to 32 expected", g->bits_orig_rank);
      if (m0 != 0 || m1 != 2)
        PKX_REFUSE("packed index reader: sort modes (%u, %u), letters by value and specials by rank (0, 2) expected", m0, m1);
    } else
      PKX_REFUSE("packed index reader: extension header %u at byte %llu is not known here", id, (unsigned long long) (o - 8));
  }
  if (has_ext != have_loc)
    PKX_REFUSE("packed index reader: the header %s locate fields, the locate header is %s",
               has_ext ? "has" : "lacks", have_loc ? "present" : "absent");
  if (g->reversible != (g->bits_orig_rank != 0))
    PKX_REFUSE("packed index reader: reversibly sorted specials %s, their sort-mode header is %s",
               g->reversible ? "stated" : "not stated", g->bits_orig_rank ? "present" : "absent");
  if (cw_ext_bits != (g->loc_bitmap ? g->L : 0))
    PKX_REFUSE("packed index reader: %llu extension bits in a record, the locate flavour implies %u",
               (unsigned long long) cw_ext_bits, g->loc_bitmap ? g->L : 0);
  if (g->locint) g->bits_orig_pos = pkx_reqbits(g->reversible ? (g->N - 1) / g->locint : g->N - 1);
  // the sections: records, var parts, region list, in this order, inside the image
  g->pre_var_idx = off;
  g->pre_cb_off = g->pre_var_idx + g->var_off_bits;
  g->pre_comp_idx = g->pre_cb_off + g->cb_off_bits;
  g->pre_cw_ext = g->pre_comp_idx + g->comp_idx_bits * g->K;
  g->cw_bits = g->pre_cw_ext + (u32) cw_ext_bits;
  g->nb = (g->N + 1) / g->L + (((g->N + 1) % g->L) ? 1 : 0);       // numBuckets, eis-blockcomp.c:1633-1638
  const u64 cw_data_pos = (o + 8191) / 8192 * 8192;
  const u64 cw_len = ((u64) g->cw_bits * g->nb + 7) / 8;
  if (var_data_pos != cw_data_pos + cw_len)
    PKX_REFUSE("packed index reader: var parts stated at byte %llu, the %llu records of %u bits from byte %llu on "
               "end at %llu", (unsigned long long) var_data_pos, (unsigned long long) g->nb, g->cw_bits,
               (unsigned long long) cw_data_pos, (unsigned long long) (cw_data_pos + cw_len));
  if (g->range_enc_pos < var_data_pos || g->range_enc_pos > bytes || bytes - g->range_enc_pos < 24)
    PKX_REFUSE("packed index reader: region list stated at byte %llu, between the var parts at %llu and the end of "
               "the image at %llu (less a list of one record) expected", (unsigned long long) g->range_enc_pos,
               (unsigned long long) var_data_pos, (unsigned long long) bytes);
  g->cw_base_bit = cw_data_pos * 8;
  g->cw_end_bit = g->cw_base_bit + (u64) g->cw_bits * g->nb;
  g->var_base_bit = var_data_pos * 8;
  g->var_end_bit = g->range_enc_pos * 8;
  return 0;
#undef PKX_TAG
#undef PKX_NEED
}

// The region list, gt_SRLSaveToStream src/match/eis-seqranges.c:459-468: list =
// the bytes of the image from g->range_enc_pos on.  Fills the three arrays (pre
// with one entry more) and what of g depends on them.
static inline int pkx_parse_regions(const u8 *list, u64 list_bytes, PkxGeom *g, std::vector<u32> &start,
                                    std::vector<u32> &pre, std::vector<u8> &sym, char *msg, size_t msg_len) {
  if (list_bytes != g->bytes - g->range_enc_pos || list_bytes < 24)
    PKX_REFUSE("packed index reader: %llu bytes of region list given, the image has %llu",
               (unsigned long long) list_bytes, (unsigned long long) (g->bytes - g->range_enc_pos));
  const u64 nr = pkx_le64(list);
  if (nr < 1 || nr > g->N + 1 || list_bytes != 8 + 16 * nr)
    PKX_REFUSE("packed index reader: %llu region records stated, the %llu bytes behind byte %llu hold %llu",
               (unsigned long long) nr, (unsigned long long) list_bytes, (unsigned long long) g->range_enc_pos,
               (unsigned long long) ((list_bytes - 8) / 16));
  g->nregions = nr - 1;
  start.assign((size_t) g->nregions, 0);
  pre.assign((size_t) g->nregions + 1, 0);
  sym.assign((size_t) g->nregions, 0);
  u64 end = 0, total = 0;
  for (u64 i = 0; i < nr; i++) {
    const u8 *r = list + 8 + 16 * i;
    const u64 st = pkx_le64(r);
    u64 be = 0;
    for (int k = 0; k < 8; k++) be = (be << 8) | r[8 + k];
    const u64 len = be & ~(1ull << 63);
    if (i + 1 == nr) {          // the closing record just beyond the sequence, eis-blockcomp.c:2461-2464
      if (st < g->N) PKX_REFUSE("packed index reader: the closing region record starts at row %llu of %llu", (unsigned long long) st, (unsigned long long) g->N);
      break;
    }
    if (st < end || (i && st == end && sym[(size_t) i - 1] == (u8) (be >> 63)) || len < 1 || st >= g->N || len > g->N - st)
      PKX_REFUSE("packed index reader: region record %llu (rows %llu, +%llu) does not follow the one before inside the %llu rows",
                 (unsigned long long) i, (unsigned long long) st, (unsigned long long) len, (unsigned long long) g->N);
    start[(size_t) i] = (u32) st;
    pre[(size_t) i] = (u32) total;
    sym[(size_t) i] = (u8) (be >> 63);
    end = st + len;
    total += len;
  }
  pre[(size_t) g->nregions] = (u32) total;
  if (total < 1 || total > g->N)
    PKX_REFUSE("packed index reader: %llu special rows in the region list of %llu rows", (unsigned long long) total, (unsigned long long) g->N);
  g->first_special_row = g->N - total;
  g->total_specials = total - 1;          // the undefined symbol before suffix 0 is one of the rows
  if (g->locint) {
    // the terminator row holds a wildcard: the undefined symbol
    PkxRegions rg = { start.data(), pre.data(), sym.data(), (u32) g->nregions };
    const u32 ri = pkx_region_from(rg, g->rot0);
    if (ri >= rg.n || rg.start[ri] > g->rot0 || rg.sym[ri] != 0)
      PKX_REFUSE("packed index reader: row %llu of suffix 0 holds no special in the region list", (unsigned long long) g->rot0);
  }
  if (g->bits_orig_rank && g->bits_orig_rank != pkx_reqbits(g->total_specials))
    PKX_REFUSE("packed index reader: ranks of specials of %u bits, the %llu specials imply %u", g->bits_orig_rank,
               (unsigned long long) g->total_specials, pkx_reqbits(g->total_specials));
  return 0;
}
#undef PKX_REFUSE
