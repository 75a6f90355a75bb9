// pckidx_core_shim.cpp -- TEST INFRASTRUCTURE: genometools_amd/csrc/esa_pckidx_core.h,
// the code the lanes of esa_pckidx.hip run, compiled with g++ for the CPU.  As a
// shared library for tests/test_pckidx_core.py; with -DPKX_SHIM_MAIN as a program
// of its own (built with the sanitizers there): pckidx_core_shim FILE... decodes
// every bucket and every locate record of each image and prints one line per
// file: path, 0 or -1, the error word, the message.
#include <stdio.h>
#include <stdlib.h>
#include <string>
#include <vector>
#include "../genometools_amd/csrc/esa_pckidx_core.h"

namespace {

struct Shim {
  std::vector<u8> image, comp_tab, sym;
  std::vector<u32> start, pre, wrap_count;
  PkxGeom g;
  const u32 *wraps() const { return wrap_count.empty() ? nullptr : wrap_count.data(); }
  PkxImage im() const { return PkxImage{ image.data(), image.size() }; }
  PkxRegions rg() const { return PkxRegions{ start.data(), pre.data(), sym.data(), (u32) g.nregions }; }
};

constexpr u32 SHIM_E_COUNTERS = 200;   // the counters of a record are not the letters before its bucket
constexpr u32 SHIM_E_ROWS = 201;       // rows left out or visited twice

struct RowSink {
  u8 *bwt; u64 *totals; u64 next; u64 seen[PKX_MAX_SIGMA + 2]; u32 sigma; u32 err; bool ended;
  void row(u64 r, u32 code, const u32 *run) {
    if (r != next) err = err ? err : SHIM_E_ROWS;
    next = r + 1;
    for (u32 s = 0; s < sigma; s++)
      if (run[s] != seen[s]) err = err ? err : SHIM_E_COUNTERS;
    if (code < 254) seen[code]++;
    bwt[r] = (u8) code;
  }
  void end(const u32 *run) {
    ended = true;
    for (u32 s = 0; s < sigma; s++) totals[s] = run[s];
  }
};

struct MarkSink {
  u64 *stored, *rank, scale;
  void mark(u64 row, u64 val) { stored[row] = val * scale; }
  void sprank(u32, u64 row, u64 r) { rank[row] = r; }
};

Shim *open_image(const u8 *img, u64 bytes, char *msg, size_t msg_len) {
  Shim *h = new Shim();
  h->image.assign(img, img + bytes);
  const u64 head = bytes < 8192 ? bytes : 8192;
  if (pkx_parse_header(h->image.data(), head, bytes, &h->g, msg, msg_len) != 0 ||
      pkx_parse_regions(h->image.data() + h->g.range_enc_pos, bytes - h->g.range_enc_pos, &h->g, h->start, h->pre,
                        h->sym, msg, msg_len) != 0) {
    delete h;
    return nullptr;
  }
  h->comp_tab.resize((size_t) (h->g.ncomp * h->g.sigma));
  pkx_comp_table(h->g.sigma, h->g.B, h->comp_tab.data());
  if (pkx_offsets_wrap(h->g)) {
    u32 err = PKX_OK, sum = 0;
    h->wrap_count.resize((size_t) h->g.nb);
    for (u64 b = 0; b < h->g.nb; b++) h->wrap_count[(size_t) b] = sum += pkx_wrap_flag(h->g, h->im(), b, &err);
  }
  return h;
}

}  // namespace

extern "C" {

void *pkx_shim_open(const u8 *img, u64 bytes, char *msg, size_t msg_len) { return open_image(img, bytes, msg, msg_len); }
void pkx_shim_close(void *h) { delete (Shim *) h; }

// rows, buckets, sigma, B, K, locate interval, bitmap, counts, reversible, rot0,
// first special row, regions; then what a test needs to find a field of a bucket:
// cw_base_bit, cw_bits, pre_var_idx, var_off_bits, pre_cb_off, cb_off_bits,
// var_base_bit, var_end_bit, bits_orig_pos, bits_orig_rank, pre_cw_ext, range_enc_pos
void pkx_shim_geom(const void *hv, u64 *out) {
  const PkxGeom &g = ((const Shim *) hv)->g;
  const u64 v[] = { g.N, g.nb, g.sigma, g.B, g.K, g.locint, g.loc_bitmap, g.loc_count, g.reversible, g.rot0,
                    g.first_special_row, g.nregions, g.cw_base_bit, g.cw_bits, g.pre_var_idx, g.var_off_bits,
                    g.pre_cb_off, g.cb_off_bits, g.var_base_bit, g.var_end_bit, g.bits_orig_pos, g.bits_orig_rank,
                    g.pre_cw_ext, g.range_enc_pos, (u64) pkx_offsets_wrap(g) };
  memcpy(out, v, sizeof v);
}

// every bucket: the rows -> bwt[N], the totals of the letters -> totals[sigma];
// the error word of the first bucket that has one (0: none)
u32 pkx_shim_decode(const void *hv, u8 *bwt, u64 *totals) {
  const Shim *h = (const Shim *) hv;
  RowSink sink = { bwt, totals, 0, { 0 }, h->g.sigma, 0, false };
  for (u64 b = 0; b < h->g.nb; b++) {
    u32 err = PKX_OK;
    pkx_decode_bucket(h->g, h->im(), h->comp_tab.data(), h->rg(), h->wraps(), b, sink, &err);
    if (err) return err;
    if (sink.err) return sink.err;
  }
  return sink.next == h->g.N && sink.ended ? 0 : SHIM_E_ROWS;
}

// every bucket: stored[row] = the text position stored for a marked row (else
// untouched), rank[row] = the stored rank of a special row (-sprank)
u32 pkx_shim_marks(const void *hv, u64 *stored, u64 *rank) {
  const Shim *h = (const Shim *) hv;
  MarkSink sink = { stored, rank, h->g.reversible ? h->g.locint : 1 };
  for (u64 b = 0; b < h->g.nb; b++) {
    u32 err = PKX_OK;
    pkx_bucket_marks(h->g, h->im(), h->rg(), h->wraps(), b, sink, &err);
    if (err) return err;
  }
  return 0;
}

const char *pkx_shim_error_text(u32 e) { return pkx_error_text(e); }

}  // extern "C"

#ifdef PKX_SHIM_MAIN
int main(int argc, char **argv) {
  for (int a = 1; a < argc; a++) {
    FILE *f = fopen(argv[a], "rb");
    if (f == nullptr) { printf("%s\t-1\t0\tcannot open\n", argv[a]); continue; }
    std::vector<u8> img;
    u8 buf[65536];
    size_t got;
    while ((got = fread(buf, 1, sizeof buf, f)) > 0) img.insert(img.end(), buf, buf + got);
    fclose(f);
    char msg[512] = "";
    Shim *h = open_image(img.data(), img.size(), msg, sizeof msg);
    if (h == nullptr) { printf("%s\t-1\t0\t%s\n", argv[a], msg); continue; }
    std::vector<u8> bwt((size_t) h->g.N);
    std::vector<u64> totals(PKX_MAX_SIGMA + 2), stored((size_t) h->g.N, ~0ull), rank((size_t) h->g.N, ~0ull);
    u32 err = pkx_shim_decode(h, bwt.data(), totals.data());
    if (err == 0) err = pkx_shim_marks(h, stored.data(), rank.data());
    printf("%s\t%d\t%u\t%s\n", argv[a], err ? -1 : 0, err, pkx_error_text(err));
    pkx_shim_close(h);
  }
  return 0;
}
#endif
