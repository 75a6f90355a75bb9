// esa_index.h -- the host side that the consumers of a resident index share: the
// checker, the matching statistics, the maximal pairs, the query matches, the
// suffix-prefix matches (all and irreducible), the tag matches and the local
// alignments (esa_check.hip, esa_mstat.hip, esa_maxpairs.hip, esa_qmatch.hip,
// esa_spm.hip, esa_spmred.hip, esa_tagmatch.hip, esa_locali.hip).  A new consumer
// starts here: its object is a ConsumerBase with a ResidentIndex -- an IndexSlot
// if a reader of the packed index may be its index too -- made by
// create_consumer; what it reads back goes through fetch, the records it hands
// out through a RecordStage, after refuse_window; the 64-bit places of its
// records are offsets_u64 of esa_prims.h.  One that walks the intervals of .suf,
// or of the rows of a packed index, job by job goes on in esa_jobs.h.
//
// `feature` is what a message starts with ("maximal pairs").  Only .hip files
// include this header: the *_core.h, *_search.h and *_walk.h lane headers also
// compile with g++ alone.
#pragma once
#include <initializer_list>
#include "esa_own.h"
#include "esa_pckidx.h"
#include "../../include/gtamd_esa.h"

// ---- device to host ------------------------------------------------------------
struct Fetch { const void *src; void *dst; u64 bytes; };

// The copies (an item of 0 bytes is none), then one wait for the stream, which is
// idle when this returns, with an error too: no copy is still on its way into a
// frame that has been left.
static inline int fetch(hipStream_t st, std::initializer_list<Fetch> items) {
  hipError_t copied = hipSuccess;
  for (const Fetch &f : items)
    if (copied == hipSuccess && f.bytes) copied = hipMemcpyAsync(f.dst, f.src, f.bytes, hipMemcpyDeviceToHost, st);
  const hipError_t waited = hipStreamSynchronize(st);
  HIP_TRY(copied);
  HIP_TRY(waited);
  return 0;
}

// Records of a consumer on their way out.  begin: dst is where `most` of them are
// written, the caller's device memory or `buf`, grown to hold them.  finish: `count`
// of them are in the caller's memory and the stream is idle.
template <typename R> struct RecordStage {
  static_assert(sizeof(R) % 8 == 0, "a record is a whole number of 64-bit numbers");
  void *out;
  bool on_device;
  R *dst;
  RecordStage(void *out_, int out_on_device) : out(out_), on_device(out_on_device != 0), dst((R *) out_) {}
  hipError_t begin(Dev<u8> &buf, u64 most) {
    if (on_device) return hipSuccess;
    const hipError_t e = buf.grow(most * sizeof(R));
    dst = (R *) buf.p;
    return e;
  }
  int finish(u64 count, hipStream_t st) {
    return fetch(st, { { dst, out, on_device ? 0 : count * sizeof(R) } });
  }
};

// device memory for `entries` of something (`of`: "records") is not to be had
static inline int out_of_memory(const char *feature, u64 entries, const char *of) {
  gtamd_set_error("%s: cannot allocate device memory for %llu %s", feature, (unsigned long long) entries, of);
  return -1;
}

// what every emit refuses first: a cursor that is none of `total` `noun`s, a capacity below `least`
static inline int refuse_window(const char *feature, const char *noun, u64 cur, u64 total, u64 capacity, u64 least) {
  if (cur > total) {
    gtamd_set_error("%s: cursor %llu is not one of this enumeration (%llu %s)", feature, (unsigned long long) cur,
                    (unsigned long long) total, noun);
    return -1;
  }
  if (capacity < least) {
    gtamd_set_error("%s: a capacity of %llu records is too small: a capacity of at least %llu is needed", feature,
                    (unsigned long long) capacity, (unsigned long long) least);
    return -1;
  }
  return 0;
}

// ---- host to device ------------------------------------------------------------
constexpr u64 UPLOAD_PIECE = 64ull << 20;

// host memory -> a device buffer of its own, piece by piece
template <typename T> static int upload(Dev<T> &d, const void *src, u64 bytes, const char *feature, const char *what) {
  if (d.alloc(bytes ? bytes : 1) != hipSuccess) {
    gtamd_set_error("%s: cannot allocate %llu bytes of device memory for %s", feature, (unsigned long long) bytes,
                    what);
    return -1;
  }
  for (u64 off = 0; off < bytes; off += UPLOAD_PIECE) {
    const u64 cnt = bytes - off < UPLOAD_PIECE ? bytes - off : UPLOAD_PIECE;
    HIP_TRY(hipMemcpy((u8 *) d.p + off, (const u8 *) src + off, cnt, hipMemcpyHostToDevice));
  }
  return 0;
}

// ---- the index -----------------------------------------------------------------
// n symbols, n + 1 entries of .suf and, for those that read it, of .lcp, with the
// pairs of .llv; whose memory it is the view does not say
struct IndexView {
  const u8 *enc = nullptr;
  u64 n = 0;
  const void *suf = nullptr;
  u32 suf_bytes = 0;
  const u8 *lcp = nullptr;
  const u64 *llv = nullptr;
  u64 llv_pairs = 0;
};

// what every consumer refuses in the width of the .suf entries ...
static inline int refuse_suf_bytes(const char *feature, u32 suf_bytes) {
  if (suf_bytes == 4 || suf_bytes == 8) return 0;
  gtamd_set_error("%s: .suf entries of %u bytes, 4 or 8 expected", feature, suf_bytes);
  return -1;
}

// ... and in the sizes; `verb`: what is not done with the slices of a build in parts
static inline int refuse_sizes(const char *feature, u64 n, u64 llv_pairs, const char *verb = "searched") {
  if (n >= SINGLE_LIMIT) {
    gtamd_set_error("%s: sequence of %llu symbols is beyond the limit of a single build "
                    "(%llu table entries); the slices of a build in parts are not %s",
                    feature, (unsigned long long) n, (unsigned long long) SINGLE_LIMIT, verb);
    return -1;
  }
  if (llv_pairs > n) {
    gtamd_set_error("%s: %llu .llv pairs for %llu symbols", feature, (unsigned long long) llv_pairs,
                    (unsigned long long) n);
    return -1;
  }
  return 0;
}

// The whole .suf table an engine holds after its last run, with its .lcp and .llv
// tables (with_lcp), over the n symbols at enc.  Nothing is touched.
static inline int engine_tables(const char *feature, const gtamd_esa_ctx *esa, const u8 *enc, u64 n, bool with_lcp,
                                IndexView *v, const char *verb = "searched") {
  *v = IndexView();
  v->enc = enc;
  v->n = n;
  v->suf = gtamd_esa_table_device(esa, GTAMD_TAB_SUF);
  v->suf_bytes = 8;
  if (with_lcp) {
    v->lcp = (const u8 *) gtamd_esa_table_device(esa, GTAMD_TAB_LCP);
    v->llv_pairs = gtamd_esa_table_entries(esa, GTAMD_TAB_LLV);
    v->llv = v->llv_pairs ? (const u64 *) gtamd_esa_table_device(esa, GTAMD_TAB_LLV) : nullptr;
  }
  if (v->suf == nullptr || (with_lcp && (v->lcp == nullptr || (v->llv_pairs && v->llv == nullptr)))) {
    gtamd_set_error("%s: the last run did not produce the %s", feature,
                    with_lcp ? ".suf and .lcp tables" : ".suf table");
    return -1;
  }
  if (gtamd_esa_table_offset(esa) != 0 || gtamd_esa_table_entries(esa, GTAMD_TAB_SUF) != n + 1) {
    gtamd_set_error("%s: the context holds %llu entries from table index %llu on, not the "
                    "whole table of %llu symbols; the slices of a build in parts are not %s", feature,
                    (unsigned long long) gtamd_esa_table_entries(esa, GTAMD_TAB_SUF),
                    (unsigned long long) gtamd_esa_table_offset(esa), (unsigned long long) n, verb);
    return -1;
  }
  return 0;
}

// the index of a consumer: the caller's or an engine's memory, or buffers of its own
struct ResidentIndex : IndexView {
  struct { Dev<u8> enc, suf, lcp; Dev<u64> llv; } own;      // an index set from host memory
  bool set = false;

  void drop() {
    set = false;
    own.enc.reset(); own.suf.reset(); own.lcp.reset(); own.llv.reset();
    static_cast<IndexView &>(*this) = IndexView();
  }
  // device memory that outlives the calls
  void borrow(const IndexView &v) {
    drop();
    static_cast<IndexView &>(*this) = v;
    set = true;
  }
  // host memory; .lcp and .llv where there is an .lcp table
  int upload_from_host(const char *feature, const IndexView &v) {
    drop();
    TRY(upload(own.enc, v.enc, v.n, feature, "the sequence"));
    TRY(upload(own.suf, v.suf, (v.n + 1) * v.suf_bytes, feature, "the .suf table"));
    if (v.lcp != nullptr) {
      TRY(upload(own.lcp, v.lcp, v.n + 1, feature, "the .lcp table"));
      TRY(upload(own.llv, v.llv, v.llv_pairs * 16, feature, "the .llv table"));
    }
    static_cast<IndexView &>(*this) = v;
    enc = own.enc; suf = own.suf.p; lcp = own.lcp; llv = own.llv;
    set = true;
    return 0;
  }
  u64 bytes() const { return own.enc.bytes + own.suf.bytes + own.lcp.bytes + own.llv.bytes; }
};

// The index of a consumer that a reader of the packed index may be as well: the
// tables, or the reader, never both.  `name` is the consumer's in its entry points
// (gtamd_<name>_...), `noun` what a message calls its object ("the matcher").
struct IndexSlot {
  ResidentIndex tab;
  const gtamd_pckidx *pck = nullptr;     // the index is a reader of the packed index ...
  u64 opens = 0;                         // ... and the image of it that stamp() saw

  bool is_set() const { return tab.set || pck != nullptr; }
  int refuse_unset(const char *feature, const char *name) const {
    if (is_set()) return 0;
    gtamd_set_error("%s: no index is set (gtamd_%s_set_index)", feature, name);
    return -1;
  }
  // tables: device memory that outlives the calls, or host memory
  int set_tables(const char *feature, const IndexView &v, bool from_host) {
    pck = nullptr;
    if (from_host) return tab.upload_from_host(feature, v);
    tab.borrow(v);
    return 0;
  }
  // a reader, in two steps, between which a consumer looks at the image: what
  // every consumer refuses of the reader px as the index of its object c ...
  template <typename T> static int refuse_reader(const char *feature, const char *name, const char *noun, const T *c,
                                                 const gtamd_pckidx *px) {
    if (c == nullptr || px == nullptr) { gtamd_set_error("invalid argument to gtamd_%s_set_index_pckidx", name); return -1; }
    if (!pckidx_is_open(px)) { gtamd_set_error("%s: the packed index reader has no image open", feature); return -1; }
    if (pckidx_device(px) != c->device) {
      gtamd_set_error("%s: the packed index lives on device %d, %s on %d", feature, pckidx_device(px), noun, c->device);
      return -1;
    }
    return 0;
  }
  // ... and px is the index
  void set_reader(const gtamd_pckidx *px) {
    tab.drop();
    pck = px;
  }
  // the reader that is the index must still hold the image it held when it was set
  int refuse_lost_reader(const char *feature) const {
    if (pckidx_is_open(pck)) return 0;
    gtamd_set_error("%s: the packed index reader that is the index has no image open any more "
                    "(its last gtamd_pckidx_open_* failed)", feature);
    return -1;
  }
  // positions come from the locate information of the image; tail, with what it ends in: what the caller cannot have
  int refuse_no_locate(const char *feature, const char *tail, const char *tail_end = "") const {
    if (pckidx_can_locate(pck)) return 0;
    gtamd_set_error("%s: the packed index holds no locate information (locate interval 0): %s%s", feature, tail,
                    tail_end);
    return -1;
  }
  // What a prepare leaves for later calls is of the image the reader held then:
  // stamp() at prepare, and a reader opened again since holds another one.
  void stamp() { opens = pckidx_opens(pck); }
  int refuse_other_image(const char *feature, const char *prepare_fn) const {
    if (pckidx_opens(pck) == opens) return 0;
    gtamd_set_error("%s: the packed index reader was opened again since %s: what was prepared is of the image "
                    "before (prepare again)", feature, prepare_fn);
    return -1;
  }
  u64 bytes() const { return tab.bytes() + (pck != nullptr ? pckidx_decoded_bytes(pck) : 0); }
};

// ---- the object ----------------------------------------------------------------
// what every consumer's object starts with; words: what its kernels report through
template <int EVENTS = 2> struct ConsumerBase {
  int device = 0;
  Stream st;             // (before the buffers: they go first)
  Event ev[EVENTS];
  Dev<u64> words;
};

// a T on `device` with its stream, its events and `words` words; noun: "the index checker"
template <typename T> static T *create_consumer(int device, u64 words, const char *noun) {
  if (gtamd_device_count() <= device || device < 0) {
    gtamd_set_error("no HIP device %d available (this library has no CPU fallback)", device);
    return nullptr;
  }
  if (hipSetDevice(device) != hipSuccess) { gtamd_set_error("hipSetDevice(%d) failed", device); return nullptr; }
  T *c = new T();
  c->device = device;
  bool ok = create(c->st) == hipSuccess && c->words.alloc(words * sizeof(u64)) == hipSuccess;
  for (Event &e : c->ev) ok = ok && create(e) == hipSuccess;
  if (!ok) {
    gtamd_set_error("cannot create %s on device %d", noun, device);
    delete c;
    return nullptr;
  }
  return c;
}

template <typename T> static void destroy_consumer(T *c) {
  if (c == nullptr) return;
  (void) hipSetDevice(c->device);
  (void) hipStreamSynchronize(c->st);
  delete c;
}

// *info = c->info; fn: the entry point, for the message
template <typename T, typename I> static int consumer_info(const T *c, I *info, const char *fn) {
  if (c == nullptr || info == nullptr) { gtamd_set_error("invalid argument to %s", fn); return -1; }
  *info = c->info;
  return 0;
}
