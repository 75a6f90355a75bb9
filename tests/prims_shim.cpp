// prims_shim.cpp -- TEST INFRASTRUCTURE ONLY: host glue between
// tests/test_prims_gpu.py and the device-wide primitives of
// genometools_amd/csrc/esa_prims.h as libgtamd_esa.so exports them (C++ names,
// the four explicit instances of radix_sort_pairs included).  No kernel here:
// the tests run the code object the engine runs.
//
// Every entry takes HOST arrays, holds its device buffers in the owning types
// of esa_own.h, copies in, calls ONE primitive on a stream of its own, waits for
// it and copies out.  A workspace has exactly the words its *_workspace_words
// function names, followed by GUARD words of a pattern that travel back to the
// caller.  Returns: what the primitive returned, or SHIM_FAIL where the glue
// itself could not go on (a HIP call failed, an instance code it does not know).
#include "../genometools_amd/csrc/esa_prims.h"
#include "../genometools_amd/csrc/esa_own.h"

namespace {

constexpr int GUARD = 64;
constexpr int SHIM_FAIL = -100;
constexpr u32 GUARD_SEED = 0xC0DE0000u;

#define SHIM_HIP(expr)                                                          \
  do {                                                                          \
    const hipError_t e_ = (expr);                                               \
    if (e_ != hipSuccess) {                                                     \
      fprintf(stderr, "prims_shim: %s failed: %s (line %d)\n", #expr,           \
              hipGetErrorString(e_), __LINE__);                                 \
      return SHIM_FAIL;                                                         \
    }                                                                           \
  } while (0)

// `words` words of workspace (filled with a pattern the primitive has to
// overwrite before it reads) and the guard behind them
struct Workspace {
  Dev<u32> d;
  u64 words = 0;
  int make(u64 w) {
    words = w;
    SHIM_HIP(d.alloc((w + GUARD) * sizeof(u32)));
    if (w) SHIM_HIP(hipMemset(d, 0x5A, w * sizeof(u32)));
    u32 g[GUARD];
    for (int i = 0; i < GUARD; i++) g[i] = GUARD_SEED + (u32) i;
    SHIM_HIP(hipMemcpy(d + w, g, sizeof g, hipMemcpyHostToDevice));
    return 0;
  }
  int guard_out(u32 *guard) const {
    SHIM_HIP(hipMemcpy(guard, d + words, GUARD * sizeof(u32), hipMemcpyDeviceToHost));
    return 0;
  }
};

// a device array of n + off elements; `at` is its element `off`
template <typename T> struct Shifted {
  Dev<T> d;
  T *at = nullptr;
  u64 n = 0;
  int make(u64 count, u64 off, const T *host, int fill) {
    n = count;
    SHIM_HIP(d.alloc((count + off + 1) * sizeof(T)));
    at = d + off;
    if (host != nullptr) {
      if (count) SHIM_HIP(hipMemcpy(at, host, count * sizeof(T), hipMemcpyHostToDevice));
    } else SHIM_HIP(hipMemset(d, fill, (count + off + 1) * sizeof(T)));
    return 0;
  }
  int out(T *host) const {
    if (n) SHIM_HIP(hipMemcpy(host, at, n * sizeof(T), hipMemcpyDeviceToHost));
    return 0;
  }
};

#define SHIM_TRY(...)                                                           \
  do {                                                                          \
    if ((__VA_ARGS__) != 0) return SHIM_FAIL;                                   \
  } while (0)

int finish(hipStream_t st) {
  SHIM_HIP(hipStreamSynchronize(st));
  SHIM_HIP(hipGetLastError());
  return 0;
}

// keys_b / vals_b start as bytes 0xA5, so that a pair nobody wrote shows
template <typename K, typename V>
int sort_pairs(const K *keys, const V *vals, K *keys_a_out, V *vals_a_out, K *keys_b_out,
               V *vals_b_out, u64 n, u64 off, const int *shifts, const int *widths, int npasses,
               int with_events, int *n_ev, u32 *guard) {
  Stream st;
  SHIM_HIP(create(st));
  Shifted<K> ka, kb;
  Shifted<V> va, vb;
  Workspace ws;
  SHIM_TRY(ka.make(n, off, keys, 0));
  SHIM_TRY(va.make(n, off, vals, 0));
  SHIM_TRY(kb.make(n, off, nullptr, 0xA5));
  SHIM_TRY(vb.make(n, off, nullptr, 0xA5));
  SHIM_TRY(ws.make(radix_workspace_words(n)));
  Event ev[16];
  hipEvent_t raw[16];
  if (with_events) {
    if (npasses > 8) return SHIM_FAIL;
    for (int i = 0; i < 2 * npasses; i++) {
      SHIM_HIP(create(ev[i]));
      raw[i] = ev[i];
    }
  }
  *n_ev = 0;
  const int rc = radix_sort_pairs<K, V>(ka.at, va.at, kb.at, vb.at, n, shifts, widths, npasses,
                                        ws.d, st, with_events ? raw : nullptr, n_ev);
  SHIM_TRY(finish(st));
  SHIM_TRY(ka.out(keys_a_out));
  SHIM_TRY(va.out(vals_a_out));
  SHIM_TRY(kb.out(keys_b_out));
  SHIM_TRY(vb.out(vals_b_out));
  SHIM_TRY(ws.guard_out(guard));
  return rc;
}

// a call that has to be refused, or to do nothing, before it looks at a pointer
template <typename K, typename V> int sort_no_pointers(u64 n, int npasses) {
  const int shifts[8] = {0, 8, 16, 24, 0, 8, 16, 24}, widths[8] = {8, 8, 8, 8, 8, 8, 8, 8};
  int n_ev = 0;
  return radix_sort_pairs<K, V>(nullptr, nullptr, nullptr, nullptr, n, shifts, widths, npasses,
                                nullptr, nullptr, nullptr, &n_ev);
}

}  // namespace

extern "C" {

int ps_guard_words(void) { return GUARD; }
u32 ps_guard_seed(void) { return GUARD_SEED; }

// the host-only sizes: scan, sort, row scan
void ps_workspace_words(u64 n, u64 *out3) {
  out3[0] = scan_workspace_words(n);
  out3[1] = radix_workspace_words(n);
  out3[2] = radix_rows_workspace_words(n);
}

// `out` (cap >= n elements) goes to the device as it is and comes back whole;
// inplace: the input is laid over its first n elements and in == out
int ps_scan(int op, const u32 *in, u32 *out, u64 n, u64 cap, int inclusive, int inplace, u32 *guard) {
  Stream st;
  SHIM_HIP(create(st));
  Shifted<u32> din, dout;
  Workspace ws;
  SHIM_TRY(din.make(cap, 0, nullptr, 0));
  SHIM_TRY(dout.make(cap, 0, out, 0));
  u32 *src = inplace ? dout.at : din.at;
  if (n) SHIM_HIP(hipMemcpy(src, in, n * sizeof(u32), hipMemcpyHostToDevice));
  SHIM_TRY(ws.make(scan_workspace_words(n)));
  const int rc = scan_u32(op, src, dout.at, n, inclusive != 0, ws.d, st);
  SHIM_TRY(finish(st));
  SHIM_TRY(dout.out(out));
  SHIM_TRY(ws.guard_out(guard));
  return rc;
}

// tsum (one word per 256 counts) goes in as it is and comes back; off has count + 1 words
int ps_offsets(int counted, const u32 *cnt, u64 count, u64 *tsum, u64 *off, u64 *total) {
  Stream st;
  SHIM_HIP(create(st));
  const u64 tiles = div_up(count, 256);
  Shifted<u32> dcnt;
  Shifted<u64> dtsum, doff, dtotal;
  SHIM_TRY(dcnt.make(count, 0, cnt, 0));
  SHIM_TRY(dtsum.make(tiles, 0, tsum, 0));
  SHIM_TRY(doff.make(count + 1, 0, nullptr, 0xA5));
  SHIM_TRY(dtotal.make(1, 0, nullptr, 0xA5));
  const int rc = counted ? offsets_u64_counted(dcnt.at, count, dtsum.at, doff.at, dtotal.at, st)
                         : offsets_u64(dcnt.at, count, dtsum.at, doff.at, dtotal.at, st);
  SHIM_TRY(finish(st));
  SHIM_TRY(dtsum.out(tsum));
  SHIM_TRY(doff.out(off));
  SHIM_TRY(dtotal.out(total));
  return rc;
}

// hist: rows * 256 counters, scanned in place.  as_hist: through
// radix_scan_tile_hist, the histogram at the front of a sort workspace of
// n pairs (ceil(n / 4096) == rows); else radix_scan_tile_rows with the
// histogram in a buffer of its own
int ps_scan_rows(int as_hist, u32 *hist, u32 rows, u64 n, u32 *guard) {
  Stream st;
  SHIM_HIP(create(st));
  Workspace ws;
  Shifted<u32> dh;
  int rc;
  if (as_hist) {
    if (div_up(n, 4096) != rows) return SHIM_FAIL;
    SHIM_TRY(ws.make(radix_workspace_words(n)));
    SHIM_HIP(hipMemcpy(ws.d, hist, (u64) rows * 256 * sizeof(u32), hipMemcpyHostToDevice));
    rc = radix_scan_tile_hist(ws.d, n, st);
    SHIM_TRY(finish(st));
    SHIM_HIP(hipMemcpy(hist, ws.d, (u64) rows * 256 * sizeof(u32), hipMemcpyDeviceToHost));
  } else {
    SHIM_TRY(dh.make((u64) rows * 256, 0, hist, 0));
    SHIM_TRY(ws.make(radix_rows_workspace_words(rows)));
    rc = radix_scan_tile_rows(dh.at, rows, ws.d, st);
    SHIM_TRY(finish(st));
    SHIM_TRY(dh.out(hist));
  }
  SHIM_TRY(ws.guard_out(guard));
  return rc;
}

// instance: key bytes * 10 + value bytes (84, 44, 48, 88).  The four arrays
// a / b come back as the sort left them; off: elements by which every key and
// value pointer is moved off its allocation's start
int ps_sort(int instance, const void *keys, const void *vals, void *keys_a, void *vals_a,
            void *keys_b, void *vals_b, u64 n, u64 off, const int *shifts, const int *widths,
            int npasses, int with_events, int *n_ev, u32 *guard) {
  switch (instance) {
    case 84: return sort_pairs<u64, u32>((const u64 *) keys, (const u32 *) vals, (u64 *) keys_a, (u32 *) vals_a,
                                         (u64 *) keys_b, (u32 *) vals_b, n, off, shifts, widths, npasses,
                                         with_events, n_ev, guard);
    case 44: return sort_pairs<u32, u32>((const u32 *) keys, (const u32 *) vals, (u32 *) keys_a, (u32 *) vals_a,
                                         (u32 *) keys_b, (u32 *) vals_b, n, off, shifts, widths, npasses,
                                         with_events, n_ev, guard);
    case 48: return sort_pairs<u32, u64>((const u32 *) keys, (const u64 *) vals, (u32 *) keys_a, (u64 *) vals_a,
                                         (u32 *) keys_b, (u64 *) vals_b, n, off, shifts, widths, npasses,
                                         with_events, n_ev, guard);
    case 88: return sort_pairs<u64, u64>((const u64 *) keys, (const u64 *) vals, (u64 *) keys_a, (u64 *) vals_a,
                                         (u64 *) keys_b, (u64 *) vals_b, n, off, shifts, widths, npasses,
                                         with_events, n_ev, guard);
  }
  return SHIM_FAIL;
}

// radix_sort_pairs with null pointers everywhere: n = 0 and n >= 2^32
int ps_sort_no_pointers(int instance, u64 n, int npasses) {
  switch (instance) {
    case 84: return sort_no_pointers<u64, u32>(n, npasses);
    case 44: return sort_no_pointers<u32, u32>(n, npasses);
    case 48: return sort_no_pointers<u32, u64>(n, npasses);
    case 88: return sort_no_pointers<u64, u64>(n, npasses);
  }
  return SHIM_FAIL;
}

int ps_partition(const u32 *keys, const u32 *vals, u32 *keys_b, u32 *vals_b, u64 n, u64 off,
                 int shift, int width, u32 *guard) {
  Stream st;
  SHIM_HIP(create(st));
  Shifted<u32> ka, va, kb, vb;
  Workspace ws;
  SHIM_TRY(ka.make(n, off, keys, 0));
  SHIM_TRY(va.make(n, off, vals, 0));
  SHIM_TRY(kb.make(n, off, nullptr, 0xA5));
  SHIM_TRY(vb.make(n, off, nullptr, 0xA5));
  SHIM_TRY(ws.make(radix_workspace_words(n)));
  const int rc = radix_partition_u32(ka.at, va.at, kb.at, vb.at, n, shift, width, ws.d, st);
  SHIM_TRY(finish(st));
  SHIM_TRY(kb.out(keys_b));
  SHIM_TRY(vb.out(vals_b));
  SHIM_TRY(ws.guard_out(guard));
  return rc;
}

// swp: null, or 2 * nwords words
int ps_group_heads(const u32 *keys, const u64 *tiebits, const u32 *carry, u64 nwords, u32 offset,
                   const u64 *swp, u32 *keys_b, u32 *vals_b, u64 n, int shift, int width, u32 *guard) {
  Stream st;
  SHIM_HIP(create(st));
  Shifted<u32> ka, kb, vb, dcarry;
  Shifted<u64> dtie, dswp;
  Workspace ws;
  SHIM_TRY(ka.make(n, 0, keys, 0));
  SHIM_TRY(kb.make(n, 0, nullptr, 0xA5));
  SHIM_TRY(vb.make(n, 0, nullptr, 0xA5));
  SHIM_TRY(dtie.make(nwords, 0, tiebits, 0));
  SHIM_TRY(dcarry.make(nwords, 0, carry, 0));
  if (swp != nullptr) SHIM_TRY(dswp.make(2 * nwords, 0, swp, 0));
  SHIM_TRY(ws.make(radix_workspace_words(n)));
  GroupHeadValues g;
  g.tiebits = dtie.at;
  g.carry = dcarry.at;
  g.nwords = nwords;
  g.offset = offset;
  g.swp = swp != nullptr ? dswp.at : nullptr;
  const int rc = radix_pass_group_heads(ka.at, g, kb.at, vb.at, n, shift, width, ws.d, st);
  SHIM_TRY(finish(st));
  SHIM_TRY(kb.out(keys_b));
  SHIM_TRY(vb.out(vals_b));
  SHIM_TRY(ws.guard_out(guard));
  return rc;
}

}  // extern "C"
