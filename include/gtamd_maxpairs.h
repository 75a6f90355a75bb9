/*
  gtamd_maxpairs.h -- C ABI of what an ENHANCED suffix array exists for:
  enumerating the maximal exact repeats of the indexed sequences from .suf and
  .lcp together, `gt repfind -l L -ii INDEX` (tool src/tools/gt_repfind.c; the
  reference's suite: testsuite/gt_repfind_include.rb:37-53), on the device.

  What it restates:

    gt_enumeratemaxpairs                src/match/esa-maxpairs.c
      (the bottom-up traversal of the lcp-intervals; left characters >= the
       alphabet size go to its `uniquechar` list, position 0 gets INITIALCHAR)
    the default display of an exact match, `len seqnum relpos F len seqnum
    relpos`                             src/match/querymatch-display.c

  Sequence: n symbols enc[0..n) -- letters 0..253, 254 wildcard, 255 separator
  -- read forward; tables of N = n + 1 entries: suf, lcp (one byte per entry,
  255 = "look in llv"), llv (pairs (table index, value) of two uint64, sorted
  by index).

  A MAXIMAL PAIR of minimum length L is a triple (len, p1, p2), p1 < p2, with

    len >= L;
    the len symbols from p1 equal the len symbols from p2, all of them letters;
    right-maximal: the symbols at p1 + len and p2 + len differ, or one of them
                   is a special or the end;
    left-maximal:  p1 = 0, or the symbols at p1 - 1 and p2 - 1 differ, or one
                   of them is a special.

  A special never equals anything, itself included.

  In table terms: for table indices i < j of suffixes that start with a
  letter, len = min(lcp[i+1..j]) is the number of letters the two suffixes
  share, so the pair (suf[i], suf[j]) is right-maximal by itself.  It is
  reported when len >= L and the LEFT CLASSES of the two suffixes differ: the
  class of table index i is the letter enc[suf[i] - 1], or "unique" when that
  symbol is a special or suf[i] = 0; unique differs from everything, unique
  included.

  ORDER.  The reference emits in the order of its stack traversal, a
  by-product that is not part of the semantics.  This library emits in TABLE
  ORDER: ascending i, then ascending j, where i < j are the table indices of
  the two suffixes; a record holds pos1 = min(suf[i], suf[j]), pos2 = the
  other.  The output is deterministic: two calls give the same bytes.
  Comparisons with the reference are made on sorted lines.

  How it is computed (genometools_amd/csrc/esa_maxpairs.hip).
  A RUN is a maximal range [a, b] of table indices with lcp[a+1..b] all >= L;
  every pair lies inside one run, and M is the number of suffixes in runs.

    1 flag and compact   one pass over .lcp marks the entries >= L (.llv by
                         binary search, needed for the mark only when L > 255);
                         the M in-run suffixes are compacted, each with its
                         true LCP value (32 bits) and its left class, gathered
                         from the sequence.  .bwt is not needed.
    2 segments           consecutive entries of a run with the same letter
                         class form a segment (every unique entry one of its
                         own), with the minimum of the LCP values inside it;
                         every entry gets the minimum over the rest of its
                         segment.
    3 count              one lane per in-run suffix walks the segments behind
                         it to the end of its run: a segment of another class
                         adds its size, one of its own class costs one step and
                         adds nothing.  Two skipped segments never follow each
                         other, so a lane's steps are at most 2 * (its pairs)
                         + 1.  A 64-bit scan of the counts gives every suffix
                         its place in the output.
    4 emit               the same walk carrying the running minimum of the
                         values: a skipped segment is folded in one step, a
                         reporting one is gone through entry by entry.

  The work is O(N + M + segments + z) and a binary search per byte 255 that is
  looked at: not the sum of squared run sizes.  Every working array has M (or
  N / 1024) entries, never N: 29 bytes per in-run suffix, 10 per segment.

  Limits: N <= 2^32 - 4096 (whole-table builds; the slices of a build in parts
  and anything beyond are refused with a message, since the values and indices
  are kept in 32 bits).  The tables are trusted, as by the reference: check an
  index with gtamd_check_tables first if it may be damaged; a suffix entry
  beyond n is treated as unique and read nowhere.

  Conventions as in gtamd_check.h: 0 / -1, message from
  gtamd_esa_last_error().  Plain C; no CPU fallback: -1 without a device.
*/
#ifndef GTAMD_MAXPAIRS_H
#define GTAMD_MAXPAIRS_H

#include <stddef.h>
#include <stdint.h>
#include "gtamd_esa.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct { uint64_t pos1, pos2, len; } gtamd_maxpairs_record;

typedef struct {
  uint64_t pairs;                    /* z: records the emit calls will give */
  uint64_t run_suffixes;             /* M */
  uint64_t runs;
  uint64_t segments;
  uint64_t max_pairs_of_one_suffix;  /* the smallest capacity gtamd_maxpairs_emit takes */
  uint64_t max_len;                  /* largest len of a record, 0 without one */
  uint64_t walk_steps;               /* segments the lanes of the count pass looked at */
  uint64_t device_bytes;             /* device memory the object holds */
  float device_ms;                   /* device time of gtamd_maxpairs_prepare (HIP events) */
} gtamd_maxpairs_info;

typedef struct gtamd_maxpairs gtamd_maxpairs;

/* an enumerator on HIP device `device`; NULL on failure.  It keeps its working
   memory between calls; one thread at a time per object. */
gtamd_maxpairs *gtamd_maxpairs_create(int device);
void gtamd_maxpairs_destroy(gtamd_maxpairs *mp);

/* Set the index; each call replaces the one before and what was prepared.
   From device pointers, which stay the caller's and must outlive the calls: n
   symbols, n + 1 entries of suf_bytes = 4 or 8 bytes (.suf with and without
   -suftabuint), n + 1 bytes of lcp, llv_pairs pairs of two uint64 (llv may be
   NULL when llv_pairs is 0). */
int gtamd_maxpairs_set_index(gtamd_maxpairs *mp, const uint8_t *enc_device, uint64_t n,
                             const void *suf_device, uint32_t suf_bytes,
                             const uint8_t *lcp_device, const uint64_t *llv_device,
                             uint64_t llv_pairs);
/* from HOST memory (read back from the files of an index, or mapped): uploaded
   piece by piece into memory the object owns */
int gtamd_maxpairs_set_index_host(gtamd_maxpairs *mp, const uint8_t *enc_host, uint64_t n,
                                  const void *suf_host, uint32_t suf_bytes,
                                  const uint8_t *lcp_host, const uint64_t *llv_host,
                                  uint64_t llv_pairs);
/* the tables an engine context holds after gtamd_esa_run with GTAMD_WANT_SUF |
   GTAMD_WANT_LCP (whole-table build, forward read mode), with the n symbols at
   enc_device.  The context must outlive the calls. */
int gtamd_maxpairs_set_index_esa(gtamd_maxpairs *mp, const gtamd_esa_ctx *esa,
                                 const uint8_t *enc_device, uint64_t n);

/* steps 1 to 3 for minimum length min_len >= 1 (0 is refused); fills *info
   (may be NULL).  Synchronous. */
int gtamd_maxpairs_prepare(gtamd_maxpairs *mp, uint32_t min_len, gtamd_maxpairs_info *info);

/* Step 4, in pieces.  *cursor is a number of SUFFIXES IN RUNS, not of records:
   the place, among the M in-run suffixes in table order, of the first suffix
   whose records are written; 0 for the first call after a prepare, advanced by
   the call to the suffix behind the last one written, and to M when no record
   is left.  Any value from 0 to M (`run_suffixes` of the info) may be passed, to
   resume an enumeration or to start in its middle; a value beyond M is refused
   with a message.  Writes the records of whole
   suffixes, in table order, from the cursor on, as many as fit `capacity`
   records, to out (device memory when out_on_device, else host memory);
   *written = their number, 0 when all z records have been given.  A capacity
   below max_pairs_of_one_suffix is refused with a message that names the
   capacity needed.  Synchronous. */
int gtamd_maxpairs_emit(gtamd_maxpairs *mp, uint64_t *cursor, gtamd_maxpairs_record *out,
                        uint64_t capacity, int out_on_device, uint64_t *written);

/* figures of the last prepare */
int gtamd_maxpairs_get_info(const gtamd_maxpairs *mp, gtamd_maxpairs_info *info);

#ifdef __cplusplus
}
#endif
#endif
