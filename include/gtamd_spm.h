/*
  gtamd_spm.h -- C ABI of all suffix-prefix matches of a sequence set: the
  overlap phase of a string-graph assembler, what `gt encseq2spm -l L -ii READS
  -spm show|count` computes (tool src/tools/gt_encseq2spm.c), from .suf and .lcp
  together, on the device.

  What it restates:

    processleafedge_spmsk               src/match/esa-spmsk.c:59-85
      (a leaf whose suffix starts a sequence goes to the set W, one whose
       suffix runs to the end of its sequence to the set L)
    processlcpinterval_spmsk            src/match/esa-spmsk.c:87-124
      (at an lcp-interval of depth >= L every member of L is reported with
       every member of W of that interval)
    the bottom-up traversal that calls them   src/match/esa-bottomup-spmsk.inc

  INPUTS.  n symbols enc[0..n) -- letters 0..253, 254 wildcard, 255 separator:
  the sequences S_0 .. S_(K-1) with a separator between two of them.  Tables of
  N = n + 1 entries: suf of 4 or 8 bytes, lcp (one byte per entry, 255 = "look
  in llv"), llv (pairs (table index, value) of two uint64, sorted by index).  A
  special never equals anything, itself included.

  A MATCH of minimum length L >= 1 is a triple (s, t, len) with all of

    len >= L;
    the last len symbols of S_s equal the first len symbols of S_t, all of
    them letters;
    len <= min(|S_s|, |S_t|).

  Self-overlaps s = t with len < |S_s| count.  The trivial triple (s, s, |S_s|)
  is a match if and only if the letters of S_s occur at some other place of the
  set as well, that is if at least two suffixes start with them: the reference
  reports from lcp-intervals only (esa-spmsk.c:92), and an lcp-interval holds
  two suffixes at least.

  The library works on the sequence it is given and never mirrors it.  `gt
  encseq2spm` always works on both strands: its sequence set is the mirrored one
  (R reads give K = 2R sequences, number R + j the reverse complement of read
  R - 1 - j), which is what gtamd_mirror of gtamd_host.h makes.  Mirroring is the
  caller's business.

  RECORD.  { suffix_seq = s, prefix_seq = t, len }, three uint64.

  ORDER.  Ascending table index of the suffix of S_s that matches, then
  ascending table index of the suffix that is all of S_t.  It is deterministic:
  two calls give the same bytes.  It is not the reference's order, which is a
  by-product of its stack traversal: outputs are compared with the reference as
  sorted lines.

  How it is computed (genometools_amd/csrc/esa_spm.hip, esa_spm_core.h;
  DESIGN.md 9f).  Specials sort behind all letters, so a suffix x that runs to
  the end of its sequence stands at the end of the interval of the suffixes that
  start with x.

    1 terminal suffixes  one lane per table entry i, p = suf[i]: h = max(lcp[i],
                         lcp[i + 1]) (byte 255 by binary search in .llv); the
                         entry is kept when h >= L and the symbol at p + h is a
                         separator, or p + h = n.  An LCP value never counts a
                         special, so the test holds exactly when the h letters
                         in front of the separator are shared with a neighbour:
                         the interval of x has two suffixes at least, which is
                         the rule of the trivial triple.  (i, h) are compacted in
                         table order: ballots of the waves, a scan of the
                         workgroups' counts.
    2 read starts        the same lanes: the table indices whose suffix starts a
                         sequence (p = 0 or enc[p - 1] = 255) with a letter,
                         ascending, one per sequence at most; and the positions
                         of the separators, which turn a position into a
                         sequence number.
    3 intervals          one lane per terminal suffix: the interval [lo, lo +
                         width) of the suffixes that start with its h letters.
                         The lane stands inside it: it walks over .lcp to both
                         sides while the values reach h, up to 64 entries each
                         way; only an interval that reaches further is searched
                         for in the text (the two binary searches of
                         esa_qmatch_core.h, the sequence being its own query).
                         Then two binary searches in the list of step 2: the
                         read starts inside.
    4 scan               a 64-bit exclusive scan of those numbers: Z and every
                         terminal suffix's place in the output.  Counting ends
                         here.
    5 emit               in chunks, one lane per (terminal suffix, read start)
                         pair, found by a search in the scanned places: a prefix
                         that 50,000 reads share spreads over 50,000 lanes.
                         Every pair is a record; both positions become sequence
                         numbers by a search in the separator list.

  Working memory: 24 bytes per terminal suffix, 4 per read start, 4 per
  separator, 12 per 1024 table entries.  Nothing else has N entries.

  LIMITS.  N <= 2^32 - 4096 (whole-table builds; the slices of a build in parts
  are refused with a message); Z is 64 bits.  No symbol is read at or beyond n
  and no table entry at or beyond N.  The tables are trusted otherwise: check an
  index with gtamd_check_tables first if it may be damaged.

  Conventions as in gtamd_maxpairs.h: 0 / -1, message from
  gtamd_esa_last_error().  Plain C; no CPU fallback: -1 without a device.
*/
#ifndef GTAMD_SPM_H
#define GTAMD_SPM_H

#include <stddef.h>
#include <stdint.h>
#include "gtamd_esa.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct { uint64_t suffix_seq, prefix_seq, len; } gtamd_spm_record;

typedef struct {
  uint64_t table_entries;              /* N */
  uint64_t terminal_suffixes;          /* entries step 1 keeps */
  uint64_t read_starts;                /* entries step 2 keeps */
  uint64_t matches;                    /* Z: records the emit calls will give */
  uint64_t max_width;                  /* the widest interval of a terminal suffix */
  uint64_t max_matches_of_one_suffix;  /* most read starts inside one interval */
  uint64_t search_symbols;             /* symbol comparisons of the intervals searched for in the text */
  uint64_t device_bytes;               /* device memory the object holds */
  float device_ms;                     /* device time of gtamd_spm_prepare (HIP events) */
} gtamd_spm_info;

typedef struct gtamd_spm gtamd_spm;

/* a matcher on HIP device `device`; NULL on failure.  It keeps its working
   memory between calls; one thread at a time per object. */
gtamd_spm *gtamd_spm_create(int device);
void gtamd_spm_destroy(gtamd_spm *sp);

/* Host only.  tile_suffixes: terminal suffixes of one workgroup of step 3, and
   records of one workgroup of step 5; min_capacity: the smallest capacity
   gtamd_spm_emit takes.  Either may be NULL. */
void gtamd_spm_geometry(uint32_t *tile_suffixes, uint64_t *min_capacity);

/* Set the index; each call replaces the one before and what was prepared.
   From device pointers, which stay the caller's and must outlive the calls: n
   symbols, n + 1 entries of suf_bytes = 4 or 8 bytes (.suf with and without
   -suftabuint), n + 1 bytes of lcp (NULL is refused with a message), llv_pairs
   pairs of two uint64 (llv may be NULL when llv_pairs is 0). */
int gtamd_spm_set_index(gtamd_spm *sp, const uint8_t *enc_device, uint64_t n,
                        const void *suf_device, uint32_t suf_bytes,
                        const uint8_t *lcp_device, const uint64_t *llv_device,
                        uint64_t llv_pairs);
/* from HOST memory: uploaded piece by piece into memory the object owns */
int gtamd_spm_set_index_host(gtamd_spm *sp, const uint8_t *enc_host, uint64_t n,
                             const void *suf_host, uint32_t suf_bytes,
                             const uint8_t *lcp_host, const uint64_t *llv_host,
                             uint64_t llv_pairs);
/* the tables an engine context holds after gtamd_esa_run with GTAMD_WANT_SUF |
   GTAMD_WANT_LCP (whole-table build, forward read mode), with the n symbols at
   enc_device.  The context must outlive the calls. */
int gtamd_spm_set_index_esa(gtamd_spm *sp, const gtamd_esa_ctx *esa,
                            const uint8_t *enc_device, uint64_t n);

/* steps 1 to 4 for minimum length min_len >= 1 (0 is refused); fills *info
   (may be NULL).  Synchronous. */
int gtamd_spm_prepare(gtamd_spm *sp, uint32_t min_len, gtamd_spm_info *info);

/* Step 5, in pieces.  *cursor is the number of the first record to write,
   counted over all Z records in the order stated above: 0 for the first call
   after a prepare, advanced by the call to the record behind the last one
   written.  Any value from 0 to Z (`matches` of the info) may be passed, to
   resume an enumeration or to take a piece out of its middle; a value beyond Z
   is refused with a message.  Writes the next records in the
   order stated above, as many as fit `capacity`, to out (device memory when
   out_on_device, else host memory); *written = their number, 0 when all Z
   records have been given.  A capacity below min_capacity is refused with a
   message that names it.  Synchronous. */
int gtamd_spm_emit(gtamd_spm *sp, uint64_t *cursor, gtamd_spm_record *out,
                   uint64_t capacity, int out_on_device, uint64_t *written);

/* figures of the last prepare */
int gtamd_spm_get_info(const gtamd_spm *sp, gtamd_spm_info *info);

#ifdef __cplusplus
}
#endif
#endif
