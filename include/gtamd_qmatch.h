/*
  gtamd_qmatch.h -- C ABI of the maximal exact matches of a query against an
  indexed sequence: what `gt repfind` computes with -q FILE, and with -r and -p
  (the reference's gt_callenumquerymatches, src/tools/gt_repfind.c:562-757),
  from the .suf table and the sequence, on the device.

  What it restates:

    GtQuerysubstringmatchiterator       src/match/esa-mmsearch.c:713-943
      (for every query offset: the interval of the suffixes that start with
       the next L query symbols; the occurrences that are left-maximal are
       extended to the right)
    gt_mmsearch_isleftmaximal           src/match/esa-mmsearch.c:347-368
    gt_mmsearch_extendright             src/match/esa-mmsearch.c:392-421
    gt_mmsearch_accessquery             src/match/esa-mmsearch.c:48-78
    gt_querymatch_position_convert      src/match/querymatch.c:202-213

  INPUTS.  Subject: n symbols enc[0..n) -- letters 0..253, 254 wildcard, 255
  separator.  Suffix table: suf, N = n + 1 entries of 4 or 8 bytes.  Query: m
  symbols q[0..m) in the same coding; several query sequences go into one call
  with a separator between them, as in gtamd_mstat.h.  A special never equals
  anything, itself included; the ends of both sequences never match.

  A MATCH of minimum length L >= 1 is a triple (i, p, len) with all of

    len >= L;
    q[i..i+len) equals enc[p..p+len), all of them letters;
    left-maximal:  i = 0, or p = 0, or enc[p-1] is a special, or enc[p-1] !=
                   q[i-1] (a separator in front of a query sequence satisfies
                   the last clause by itself);
    right-maximal: p + len = n, or i + len = m, or one of the two next symbols
                   is a special, or they differ.

  Equivalently: one record per maximal run of equal letters of length >= L on a
  diagonal p - i.

  ORDER.  Ascending i, then ascending table index of suffix p.  This is the
  reference's own order (query unit, offset, `sufindex` left to right), and it
  is deterministic: outputs are compared unsorted.

  RECORD.  { dbpos = p, qpos = i, len }, three uint64.

  QUERY READ MODE is the caller's business, as gt_mmsearch_accessquery defines
  it: for a reverse match each query sequence is reversed on its own; for a
  reverse-complement match the letters c become 3 - c in addition, specials
  unchanged.  The records are in the coordinates of the transformed query; for
  display, the query start on the forward strand is seqlen - offset - len
  (gt_querymatch_position_convert).

  How it is computed (genometools_amd/csrc/esa_qmatch.hip, esa_qmatch_core.h;
  DESIGN.md 9e).

    a intervals   one lane per query position: [lo, lo + width) of the suffixes
                  that start with the L symbols from there, by two binary
                  searches over the table that carry the shared prefix lengths
                  of both borders and compare 16 symbols at a time
                  (esa_mstat_search.h); empty when one of the L symbols is a
                  special or lies at or beyond m
    b scan        an exclusive 64-bit scan of the widths: the place of every
                  position's first CANDIDATE (an occurrence before the
                  left-maximality test), and C, their number
    c emit        in chunks of candidates, one lane per candidate: a seed with
                  50,000 occurrences spreads over 50,000 lanes.  A lane finds
                  its position by a search in the scanned offsets, reads
                  suf[lo + k], tests left-maximality and only then extends to
                  the right.  The kept records of a workgroup are compacted in
                  candidate order and written at an offset from a scan of the
                  workgroups' counts: the order above, without a sort.

  Working memory is per query position (lo, width and the 64-bit offset: 16
  bytes) and per chunk (4 bytes per 256 candidates), never per table entry.

  LIMITS.  N <= 2^32 - 4096 (whole-table builds; the slices of a build in
  parts are refused with a message); m <= 2^32 - 1 per call; C is 64 bits.  No
  symbol is read at or beyond n or m and no table entry at or beyond N; a
  suffix entry beyond n is treated as no occurrence.  The table is trusted
  otherwise: check an index with gtamd_check_tables first if it may be damaged.

  Conventions as in gtamd_maxpairs.h: 0 / -1, message from
  gtamd_esa_last_error().  Plain C; no CPU fallback: -1 without a device.
*/
#ifndef GTAMD_QMATCH_H
#define GTAMD_QMATCH_H

#include <stddef.h>
#include <stdint.h>
#include "gtamd_esa.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct { uint64_t dbpos, qpos, len; } gtamd_qmatch_record;

typedef struct {
  uint64_t positions;          /* m */
  uint64_t seeds;              /* positions with a non-empty interval */
  uint64_t candidates;         /* C: the sum of the widths */
  uint64_t max_width;          /* the widest interval */
  uint64_t matches;            /* records the emit calls have given so far */
  uint64_t search_symbols;     /* symbol comparisons of the binary searches */
  uint64_t extension_symbols;  /* symbol comparisons of the right extensions so far */
  uint64_t device_bytes;       /* device memory the object holds */
  float device_ms;             /* device time of gtamd_qmatch_prepare (HIP events) */
} gtamd_qmatch_info;

typedef struct gtamd_qmatch gtamd_qmatch;

/* a matcher on HIP device `device`; NULL on failure.  It keeps its working
   memory between calls; one thread at a time per object. */
gtamd_qmatch *gtamd_qmatch_create(int device);
void gtamd_qmatch_destroy(gtamd_qmatch *qm);

/* Host only.  tile_positions: query positions of one workgroup of step a;
   min_capacity: the smallest capacity gtamd_qmatch_emit takes, which is also
   its smallest chunk of candidates.  Either may be NULL. */
void gtamd_qmatch_geometry(uint32_t *tile_positions, uint64_t *min_capacity);

/* Set the index; each call replaces the one before and what was prepared.
   From device pointers, which stay the caller's and must outlive the calls: n
   symbols, n + 1 entries of suf_bytes = 4 or 8 bytes. */
int gtamd_qmatch_set_index(gtamd_qmatch *qm, const uint8_t *enc_device, uint64_t n,
                           const void *suf_device, uint32_t suf_bytes);
/* from HOST memory: uploaded piece by piece into memory the object owns */
int gtamd_qmatch_set_index_host(gtamd_qmatch *qm, const uint8_t *enc_host, uint64_t n,
                                const void *suf_host, uint32_t suf_bytes);
/* the .suf table an engine context holds after gtamd_esa_run with
   GTAMD_WANT_SUF (whole-table build, forward read mode), with the n symbols at
   enc_device.  The context must outlive the calls. */
int gtamd_qmatch_set_index_esa(gtamd_qmatch *qm, const gtamd_esa_ctx *esa,
                               const uint8_t *enc_device, uint64_t n);

/* Steps a and b for the m symbols at query (device memory when is_device, which
   then must outlive the emit calls; else host memory, copied) and minimum
   length min_len >= 1 (0 is refused); fills *info (may be NULL).  Synchronous. */
int gtamd_qmatch_prepare(gtamd_qmatch *qm, const uint8_t *query, uint64_t m, int is_device,
                         uint32_t min_len, gtamd_qmatch_info *info);

/* Step c, in pieces.  *cursor is a number of CANDIDATES, not of records: the
   place, in the scan of step b, of the first candidate to go through; 0 for
   the first call after a prepare, advanced by the call to the candidate behind
   the last one it went through.  Any value from 0 to C (`candidates` of the
   info) may be passed, to resume an enumeration or to start in its middle; a
   value beyond C is refused with a message.  Goes through the candidates
   from the cursor on in chunks of at most (capacity - records written so far)
   candidates, and writes the records in the order stated above to out (device
   memory when out_on_device, else host memory).  It stops when that room falls
   below min_capacity or no candidate is left; *written = the number of
   records, 0 only when all candidates have been gone through.  A capacity below
   min_capacity is refused with a message that names it.  Synchronous. */
int gtamd_qmatch_emit(gtamd_qmatch *qm, uint64_t *cursor, gtamd_qmatch_record *out,
                      uint64_t capacity, int out_on_device, uint64_t *written);

/* figures of the last prepare and of the emit calls since */
int gtamd_qmatch_get_info(const gtamd_qmatch *qm, gtamd_qmatch_info *info);

#ifdef __cplusplus
}
#endif
#endif
