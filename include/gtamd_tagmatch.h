/*
  gtamd_tagmatch.h -- C ABI of the approximate matches of short tags against an
  indexed sequence: what `gt tagerator -e K -esa INDEX -q TAGS` computes
  (src/tools/gt_tagerator.c, src/match/tagerator.c), from the .suf table and
  the sequence, on the device.

  What it restates:

    gt_indexbasedapproxpatternmatching  src/match/idx-limdfs.c
      (a depth-first walk over the intervals of the suffix table, one symbol a
       level; esa_splitandprocess, processchildinterval, esa_overcontext)
    apme_nextLimdfsstate, apme_fullmatchLimdfsstate   src/match/apmeoveridx.c
      (Myers' bit-vector column of the tag, the largest row that is <= K)
    gt_indexbasedexactpatternmatching   (the same question for K = 0)
    searchoverstrands                   src/match/tagerator.c:468-536

  INPUTS.  Subject: n symbols enc[0..n) -- letters 0..sigma-1 with sigma <= 32,
  254 wildcard, 255 separator --, read forward.  Suffix table: suf, N = n + 1
  entries of 4 or 8 bytes.  Tags: T tags as one array of symbols and T + 1
  ascending offsets into it, offsets[0] = 0; tag t is symbols
  [offsets[t], offsets[t + 1]): m letters with 1 <= m <= 64 (the reference's
  MAXTAGSIZE, the bits of a word), every one of them below sigma.  K: the
  number of differences, 0 <= K < m for every tag (the reference's rule).
  Differences are those of the edit distance: a replacement, an insertion and a
  deletion cost one each.

  For a tag P, a strand and a start position p let D(d) be the edit distance
  of P and enc[p..p+d).  D(d) is defined only while all of enc[p..p+d) are
  letters and p + d <= n; with GTAMD_TAGMATCH_WITH_WILDCARDS (taken only when
  K > 0) a wildcard counts as a symbol too, one that equals nothing.  A
  separator and the end of the sequence never pass.

  A MATCH is (tag, strand, p, len, dist) with

    len  = the smallest d for which D(d) is defined and D(d) <= K,
    dist = D(len).

  There is at most one match per (tag, strand, p), and len <= m + K.  (D
  changes by at most one from d to d + 1 and D(0) = m > K, so dist is K in
  every match of a search with K; it is a field all the same, because with
  GTAMD_TAGMATCH_BEST the K of a tag is not the caller's.)  This is the value
  of the index-based tool; the reference's online scan reports the smallest
  distance over all lengths instead.

  STRANDS.  The reverse-complement strand searches the tag reversed, with the
  letters c turned into 3 - c.  This is defined for sigma = 4 only: with
  another alphabet GTAMD_TAGMATCH_REVCOMP is refused with a message.

  BEST.  With GTAMD_TAGMATCH_BEST, K' of a tag is the smallest of 0..K for
  which the tag has a match on one of the strands asked for, and the matches
  of the tag are those for K' (on both strands; len is then the smallest length
  under K').  A tag without a match for K has no K' (GTAMD_TAGMATCH_NO_K).

  ORDER.  Ascending tag, then the forward strand before the reverse complement,
  then ascending table index of the suffix p.  A depth-first walk that takes
  the children of an interval from left to right gives this order without a
  sort; it is deterministic.  (The reference's order inside one tag and strand
  is that of its stack, a by-product: outputs are compared with the lines of
  one tag sorted.)  With a reader of the packed index as the index
  (include/gtamd_pcktag.h) the order inside one tag and strand is another one,
  stated there: that of the rows of the index.

  RECORD.  { tag = 2 * tagnumber + (1 for the reverse complement), dbstart = p,
  lendist = len | dist << 32 }, three uint64.

  How it is computed (genometools_amd/csrc/esa_tagmatch.hip,
  esa_tagmatch_core.h).  A job is (tag, strand); one wave of 64
  lanes walks one job.  The walk keeps one level per depth in LDS: the interval,
  the left bound of the next child and the column.  The letter of the next
  child is the symbol of the suffix at the cursor; its right bound comes from a
  search all lanes share (64 probes a round); the child's column is one step of
  the bit-vector algorithm.  A child without a row <= K is dropped; one whose
  row m is <= K gives all its suffixes as matches; one of at most 64 suffixes
  is finished by its lanes alone, one suffix a lane in the text; a wider one
  becomes the next level.

    count      every job walked once: matches per job
    offsets    a 64-bit exclusive scan: the place of every job's first record
    emit       the same walk again, for the jobs whose records fall into the
               window [cursor, cursor + capacity), writing those

  LIMITS.  N <= 2^32 - 4096 (whole-table builds; the slices of a build in
  parts are refused with a message); T <= 2^30.  No symbol is read at or beyond
  n and no table entry at or beyond N; a suffix entry beyond n is no
  occurrence.  A table that is no suffix table may give wrong matches, never an
  endless loop or a read outside the arrays.

  Conventions as in gtamd_qmatch.h: 0 / -1, message from
  gtamd_esa_last_error().  Plain C; no CPU fallback: -1 without a device.
*/
#ifndef GTAMD_TAGMATCH_H
#define GTAMD_TAGMATCH_H

#include <stddef.h>
#include <stdint.h>
#include "gtamd_esa.h"

#ifdef __cplusplus
extern "C" {
#endif

enum {
  GTAMD_TAGMATCH_FORWARD = 1,
  GTAMD_TAGMATCH_REVCOMP = 2,
  GTAMD_TAGMATCH_BEST = 4,
  GTAMD_TAGMATCH_WITH_WILDCARDS = 8
};

#define GTAMD_TAGMATCH_NO_K 0xffffffffu

typedef struct { uint64_t tag, dbstart, lendist; } gtamd_tagmatch_record;

typedef struct {
  uint64_t jobs;                     /* (tag, strand) pairs walked */
  uint64_t matches;                  /* records of the enumeration */
  uint64_t max_matches_of_one_job;
  /* the next three are figures of the count passes only, not of emit.  With
     GTAMD_TAGMATCH_BEST there is one count pass per k = 0 .. K, each over the
     tags still without a match, and the three are the sums over all these passes,
     not the figures of the walks with each tag's K'. */
  uint64_t levels_pushed;            /* children that became a level of a walk */
  uint64_t children_examined;        /* children whose right bound was searched */
  uint64_t single_walks;             /* suffixes finished by one lane in the text */
  uint64_t emitted;                  /* records the emit calls have given so far */
  uint64_t device_bytes;             /* device memory the object holds */
  float device_ms;                   /* device time of gtamd_tagmatch_prepare (HIP events) */
} gtamd_tagmatch_info;

typedef struct gtamd_tagmatch gtamd_tagmatch;

/* a matcher on HIP device `device`; NULL on failure.  It keeps its working
   memory between calls; one thread at a time per object. */
gtamd_tagmatch *gtamd_tagmatch_create(int device);
void gtamd_tagmatch_destroy(gtamd_tagmatch *tm);

/* Host only.  jobs_per_workgroup: the waves, one job each, of a workgroup;
   min_capacity: the smallest capacity gtamd_tagmatch_emit takes; max_levels:
   the levels a walk has room for (64 + 63 + 1).  Any may be NULL. */
void gtamd_tagmatch_geometry(uint32_t *jobs_per_workgroup, uint64_t *min_capacity, uint32_t *max_levels);

/* Set the index; each call replaces the one before and what was prepared.
   From device pointers, which stay the caller's and must outlive the calls: n
   symbols, n + 1 entries of suf_bytes = 4 or 8 bytes, numofchars = sigma
   (1..32). */
int gtamd_tagmatch_set_index(gtamd_tagmatch *tm, const uint8_t *enc_device, uint64_t n,
                             const void *suf_device, uint32_t suf_bytes, uint32_t numofchars);
/* from HOST memory: uploaded piece by piece into memory the object owns */
int gtamd_tagmatch_set_index_host(gtamd_tagmatch *tm, const uint8_t *enc_host, uint64_t n,
                                  const void *suf_host, uint32_t suf_bytes, uint32_t numofchars);
/* the .suf table an engine context holds after gtamd_esa_run with
   GTAMD_WANT_SUF (whole-table build, forward read mode), with the n symbols at
   enc_device.  The context must outlive the calls. */
int gtamd_tagmatch_set_index_esa(gtamd_tagmatch *tm, const gtamd_esa_ctx *esa,
                                 const uint8_t *enc_device, uint64_t n, uint32_t numofchars);

/* Count and offsets for T tags (symbols and the T + 1 offsets in device memory
   when is_device, which then must outlive the emit calls; else host memory,
   copied), K differences and flags, an OR of GTAMD_TAGMATCH_*: at least one of
   FORWARD and REVCOMP.  Refused with a message that names the first such tag: a
   tag of no or of more than 64 letters, one not longer than K, a symbol that
   is no letter of the alphabet.  Fills *info (may be NULL).  Synchronous. */
int gtamd_tagmatch_prepare(gtamd_tagmatch *tm, const uint8_t *tags, const uint64_t *offsets, uint64_t T,
                           int is_device, uint32_t K, uint32_t flags, gtamd_tagmatch_info *info);

/* The records of the last prepare in pieces.  *cursor is the number of the
   first record to write, counted over the whole enumeration in the order stated
   above: 0 for the first call after a prepare, advanced by the call to the
   record behind the last one written.  Any value from 0 to `matches` of the
   info may be passed, to resume an enumeration or to take a piece out of its
   middle; a value beyond it is refused with a message.  Writes
   the records whose places are [*cursor, *cursor + capacity) in the order
   stated above to out (device memory when out_on_device, else host memory);
   *written = their number, 0 only when no record is left.  A job whose
   records lie in several pieces is walked once for each.  A capacity below
   min_capacity is refused with a message that names it; nothing is refused
   because one tag has many matches.  Synchronous. */
int gtamd_tagmatch_emit(gtamd_tagmatch *tm, uint64_t *cursor, gtamd_tagmatch_record *out,
                        uint64_t capacity, int out_on_device, uint64_t *written);

/* K' of the T tags of the last prepare to host memory, GTAMD_TAGMATCH_NO_K for
   a tag without a match; without GTAMD_TAGMATCH_BEST K' is K or none. */
int gtamd_tagmatch_best_k(gtamd_tagmatch *tm, uint32_t *k_host, uint64_t T);

/* figures of the last prepare and of the emit calls since */
int gtamd_tagmatch_get_info(const gtamd_tagmatch *tm, gtamd_tagmatch_info *info);

#ifdef __cplusplus
}
#endif
#endif
