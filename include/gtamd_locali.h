/*
  gtamd_locali.h -- C ABI of the local alignments of queries against an indexed
  sequence: what `gt dev idxlocali -th T -esa INDEX -q FILES` computes
  (src/tools/gt_idxlocali.c, src/match/idxlocali.c), from the .suf table and the
  sequence, on the device.

  What it restates:

    gt_indexbasedlocali, runlimdfs with keepexpandedonstack   src/match/idx-limdfs.c
      (the depth-first walk over the intervals of the suffix table that
       tagerator uses too, here with every column of the path kept)
    secondcolumn, nextcolumn, locali_fullmatchLimdfsstate,
    gt_processelemLocaliTracebackstate                         src/match/idxlocalidp.c
      (the column, its maximum, the traceback)

  The AFFINE variant of the reference is compiled out: a gap of length l costs
  l * gapextend, and -gapstart has no effect there or here.

  INPUTS.  Subject: n symbols enc[0..n) -- letters 0..sigma-1 with sigma <= 32,
  254 wildcard, 255 separator.  Suffix table: suf, N = n + 1 entries of 4 or 8
  bytes.  Queries: Q queries as one array of symbols and Q + 1 ascending
  offsets into it, offsets[0] = 0; query t is symbols [offsets[t],
  offsets[t + 1]): m symbols, 1 <= m <= 16384, each a letter below sigma or the
  wildcard 254, which equals nothing.  Scores: match in 1..32767, mismatch and
  gapextend in -32767..-1; anything else is refused with a message.  (The
  reference does not check the signs; with a gapextend >= 0 its walk need not
  end.)  match * m <= 65535 for every query: the width of a stored score.
  Threshold T >= 1.

  COLUMNS.  For a start position p the columns C_d[0..m], d = 1, 2, ..., are
  defined while enc[p+d-1] is a letter and p + d <= n: a wildcard, a separator
  or the end of the sequence ends them.  With c = enc[p+d-1] and R(i) = match
  if Q[i] == c, else mismatch:

    C_d[0] = -1.
    C_d[i], i = 1..m: start from -1 and take each of these candidates, in this
    order, only if it is STRICTLY GREATER than the value so far:
      Delete   C_d[i-1] + gapextend                    if C_d[i-1] > 0
      Replace  d = 1: R(i);  d > 1: C_{d-1}[i-1] + R(i)  if C_{d-1}[i-1] > 0
      Insert   d > 1: C_{d-1}[i] + gapextend           if C_{d-1}[i] > 0
               (d = 1: the bare gapextend, which is negative and never wins)
    The candidate taken last is the trace of the cell: on equal scores Delete
    beats Replace, Replace beats Insert.  A cell may be 0; it has a trace and
    nothing extends it.
    M_d = the largest cell > 0, or 0 without one; e_d = the smallest row that
    holds M_d.

  A MATCH.  p has a match iff some defined d has M_d >= T.  Then dblen = the
  smallest such d, score = M_dblen, the end in the query is e = e_dblen.  The
  traceback starts at (e, dblen): Insert does d--, Replace d-- and i--, Delete
  i-- in the same column, until d is 0; qstart = the row left over, qlen = e -
  qstart.  Once M_d = 0 every later column is all -1.  At most one match per
  (query, p); the entry n of the table is no position.

  DEPTH.  A cell > 0 of column d aligns d symbols with at most m letters: at
  most m replacements, worth at most match * m, and at least d - m insertions.
  So match * m + gapextend * (d - m) > 0, and no column beyond

    d_max(m) = m + ceil(match * m / -gapextend) - 1

  has a cell > 0.  Every walk stops there whatever the table and the text hold.

  ORDER.  Ascending query, then ascending table index of the suffix p.  (The
  reference's order inside a query is that of its stack; outputs are compared
  with the match blocks of one query sorted.)

  RECORD.  { query, dbstart = p, dblen | score << 32, qstart | qlen << 32 },
  four uint64.

  How it is computed (genometools_amd/csrc/esa_locali.hip, esa_locali_core.h;
  DESIGN.md 9i).  set_index* cuts the table once into consecutive groups by the
  first symbols of the suffixes, down to the largest depth the alphabet allows
  with at most 2^16 groups; a suffix with a special or the end before that depth
  forms a group with the suffixes that share its shorter prefix.  A prepare
  takes the cuts above a depth q, chosen as the smallest that gives 2^14 jobs: a
  JOB is (query, group).  One wave of 64 lanes walks a job depth first over the
  intervals of its group, the columns of the group's prefix included, one row
  of a column per lane and 64 rows a step.  A column is kept as the band of
  rows that holds its cells > 0; the bands of the path are a stack in global
  memory, one stack per wave of the grid.  A child whose column reaches T gives
  all its suffixes as matches; one without a cell > 0 is dropped; a child of one
  suffix is finished in the text with two columns of its own; a wider one is
  pushed.  A child for which the stack has no room is finished suffix by suffix
  in the text as well (info.jobs_finished_alone counts the jobs with such a
  child): slower, never lost.

    count      every job walked once: matches per job
    offsets    a 64-bit exclusive scan: the place of every job's first record
    emit       the same walk again, for the jobs whose records fall into the
               window [cursor, cursor + capacity), writing those

  LIMITS.  N <= 2^32 - 4096 (whole-table builds; the slices of a build in
  parts are refused with a message); sigma <= 32; m <= 16384; Q <= 2^24; Q
  times the groups <= 2^31.  No symbol is read at or beyond n and no table entry
  at or beyond N; a suffix entry beyond n is no position.  A table that is no
  suffix table may give wrong matches, never an endless loop or a read outside
  the arrays.

  Conventions as in gtamd_tagmatch.h: 0 / -1, message from
  gtamd_esa_last_error().  Plain C; no CPU fallback: -1 without a device.
*/
#ifndef GTAMD_LOCALI_H
#define GTAMD_LOCALI_H

#include <stddef.h>
#include <stdint.h>
#include "gtamd_esa.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GTAMD_LOCALI_AUTO 0xffffffffu

typedef struct { uint64_t query, dbstart, lenscore, qspan; } gtamd_locali_record;

typedef struct {
  uint64_t jobs;                     /* (query, group) pairs walked */
  uint64_t matches;                  /* records of the enumeration */
  uint64_t max_matches_of_one_job;
  /* the next four are figures of the count pass only, not of emit */
  uint64_t levels_pushed;            /* children whose band went onto a stack */
  uint64_t children_examined;        /* children whose right bound was searched */
  uint64_t single_walks;             /* suffixes finished alone in the text */
  uint64_t jobs_finished_alone;      /* jobs with a child that found no room on the stack */
  uint64_t emitted;                  /* records the emit calls have given so far */
  uint64_t device_bytes;             /* device memory the object holds */
  uint64_t groups;                   /* groups of the table in this prepare */
  uint32_t cut_depth;                /* q: the symbols the groups are cut by */
  uint32_t stack_words;              /* 32-bit words of one wave's stack */
  float device_ms;                   /* device time of gtamd_locali_prepare (HIP events) */
} gtamd_locali_info;

typedef struct gtamd_locali gtamd_locali;

/* an aligner on HIP device `device`; NULL on failure.  It keeps its working
   memory between calls; one thread at a time per object. */
gtamd_locali *gtamd_locali_create(int device);
void gtamd_locali_destroy(gtamd_locali *lc);

/* Host only.  jobs_per_workgroup: the waves of a workgroup; min_capacity: the
   smallest capacity gtamd_locali_emit takes; max_query: the letters a query may
   have; min_stack_words: the smallest stack gtamd_locali_set_limits takes (the
   root of a walk alone: every child is then finished in the text).  Any may be
   NULL. */
void gtamd_locali_geometry(uint32_t *jobs_per_workgroup, uint64_t *min_capacity, uint32_t *max_query,
                           uint32_t *min_stack_words);

/* Set the index and cut its table into groups; each call replaces the index
   before and what was prepared.  From device pointers, which stay the caller's
   and must outlive the calls: n symbols, n + 1 entries of suf_bytes = 4 or 8
   bytes, numofchars = sigma (1..32). */
int gtamd_locali_set_index(gtamd_locali *lc, const uint8_t *enc_device, uint64_t n,
                           const void *suf_device, uint32_t suf_bytes, uint32_t numofchars);
/* from HOST memory: uploaded piece by piece into memory the object owns */
int gtamd_locali_set_index_host(gtamd_locali *lc, const uint8_t *enc_host, uint64_t n,
                                const void *suf_host, uint32_t suf_bytes, uint32_t numofchars);
/* the .suf table an engine context holds after gtamd_esa_run with
   GTAMD_WANT_SUF (whole-table build, forward read mode), with the n symbols at
   enc_device.  The context must outlive the calls. */
int gtamd_locali_set_index_esa(gtamd_locali *lc, const gtamd_esa_ctx *esa,
                               const uint8_t *enc_device, uint64_t n, uint32_t numofchars);

/* What the next prepare sizes itself by.  stack_words: the 32-bit words of one
   wave's stack, 0 for the default (32 columns of the longest query and 4096
   words) or min_stack_words .. 2^28; cut_depth: q, GTAMD_LOCALI_AUTO or 0..16 (0:
   the table is one group; beyond what the alphabet allows: the largest it
   allows).  Neither changes a record, nor what is already prepared: the emit
   calls of a prepare go on with the sizes it took. */
int gtamd_locali_set_limits(gtamd_locali *lc, uint32_t stack_words, uint32_t cut_depth);

/* Count and offsets for Q queries (symbols and the Q + 1 offsets in device
   memory when is_device, which then must outlive the emit calls; else host
   memory, copied), the three scores and the threshold.  Refused with a message:
   scores of the wrong sign or beyond 32767, a threshold of 0, and, naming the
   first such query: a query of no or of more than 16384 letters, one with
   match * m > 65535, a symbol that is neither a letter nor the wildcard.  Fills
   *info (may be NULL).  Synchronous. */
int gtamd_locali_prepare(gtamd_locali *lc, const uint8_t *queries, const uint64_t *offsets, uint64_t Q,
                         int is_device, int32_t match, int32_t mismatch, int32_t gapextend,
                         uint32_t threshold, gtamd_locali_info *info);

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
   min_capacity is refused with a message that names it.  Synchronous. */
int gtamd_locali_emit(gtamd_locali *lc, uint64_t *cursor, gtamd_locali_record *out,
                      uint64_t capacity, int out_on_device, uint64_t *written);

/* figures of the last prepare and of the emit calls since */
int gtamd_locali_get_info(const gtamd_locali *lc, gtamd_locali_info *info);

#ifdef __cplusplus
}
#endif
#endif
