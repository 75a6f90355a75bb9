/*
  gtamd_check.h -- C ABI of the index checker: `gt dev sfxmap -suf -lcp -bwt
  -esa INDEX` for this path (tool src/tools/gt_sfxmap.c; the reference's test
  suite runs it after nearly every suffixerator call,
  testsuite/gt_suffixerator_include.rb:57-69).

  What it restates: the reference's linear-time checkers

    gt_suftab_lightweightcheck   src/match/sfx-lwcheck.c:181-337
    gt_lcptab_lightweightcheck   src/match/sfx-linlcp.c:548
    the BWT the driver writes    src/match/sfx-run.c:173-210

  as kernels over tables in device memory: every entry of .suf, .lcp, .llv and
  .bwt is checked against the encoded sequence, in time linear in the length.
  The tables of a sequence are unique, so a set of tables is accepted exactly
  when it is the index of the sequence.

  Notation: n symbols enc[0..n), N = n + 1 table entries; a symbol >= 254 is a
  special; "the end" is position n and every position beyond it, and counts as
  a special.  c(p) is the letter at p, or 256 + p for a special and for the
  end (specials are unique and larger than every letter, larger at larger
  positions: src/core/encseq.h:640, src/match/sfx-bentsedg.c:75-80).

  The criteria, in the order they are applied.  The first one that fails ends
  the check and is reported; `index` is the smallest index that fails it, so
  the report does not depend on the order the device works in.

  1 SUF, range and permutation (GTAMD_CHECK_SUF)
      CRIT_RANGE  suf[i] <= n for every table index i; index = i.
      CRIT_PERM   with rank[] filled with a sentinel and then rank[suf[i]] = i
                  written for every i: rank[p] is set and suf[rank[p]] == p for
                  every position p in [0, n]; index = p, a POSITION (a value
                  that is missing from the table, or one of a duplicate's
                  losers).  claimed = rank[p] (2^32 - 1: missing).
      A damaged table is never used as an index after this point: 2 to 5 run
      only on a table that is a permutation of [0, n].
  2 SUF, order (GTAMD_CHECK_SUF, CRIT_ORDER): for every i >= 1, with
      a = suf[i-1], b = suf[i]: c(a) < c(b), or c(a) == c(b) is a letter and
      rank[a+1] < rank[b+1].  index = i, pos_a = a, pos_b = b.  (Sortedness is
      this local property once the table is a permutation: induction over the
      common prefix.)
  3 BWT (GTAMD_CHECK_BWT, CRIT_BWT): bwt[i] == (suf[i] ? enc[suf[i]-1] : 254);
      index = i, pos_b = suf[i], claimed = bwt[i], found = the expected symbol.
  4 LCP and LLV, structure.  .llv is m pairs (table index, value).
      CRIT_LCP0     (GTAMD_CHECK_LCP) lcp[0] == 0; index = 0.
      CRIT_LLV_ENTRY (GTAMD_CHECK_LLV) for every pair j: its index lies in
                  [1, n] and is larger than the index of pair j-1, lcp[index]
                  == 255, its value lies in [255, n].  llv_entry = j, index =
                  the table index the pair names, claimed = its value.
      CRIT_LLV_MISSING (GTAMD_CHECK_LLV) the number of bytes 255 in .lcp equals
                  m, that is (after the pairs passed) every byte 255 has its
                  pair.  index = the first table index with a byte 255 and no
                  pair, llv_entry = where the pair would stand.
  5 LCP and LLV, every value (GTAMD_CHECK_LCP where the byte is < 255,
      GTAMD_CHECK_LLV where the value comes from .llv): Kasai's inheritance
      argument (src/match/sfx-linlcp.c) as a check.  C[i] is the claimed value
      of table index i: the byte, or the value of the pair found by binary
      search where the byte is 255.  For every position p with rank[p] >= 1,
      q = suf[rank[p]-1]:
      (a) suffixes p and q do not hold equal letters at offset C[rank[p]]
          (they differ, or one meets a special or the end there);
      (b) they hold equal letters at every offset in [s, C[rank[p]]), with
          s = max(C[rank[p-1]] - 1, 0), and s = 0 for p = 0 and for
          rank[p-1] = 0.  Offsets below s agree by induction over p: suffixes
          suf[rank[p-1]-1] + 1 and p share C[rank[p-1]] - 1 symbols and q lies
          between them in the table.
      index = rank[p], the smallest table index for which (a) or (b) fails;
      pos_a = q, pos_b = p, claimed = C[index], found = the length of the
      common prefix of letters of the two suffixes, counted from offset 0;
      CRIT_LCP_SMALL when claimed < found, CRIT_LCP_LARGE when claimed > found.
      (b) compares at most 2N symbol pairs on a correct table, unevenly: the
      position at the start of a long repeat compares the whole repeat.  A
      position whose range [s, C) is longer than `long_claim` symbols goes to
      a work list that whole workgroups compare with wide loads, leaving at
      the first difference; every other position is one lane.

  No symbol is read at or beyond position n: such an offset is the end.

  Device memory beyond the tables: the 4N-byte inverse, the work list of at
  most 2N / long_claim + 1 positions of 4 bytes, and a few words.

  Conventions as in gtamd_esa.h: 0 / -1, message from gtamd_esa_last_error().
  0 means the check RAN; its verdict is report.ok.  -1: it could not run (no
  device, tables that are a slice of a part build, more than 2^32 - 4096
  entries, out of memory).  Plain C; no CPU fallback.
*/
#ifndef GTAMD_CHECK_H
#define GTAMD_CHECK_H

#include <stddef.h>
#include <stdint.h>
#include "gtamd_esa.h"

#ifdef __cplusplus
extern "C" {
#endif

/* report.table, and the bits of report.checked */
#define GTAMD_CHECK_SUF 1
#define GTAMD_CHECK_LCP 2
#define GTAMD_CHECK_LLV 4
#define GTAMD_CHECK_BWT 8

/* report.criterion */
#define GTAMD_CHECK_CRIT_NONE        0
#define GTAMD_CHECK_CRIT_RANGE       1
#define GTAMD_CHECK_CRIT_PERM        2
#define GTAMD_CHECK_CRIT_ORDER       3
#define GTAMD_CHECK_CRIT_BWT         4
#define GTAMD_CHECK_CRIT_LCP0        5
#define GTAMD_CHECK_CRIT_LLV_ENTRY   6
#define GTAMD_CHECK_CRIT_LLV_MISSING 7
#define GTAMD_CHECK_CRIT_LCP_SMALL   8   /* the suffixes share more than the claim */
#define GTAMD_CHECK_CRIT_LCP_LARGE   9   /* the suffixes share less than the claim */

#define GTAMD_CHECK_NONE (~(uint64_t) 0)   /* a field of the report without a value */
#define GTAMD_CHECK_PHASES 5               /* criteria 1 to 5 above */

typedef struct {
  int32_t ok;               /* 1: every table handed in is accepted */
  uint32_t table;           /* GTAMD_CHECK_* of the table that fails, 0 when ok */
  uint32_t criterion;       /* GTAMD_CHECK_CRIT_* */
  uint32_t checked;         /* GTAMD_CHECK_* of the tables handed in */
  uint64_t index;           /* as the criterion defines it */
  uint64_t llv_entry;       /* pair of .llv involved, or GTAMD_CHECK_NONE */
  uint64_t pos_a, pos_b;    /* the two suffixes involved, or GTAMD_CHECK_NONE */
  uint64_t claimed, found;  /* or GTAMD_CHECK_NONE */
  /* what INDEX.prj says about the tables; valid for the phases that ran */
  uint64_t longest;         /* table index of suffix 0 (phase 1) */
  uint64_t largelcpvalues;  /* bytes 255 in .lcp (phase 4) */
  uint64_t maxbranchdepth;  /* largest claimed value (phase 5) */
  uint64_t long_claims;     /* positions that went to the work list */
  float check_ms;           /* device time of the whole check (HIP events) */
  float phase_ms[GTAMD_CHECK_PHASES];   /* 0 for a phase that did not run */
} gtamd_check_report;

typedef struct gtamd_check gtamd_check;

/* a checker on HIP device `device`; NULL on failure.  It keeps its working
   memory between checks; one thread at a time per checker. */
gtamd_check *gtamd_check_create(int device);
void gtamd_check_destroy(gtamd_check *chk);

/* table entries one workgroup takes, and the length of a range (b) from which
   a position goes to the work list; host only, needs no device */
void gtamd_check_geometry(uint32_t *tile_entries, uint32_t *long_claim);

/* Check device-resident tables of the n symbols at enc: suf (n + 1 entries of
   suf_bytes = 4 or 8 bytes, .suf with and without -suftabuint), and, each
   optional (NULL), lcp (n + 1 bytes) with llv (llv_pairs pairs of two uint64;
   may be NULL when llv_pairs is 0) and bwt (n + 1 bytes).  Synchronous. */
int gtamd_check_tables(gtamd_check *chk, const uint8_t *enc_device, uint64_t n,
                       const void *suf_device, uint32_t suf_bytes,
                       const uint8_t *lcp_device, const uint64_t *llv_device,
                       uint64_t llv_pairs, const uint8_t *bwt_device,
                       gtamd_check_report *report);

/* the same from HOST memory (tables read back from the files of an index, or
   mapped): uploaded piece by piece, then checked as above */
int gtamd_check_tables_host(gtamd_check *chk, const uint8_t *enc_host, uint64_t n,
                            const void *suf_host, uint32_t suf_bytes,
                            const uint8_t *lcp_host, const uint64_t *llv_host,
                            uint64_t llv_pairs, const uint8_t *bwt_host,
                            gtamd_check_report *report);

/* the tables an engine context holds after gtamd_esa_run (whole-table build;
   `want`: GTAMD_WANT_SUF, which is required, | GTAMD_WANT_LCP | GTAMD_WANT_BWT,
   each produced by the run), against the n symbols at enc_device: the sequence
   the tables describe, that is, as the read mode of the context reads it */
int gtamd_check_esa(gtamd_check *chk, const gtamd_esa_ctx *esa,
                    const uint8_t *enc_device, uint64_t n, uint32_t want,
                    gtamd_check_report *report);

/* the report as one line of text ("" when ok); returns the length the text
   has, as snprintf does.  Host only. */
int gtamd_check_message(const gtamd_check_report *report, char *buf, size_t buflen);

#ifdef __cplusplus
}
#endif
#endif
