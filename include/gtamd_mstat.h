/*
  gtamd_mstat.h -- C ABI of the two simplest questions a suffix array answers,
  `gt matstat -esa INDEX` and `gt uniquesub -esa INDEX` (tool
  src/tools/gt_matstat.c; the reference's suite runs both over its fixtures,
  testsuite/gt_idxsearch_include.rb, createandcheckgreedyfwdmat), on the
  device: one search per query position over tables in device memory.

  What it restates:

    gt_suffixarraymstats, gt_suffixarrayuniqueforward
                                        src/match/esa-minunique.c:26-105
    gt_lcpintervalfindcharchildintv     src/match/esa-splititv.c:24-103
    the loop over the query positions   src/match/greedyfwdmat.c:102-166

  Subject: n symbols enc[0..n) -- letters 0..sigma-1, 254 wildcard, 255
  separator, as the index's read mode reads them -- and their suffix table suf
  of N = n + 1 entries.  Query: m symbols q[0..m) in the same coding.  A
  special in the query ends every match (several query sequences go into one
  call with a separator between them); a special in the subject, and the
  subject's end, never match anything.

  For a query position i, occ(i, l) is the set of table indices whose suffix
  starts with the l letters q[i..i+l): a contiguous interval, empty as soon as
  one of those symbols is a special or lies at or beyond m.

    matching statistics   ms(i) = the largest l with occ(i, l) not empty; 0
                          when q[i] is a special or a letter the subject lacks.
    witness               w(i) = suf[min occ(i, ms(i))], the suffix at the
                          smallest table index (the reference reports
                          suftab[itv.left]); defined for ms(i) > 0, reported
                          as 0 otherwise.
    minimum unique prefix mu(i) = the smallest l >= 1 with |occ(i, l)| == 1; 0
                          if there is none: the prefix stops occurring, or the
                          query ends, before it is unique.
    length cap            max_len > 0: lengths are exact up to max_len; a
                          position whose value exceeds max_len reports
                          max_len + 1, its witness is unspecified (some entry
                          of the table).  0: no cap.

  How it is computed.  One lane per query position.  With Q = q[i..) up to its
  first special, a binary search over the whole table finds lb, the first
  table index whose suffix is not smaller than Q (a query that ends sorts in
  front of everything it is a prefix of; a special of the subject behind every
  letter), carrying the number of letters Q shares with both borders of the
  search, so that a comparison starts where the shorter of the two ends.  With
  L and R the letters Q shares with the suffixes at lb - 1 and lb:

    ms(i) = max(L, R)
    w(i)  = suf[lb] when R > L; otherwise the first index of [0, lb - 1] whose
            suffix shares ms(i) letters with Q: a second binary search
    mu(i) = 0 when L == R; for L > R, with L2 the letters Q shares with the
            suffix at lb - 2: max(R, L2) + 1 if that is at most L, else 0; the
            mirror image with lb + 1 for R > L

  Letters are compared `word_symbols` at a time through 4-byte words wherever
  both sides lie `word_symbols + 4` bytes inside their sequence, byte by byte
  at the borders and for fewer than `word_min` symbols.  With a cap, Q is cut
  to max_len + 1 letters.  For uniquesub a position whose cut Q still occurs
  twice is searched once more without the cut: only that tells mu(i) = 0 from
  mu(i) > max_len.

  No symbol of the subject is read at or beyond n, no table entry at or beyond
  N and no query symbol at or beyond m, whatever the query holds.

  Limits: N <= 2^32 - 4096 (whole-table builds; the slices of a build in parts
  are refused) and at most 2^32 - 1 query symbols per call; both are refused
  with a message, not truncated.

  Conventions as in gtamd_check.h: 0 / -1, message from
  gtamd_esa_last_error().  Plain C; no CPU fallback: -1 without a device.
*/
#ifndef GTAMD_MSTAT_H
#define GTAMD_MSTAT_H

#include <stddef.h>
#include <stdint.h>
#include "gtamd_esa.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
  float device_ms;             /* device time of the last call (HIP events) */
  uint32_t reruns;             /* uniquesub with a cap: positions searched again without it */
  uint64_t positions;          /* query positions of the last call */
  uint64_t symbols_compared;   /* symbol pairs the last call looked at */
  uint64_t device_bytes;       /* device memory the object holds */
} gtamd_mstat_info;

typedef struct gtamd_mstat gtamd_mstat;

/* a searcher on HIP device `device`; NULL on failure.  It keeps its working
   memory between calls; one thread at a time per object. */
gtamd_mstat *gtamd_mstat_create(int device);
void gtamd_mstat_destroy(gtamd_mstat *ms);

/* query positions one workgroup takes, symbols of one wide comparison, and the
   number of symbols from which the wide comparison is used; host only, needs
   no device */
void gtamd_mstat_geometry(uint32_t *tile_positions, uint32_t *word_symbols,
                          uint32_t *word_min);

/* Set the index; each call replaces the one before.
   From device pointers, which stay the caller's and must outlive the searches:
   n symbols, n + 1 entries of suf_bytes = 4 or 8 bytes (.suf with and without
   -suftabuint), numofchars = sigma (1..253). */
int gtamd_mstat_set_index(gtamd_mstat *ms, const uint8_t *enc_device, uint64_t n,
                          const void *suf_device, uint32_t suf_bytes,
                          uint32_t numofchars);
/* from HOST memory (read back from the files of an index, or mapped):
   uploaded piece by piece into memory the object owns */
int gtamd_mstat_set_index_host(gtamd_mstat *ms, const uint8_t *enc_host, uint64_t n,
                               const void *suf_host, uint32_t suf_bytes,
                               uint32_t numofchars);
/* the .suf table an engine context holds after gtamd_esa_run with
   GTAMD_WANT_SUF (whole-table build), with the n symbols at enc_device: the
   sequence as the read mode of the context reads it.  The context must
   outlive the searches. */
int gtamd_mstat_set_index_esa(gtamd_mstat *ms, const gtamd_esa_ctx *esa,
                              const uint8_t *enc_device, uint64_t n,
                              uint32_t numofchars);

/* ms(i) -> length_out[i] and, unless subjectpos_out is NULL, w(i) ->
   subjectpos_out[i], for the m symbols at query (device memory when is_device,
   else host memory); the outputs are device memory when out_is_device.
   Synchronous. */
int gtamd_mstat_matstat(gtamd_mstat *ms, const uint8_t *query, uint64_t m,
                        int is_device, uint32_t max_len, uint32_t *length_out,
                        uint64_t *subjectpos_out, int out_is_device);
/* mu(i) -> length_out[i] */
int gtamd_mstat_uniquesub(gtamd_mstat *ms, const uint8_t *query, uint64_t m,
                          int is_device, uint32_t max_len, uint32_t *length_out,
                          int out_is_device);

/* figures of the last call */
int gtamd_mstat_get_info(const gtamd_mstat *ms, gtamd_mstat_info *info);

#ifdef __cplusplus
}
#endif
#endif
