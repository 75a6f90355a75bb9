/*
  gtamd_kcorrect.h -- C ABI of the K-MER CORRECTION of a read set: which letters
  `gt readjoiner correct -k K -c C -ii INDEX` rewrites, decided and applied on
  the device from .suf and .lcp of the (mirrored) read set (tool
  src/tools/gt_readjoiner_correct.c, src/match/rdj-errfind.c,
  src/match/rdj-twobitenc-editor.c, traversal src/match/esa-bottomup-errfind.inc).

  INPUT.  The text T of n symbols is either reads joined by separators (255) or
  their MIRRORED set: the reads, a separator, the reverse complement of the
  whole (gtamd_mirror, gtamd_contained_mirror).  Letters are 0..3, specials 254
  and 255.  The tables are .suf and .lcp of T: specials sort after letters, an
  LCP never spans a special, and only the N non-special suffixes, table entries
  0 .. N - 1, take part.  lcp[i] is the common prefix of entries i - 1 and i.

  GROUPS AND CHILDREN, for k >= 2.  A group is a maximal run of entries i .. j - 1
  with lcp[i] < k - 1 and lcp[x] >= k - 1 for i < x < j: the suffixes that share
  their first k - 1 letters.  A group of one entry, or one whose inner LCP values
  all reach k, is skipped: it has no interval of depth k - 1.  A child of a group
  is a maximal run inside it with inner lcp >= k: one k-mer, whose count is its
  width.  A child is valid if the k-th symbol of its suffixes, T[suf + k - 1], is
  a letter; the invalid children are single entries and stand last in the
  group, so at most 4 children are valid.

  RULE for one group.  If all four letters are present as valid children and
  every count is >= c, nothing happens.  Otherwise the trusted child is the
  FIRST valid child in table order with count >= c (not the largest); without
  one nothing happens.  Otherwise every valid child with count < c gives one
  record per entry e of it: target suf[e] + k - 1, source suf[head of the
  trusted child] + k - 1.  The records of the table are ordered by e.

  APPLYING the records, one after the other.  A position p >= firstmirror is
  normalised to n - 1 - p with the letter complemented (3 - x); firstmirror is
  n >> 1 for a mirrored text and n otherwise.  The letter written is the letter
  that stands at the source when the record's GROUP is reached, complemented as
  source and target require: the reference edits the sequence file through a
  second shared mapping of the file its traversal reads, so a source that a
  record of an EARLIER group wrote gives the written letter, and it reads the
  trusted letter once per group, before that group's own records.  The last
  record of a position wins.  k = 1, k beyond the read length and a set without
  a trusted k-mer give no record.

  All of this is pinned by the reference itself: tests/golden/golden_correct.json
  holds its results on sets where reading the sources from the original text, or
  once per record, gives other reads (tests/golden/make_golden_correct.py).

  How it is computed (genometools_amd/csrc/esa_kcorrect.hip, esa_kcorrect_core.h):

    1 heads     one lane per entry below N reads lcp[i] as a byte stream and
                flags child heads (lcp[i] < k); a tile's flags are counted by
                ballot, so that the 64-bit offsets scan (esa_prims) needs no
                launch of its own for the sums
    2 children  the table indices of the heads, compacted; a child's width is
                the distance to the next head
    3 groups    one lane per child: group start (lcp[head] < k - 1), validity
                (one load of T[suf[head] + k - 1]), at most 3 children to the
                left for the group's first, to the right up to the first invalid
                child or the next group: counts, the all-trusted test, the
                trusted child; an untrusted child reports its records
    4 emit      the record counts scanned; (entry, target, source) per record,
                positions normalised with their complement bits, and the first
                record of the record's group
    5 resolve   the records sorted by (target, order) with radix_sort_pairs on
                the digits the text length and the record count need; every
                record searches the sorted list for the last record in front of
                its group that wrote its source; those without one take the
                original letter, the others follow their chain by pointer
                doubling with the parity of the complements (a dependency
                points to an earlier record: the chains are a forest); the last
                record of every target gives the final letter, and the changed
                positions and letter counts are tallied per wave
    6 apply     one lane per final (position, letter) writes into a copy of the
                symbols

  Working memory: 12 bytes per non-special suffix for flags and places, 4 per
  child head plus 12 per child, about 50 per record.

  LIMITS.  Only .suf (4- or 8-byte entries) and the byte table .lcp are read:
  a byte of 255 means ">= 255" and the rule only asks >= k - 1 and >= k, so .llv
  is not needed and 1 <= k <= 255; k >= 256 is refused in words.  c >= 1.
  Otherwise the limits of gtamd_spm.h for the text.  Wildcards and reads of
  several lengths are accepted (a child whose k-th symbol is a wildcard is
  invalid); only the tool keeps the reference's restriction to one length.

  Conventions as in gtamd_spm.h: 0 / -1, message from gtamd_esa_last_error().
  Plain C; no CPU fallback: -1 without a device.
*/
#ifndef GTAMD_KCORRECT_H
#define GTAMD_KCORRECT_H

#include <stddef.h>
#include <stdint.h>
#include "gtamd_esa.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GTAMD_KCORRECT_MAX_K 255u

typedef struct {
  uint64_t table_entries;       /* n + 1 */
  uint64_t suffixes;            /* N: the non-special suffixes */
  uint64_t groups;              /* groups examined: those with an interval of depth k - 1 */
  uint64_t untrusted_groups;    /* of which give records */
  uint64_t records;
  uint64_t dependent;           /* records whose source an earlier record wrote */
  uint64_t rounds;              /* rounds of the pointer doubling */
  uint64_t changed;             /* positions whose final letter differs from the original */
  int64_t delta[4];             /* change of the four letter counts */
  uint64_t device_bytes;        /* device memory the object holds */
  float device_ms;              /* device time of gtamd_kcorrect_decide (HIP events) */
  uint32_t k, c;                /* of the last decide */
} gtamd_kcorrect_info;

typedef struct gtamd_kcorrect gtamd_kcorrect;

gtamd_kcorrect *gtamd_kcorrect_create(int device);
void gtamd_kcorrect_destroy(gtamd_kcorrect *kc);

/* Host only.  tile_entries: table entries, children or records of one workgroup. */
void gtamd_kcorrect_geometry(uint32_t *tile_entries);

/* The index, in the three ways of gtamd_spm.h; mirrored != 0: the text is a
   mirrored set (odd n, a separator in the middle: anything else is refused). */
int gtamd_kcorrect_set_index(gtamd_kcorrect *kc, const uint8_t *enc_device, uint64_t n,
                             const void *suf_device, uint32_t suf_bytes, const uint8_t *lcp_device,
                             int mirrored);
int gtamd_kcorrect_set_index_host(gtamd_kcorrect *kc, const uint8_t *enc_host, uint64_t n,
                                  const void *suf_host, uint32_t suf_bytes, const uint8_t *lcp_host,
                                  int mirrored);
int gtamd_kcorrect_set_index_esa(gtamd_kcorrect *kc, const gtamd_esa_ctx *esa,
                                 const uint8_t *enc_device, uint64_t n, int mirrored);

/* steps 1 to 5.  Fills *info (may be NULL).  Synchronous. */
int gtamd_kcorrect_decide(gtamd_kcorrect *kc, uint32_t k, uint32_t c, gtamd_kcorrect_info *info);

/* the records of the last decide in record order, three 64-bit numbers each:
   table entry, normalised position, letter written; to host or device memory
   with room for info.records of them */
int gtamd_kcorrect_records(const gtamd_kcorrect *kc, uint64_t *out, int out_on_device);

/* Step 6: the corrected UNMIRRORED symbols.  enc_device: the symbols to correct,
   n of them (the first half of a mirrored index, the whole of an unmirrored
   one), device memory; NULL: those of the index.  *out_device: the result,
   *out_n symbols, device memory of the object that the next apply overwrites. */
int gtamd_kcorrect_apply(gtamd_kcorrect *kc, const uint8_t *enc_device, uint64_t n,
                         uint8_t **out_device, uint64_t *out_n);

/* the symbols of the last apply, copied to host or device memory of the caller's */
int gtamd_kcorrect_result(const gtamd_kcorrect *kc, uint8_t *out, int out_on_device);

/* figures of the last decide */
int gtamd_kcorrect_get_info(const gtamd_kcorrect *kc, gtamd_kcorrect_info *info);

#ifdef __cplusplus
}
#endif
#endif
