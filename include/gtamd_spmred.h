/*
  gtamd_spmred.h -- C ABI of the IRREDUCIBLE suffix-prefix matches of a read set:
  the overlaps a string graph keeps, what `gt readjoiner overlap -readset X -l L`
  computes (tool src/tools/gt_readjoiner_overlap.c), from .suf and .lcp
  together, on the device.

  What it restates:

    combine_terminal_with_wset          src/match/rdj-spmfind.c:328-391
      (every terminal suffix of an lcp-interval with every whole read of that
       interval; a match is transitive when the blind trie of the whole read
       holds the reversed left part of a read that matched it deeper)
    gt_blindtrie_retrieve               src/match/sfx-bltrie.c:1250
    GT_READJOINER_IS_CORRECT_REVCOMPL_CASE   src/match/rdj-revcompl-def.h:40-46

  INPUTS, MATCHES.  Those of gtamd_spm.h: the sequences S_0 .. S_(K-1) with a
  separator between two of them, tables of N = n + 1 entries; a match (r, w, l)
  of minimum length L: the last l >= L symbols of S_r are the first l of S_w, all
  letters.  The set of all matches is Z records in the order stated there.

  TRANSITIVE.  Let left(x, k) be S_x without its last k symbols.  A match (r, w,
  l) is transitive if and only if there is a match (t, w, l') with l' > l such
  that left(t, l') is a suffix of left(r, l); the empty string is a suffix of
  every string, and a special equals nothing, so a left part that holds one is
  the suffix of none.  Otherwise it is IRREDUCIBLE.  Ties never reduce: l' = l does not
  count.  The definition names no order of traversal: the reference keeps, per
  whole read w, a trie of the left parts seen so far, deeper intervals first,
  which decides the same thing for a set in which no sequence occurs whole at
  another place of the set (no duplicate, no contained read, no read equal to its
  own reverse complement: the output of `gt readjoiner prefilter`).  For a set
  with such sequences the reference's result depends on its traversal (and an
  equal-length set with a duplicate ends it on an assertion); the library answers
  by the definition as written and counts them: contained_sequences, the read
  starts whose whole length is a terminal suffix of step 1.

  With left(t, l') a suffix of left(r, l) and both matches read on w, the first m
  = |S_t| - l' + l symbols of S_t are the last m of S_r, m >= l: the match from r
  to t that the definition implies is never shorter than l, and so never shorter
  than L.

  MIRRORED.  The set is the mirrored one of R reads (gtamd_mirror of
  gtamd_host.h), K = 2R: sequence s < R is read s, direct; sequence s >= R is read
  K - 1 - s, reverse.  Every overlap occurs as two mirror images; of them the one
  is kept for which, with (sn, sd) the read and direction of the suffix sequence
  and (pn, pd) of the prefix sequence,

    (sd and pd) or (sn = pn and (sd or pd)) or (sd and not pd and pn > sn) or
    (not sd and pd and pn < sn).

  The transitive test comes first and runs on all K sequences; the filter then
  drops a record whether it is irreducible or not.

  KEPT.  A record of the Z is kept when it is irreducible (with
  GTAMD_SPMRED_ELIMTRANS; all are without it) and passes the filter (with
  GTAMD_SPMRED_MIRRORED; all do without it).

  RECORD.  { suffix_read, prefix_read, len, flags }, four uint64.  flags is
  GTAMD_SPMRED_SUFFIX_DIRECT | GTAMD_SPMRED_PREFIX_DIRECT, the low two bits of
  the third word of Readjoiner's binary lists.  Without MIRRORED the two numbers
  are sequence numbers and both bits are set.

  ORDER.  The order of gtamd_spm.h restricted to the kept records: ascending
  table index of the suffix of the suffix sequence, then ascending table index of
  the start of the prefix sequence.  Deterministic: two calls give the same
  bytes.  It is not the reference's order; outputs are compared as sorted lines.

  How it is computed (genometools_amd/csrc/esa_spmred.hip, esa_spmred_core.h;
  DESIGN.md 9m).  The object owns a gtamd_spm and runs its steps 1 to 4.  Then

    5 group      position and length of the sequence of every read start; the
                 terminal suffixes sorted by text position (radix sort of
                 esa_prims), which puts those of one sequence side by side, the
                 longest first, with the permutation back to table order
    6 decide     one lane per pair (terminal suffix of r with l letters, read
                 start w), in the pair numbering of step 4, in chunks: the lane
                 walks the terminal suffixes of r of m >= l letters, longest
                 first, and the read starts t inside the interval of each; t
                 proves the pair transitive when |t| > m, |t| - m + l <= |w| and
                 t[m .. |t|) = w[l .. |t| - m + l).  It stops at the first that
                 does, and evaluates the filter.  The 64 verdicts of a wave are
                 one ballot, stored as one word of a bitmap of Z bits
    7 place      the set bits of every word, and a 64-bit exclusive scan over
                 the words: `kept`, and the place of every word's first record
    8 emit       in chunks, one lane per kept record: the word by a search in
                 the scanned places, the pair by a select in the word, then as
                 step 5 of gtamd_spm.h, then read numbers and directions

  Working memory beside the gtamd_spm's: 8 bytes per read start, 16 per terminal
  suffix and the sort's workspace, and for Z pairs Z / 8 bytes of bitmap, Z / 16
  of counts and Z / 8 of places.

  A pair's walk is as long as the other overlaps of its read are many: in a
  homopolymer or a tandem repeat every m is a terminal suffix and every interval
  is wide.  That is load imbalance, not an error; the info reports it
  (candidates_examined, max_candidates_of_one_pair, letters_compared).

  LIMITS.  Those of gtamd_spm.h, and Z <= 2^38 - 2^14 (the words of the bitmap
  are scanned as 32-bit counts); a larger Z, or one whose bitmap cannot be
  allocated, is refused with a message that names the bytes.

  Conventions as in gtamd_spm.h: 0 / -1, message from gtamd_esa_last_error().
  Plain C; no CPU fallback: -1 without a device.
*/
#ifndef GTAMD_SPMRED_H
#define GTAMD_SPMRED_H

#include <stddef.h>
#include <stdint.h>
#include "gtamd_esa.h"

#ifdef __cplusplus
extern "C" {
#endif

/* flags of gtamd_spmred_prepare */
#define GTAMD_SPMRED_ELIMTRANS 1u
#define GTAMD_SPMRED_MIRRORED  2u
/* flags of a record */
#define GTAMD_SPMRED_PREFIX_DIRECT 1u
#define GTAMD_SPMRED_SUFFIX_DIRECT 2u

typedef struct { uint64_t suffix_read, prefix_read, len, flags; } gtamd_spmred_record;

typedef struct {
  /* the figures of gtamd_spm_info */
  uint64_t table_entries, terminal_suffixes, read_starts;
  uint64_t matches;                     /* Z: the pairs decided */
  uint64_t max_width, max_matches_of_one_suffix, search_symbols;
  /* the reduction */
  uint64_t kept;                        /* records the emit calls will give */
  uint64_t transitive_same_read;        /* transitive pairs of one read with itself (MIRRORED: on either strand) */
  uint64_t transitive_other;            /* the other transitive pairs; both counted before the filter */
  uint64_t contained_sequences;         /* read starts whose whole length is a terminal suffix */
  uint64_t candidates_examined;         /* read starts the walks looked at */
  uint64_t max_candidates_of_one_pair;
  uint64_t letters_compared;            /* symbol comparisons of the walks */
  uint64_t device_bytes;                /* device memory the object holds, its gtamd_spm included */
  float device_ms;                      /* device time of gtamd_spmred_prepare (HIP events) */
  float spm_ms;                         /* of which steps 1 to 4 */
  float decide_ms;                      /* of which step 6 */
} gtamd_spmred_info;

typedef struct gtamd_spmred gtamd_spmred;

gtamd_spmred *gtamd_spmred_create(int device);
void gtamd_spmred_destroy(gtamd_spmred *sr);

/* Host only.  chunk_pairs: pairs of one launch of step 6, a multiple of 64;
   min_capacity: the smallest capacity gtamd_spmred_emit takes.  Either may be NULL. */
void gtamd_spmred_geometry(uint64_t *chunk_pairs, uint64_t *min_capacity);

/* the index, in the three ways of gtamd_spm.h */
int gtamd_spmred_set_index(gtamd_spmred *sr, const uint8_t *enc_device, uint64_t n,
                           const void *suf_device, uint32_t suf_bytes,
                           const uint8_t *lcp_device, const uint64_t *llv_device,
                           uint64_t llv_pairs);
int gtamd_spmred_set_index_host(gtamd_spmred *sr, const uint8_t *enc_host, uint64_t n,
                                const void *suf_host, uint32_t suf_bytes,
                                const uint8_t *lcp_host, const uint64_t *llv_host,
                                uint64_t llv_pairs);
int gtamd_spmred_set_index_esa(gtamd_spmred *sr, const gtamd_esa_ctx *esa,
                               const uint8_t *enc_device, uint64_t n);

/* steps 1 to 7 for minimum length min_len >= 1 and flags (GTAMD_SPMRED_*);
   MIRRORED needs an even number of sequences.  Fills *info (may be NULL).
   Synchronous. */
int gtamd_spmred_prepare(gtamd_spmred *sr, uint32_t min_len, uint32_t flags, gtamd_spmred_info *info);

/* Step 8, in pieces, as gtamd_spm_emit: *cursor counts the KEPT records, 0 to
   `kept` of the info; a value beyond is refused with a message, and so is a
   capacity below min_capacity. */
int gtamd_spmred_emit(gtamd_spmred *sr, uint64_t *cursor, gtamd_spmred_record *out,
                      uint64_t capacity, int out_on_device, uint64_t *written);

/* figures of the last prepare */
int gtamd_spmred_get_info(const gtamd_spmred *sr, gtamd_spmred_info *info);

#ifdef __cplusplus
}
#endif
#endif
