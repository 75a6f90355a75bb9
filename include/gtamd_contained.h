/*
  gtamd_contained.h -- C ABI of the CONTAINED READS of a read set: which reads
  are duplicates of, or stand whole inside, another read on either strand, and
  the read set without them, decided and compacted on the device.  It is the
  decision of `gt readjoiner prefilter` (tool src/tools/gt_readjoiner_prefilter.c,
  src/match/rdj-contfinder.c), the step in front of `gt readjoiner overlap`.

  INPUT.  R reads of letters (symbols 0..3), numbered in input order, a separator
  (255) between two of them; no read is empty and none holds a wildcard (254):
  gtamd_contained_drop_wildcards makes such a set.  rc(x) is the reverse
  complement of x.  The decision reads the tables of the MIRRORED set of the
  reads (gtamd_contained_mirror, gtamd_mirror of gtamd_host.h): 2R sequences,
  sequence s < R read s, sequence s >= R the reverse complement of read 2R - 1 - s.

  VERDICT.  Every read a gets exactly one, the first that applies:

    GTAMD_CONTAINED_DUPLICATE           some read b < a has b = a or rc(b) = a
    GTAMD_CONTAINED_AFFIX               a is a proper prefix or a proper suffix of
                                        another read or of the reverse complement
                                        of another read
    GTAMD_CONTAINED_INTERNAL            a stands strictly inside another read or
                                        its reverse complement: neither at its
                                        start nor at its end
    GTAMD_CONTAINED_SELF_COMPLEMENTARY  a = rc(a)
    GTAMD_CONTAINED_KEPT                otherwise

  TIE RULE.  Of a class of equal reads (up to reverse complement) the
  lowest-numbered one is no DUPLICATE, as in gt_contfinder_mark_as_contained; it
  may still get one of the other verdicts.

  MASKS.  GTAMD_CONTAINED_MASK_DEFAULT drops DUPLICATE and AFFIX: the reference's
  suffix-prefix-free set.  In a set of reads of one length only DUPLICATE can
  occur.  GTAMD_CONTAINED_MASK_STRICT drops INTERNAL and SELF_COMPLEMENTARY as
  well.  What is left is exactly a set in which no sequence stands whole at
  another place on either strand: the set for which the irreducible matches of
  gtamd_spmred.h are the reference's (contained_sequences = 0 there).

  THE REFERENCE is pinned by this definition where it is reliable, and is no
  yardstick elsewhere.  Measured against a brute force of the definition on
  seeded sets of 60 to 80 reads with planted duplicates, reverse-complement
  duplicates, prefixes, suffixes, inner pieces and self-complementary reads:
  for reads of one length (36 letters, 40 seeds, and one read 70 times on both
  strands) its kept reads are the definition's in every run.  For reads of 20 to
  60 letters (40 seeds) 3 runs end on an assertion (reads2twobit.c:1973), 32 of
  the other 37 keep reads the definition removes -- duplicates that are also a
  prefix or suffix of a third read among them --, none removes a read the
  definition keeps, and in 12 the sequence file written decodes to something
  other than the reads listed with -fasta.  Sets of reads of 3 or 4 letters that
  are almost all duplicates end on the same assertion.

  How it is computed (genometools_amd/csrc/esa_contained.hip,
  esa_contained_core.h).  The object owns a gtamd_spm and runs its
  steps 1 and 2 for the read starts and the separators.  Then

    3 starts    one lane per read start: position and length of its sequence
    4 images    one lane per sequence of the 2R.  With m letters at table entry
                i: if neither LCP value beside i reaches m, the letters stand
                nowhere else (two byte loads, and most lanes end here).
                Otherwise the interval of the m letters and the read starts
                inside it: a separator is larger than every letter, so the
                longer sequences come first and the whole sequences equal to
                this one last, in text order -- direct copies by ascending read
                number, then mirror images by descending read number.  The
                lowest read of the class is read off the first and the last of
                that run, found by a search over the lengths: a run of k copies
                costs k lanes a few searches each, none looks at the others.
                A longer sequence in the interval: the read is a proper prefix.
                An interval wider than its read starts: it stands elsewhere.
    5 verdicts  one lane per read: the two images of a read give its verdict (a
                suffix is the prefix of the mirror image); counted per class by
                a ballot and one atomic per wave
    compact     the kept lengths, each + 1 for a separator, scanned in 64 bits
                (esa_prims); one lane per symbol of the result finds its read by
                a search in the scanned places and copies a letter or sets the
                separator

  Working memory beside the gtamd_spm's: 8 bytes per sequence, 1 per sequence
  and per read, 12 per read and the result for a compaction.

  LIMITS.  Those of gtamd_spm.h for the mirrored set (2n + 1 symbols below 2^32 -
  4096, so the reads are far fewer than 2^32 - 1; more are refused).  A set
  with an odd number of sequences, with an empty sequence or with one that
  starts with a wildcard is refused in words.

  Conventions as in gtamd_spm.h: 0 / -1, message from gtamd_esa_last_error().
  Plain C; no CPU fallback: -1 without a device.
*/
#ifndef GTAMD_CONTAINED_H
#define GTAMD_CONTAINED_H

#include <stddef.h>
#include <stdint.h>
#include "gtamd_esa.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GTAMD_CONTAINED_KEPT               0u
#define GTAMD_CONTAINED_DUPLICATE          1u
#define GTAMD_CONTAINED_AFFIX              2u
#define GTAMD_CONTAINED_INTERNAL           3u
#define GTAMD_CONTAINED_SELF_COMPLEMENTARY 4u
#define GTAMD_CONTAINED_VERDICTS           5u

#define GTAMD_CONTAINED_MASK_DEFAULT (1u << GTAMD_CONTAINED_DUPLICATE | 1u << GTAMD_CONTAINED_AFFIX)
#define GTAMD_CONTAINED_MASK_STRICT  (GTAMD_CONTAINED_MASK_DEFAULT | 1u << GTAMD_CONTAINED_INTERNAL | \
                                      1u << GTAMD_CONTAINED_SELF_COMPLEMENTARY)

typedef struct {
  uint64_t table_entries;               /* N of the mirrored set */
  uint64_t sequences;                   /* 2R */
  uint64_t reads;                       /* R */
  uint64_t count[GTAMD_CONTAINED_VERDICTS];   /* reads of every verdict */
  uint64_t device_bytes;                /* device memory the object holds, its gtamd_spm included */
  float device_ms;                      /* device time of gtamd_contained_decide (HIP events) */
  float lists_ms;                       /* of which steps 1 and 2 */
} gtamd_contained_info;

typedef struct gtamd_contained gtamd_contained;

gtamd_contained *gtamd_contained_create(int device);
void gtamd_contained_destroy(gtamd_contained *ct);

/* Host only.  tile_reads: reads, sequences or symbols of one workgroup, one a lane. */
void gtamd_contained_geometry(uint32_t *tile_reads);

/* the index of the MIRRORED set, in the three ways of gtamd_spm.h */
int gtamd_contained_set_index(gtamd_contained *ct, const uint8_t *enc_device, uint64_t n,
                              const void *suf_device, uint32_t suf_bytes,
                              const uint8_t *lcp_device, const uint64_t *llv_device,
                              uint64_t llv_pairs);
int gtamd_contained_set_index_host(gtamd_contained *ct, const uint8_t *enc_host, uint64_t n,
                                   const void *suf_host, uint32_t suf_bytes,
                                   const uint8_t *lcp_host, const uint64_t *llv_host,
                                   uint64_t llv_pairs);
int gtamd_contained_set_index_esa(gtamd_contained *ct, const gtamd_esa_ctx *esa,
                                  const uint8_t *enc_device, uint64_t n);

/* the verdict of every read.  Fills *info (may be NULL).  Synchronous. */
int gtamd_contained_decide(gtamd_contained *ct, gtamd_contained_info *info);

/* the R verdicts of the last decide, one byte a read, to host or device memory */
int gtamd_contained_verdicts(const gtamd_contained *ct, uint8_t *out, int out_on_device);

/* The reads without those whose verdict is a bit of mask (GTAMD_CONTAINED_MASK_*),
   in input order, a separator between two.  enc_device: the n symbols of the
   UNMIRRORED reads, device memory; NULL: the first half of the index, which is
   them.  *out_device: the result, *out_n symbols (0: no read is left), device
   memory of the object that the next call of compact or drop_wildcards
   overwrites.  Synchronous. */
int gtamd_contained_compact(gtamd_contained *ct, uint32_t mask, const uint8_t *enc_device, uint64_t n,
                            uint8_t **out_device, uint64_t *out_n);

/* the symbols of the last compact or drop_wildcards, copied to host or device
   memory of the caller's with room for *out_n of them */
int gtamd_contained_result(const gtamd_contained *ct, uint8_t *out, int out_on_device);

/* figures of the last decide */
int gtamd_contained_get_info(const gtamd_contained *ct, gtamd_contained_info *info);

/* The mirrored set of n symbols in device memory: the symbols, a separator, the
   symbols reversed with every letter complemented (3 - c below 254), 2n + 1
   symbols to out_device.  What gtamd_mirror of gtamd_host.h does on the host.
   Needs no index. */
int gtamd_contained_mirror(gtamd_contained *ct, const uint8_t *enc_device, uint64_t n, uint8_t *out_device);

/* The first filter: the n symbols at enc_device without the reads that hold a
   wildcard (254), by the same compaction.  separators_host: the ascending
   positions of the separators of the set, host memory, count of them (the
   reads are count + 1), as gtamd_encoder_get_separators hands them out;
   positions that do not ascend or lie beyond n are refused.  *out_device,
   *out_n as for compact; *dropped (may be NULL) = the reads that went.  Needs
   no index. */
int gtamd_contained_drop_wildcards(gtamd_contained *ct, const uint8_t *enc_device, uint64_t n,
                                   const uint64_t *separators_host, uint64_t count,
                                   uint8_t **out_device, uint64_t *out_n, uint64_t *dropped);

/* the flags of the last drop_wildcards, one byte a read of its input: 1 for a
   read that went */
int gtamd_contained_wildcard_flags(const gtamd_contained *ct, uint8_t *out, int out_on_device);

/* The mirrored set of the symbols of the last compact or drop_wildcards, made
   where they lie: *out_device, *out_n = 2 * (their number) + 1 symbols, device
   memory of the object that the next call of this function overwrites and that
   may be the sequence of an engine and the index of this object. */
int gtamd_contained_mirror_result(gtamd_contained *ct, uint8_t **out_device, uint64_t *out_n);

#ifdef __cplusplus
}
#endif
#endif
