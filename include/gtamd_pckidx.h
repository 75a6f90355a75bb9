/*
  gtamd_pckidx.h -- C ABI of the reader of the packed index: what opens an
  INDEX.bdx image (this project's, include/gtamd_pck.h, or one `gt packedindex
  mkindex` / `trsuftab` wrote) and answers on the device what the reference's
  BWTSeq answers on the host -- the BWT symbol of a row, the occurrences of a
  letter before a row, the text position of a row -- and `gt matstat -pck` and
  `gt uniquesub -pck` through it.

  What it restates:

    the block decoder                   src/match/eis-blockcomp.c (blockCompSeqGet,
                                        blockCompSeqPosPairRank), eis-seqblocktranslate.c
    locate                              gt_BWTSeqLocateMatch, gt_BWTSeqPosHasLocateInfo,
                                        gt_BWTSeqGetRankSort
                                        src/match/eis-bwtseq-extinfo.c:674-823
    LF                                  BWTSeqLFMap src/match/eis-bwtseq-siop.h:180-213
    the two searches                    gt_packedindexmstatsforward,
                                        gt_packedindexuniqueforward
                                        src/match/eis-bwtseq.c:225-364
    the witness                         gt_voidpackedfindfirstmatchconvert
                                        src/match/eis-voiditf.c:428-438

  Geometry.  All of it comes from the image's own headers: block size, blocks
  per bucket, alphabet size, the widths of the occurrence counters, of the var
  offsets and of the composition indices, the locate flavour (bitmap or counts,
  reversibly sorted specials), the locate interval, the row of suffix 0 and the
  region list of the specials.  Before a kernel runs the host checks every
  header field the kernels index with, that the records, the var parts and the
  region list lie inside the image in this order, that the bucket count fits the
  rows and that the widths are those the geometry implies; anything else is
  refused with a message.  Limits: at most 2^32 - 4096 rows and the alphabets
  and block sizes the builder accepts; an image beyond them is refused, not
  truncated.

  Decode once, search the decoded form.  The image is compressed for a CPU's
  memory; a rank query on it unranks a permutation index, which is divergent
  lane work.  Opening an image decodes it in one pass, one thread per bucket
  (the inverse of the builder's tile kernel), into a form of this project's own:

    alphabets of up to 4 letters   lines of 64 bytes: the occurrences of the
        four letters before the line (4 x uint32) and 192 rows at 2 bits.  One
        rank query touches one line; 2.67 bits a row.  A special sits in its row
        as letter 0; lines that hold one are flagged in a bitmap, and only for
        those the rank of letter 0 (and the symbol of a row) consults the regions.
    larger alphabets               the rows as bytes (letters, 254, 255) and the
        occurrences of every letter before every 64th row (uint32): sigma
        counters do not fit a line beside its rows, so the counters are a table
        of their own and a rank query touches two places.  8 + sigma / 2 bits a row.
    locate                         a bitmap of the marked rows with the marks
        before every 64-row word, the stored numbers in row order (uint32) and,
        for reversibly sorted images, the stored rank of every special row.
    the regions                    start, prefix sum of the lengths and symbol
        of every run of specials.

  The image itself is not needed after the decode.

  Locate.  From a row, walk LF on the decoded form until a marked row: the
  stored number (times the locate interval for reversibly sorted images) plus
  the steps.  The step from a row whose symbol is a special -- only reversibly
  sorted images leave such rows unmarked -- goes to (first row of the special
  suffixes) + (stored rank of that special).  An image with locate interval 0
  has no locate: a call that needs positions is refused.

  matstat and uniquesub.  gtamd_mstat_set_index_pckidx makes a reader the index
  of a gtamd_mstat; its two search calls, its cap contract and its info struct
  stay as include/gtamd_mstat.h states them.  The search is a backward search,
  one lane per query position: the bounds start at the count[] of the first
  letter, every next letter costs one rank pair (one line when both bounds fall
  into the same line); a special in the query, or a letter beyond the
  alphabet, ends it.  ms(i) and mu(i) are those of the TEXT THE INDEX WAS BUILT
  FROM read backwards: an index of the reversed subject (-dir rev, what the
  reference's suite builds) answers for the subject.  The witness is the
  reference's: with `located` the text position of the lower bound of the last
  interval that was not empty, rows - 1 - (located + ms(i)), whatever the read
  mode of the index was.  info: symbols_compared counts the rank pairs, reruns
  is 0.

  Conventions as in gtamd_check.h: 0 / -1, message from
  gtamd_esa_last_error().  Plain C; no CPU fallback: -1 without a device
  (gtamd_pckidx_check_image is host only).
*/
#ifndef GTAMD_PCKIDX_H
#define GTAMD_PCKIDX_H

#include <stddef.h>
#include <stdint.h>
#include "gtamd_esa.h"
#include "gtamd_mstat.h"
#include "gtamd_pck.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
  uint64_t rows;              /* n + 1 */
  uint64_t buckets;
  uint64_t regions;           /* runs of specials in the BWT */
  uint64_t special_rows;      /* rows whose BWT symbol is a special (the one of suffix 0 included) */
  uint64_t marks;             /* rows with a stored text position */
  uint64_t rot0_row;          /* row of suffix 0 (0 without locate information) */
  uint64_t image_bytes;
  uint64_t decoded_bytes;     /* device memory of the decoded form */
  uint32_t numofchars;
  uint32_t block_size;
  uint32_t bucket_blocks;
  uint32_t locate_interval;   /* 0: no locate */
  uint32_t feature_toggles;   /* GTAMD_PCK_LOCATE_* | GTAMD_PCK_REVERSIBLY_SORTED */
  uint32_t two_bit;           /* 1: the 2-bit lines, 0: bytes and a counter table */
  float decode_ms;            /* device time of the decode */
  uint32_t line_rows;         /* rows of one line (192) or between two counter rows (64) */
} gtamd_pckidx_info;

typedef struct gtamd_pckidx gtamd_pckidx;

/* host only, needs no device: 0 if the headers and the region list of the image
   pass every check made before a kernel runs, else -1 and the message */
int gtamd_pckidx_check_image(const void *image_host, uint64_t bytes);

/* a reader on HIP device `device`; NULL on failure.  One thread at a time per
   object. */
gtamd_pckidx *gtamd_pckidx_create(int device);
void gtamd_pckidx_destroy(gtamd_pckidx *px);

/* Open an image: each call replaces the one before, and decodes.  From the
   bytes of a file in HOST memory; from device memory (which is only read during
   the call); from a builder whose image is still resident (gtamd_pck_build*):
   nothing leaves the device.  Synchronous. */
int gtamd_pckidx_open_host(gtamd_pckidx *px, const void *image_host, uint64_t bytes);
int gtamd_pckidx_open_device(gtamd_pckidx *px, const void *image_device, uint64_t bytes);
int gtamd_pckidx_open_builder(gtamd_pckidx *px, const gtamd_pck *builder);

int gtamd_pckidx_get_info(const gtamd_pckidx *px, gtamd_pckidx_info *info);

/* the decoded form, part by part (0 lines or rows, 1 line flags or counter
   table, 2 mark bitmap, 3 marks before each word, 4 stored numbers, 5 ranks of
   the special rows, 6 region starts, 7 count[]): *bytes gets the size of the
   part, and up to `capacity` bytes of it are copied to dst_host (may be NULL) */
int gtamd_pckidx_decoded_copy(gtamd_pckidx *px, uint32_t part, void *dst_host, uint64_t capacity,
                              uint64_t *bytes);

/* ---- batch entry points; inputs and outputs in device memory when is_device ---- */
/* the BWT symbols of rows [row0, row0 + count): letters 0..sigma-1, 254, 255 */
int gtamd_pckidx_bwt(gtamd_pckidx *px, uint64_t row0, uint64_t count, uint8_t *out, int is_device);
/* out[i] = occurrences of letter symbols[i] (< numofchars) in rows [0, rows_[i]),
   rows_[i] <= rows, as BWTSeqTransformedOcc counts them: specials count for nobody */
int gtamd_pckidx_rank(gtamd_pckidx *px, const uint8_t *symbols, const uint64_t *rows_, uint64_t count,
                      uint64_t *out, int is_device);
/* out[i] = the text position of the suffix of row rows_[i] (< rows); refused for
   an image without locate information */
int gtamd_pckidx_locate(gtamd_pckidx *px, const uint64_t *rows_, uint64_t count, uint64_t *out,
                        int is_device);

/* the reader as the index of a searcher (each set_index* call replaces the one
   before); the reader must outlive the searches and live on the same device.
   gtamd_mstat_matstat with subjectpos_out on an image without locate
   information is refused. */
int gtamd_mstat_set_index_pckidx(gtamd_mstat *ms, const gtamd_pckidx *px);

#ifdef __cplusplus
}
#endif
#endif
