/* correct_host.c -- `gt readjoiner correct -ii INDEX [-k K] [-c C]` for this path
   (tool src/tools/gt_readjoiner_correct.c): the k-mer based error correction of
   an encoded read set, INDEX.esq edited in place.  Like encseq2spm it needs no
   table on disk: the engine builds .suf and .lcp of the mirrored reads in this
   process and hands them to include/gtamd_kcorrect.h, which decides the edits;
   here they are written as src/match/rdj-twobitenc-editor.c writes them. */
#include "host_internal.h"
#include "gtamd_kcorrect.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#define EQUALLENGTH_ONLY "twobitencoding correction is currently only implemented if the sequence access type is " \
                         "EQUALLENGTH"

static int read_file(const char *path, uint8_t **data, uint64_t *len)
{
  FILE *fp = fopen(path, "rb");
  long size;
  *data = NULL;
  if (fp == NULL) return -1;
  if (fseek(fp, 0, SEEK_END) != 0 || (size = ftell(fp)) < 0 || fseek(fp, 0, SEEK_SET) != 0 ||
      (*data = malloc(size > 0 ? (size_t) size : 1)) == NULL || fread(*data, 1, (size_t) size, fp) != (size_t) size) {
    free(*data); *data = NULL;
    fclose(fp);
    return -1;
  }
  fclose(fp);
  *len = (uint64_t) size;
  return 0;
}

int gtamd_correct_patch_esq(const char *indexname, const uint64_t *positions, const uint8_t *letters,
                            uint64_t count, char *err, size_t errlen)
{
  char path[4096];
  uint8_t *data = NULL;
  uint64_t len = 0, sat, n, dist_off, chars, twobit_off, dist[4];
  FILE *fp = NULL;
  int rc = -1;

  snprintf(path, sizeof path, "%s.esq", indexname);
  if (read_file(path, &data, &len) != 0) return gtamd_fail(err, errlen, "cannot open file '%s'", path);
  if (gtamd_esq_locate(data, len, &sat, &n, &dist_off, &chars, &twobit_off) != 0) {
    gtamd_fail(err, errlen, "file '%s' is no encoded sequence of this format", path);
    goto done;
  }
  if (sat != GTAMD_SAT_EQUALLENGTH || chars != 4) { gtamd_fail(err, errlen, "%s", EQUALLENGTH_ONLY); goto done; }
  for (uint64_t r = 0; r < count; r++)
    if (positions[r] >= n || letters[r] > 3) {
      gtamd_failf(err, errlen, "edit %llu: letter %u at position %llu of %llu symbols", (unsigned long long) r,
                  (unsigned) letters[r], (unsigned long long) positions[r], (unsigned long long) n);
      goto done;
    }
  if (count == 0) { rc = 0; goto done; }
  if ((fp = fopen(path, "r+b")) == NULL) { gtamd_fail(err, errlen, "cannot open file '%s' for writing", path); goto done; }
  memcpy(dist, data + dist_off, sizeof dist);
  for (uint64_t r = 0; r < count; r++) {
    const uint64_t at = twobit_off + 8 * (positions[r] / 32);
    const unsigned shift = 62 - 2 * (unsigned) (positions[r] % 32);
    uint64_t word;
    memcpy(&word, data + at, 8);
    /* (the reference's count of the letter that goes: exact in the low byte of the word only) */
    dist[shift < 8 ? (word >> shift) & 3 : 0]--;
    dist[letters[r]]++;
    word = (word & ~((uint64_t) 3 << shift)) | (uint64_t) letters[r] << shift;
    memcpy(data + at, &word, 8);
    if (fseek(fp, (long) at, SEEK_SET) != 0 || fwrite(&word, 8, 1, fp) != 1) {
      gtamd_fail(err, errlen, "cannot write to file '%s'", path);
      goto done;
    }
  }
  if (fseek(fp, (long) dist_off, SEEK_SET) != 0 || fwrite(dist, sizeof dist, 1, fp) != 1 || fflush(fp) != 0) {
    gtamd_fail(err, errlen, "cannot write to file '%s'", path);
    goto done;
  }
  rc = 0;
done:
  if (fp != NULL && fclose(fp) != 0 && rc == 0) rc = gtamd_fail(err, errlen, "cannot write to file '%s'", path);
  free(data);
  return rc;
}

int gtamd_readjoiner_correct(int argc, const char **argv, char *err, size_t errlen)
{
  /* development options of the reference: what they switch has no counterpart here */
  static const char *const refused[] = { "-encseq", "-dbg", NULL };
  const char *index = NULL;
  unsigned long long k = 31, c = 3, readmode = 0, mirrored = 0;
  char path[4096];
  uint8_t *enc = NULL, *both = NULL, *file = NULL, *letters = NULL;
  const uint8_t *dev;
  uint64_t n = 0, n2, len = 0, sat, nn, dist_off, chars, twobit_off, *rec = NULL;
  int rc = -1;
  gtamd_alphabet alpha;
  gtamd_seqstats ss;
  gtamd_encoder *de = NULL;
  gtamd_esa_ctx *ctx = NULL;
  gtamd_kcorrect *kc = NULL;
  gtamd_kcorrect_info info;

  for (int i = 1; i < argc; i++) {
    const char *a = argv[i];
    if (!strcmp(a, "-ii")) { if (gtamd_opt_name(argc, argv, &i, &index, err, errlen) != 0) return -1; }
    else if (!strcmp(a, "-k")) { if (gtamd_opt_length(argc, argv, &i, ~0ull, &k, err, errlen) != 0) return -1; }
    else if (!strcmp(a, "-c")) { if (gtamd_opt_length(argc, argv, &i, 0xffffffffull, &c, err, errlen) != 0) return -1; }
    else if (!strcmp(a, "-help")) {
      puts("Usage: gt-suffixerator-amd readjoiner correct -ii INDEX [-k K] [-c C]\n"
           "Readjoiner k-mer based error correction, on the device.\n\n"
           "-ii    the encoded reads: INDEX.prj and INDEX.esq (.ssp), DNA, reads of one length; no table is\n"
           "       read: .suf and .lcp of the mirrored reads are built on the device in this process\n"
           "-k     k-mer length (default: 31; 255 at most)\n"
           "-c     minimal trusted count (default: 3)\n\n"
           "Among the k-mers that share their first k - 1 letters, the last letter of every k-mer seen fewer\n"
           "than c times is overwritten with that of the first k-mer seen c times, on both strands.\n"
           "INDEX.esq is edited in place: the 2-bit words of the changed positions and the character\n"
           "distribution.  Nothing is printed.  INDEX.suf and INDEX.lcp, if there are any, are left alone\n"
           "and describe the reads as they were, as after the reference.");
      return 0;
    } else return gtamd_opt_tail(a, refused, GTAMD_UNKNOWN_SHOWS, GTAMD_UNNECESSARY, err, errlen);
  }
  if (index == NULL) return gtamd_fail(err, errlen, "option \"-%s\" is mandatory", "ii");
  if (k > GTAMD_KCORRECT_MAX_K)
    return gtamd_failf(err, errlen, "k-mers of %llu letters: 255 at most are supported (the correction reads the byte "
                       "table of the LCP values alone)", k);

  snprintf(path, sizeof path, "%s.prj", index);
  if (access(path, R_OK) != 0) return gtamd_fail(err, errlen, "cannot open file '%s'", path);
  (void) gtamd_prj_value(path, "readmode", &readmode);
  (void) gtamd_prj_value(path, "mirrored", &mirrored);
  if (readmode != 0)
    return gtamd_fail(err, errlen, "file '%s' gives a read mode other than forward", path);
  /* (a project written with -mirrored stores the reads alone, as every other: they are mirrored here) */
  snprintf(path, sizeof path, "%s.esq", index);
  if (read_file(path, &file, &len) != 0) return gtamd_fail(err, errlen, "cannot open file '%s'", path);
  if (gtamd_esq_locate(file, len, &sat, &nn, &dist_off, &chars, &twobit_off) == 0 &&
      (sat != GTAMD_SAT_EQUALLENGTH || chars != 4)) {
    free(file);
    return gtamd_fail(err, errlen, "%s", EQUALLENGTH_ONLY);
  }
  free(file);
  if (gtamd_read_esq_alpha(index, &enc, &n, &alpha, &ss, err, errlen) != 0) return -1;
  if (2 * n + 2 > GTAMD_MAX_ENTRIES) {
    snprintf(err, errlen, "%llu symbols on both strands are beyond the limit of a single build (%llu table "
             "entries); the slices of a build in parts are not corrected", (unsigned long long) n, GTAMD_MAX_ENTRIES);
    goto done;
  }
  both = gtamd_mirror(enc, n);
  if (both == NULL) { gtamd_fail(err, errlen, "out of memory (%s)", "mirrored reads"); goto done; }
  n2 = 2 * n + 1;
  if ((de = gtamd_encoder_create(0, 0)) == NULL || gtamd_encoder_set_symbols(de, both, n2) != 0 ||
      (dev = gtamd_encoder_device_symbols(de)) == NULL ||
      (ctx = gtamd_esa_create(0, n2, 4)) == NULL || gtamd_esa_set_sequence_bytes(ctx, dev, n2, 1) != 0 ||
      gtamd_esa_run(ctx, GTAMD_WANT_SUF | GTAMD_WANT_LCP) != 0 ||
      (kc = gtamd_kcorrect_create(0)) == NULL || gtamd_kcorrect_set_index_esa(kc, ctx, dev, n2, 1) != 0 ||
      gtamd_kcorrect_decide(kc, (uint32_t) k, (uint32_t) c, &info) != 0) {
    snprintf(err, errlen, "%s", gtamd_esa_last_error());
    goto done;
  }
  if (info.records != 0) {
    rec = malloc(info.records * 3 * sizeof *rec);
    letters = malloc(info.records);
    if (rec == NULL || letters == NULL) { gtamd_fail(err, errlen, "out of memory (%s)", "records"); goto done; }
    if (gtamd_kcorrect_records(kc, rec, 0) != 0) { snprintf(err, errlen, "%s", gtamd_esa_last_error()); goto done; }
    for (uint64_t r = 0; r < info.records; r++) {        /* (entry, position, letter) -> position, letter */
      rec[r] = rec[3 * r + 1];
      letters[r] = (uint8_t) rec[3 * r + 2];
    }
    if (gtamd_correct_patch_esq(index, rec, letters, info.records, err, errlen) != 0) goto done;
  }
  rc = 0;
done:
  gtamd_kcorrect_destroy(kc);
  if (ctx != NULL) gtamd_esa_destroy(ctx);
  if (de != NULL) gtamd_encoder_destroy(de);
  gtamd_alphabet_free(&alpha);
  free(rec); free(letters); free(both); free(enc);
  return rc;
}
