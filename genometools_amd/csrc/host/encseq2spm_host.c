/* encseq2spm_host.c -- `gt encseq2spm -l L -ii INDEX -spm show|count` for this
   path (tool src/tools/gt_encseq2spm.c): all suffix-prefix matches of a read set
   on both strands.  It needs no table on disk: the engine builds .suf and .lcp
   of the mirrored reads in this process and hands them to include/gtamd_spm.h.
   Its consumer, `gt readjoiner overlap`, the irreducible ones of them, is in
   rdj_host.c.  Option handling of src/tools/gt_encseq2spm.c:94-260; the lines of
   processlcpinterval_spmsk (src/match/esa-spmsk.c:106) and the count line of
   the tool (gt_encseq2spm.c). */
#include "host_internal.h"
#include "gtamd_spm.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#define ENCSEQ2SPM_CAPACITY (1u << 20)           /* records of one gtamd_spm_emit */

int gtamd_encseq2spm(int argc, const char **argv, char *err, size_t errlen)
{
  /* how the reference's own sort is run and checked: no counterpart here */
  static const char *const refused[] = {
    "-parts", "-memlimit", "-checksuftab", "-onlyaccum", "-onlyallfirstcodes", "-addbscachedepth",
    "-phase2extra", "-radixlarge", "-radixparts", "-singlescan", "-forcek", NULL };
  const char *index = NULL, *spm = NULL;
  int have_l = 0, show = 0, count = 0, verbose = 0, rc = -1;
  unsigned long long minlen = 0, readmode = 0, mirrored = 0;
  char path[4096];
  uint8_t *enc = NULL, *both = NULL;
  const uint8_t *dev;
  uint64_t n = 0, n2, cursor = 0, written = 0, total = 0;
  gtamd_alphabet alpha;
  gtamd_seqstats ss;
  gtamd_encoder *de = NULL;
  gtamd_esa_ctx *ctx = NULL;
  gtamd_esa_timing tm;
  gtamd_spm *sp = NULL;
  gtamd_spm_info info;
  gtamd_spm_record *rec = NULL;

  for (int i = 1; i < argc; i++) {
    const char *a = argv[i];
    if (!strcmp(a, "-ii")) { if (gtamd_opt_name(argc, argv, &i, &index, err, errlen) != 0) return -1; }
    else if (!strcmp(a, "-l")) {
      if (gtamd_opt_length(argc, argv, &i, 0xffffffffull, &minlen, err, errlen) != 0) return -1;
      have_l = 1;
    } else if (!strcmp(a, "-spm")) {
      if (gtamd_opt_name(argc, argv, &i, &spm, err, errlen) != 0) return -1;
      show = !strcmp(spm, "show");
      count = !strcmp(spm, "count");
      if (!show && !count) return gtamd_fail(err, errlen, "illegal argument \"%s\" to option -spm", spm);
    } else if (!strcmp(a, "-singlestrand")) {
      if (i + 1 < argc && !strcmp(argv[i + 1], "no")) { i++; continue; }
      /* (the reference's own message, gt_encseq2spm.c) */
      return gtamd_fail(err, errlen, "option %s is not implemented", "-singlestand");
    } else if (!strcmp(a, "-v")) verbose = 1;
    else if (!strcmp(a, "-help")) {
      puts("Usage: gt-suffixerator-amd encseq2spm -l L -ii INDEX [-spm show|count] [-v]\n"
           "Compute all suffix-prefix matches of the sequences of INDEX and their reverse complements on\n"
           "the device.\n\n"
           "-ii    the encoded reads: INDEX.prj and INDEX.esq (.ssp), DNA; no table is read: .suf and .lcp\n"
           "       of the mirrored reads are built on the device in this process\n"
           "-l     minimum length of a match (mandatory)\n"
           "-spm   show: one line `s t len` per match; count: their number.  Without it nothing is computed\n"
           "-v     figures of the build and of the enumeration as lines that start with '#'\n\n"
           "The last len letters of sequence s are the first len letters of sequence t; R reads are the\n"
           "sequences 0 to R - 1, sequence R + j is the reverse complement of read R - 1 - j.  The lines come\n"
           "in TABLE ORDER: ascending table index of the matching suffix of s, then of the start of t.  The\n"
           "reference prints the same lines in the order of its traversal: compare sorted outputs.\n"
           "-singlestrand is not implemented, as in the reference; the options of its own sort are refused.");
      return 0;
    } else return gtamd_opt_tail(a, refused, GTAMD_UNKNOWN_SHOWS, GTAMD_UNNECESSARY, err, errlen);
  }
  if (!have_l) return gtamd_fail(err, errlen, "option \"-%s\" is mandatory", "l");
  if (index == NULL) return gtamd_fail(err, errlen, "option \"-%s\" is mandatory", "ii");

  /* the reads as stored: a project that reads them another way is none for this tool */
  snprintf(path, sizeof path, "%s.prj", index);
  if (access(path, R_OK) != 0) return gtamd_fail(err, errlen, "cannot open file '%s'", path);
  (void) gtamd_prj_value(path, "readmode", &readmode);
  (void) gtamd_prj_value(path, "mirrored", &mirrored);
  if (readmode != 0 || mirrored)
    return gtamd_fail(err, errlen, "file '%s' gives a read mode other than forward or describes a mirrored "
                      "index: encseq2spm mirrors the reads itself", path);
  if (gtamd_read_esq_alpha(index, &enc, &n, &alpha, &ss, err, errlen) != 0) return -1;
  if (!gtamd_alphabet_is_dna(&alpha)) {
    snprintf(err, errlen, "mirroring can only be enabled for DNA sequences, this encoded sequence has "
             "alphabet: %.*s", (int) alpha.numofchars, alpha.characters);
    goto done;
  }
  if (2 * n + 2 > GTAMD_MAX_ENTRIES) {
    snprintf(err, errlen, "%llu symbols on both strands are beyond the limit of a single build (%llu table "
             "entries); the slices of a build in parts are not searched", (unsigned long long) n,
             GTAMD_MAX_ENTRIES);
    goto done;
  }
  /* the reference ends here too when no output is asked for */
  if (!show && !count) { rc = 0; goto done; }

  both = gtamd_mirror(enc, n);
  if (both == NULL) { gtamd_fail(err, errlen, "out of memory (%s)", "mirrored reads"); goto done; }
  n2 = 2 * n + 1;
  if ((de = gtamd_encoder_create(0, 0)) == NULL || gtamd_encoder_set_symbols(de, both, n2) != 0 ||
      (dev = gtamd_encoder_device_symbols(de)) == NULL ||
      (ctx = gtamd_esa_create(0, n2, 4)) == NULL || gtamd_esa_set_sequence_bytes(ctx, dev, n2, 1) != 0 ||
      gtamd_esa_run(ctx, GTAMD_WANT_SUF | GTAMD_WANT_LCP) != 0 || gtamd_esa_get_timing(ctx, &tm) != 0 ||
      (sp = gtamd_spm_create(0)) == NULL || gtamd_spm_set_index_esa(sp, ctx, dev, n2) != 0 ||
      gtamd_spm_prepare(sp, (uint32_t) minlen, &info) != 0) {
    snprintf(err, errlen, "%s", gtamd_esa_last_error());
    goto done;
  }
  if (verbose)
    printf("# %llu table entries built in %.3f ms on the device\n"
           "# %llu matches, %llu terminal suffixes, %llu read starts, widest interval %llu, at most %llu "
           "matches of one suffix, %llu symbols compared by the searches, %llu bytes, %.3f ms on the device\n",
           (unsigned long long) info.table_entries, tm.total_ms, (unsigned long long) info.matches,
           (unsigned long long) info.terminal_suffixes, (unsigned long long) info.read_starts,
           (unsigned long long) info.max_width, (unsigned long long) info.max_matches_of_one_suffix,
           (unsigned long long) info.search_symbols, (unsigned long long) info.device_bytes, info.device_ms);
  if (count) printf("number of suffix-prefix matches=%llu\n", (unsigned long long) info.matches);
  else {
    rec = malloc(ENCSEQ2SPM_CAPACITY * sizeof *rec);
    if (rec == NULL) { gtamd_fail(err, errlen, "out of memory (%s)", "records"); goto done; }
    do {
      if (gtamd_spm_emit(sp, &cursor, rec, ENCSEQ2SPM_CAPACITY, 0, &written) != 0) {
        snprintf(err, errlen, "%s", gtamd_esa_last_error());
        goto done;
      }
      for (uint64_t k = 0; k < written; k++)
        printf("%llu %llu %llu\n", (unsigned long long) rec[k].suffix_seq, (unsigned long long) rec[k].prefix_seq,
               (unsigned long long) rec[k].len);
      total += written;
    } while (written != 0);
    if (total != info.matches) {
      snprintf(err, errlen, "%llu matches counted, %llu given", (unsigned long long) info.matches,
               (unsigned long long) total);
      goto done;
    }
  }
  if (fflush(stdout) != 0) { gtamd_fail(err, errlen, "cannot write to %s", "stdout"); goto done; }
  rc = 0;
done:
  gtamd_spm_destroy(sp);
  if (ctx != NULL) gtamd_esa_destroy(ctx);
  if (de != NULL) gtamd_encoder_destroy(de);
  gtamd_alphabet_free(&alpha);
  free(rec); free(both); free(enc);
  return rc;
}
