/* rdj_host.c -- `gt readjoiner overlap -readset X -l L` for this path (tool
   src/tools/gt_readjoiner_overlap.c, the traversal it replaces:
   src/match/rdj-spmfind.c): the irreducible suffix-prefix matches of a read set
   on both strands, on the device through the engine and include/gtamd_spmred.h,
   as lines or as Readjoiner's binary list X.0.spm (src/match/rdj-spmlist.c:45-124),
   which is what `gt readjoiner assembly` opens.  The stdout is the reference's
   byte for byte but for the order of the match lines, which is the table's here
   and the reference's traversal's there. */
#include "host_internal.h"
#include "gtamd_spmred.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#define RDJ_CAPACITY (1u << 20)                  /* records of one gtamd_spmred_emit */
#define RDJ_VERSION "1.2"                        /* GT_READJOINER_VERSION */
#define RDJ_BIN32 2                              /* GT_SPMLIST_BIN32, the header byte */

int gtamd_spmlist_bin32_header(FILE *fp)
{
  return fputc(RDJ_BIN32, fp) == EOF ? -1 : 0;
}

int gtamd_spmlist_bin32_records(FILE *fp, const gtamd_spmred_record *rec, uint64_t count, char *err, size_t errlen)
{
  uint32_t buf[3 * 1024];
  uint64_t k = 0;
  while (k < count) {
    size_t fill = 0;
    for (; k < count && fill < 1024; k++, fill++) {
      if (rec[k].suffix_read > UINT32_MAX || rec[k].prefix_read > UINT32_MAX || rec[k].len > (UINT32_MAX >> 2) ||
          rec[k].flags > 3) {
        snprintf(err, errlen, "match %llu %llu %llu does not fit the bin32 list format (three 32-bit numbers a "
                 "match, the length in 30 bits); the bin64 format is not written",
                 (unsigned long long) rec[k].suffix_read, (unsigned long long) rec[k].prefix_read,
                 (unsigned long long) rec[k].len);
        return -1;
      }
      buf[3 * fill] = (uint32_t) rec[k].suffix_read;
      buf[3 * fill + 1] = (uint32_t) rec[k].prefix_read;
      buf[3 * fill + 2] = (uint32_t) (rec[k].len << 2 | rec[k].flags);
    }
    if (fwrite(buf, 3 * sizeof buf[0], fill, fp) != fill) return gtamd_fail(err, errlen, "cannot write %s", "the list of matches");
  }
  return 0;
}

int gtamd_readjoiner_overlap(int argc, const char **argv, char *err, size_t errlen)
{
  /* how the reference's own sort and its w sets are run: no counterpart here */
  static const char *const refused[] = {
    "-parts", "-memlimit", "-wmax", "-phase2extra", "-radixparts", "-radixsmall", "-onlyallfirstcodes", NULL };
  const char *readset = NULL;
  int have_l = 0, elimtrans = 1, showspm = 0, quiet = 0, verbose = 0, rc = -1;
  unsigned long long minlen = 0;
  char path[4096];
  uint8_t *enc = NULL, *both = NULL;
  const uint8_t *dev;
  uint64_t n = 0, n2, reads = 0, cursor = 0, written = 0, total = 0;
  gtamd_alphabet alpha;
  gtamd_seqstats ss;
  gtamd_encoder *de = NULL;
  gtamd_esa_ctx *ctx = NULL;
  gtamd_esa_timing tm;
  gtamd_spmred *sr = NULL;
  gtamd_spmred_info info;
  gtamd_spmred_record *rec = NULL;
  FILE *list = NULL;

  for (int i = 1; i < argc; i++) {
    const char *a = argv[i];
    if (!strcmp(a, "-readset")) { if (gtamd_opt_name(argc, argv, &i, &readset, err, errlen) != 0) return -1; }
    else if (!strcmp(a, "-l")) {
      /* (gt_option_new_uint_min(..., 2U): the words of the reference's parser) */
      char *end;
      if (i + 1 >= argc || argv[i + 1][0] == '-') return gtamd_fail(err, errlen, "missing argument to option \"%s\"", a);
      minlen = strtoull(argv[++i], &end, 10);
      if (*end != 0 || end == argv[i] || minlen > 0xffffffffull)
        return gtamd_fail(err, errlen, "argument to option \"%s\" must be a non-negative integer <= 4294967295", a);
      if (minlen < 2) return gtamd_fail(err, errlen, "argument to option \"%s\" must be an integer >= 2", a);
      have_l = 1;
    } else if (!strcmp(a, "-elimtrans")) elimtrans = gtamd_opt_switch(argc, argv, &i);
    else if (!strcmp(a, "-showspm")) showspm = gtamd_opt_switch(argc, argv, &i);
    else if (!strcmp(a, "-q")) quiet = gtamd_opt_switch(argc, argv, &i);
    else if (!strcmp(a, "-v")) verbose = gtamd_opt_switch(argc, argv, &i);
    else if (!strcmp(a, "-singlestrand")) {
      if (!gtamd_opt_switch(argc, argv, &i)) continue;
      return gtamd_fail(err, errlen, "option %s is not implemented", a);
    } else if (!strcmp(a, "-help")) {
      puts("Usage: gt-suffixerator-amd readjoiner overlap -readset X -l L [-elimtrans yes|no] [-showspm] [-q] [-v]\n"
           "Compute the irreducible suffix-prefix matches of the reads of X and their reverse complements on\n"
           "the device.\n\n"
           "-readset    the encoded reads: X.esq (.ssp), DNA, as `gt readjoiner prefilter` or `gt encseq encode`\n"
           "            writes them; no table is read: .suf and .lcp of the mirrored reads are built on the\n"
           "            device in this process\n"
           "-l          minimum length of a match (mandatory, 2 or more)\n"
           "-elimtrans  yes (default): the irreducible matches only; no: all of them\n"
           "-showspm    one line `sn +|- pn +|- len` per match on stdout; without it the matches go to X.0.spm,\n"
           "            Readjoiner's binary list\n"
           "-q          no lines that start with '#'\n"
           "-v          figures of the build and of the reduction as lines that start with '#'\n\n"
           "The last len letters of read sn on its strand are the first len letters of read pn on its strand;\n"
           "of the two mirror images of an overlap one is given.  The matches come in TABLE ORDER (ascending\n"
           "table index of the matching suffix, then of the start of the other read); the reference gives the\n"
           "same matches in the order of its traversal: compare sorted outputs.  A set in which a read occurs\n"
           "whole at another place (a duplicate, a contained read, a read equal to its own reverse complement)\n"
           "is refused: filter it with gt readjoiner prefilter.  -singlestrand is not implemented; the options\n"
           "of the reference's own sort are refused.");
      return 0;
    } else return gtamd_opt_tail(a, refused, GTAMD_UNKNOWN_SHOWS, GTAMD_UNNECESSARY, err, errlen);
  }
  if (readset == NULL) return gtamd_fail(err, errlen, "option \"-%s\" is mandatory", "readset");
  if (!have_l) return gtamd_fail(err, errlen, "option \"-%s\" is mandatory", "l");
  if (quiet && verbose) return gtamd_fail(err, errlen, "option \"-v\" and option \"-q\" exclude %s", "each other");

  if (!quiet) printf("# gt readjoiner overlap (version " RDJ_VERSION ")\n");
  if (verbose) printf("# verbose output activated\n");
  snprintf(path, sizeof path, "%s.esq", readset);
  if (access(path, R_OK) != 0) return gtamd_fail(err, errlen, "cannot open file '%s'", path);
  if (gtamd_read_esq_alpha(readset, &enc, &n, &alpha, &ss, err, errlen) != 0) return -1;
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
  if (n == 0) { gtamd_fail(err, errlen, "readset '%s' holds no symbol", readset); goto done; }
  reads = 1;
  for (uint64_t k = 0; k < n; k++) reads += enc[k] == 255;
  if (reads > UINT32_MAX) {
    snprintf(err, errlen, "%llu reads need the bin64 list format, which is not written", (unsigned long long) reads);
    goto done;
  }
  if (!quiet) printf("# number of reads in filtered readset = %llu\n", (unsigned long long) reads);

  both = gtamd_mirror(enc, n);
  if (both == NULL) { gtamd_fail(err, errlen, "out of memory (%s)", "mirrored reads"); goto done; }
  n2 = 2 * n + 1;
  if ((de = gtamd_encoder_create(0, 0)) == NULL || gtamd_encoder_set_symbols(de, both, n2) != 0 ||
      (dev = gtamd_encoder_device_symbols(de)) == NULL ||
      (ctx = gtamd_esa_create(0, n2, 4)) == NULL || gtamd_esa_set_sequence_bytes(ctx, dev, n2, 1) != 0 ||
      gtamd_esa_run(ctx, GTAMD_WANT_SUF | GTAMD_WANT_LCP) != 0 || gtamd_esa_get_timing(ctx, &tm) != 0 ||
      (sr = gtamd_spmred_create(0)) == NULL || gtamd_spmred_set_index_esa(sr, ctx, dev, n2) != 0 ||
      gtamd_spmred_prepare(sr, (uint32_t) minlen, GTAMD_SPMRED_MIRRORED | (elimtrans ? GTAMD_SPMRED_ELIMTRANS : 0),
                           &info) != 0) {
    snprintf(err, errlen, "%s", gtamd_esa_last_error());
    goto done;
  }
  if (info.contained_sequences != 0) {
    snprintf(err, errlen, "readset '%s' holds %llu sequences, counted on both strands, that occur whole at another "
             "place of the set (duplicates, reads contained in other reads, reads equal to their own reverse "
             "complement); the matches of such a set are not those of the reference: remove them with gt "
             "readjoiner prefilter", readset, (unsigned long long) info.contained_sequences);
    goto done;
  }
  if (verbose)
    printf("# %llu table entries built in %.3f ms on the device\n"
           "# %llu suffix-prefix matches decided, %llu kept, %llu terminal suffixes, %llu read starts, widest "
           "interval %llu, at most %llu matches of one suffix\n"
           "# %llu candidates examined, at most %llu for one match, %llu letters compared, %llu bytes, %.3f ms "
           "on the device (%.3f ms the matches, %.3f ms the decisions)\n",
           (unsigned long long) info.table_entries, tm.total_ms, (unsigned long long) info.matches,
           (unsigned long long) info.kept, (unsigned long long) info.terminal_suffixes,
           (unsigned long long) info.read_starts, (unsigned long long) info.max_width,
           (unsigned long long) info.max_matches_of_one_suffix, (unsigned long long) info.candidates_examined,
           (unsigned long long) info.max_candidates_of_one_pair, (unsigned long long) info.letters_compared,
           (unsigned long long) info.device_bytes, info.device_ms, info.spm_ms, info.decide_ms);
  if (!showspm) {
    snprintf(path, sizeof path, "%s.0.spm", readset);
    if ((list = fopen(path, "wb")) == NULL) { gtamd_fail(err, errlen, "cannot open file '%s' for writing", path); goto done; }
    if (gtamd_spmlist_bin32_header(list) != 0) { gtamd_fail(err, errlen, "cannot write file '%s'", path); goto done; }
  }
  rec = malloc(RDJ_CAPACITY * sizeof *rec);
  if (rec == NULL) { gtamd_fail(err, errlen, "out of memory (%s)", "records"); goto done; }
  do {
    if (gtamd_spmred_emit(sr, &cursor, rec, RDJ_CAPACITY, 0, &written) != 0) {
      snprintf(err, errlen, "%s", gtamd_esa_last_error());
      goto done;
    }
    if (!showspm) {
      if (gtamd_spmlist_bin32_records(list, rec, written, err, errlen) != 0) goto done;
    } else
      for (uint64_t k = 0; k < written; k++)
        printf("%llu %c %llu %c %llu\n", (unsigned long long) rec[k].suffix_read,
               rec[k].flags & GTAMD_SPMRED_SUFFIX_DIRECT ? '+' : '-', (unsigned long long) rec[k].prefix_read,
               rec[k].flags & GTAMD_SPMRED_PREFIX_DIRECT ? '+' : '-', (unsigned long long) rec[k].len);
    total += written;
  } while (written != 0);
  if (total != info.kept) {
    snprintf(err, errlen, "%llu matches counted, %llu given", (unsigned long long) info.kept,
             (unsigned long long) total);
    goto done;
  }
  if (list != NULL) {
    const int closed = fclose(list);
    list = NULL;
    if (closed != 0) { gtamd_fail(err, errlen, "cannot close file '%s'", path); goto done; }
  }
  if (!quiet) {
    /* (gt_readjoiner_overlap.c:350-358) */
    printf("# number of %ssuffix-prefix matches = %llu\n", elimtrans ? "irreducible " : "",
           (unsigned long long) info.kept);
    printf("# average %sSPM/read = %.2f\n", elimtrans ? "irreducible " : "", (float) info.kept / reads);
    if (elimtrans)
      printf("# number of transitive suffix-prefix matches = %llu\n",
             (unsigned long long) (info.transitive_same_read + (info.transitive_other >> 1)));
  }
  if (fflush(stdout) != 0) { gtamd_fail(err, errlen, "cannot write to %s", "stdout"); goto done; }
  rc = 0;
done:
  if (list != NULL) fclose(list);
  gtamd_spmred_destroy(sr);
  if (ctx != NULL) gtamd_esa_destroy(ctx);
  if (de != NULL) gtamd_encoder_destroy(de);
  gtamd_alphabet_free(&alpha);
  free(rec); free(both); free(enc);
  return rc;
}
