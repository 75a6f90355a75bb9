/* prefilter_host.c -- `gt readjoiner prefilter -db FILE... [-readset X]` for this
   path (tool src/tools/gt_readjoiner_prefilter.c; what it replaces:
   src/match/reads2twobit.c and src/match/rdj-contfinder.c): the reads of FASTA or
   FASTQ files without those that hold a wildcard and without the duplicates and
   the reads contained in others on either strand, as X.esq (.ssp), which `gt
   readjoiner overlap` opens.  Encoded, filtered, mirrored, indexed, decided and
   compacted on the device (include/gtamd_encode.h, gtamd_esa.h,
   gtamd_contained.h); what the host keeps per read is a few bytes.  The stdout is
   the reference's byte for byte, and so are the files for reads of one length;
   for reads of several lengths the reference departs from its own definition
   (include/gtamd_contained.h) and the definition is followed. */
#include "host_internal.h"
#include "gtamd_contained.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>

#define RDJ_VERSION "1.2"                        /* GT_READJOINER_VERSION */

void gtamd_prefilter_filetable(const gtamd_prefilter_file *f, size_t numfiles, gtamd_filelength *tab)
{
  for (size_t k = 0; k < numfiles; k++) {
    /* (reads2twobit.c:891-892, "not necessary, but useful for the tests"; :1477-1481 for reads of one length) */
    tab[k].length = f[k].filesize - (f[k].invalid_letters + 3 * f[k].invalid_reads);
    tab[k].effectivelength = f[k].kept_letters + f[k].kept_reads - 1;       /* (no read: all ones, as there) */
  }
}

int gtamd_prefilter_write_readset(const char *readset, const char *const *paths, size_t numfiles,
                                  const gtamd_prefilter_file *f, const uint8_t *kept, uint64_t n, char *err,
                                  size_t errlen)
{
  static const char letters[4] = { 'a', 'c', 'g', 't' };
  gtamd_alphabet alpha;
  gtamd_encinfo info;
  gtamd_seqstats ss;
  int rc;
  memset(&info, 0, sizeof info);
  info.numfiles = numfiles;
  if ((info.filelengthtab = calloc(numfiles ? numfiles : 1, sizeof *info.filelengthtab)) == NULL)
    return gtamd_fail(err, errlen, "out of memory (%s)", "file table");
  gtamd_prefilter_filetable(f, numfiles, info.filelengthtab);
  /* (what the encoder would have seen of X.p.fas: the letters in lower case) */
  for (uint64_t k = 0; k < n; k++) if (kept[k] < 4) info.originaldistribution[(unsigned char) letters[kept[k]]]++;
  gtamd_alphabet_standard(&alpha, 0);
  rc = gtamd_write_esq_alpha(readset, paths, numfiles, kept, n, &alpha, &info, 0, NULL, &ss, err, errlen);
  gtamd_alphabet_free(&alpha);
  gtamd_encinfo_free(&info);
  return rc;
}

int gtamd_prefilter_write_cntlist(const char *path, const uint8_t *removed, uint64_t reads, char *err, size_t errlen)
{
  /* (rdj-cntlist.c:49-58: the bit format; read k is bit 63 - k % 64 of word k / 64) */
  const uint64_t words = (reads + 63) / 64;
  uint64_t *bits = calloc(words ? words : 1, sizeof *bits);
  FILE *fp;
  int ok;
  if (bits == NULL) return gtamd_fail(err, errlen, "out of memory (%s)", "list of contained reads");
  for (uint64_t k = 0; k < reads; k++) if (removed[k]) bits[k / 64] |= 1ull << (63 - k % 64);
  if ((fp = fopen(path, "wb")) == NULL) {
    free(bits);
    return gtamd_fail(err, errlen, "cannot open file '%s' for writing", path);
  }
  ok = fputc(0, fp) != EOF && fputc((int) sizeof reads, fp) != EOF && fwrite(&reads, sizeof reads, 1, fp) == 1 &&
       fwrite(bits, sizeof *bits, words, fp) == words;
  ok = fclose(fp) == 0 && ok;
  free(bits);
  return ok ? 0 : gtamd_fail(err, errlen, "cannot write file '%s'", path);
}

/* X.p.fas: `>` and the read on a line each, lower case (gt_reads2twobit_write_fasta) */
static int write_fasta(const char *path, const uint8_t *sym, uint64_t n, char *err, size_t errlen)
{
  FILE *fp = fopen(path, "w");
  int ok = 1;
  if (fp == NULL) return gtamd_fail(err, errlen, "cannot open file '%s' for writing", path);
  for (uint64_t k = 0; k < n && ok; k++) {
    if (k == 0 || sym[k - 1] == 255) ok = fputs(">\n", fp) != EOF;
    if (ok) ok = fputc(sym[k] == 255 ? '\n' : "acgt"[sym[k] & 3], fp) != EOF;
  }
  if (n != 0 && ok) ok = fputc('\n', fp) != EOF;
  ok = fclose(fp) == 0 && ok;
  return ok ? 0 : gtamd_fail(err, errlen, "cannot write file '%s'", path);
}

/* the reads of all files as one set in an encoder, with reads[f] = the reads of
   file f: the device reader for FASTA or four-line FASTQ; what it declines, file
   by file through the host reader */
static int encode_reads(const char *const *paths, size_t numfiles, gtamd_encoder **de, uint64_t *reads, char *err,
                        size_t errlen)
{
  gtamd_alphabet alpha;
  gtamd_encinfo info;
  uint32_t *file = NULL, *other = NULL, *third = NULL;
  uint64_t *start = NULL, *end = NULL, count, n = 0, fill = 0;
  uint8_t *all = NULL;
  int rc;
  gtamd_alphabet_standard(&alpha, 0);
  memset(&info, 0, sizeof info);
  for (size_t f = 0; f < numfiles; f++) reads[f] = 0;
  rc = gtamd_device_encode_files_alpha(paths, numfiles, &alpha, de, NULL, NULL, &info, err, errlen);
  if (rc == 0) {
    gtamd_encinfo_free(&info);
    rc = -1;
    if ((count = gtamd_encoder_num_fastq_records(*de)) != 0) {
      file = malloc(4 * count); other = malloc(4 * count); third = malloc(4 * count);
      if (file == NULL || other == NULL || third == NULL) gtamd_fail(err, errlen, "out of memory (%s)", "reads");
      else if (gtamd_encoder_get_fastq_records(*de, file, other, third, count) != 0)
        snprintf(err, errlen, "%s", gtamd_esa_last_error());
      else rc = 0;
    } else {
      count = gtamd_encoder_num_descriptions(*de);
      file = malloc(4 * (count + 1)); start = malloc(8 * (count + 1)); end = malloc(8 * (count + 1));
      if (file == NULL || start == NULL || end == NULL) gtamd_fail(err, errlen, "out of memory (%s)", "reads");
      else if (gtamd_encoder_get_descriptions(*de, file, start, end, count + 1) != 0)
        snprintf(err, errlen, "%s", gtamd_esa_last_error());
      else rc = 0;
    }
    for (uint64_t k = 0; rc == 0 && k < count; k++) if (file[k] < numfiles) reads[file[k]]++;
    goto done;
  }
  if (rc != GTAMD_DEVICE_DECLINED) goto done;
  rc = -1;
  for (size_t f = 0; f < numfiles; f++) {
    uint8_t *one = NULL, *grown;
    uint64_t n1 = 0;
    if (gtamd_encode_files_alpha(paths + f, 1, &alpha, &one, &n1, NULL, NULL, &info, err, errlen) != 0) goto done;
    gtamd_encinfo_free(&info);
    if ((grown = realloc(all, n + n1 + 2)) == NULL) {
      free(one);
      gtamd_fail(err, errlen, "out of memory (%s)", "reads");
      goto done;
    }
    all = grown;
    if (n1 != 0 && fill != 0) all[n++] = 255;
    memcpy(all + n, one, n1);
    for (uint64_t k = 0; k < n1; k++) reads[f] += one[k] == 255;
    reads[f] += n1 != 0;
    fill += n1;
    n += n1;
    free(one);
  }
  if ((*de = gtamd_encoder_create(0, 0)) == NULL || gtamd_encoder_set_symbols(*de, all, n) != 0) {
    snprintf(err, errlen, "%s", gtamd_esa_last_error());
    goto done;
  }
  rc = 0;
done:
  free(file); free(other); free(third); free(start); free(end); free(all);
  gtamd_alphabet_free(&alpha);
  return rc;
}

static void percent_line(int verbose, int quiet, const char *what, uint64_t count, uint64_t input)
{
  if (verbose) printf("# %s = %llu [%.2f %% of input]\n", what, (unsigned long long) count,
                      (float) count * 100 / (float) input);
  else if (!quiet) printf("# %s = %llu\n", what, (unsigned long long) count);
}

int gtamd_readjoiner_prefilter(int argc, const char **argv, char *err, size_t errlen)
{
  /* quality filters, descriptions, paired libraries and their table, the reference's own tests */
  static const char *const refused[] = {
    "-singlestrand", "-maxlow", "-lowqual", "-phred64", "-des", "-clipdes", "-memdes", "-copynum", "-seqnums",
    "-encseq", "-libtable", "-testrs", "-testrs-print", "-testrs-depth", "-testrs-maxdepth", NULL };
  const char *readset = NULL;
  const char *const *db = NULL;
  size_t numfiles = 0;
  int quiet = 0, verbose = 0, encodeonly = 0, fasta = 0, cnt = 0, strict = 0, rc = -1, varlen = 0;
  char path[4096];
  gtamd_encoder *de = NULL;
  gtamd_encode_summary sum;
  gtamd_contained *ct = NULL;
  gtamd_contained_info info;
  gtamd_esa_ctx *ctx = NULL;
  gtamd_prefilter_file *pf = NULL;
  uint64_t *perfile = NULL, *seps = NULL;
  uint8_t *flags = NULL, *verdict = NULL, *kept = NULL, *removed = NULL, *dev = NULL, *both = NULL;
  uint64_t input, invalid = 0, valid, n1 = 0, n2 = 0, nkept = 0, letters_valid = 0, letters_invalid = 0;
  uint64_t minlen = 0, maxlen = 0, contained = 0, output, inner = 0, selfc = 0;

  memset(&info, 0, sizeof info);
  for (int i = 1; i < argc; i++) {
    const char *a = argv[i];
    if (!strcmp(a, "-readset")) { if (gtamd_opt_name(argc, argv, &i, &readset, err, errlen) != 0) return -1; }
    else if (!strcmp(a, "-db")) { if (gtamd_opt_files(argc, argv, &i, &db, &numfiles, err, errlen) != 0) return -1; }
    else if (!strcmp(a, "-q")) quiet = gtamd_opt_switch(argc, argv, &i);
    else if (!strcmp(a, "-v")) verbose = gtamd_opt_switch(argc, argv, &i);
    else if (!strcmp(a, "-encodeonly")) encodeonly = gtamd_opt_switch(argc, argv, &i);
    else if (!strcmp(a, "-fasta")) fasta = gtamd_opt_switch(argc, argv, &i);
    else if (!strcmp(a, "-cnt")) cnt = gtamd_opt_switch(argc, argv, &i);
    else if (!strcmp(a, "-strict")) strict = gtamd_opt_switch(argc, argv, &i);
    else if (!strcmp(a, "-help")) {
      puts("Usage: gt-suffixerator-amd readjoiner prefilter -db FILE... [-readset X] [-q] [-v] [-encodeonly] [-fasta]\n"
           "       [-cnt] [-strict]\n"
           "Remove the reads with a wildcard, the duplicates and the reads contained in others on either strand,\n"
           "on the device, and write the reads that are left as X.esq.\n\n"
           "-db          FASTA or FASTQ files of unpaired reads; a paired library (a name with ':') is refused\n"
           "-readset     the name X of the output; default: the first file of -db\n"
           "-encodeonly  the reads with a wildcard go, nothing else is decided\n"
           "-fasta       also X.p.fas: `>` and the read on a line each, lower case\n"
           "-cnt         also X.cnt, the list of the reads removed (Readjoiner's bit format)\n"
           "-strict      also remove the reads that stand strictly inside another read and those equal to their\n"
           "             own reverse complement, which the reference keeps: what is left is a set `readjoiner\n"
           "             overlap` accepts.  Two more '#' lines give their numbers\n"
           "-q           no lines that start with '#'\n"
           "-v           the reference's verbose lines\n\n"
           "A read is removed when it equals a lower-numbered read or its reverse complement, or is a proper\n"
           "prefix or suffix of another read or of its reverse complement.  For reads of one length stdout, X.esq,\n"
           "X.p.fas and X.cnt are the reference's byte for byte.  For reads of several lengths the reference\n"
           "keeps reads its own definition removes (duplicates that are also a prefix of a third read, among\n"
           "others) and its files can disagree with each other; this tool follows the definition.\n"
           "X.rlt, the table of libraries, is not written and -libtable is refused: the reference's file holds\n"
           "an address of the process that wrote it and differs from run to run, and nothing here reads it.\n"
           "Quality filters (-maxlow -lowqual -phred64), descriptions (-des -clipdes -memdes), -singlestrand,\n"
           "-copynum, -seqnums, -encseq and the reference's self tests are refused by name.");
      return 0;
    } else return gtamd_opt_tail(a, refused, GTAMD_UNKNOWN_SHOWS, GTAMD_UNNECESSARY, err, errlen);
  }
  if (db == NULL) return gtamd_fail(err, errlen, "option \"-%s\" is mandatory", "db");
  if (quiet && verbose) return gtamd_fail(err, errlen, "option \"-v\" and option \"-q\" exclude %s", "each other");
  if (encodeonly && cnt) return gtamd_fail(err, errlen, "option \"-encodeonly\" and option \"-cnt\" exclude %s", "each other");
  for (size_t f = 0; f < numfiles; f++)
    if (strchr(db[f], ':') != NULL)
      return gtamd_failf(err, errlen, "library '%s' is a paired one (a name with ':'): paired libraries are not "
                         "supported by the MI355X engine, only files of unpaired reads", db[f]);
  if (readset == NULL) readset = db[0];

  if (!quiet) printf("# gt readjoiner prefilter (version " RDJ_VERSION ")\n");
  if (verbose) {
    printf("# readset name = %s\n# input files = ", readset);
    for (size_t f = 0; f < numfiles; f++) printf("%s%s", db[f], f + 1 < numfiles ? ", " : "\n");
  }
  pf = calloc(numfiles, sizeof *pf);
  perfile = calloc(numfiles, sizeof *perfile);
  if (pf == NULL || perfile == NULL) { gtamd_fail(err, errlen, "out of memory (%s)", "file table"); goto done; }
  for (size_t f = 0; f < numfiles; f++) {
    struct stat sb;
    if (stat(db[f], &sb) != 0) { gtamd_fail(err, errlen, "cannot open file '%s'", db[f]); goto done; }
    pf[f].filesize = (uint64_t) sb.st_size;
  }
  if (encode_reads(db, numfiles, &de, perfile, err, errlen) != 0) goto done;
  if (gtamd_encoder_get_summary(de, &sum) != 0) goto deverr;
  input = sum.totallength ? sum.numofsequences : 0;
  if (2 * sum.totallength + 2 > GTAMD_MAX_ENTRIES) {
    gtamd_failf(err, errlen, "%llu symbols on both strands are beyond the limit of a single build (%llu table "
                "entries); the slices of a build in parts are not searched", (unsigned long long) sum.totallength,
                GTAMD_MAX_ENTRIES);
    goto done;
  }
  {
    uint64_t counted = 0;
    for (size_t f = 0; f < numfiles; f++) counted += perfile[f];
    if (counted != input) {
      gtamd_failf(err, errlen, "%llu reads encoded, %llu counted file by file", (unsigned long long) input,
                  (unsigned long long) counted);
      goto done;
    }
  }

  /* the first filter: the reads with a wildcard, the reference's "low-quality" reads */
  seps = malloc(8 * (input + 1));
  flags = calloc(input + 1, 1);
  if (seps == NULL || flags == NULL) { gtamd_fail(err, errlen, "out of memory (%s)", "reads"); goto done; }
  if (input > 1 && gtamd_encoder_get_separators(de, seps, input) != 0) goto deverr;
  if ((ct = gtamd_contained_create(0)) == NULL) goto deverr;
  if (input != 0) {
    if (gtamd_contained_drop_wildcards(ct, gtamd_encoder_device_symbols(de), sum.totallength, seps, input - 1, &dev,
                                       &n1, &invalid) != 0 ||
        gtamd_contained_wildcard_flags(ct, flags, 0) != 0)
      goto deverr;
  }
  valid = input - invalid;
  {
    size_t f = 0;
    uint64_t left = numfiles ? perfile[0] : 0;
    for (uint64_t k = 0; k < input; k++) {
      const uint64_t begin = k ? seps[k - 1] + 1 : 0, len = (k + 1 < input ? seps[k] : sum.totallength) - begin;
      while (left == 0 && f + 1 < numfiles) left = perfile[++f];
      left--;
      if (flags[k]) { pf[f].invalid_reads++; pf[f].invalid_letters += len; letters_invalid += len; continue; }
      if (letters_valid == 0 || len < minlen) minlen = len;
      if (len > maxlen) maxlen = len;
      letters_valid += len;
      pf[f].kept_reads++; pf[f].kept_letters += len;          /* (until the verdicts are in: the valid ones) */
    }
    varlen = valid == 0 || minlen != maxlen;
  }
  if (!quiet) printf("# number of reads in complete readset = %llu\n", (unsigned long long) input);
  if (verbose) {
    /* (the lengths of the reference count the separator; its total misses the last one) */
    if (varlen) printf("# read length = variable [%llu..%llu]\n", (unsigned long long) (valid ? minlen + 1 : 0),
                       (unsigned long long) (valid ? maxlen + 1 : 0));
    else printf("# read length = %llu\n", (unsigned long long) minlen);
    printf("# total length of complete readset = %llu\n",
           (unsigned long long) ((valid ? letters_valid - 1 : 0) + letters_invalid));
  }
  percent_line(verbose, quiet, "low-quality reads", invalid, input);
  output = valid;
  nkept = n1;

  if (!encodeonly && valid != 0) {
    /* both strands, the tables, the verdicts, the reads that are left: all where the symbols lie */
    const uint32_t mask = strict ? GTAMD_CONTAINED_MASK_STRICT : GTAMD_CONTAINED_MASK_DEFAULT;
    uint64_t at = 0;
    size_t f = 0;
    if (gtamd_contained_mirror_result(ct, &both, &n2) != 0 ||
        (ctx = gtamd_esa_create(0, n2, 4)) == NULL || gtamd_esa_set_sequence_bytes(ctx, both, n2, 1) != 0 ||
        gtamd_esa_run(ctx, GTAMD_WANT_SUF | GTAMD_WANT_LCP) != 0 ||
        gtamd_contained_set_index_esa(ct, ctx, both, n2) != 0 || gtamd_contained_decide(ct, &info) != 0)
      goto deverr;
    if (info.reads != valid) {
      gtamd_failf(err, errlen, "%llu reads decided, %llu expected", (unsigned long long) info.reads,
                  (unsigned long long) valid);
      goto done;
    }
    if ((verdict = malloc(valid)) == NULL) { gtamd_fail(err, errlen, "out of memory (%s)", "verdicts"); goto done; }
    if (gtamd_contained_verdicts(ct, verdict, 0) != 0 || gtamd_contained_compact(ct, mask, NULL, n1, &dev, &nkept) != 0)
      goto deverr;
    contained = info.count[GTAMD_CONTAINED_DUPLICATE] + info.count[GTAMD_CONTAINED_AFFIX];
    if (strict) { inner = info.count[GTAMD_CONTAINED_INTERNAL]; selfc = info.count[GTAMD_CONTAINED_SELF_COMPLEMENTARY]; }
    output = valid - contained - inner - selfc;
    /* the file table counts the reads that are left */
    for (size_t g = 0; g < numfiles; g++) pf[g].kept_reads = pf[g].kept_letters = 0;
    if ((removed = calloc(valid, 1)) == NULL) { gtamd_fail(err, errlen, "out of memory (%s)", "verdicts"); goto done; }
    {
      uint64_t left = numfiles ? perfile[0] : 0;
      for (uint64_t k = 0; k < input; k++) {
        const uint64_t begin = k ? seps[k - 1] + 1 : 0, len = (k + 1 < input ? seps[k] : sum.totallength) - begin;
        while (left == 0 && f + 1 < numfiles) left = perfile[++f];
        left--;
        if (flags[k]) continue;
        if (mask >> verdict[at] & 1) removed[at] = 1;
        else { pf[f].kept_reads++; pf[f].kept_letters += len; }
        at++;
      }
    }
  }
  if (!encodeonly) {
    percent_line(verbose, quiet, "contained reads", contained, input);
    if (!quiet) printf("# number of reads in filtered readset = %llu\n", (unsigned long long) output);
  }
  if (nkept != 0 || fasta) {
    if ((kept = malloc(nkept ? nkept : 1)) == NULL) { gtamd_fail(err, errlen, "out of memory (%s)", "reads"); goto done; }
    if (nkept != 0 && gtamd_contained_result(ct, kept, 0) != 0) goto deverr;
  }
  if (cnt) {
    snprintf(path, sizeof path, "%s.cnt", readset);
    if (gtamd_prefilter_write_cntlist(path, removed != NULL ? removed : flags + input, valid, err, errlen) != 0) goto done;
    if (verbose) printf("# contained reads list saved: %s\n", path);
  }
  if (fasta) {
    snprintf(path, sizeof path, "%s.p.fas", readset);
    if (write_fasta(path, kept, nkept, err, errlen) != 0) goto done;
    if (verbose) printf("# %sreadset saved: %s\n", encodeonly ? "" : "suffix-prefix-free ", path);
  }
  if (output != 0) {
    if (gtamd_prefilter_write_readset(readset, db, numfiles, pf, kept, nkept, err, errlen) != 0) goto done;
    if (verbose) printf("# %sreadset saved: %s.%s\n", encodeonly ? "" : "suffix-prefix-free ", readset,
                        varlen ? "(esq|ssp)" : "esq");
  } else if (!encodeonly) {
    if (!quiet) printf("# no readset saved as no sequence passed the filters\n");
  } else if (verbose) printf("# readset saved: %s.%s\n", readset, varlen ? "(esq|ssp)" : "esq");
  if (encodeonly && !quiet) printf("# number of reads in output readset = %llu\n", (unsigned long long) output);
  if (strict && !encodeonly && !quiet)
    printf("# reads inside other reads removed = %llu\n# self-complementary reads removed = %llu\n",
           (unsigned long long) inner, (unsigned long long) selfc);
  if (fflush(stdout) != 0) { gtamd_fail(err, errlen, "cannot write to %s", "stdout"); goto done; }
  rc = 0;
  goto done;
deverr:
  snprintf(err, errlen, "%s", gtamd_esa_last_error());
done:
  gtamd_contained_destroy(ct);
  if (ctx != NULL) gtamd_esa_destroy(ctx);
  if (de != NULL) gtamd_encoder_destroy(de);
  free(pf); free(perfile); free(seps); free(flags); free(verdict); free(kept); free(removed);
  return rc;
}
