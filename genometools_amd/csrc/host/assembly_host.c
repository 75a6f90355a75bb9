/* assembly_host.c -- `gt readjoiner assembly -readset X` with default options for
   this path (tool src/tools/gt_readjoiner_assembly.c; the traversal it replaces:
   src/match/rdj-strgraph.c, rdj-contigpaths.c): the contigs of the string graph of
   Readjoiner's binary list X.0.spm over the reads of X.esq, on the device through
   include/gtamd_strgraph.h.  X.contigs.fas and the stdout are the reference's byte
   for byte (src/match/rdj-contigs-writer.c, src/extended/assembly_stats_calculator.c);
   X.paths, the reference's intermediate file, is not written.  The sub-command is
   `gt-suffixerator-amd assembly`: `readjoiner assembly` keeps the dispatcher's
   answer. */
#include "host_internal.h"
#include "gtamd_strgraph.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#define ASM_VERSION "1.2"                        /* GT_READJOINER_VERSION */
#define ASM_BIN32 2                              /* GT_SPMLIST_BIN32, the header byte */
#define ASM_WIDTH 60                             /* letters of a line of X.contigs.fas */
#define ASM_CAPACITY (1u << 20)                  /* contigs, or symbols, of one emit call */

/* ---- the reader of the bin32 list (the writer: rdj_host.c) ---- */

int gtamd_spmlist_bin32_read(const char *path, const uint32_t *readlen, uint64_t reads, gtamd_spmred_record **rec,
                             uint64_t *count, char *err, size_t errlen)
{
  FILE *fp = fopen(path, "rb");
  long size;
  int format, bad = 0;
  uint64_t n;
  gtamd_spmred_record *out = NULL;
  *rec = NULL;
  *count = 0;
  if (fp == NULL) return gtamd_fail(err, errlen, "cannot open file '%s'", path);
  if (fseek(fp, 0, SEEK_END) != 0 || (size = ftell(fp)) < 0 || fseek(fp, 0, SEEK_SET) != 0) {
    fclose(fp);
    return gtamd_fail(err, errlen, "cannot read file '%s'", path);
  }
  if (size == 0) { fclose(fp); return gtamd_fail(err, errlen, "file '%s' is empty: no list of matches", path); }
  format = fgetc(fp);
  if (format != ASM_BIN32) {
    fclose(fp);
    return gtamd_failf(err, errlen, "file '%s' starts with byte %d: only the bin32 list format (byte %d) is read", path,
                       format, ASM_BIN32);
  }
  if ((size - 1) % 12 != 0) {
    fclose(fp);
    return gtamd_failf(err, errlen, "file '%s' is truncated: %ld bytes behind the format byte are no whole number of "
                       "matches of 12 bytes", path, size - 1);
  }
  n = (uint64_t) (size - 1) / 12;
  out = malloc((n ? n : 1) * sizeof *out);
  if (out == NULL) { fclose(fp); return gtamd_fail(err, errlen, "out of memory (%s)", "list of matches"); }
  for (uint64_t k = 0; k < n; k++) {
    uint32_t w[3];
    if (fread(w, sizeof w, 1, fp) != 1) {
      fclose(fp); free(out);
      return gtamd_fail(err, errlen, "cannot read file '%s'", path);
    }
    out[k].suffix_read = w[0];
    out[k].prefix_read = w[1];
    out[k].len = w[2] >> 2;
    out[k].flags = w[2] & 3;
    if (w[0] >= reads || w[1] >= reads)
      bad = gtamd_failf(err, errlen, "file '%s': match %llu names read %lu, the read set holds %llu reads", path,
                        (unsigned long long) k, (unsigned long) (w[0] >= reads ? w[0] : w[1]), (unsigned long long) reads);
    else if (out[k].len > readlen[w[0]] || out[k].len > readlen[w[1]])
      bad = gtamd_failf(err, errlen, "file '%s': match %llu of reads %lu and %lu has %llu letters, more than a read of "
                        "%lu and one of %lu hold", path, (unsigned long long) k, (unsigned long) w[0], (unsigned long) w[1],
                        (unsigned long long) out[k].len, (unsigned long) readlen[w[0]], (unsigned long) readlen[w[1]]);
    else if (out[k].flags == 0)
      bad = gtamd_failf(err, errlen, "file '%s': match %llu has both reads reversed, which no list holds", path,
                        (unsigned long long) k);
    if (bad != 0) {
      fclose(fp); free(out);
      return -1;
    }
  }
  fclose(fp);
  *rec = out;
  *count = n;
  return 0;
}

/* ---- the statistics block (gt_assembly_stats_calculator_show) ---- */

static int descending(const void *a, const void *b)
{
  const uint64_t x = *(const uint64_t *) a, y = *(const uint64_t *) b;
  return x < y ? 1 : x > y ? -1 : 0;
}

int gtamd_assembly_statistics(const uint64_t *lengths, uint64_t count, char *out, size_t outlen)
{
  static const uint64_t limit[5] = { 500, 1000, 10000, 100000, 1000000 };
  static const char *const limit_name[5] = { "500 nt: ", "1K nt:  ", "10K nt: ", "100K nt:", "1M nt:  " };
  static const unsigned nvals[2] = { 50, 80 };
  uint64_t *sorted, sum = 0, larger[5] = { 0, 0, 0, 0, 0 }, min[2], nvalue[2] = { 0, 0 }, lvalue[2] = { 0, 0 };
  uint64_t half, fourth, three, median = 0, q1 = 0, q3 = 0, cur_len = 0, cur_num = 0;
  int done[2] = { 0, 0 }, at = 0;
  if (count == 0) return snprintf(out, outlen, "# no contigs respect the given cutoff parameters\n") < (int) outlen ? 0 : -1;
  sorted = malloc(count * sizeof *sorted);
  if (sorted == NULL) return -1;
  memcpy(sorted, lengths, count * sizeof *sorted);
  qsort(sorted, count, sizeof *sorted, descending);
  for (uint64_t k = 0; k < count; k++) sum += sorted[k];
  /* (the reference multiplies in single precision) */
  for (int i = 0; i < 2; i++) min[i] = (uint64_t) ((float) sum * ((float) nvals[i] / 100U));
  half = count >> 1;
  fourth = half >> 1;
  three = fourth + half;
  for (uint64_t k = 0; k < count;) {
    const uint64_t key = sorted[k];
    uint64_t value = 0;
    while (k < count && sorted[k] == key) { k++; value++; }
    cur_len += key * value;
    cur_num += value;
    for (int i = 0; i < 5; i++) if (key > limit[i]) larger[i] = cur_num;
    if (q3 == 0 && cur_num >= fourth) q3 = key;
    if (median == 0 && cur_num >= half) median = key;
    if (q1 == 0 && cur_num >= three) q1 = key;
    for (int i = 0; i < 2; i++)
      if (!done[i] && cur_len >= min[i]) { done[i] = 1; nvalue[i] = key; lvalue[i] = cur_num; }
  }
#define ASM_LINE(...) do { \
    const int w_ = snprintf(out + at, outlen - (size_t) at, __VA_ARGS__); \
    if (w_ < 0 || (size_t) (at + w_) >= outlen) { free(sorted); return -1; } \
    at += w_; } while (0)
  ASM_LINE("# number of contigs:     %llu\n", (unsigned long long) count);
  ASM_LINE("# total contigs length:  %llu\n", (unsigned long long) sum);
  ASM_LINE("# mean contig size:      %.2f\n", (double) sum / count);
  ASM_LINE("# contig size first quartile: %llu\n", (unsigned long long) q1);
  ASM_LINE("# median contig size:         %llu\n", (unsigned long long) median);
  ASM_LINE("# contig size third quartile: %llu\n", (unsigned long long) q3);
  ASM_LINE("# longest contig:             %llu\n", (unsigned long long) sorted[0]);
  ASM_LINE("# shortest contig:            %llu\n", (unsigned long long) sorted[count - 1]);
  for (int i = 0; i < 5; i++)
    ASM_LINE("# contigs > %s          %llu (%.2f %%)\n", limit_name[i], (unsigned long long) larger[i],
             (double) larger[i] * 100 / count);
  for (int i = 0; i < 2; i++) {
    if (nvalue[i] > 0) {
      ASM_LINE("# N%02u                %llu\n", nvals[i], (unsigned long long) nvalue[i]);
      ASM_LINE("# L%02u                %llu\n", nvals[i], (unsigned long long) lvalue[i]);
    } else {
      ASM_LINE("# N%02u                n.a.\n", nvals[i]);
      ASM_LINE("# L%02u                n.a.\n", nvals[i]);
    }
  }
#undef ASM_LINE
  free(sorted);
  return 0;
}

/* ---- X.contigs.fas (gt_contigs_writer_write, gt_fasta_show_entry) ---- */

static void vertex_name(char *to, size_t len, uint64_t v)
{
  snprintf(to, len, "%llu%c", (unsigned long long) (v >> 1), v & 1 ? 'E' : 'B');
}

static int write_contig(FILE *fp, uint64_t number, const gtamd_strgraph_contig *c, const uint8_t *sym)
{
  char first[32], last[32], line[ASM_WIDTH + 1];
  vertex_name(first, sizeof first, c->first_vertex);
  vertex_name(last, sizeof last, c->last_vertex);
  if (fprintf(fp, ">contig_%llu length=%llu depth=%llu %s%s%s\n", (unsigned long long) number,
              (unsigned long long) c->length, (unsigned long long) c->depth, first,
              c->depth > 2 ? "-->...-->" : c->depth > 1 ? "-->" : "", c->depth > 1 ? last : "") < 0)
    return -1;
  for (uint64_t a = 0; a < c->length; a += ASM_WIDTH) {
    const uint64_t w = c->length - a < ASM_WIDTH ? c->length - a : ASM_WIDTH;
    for (uint64_t k = 0; k < w; k++) line[k] = "acgt"[sym[a + k] & 3];
    line[w] = '\n';
    if (fwrite(line, 1, w + 1, fp) != w + 1) return -1;
  }
  return 0;
}

int gtamd_assembly(int argc, const char **argv, char *err, size_t errlen)
{
  /* error cleaning, the reference's own reduction, A-statistics, saved graphs, the files of the contig graph,
     its second phase alone and its verbose lines: no counterpart here */
  static const char *const refused[] = {
    "-redtrans", "-errors", "-bubble", "-deadend", "-deadend-depth", "-paths2seq", "-buffersize", "-vd", "-astat",
    "-cov", "-copynum", "-load", "-save", "-cinfo", "-v", NULL };
  const char *readset = NULL;
  uint32_t minlen = 0, depthcutoff = GTAMD_STRGRAPH_DEPTHCUTOFF, lengthcutoff = GTAMD_STRGRAPH_LENGTHCUTOFF, spmfiles = 1;
  int quiet = 0, rc = -1;
  char path[4096], stats[4096];
  uint8_t *enc = NULL, *sym = NULL;
  uint32_t *readlen = NULL;
  uint64_t n = 0, reads = 0, count = 0, cursor = 0, written = 0, *lengths = NULL;
  gtamd_alphabet alpha;
  gtamd_seqstats ss;
  gtamd_spmred_record *rec = NULL;
  gtamd_strgraph *sg = NULL;
  gtamd_strgraph_info info;
  gtamd_strgraph_contig *contigs = NULL;
  FILE *fas = NULL;

  memset(&alpha, 0, sizeof alpha);
  for (int i = 1; i < argc; i++) {
    const char *a = argv[i];
    uint32_t *number = !strcmp(a, "-l") ? &minlen : !strcmp(a, "-depthcutoff") ? &depthcutoff :
                       !strcmp(a, "-lengthcutoff") ? &lengthcutoff : !strcmp(a, "-spmfiles") ? &spmfiles : NULL;
    if (!strcmp(a, "-readset")) { if (gtamd_opt_name(argc, argv, &i, &readset, err, errlen) != 0) return -1; }
    else if (number != NULL) {
      /* (gt_option_new_uint_min: 2 for -l, 1 for the others) */
      const uint32_t least = number == &minlen ? 2 : 1;
      if (gtamd_opt_uint32(argc, argv, &i, number, err, errlen) != 0) return -1;
      if (*number < least) return gtamd_failf(err, errlen, "argument to option \"%s\" must be an integer >= %u", a, least);
    } else if (!strcmp(a, "-q")) quiet = gtamd_opt_switch(argc, argv, &i);
    else if (!strcmp(a, "-help")) {
      puts("Usage: gt-suffixerator-amd assembly -readset X [-l L] [-depthcutoff D] [-lengthcutoff C] [-spmfiles 1] [-q]\n"
           "Construct the string graph of the reads of X from their suffix-prefix matches and output its contigs,\n"
           "on the device: `gt readjoiner assembly` with default options.\n\n"
           "-readset       the encoded reads X.esq (.ssp), as `readjoiner prefilter` writes them, and the list of\n"
           "               matches X.0.spm (Readjoiner's bin32 format), as `readjoiner overlap` writes it, the\n"
           "               reference's or this project's\n"
           "-l             matches of fewer letters are left out (2 or more; default: none is)\n"
           "-depthcutoff   the minimal number of nodes in a contig (default 3)\n"
           "-lengthcutoff  the minimal length of a contig (default 100)\n"
           "-spmfiles      1: the one list this path reads\n"
           "-q             no lines that start with '#'\n\n"
           "Writes X.contigs.fas and prints the reference's lines, both byte for byte.  X.paths, the reference's\n"
           "intermediate file, is not written.  The contained reads a set of reads of several lengths may still\n"
           "hold (the reference's X.0.cnt) are not looked for: filter the set with readjoiner prefilter -strict.\n"
           "Error cleaning (-errors, -bubble, -deadend, -deadend-depth), -redtrans, A-statistics (-astat, -cov,\n"
           "-copynum), -load, -save, -cinfo, -paths2seq, -buffersize, -vd, -v and more than one list are refused.");
      return 0;
    } else return gtamd_opt_tail(a, refused, GTAMD_UNKNOWN_SHOWS, GTAMD_UNNECESSARY, err, errlen);
  }
  if (readset == NULL) return gtamd_fail(err, errlen, "option \"-%s\" is mandatory", "readset");
  if (spmfiles != 1)
    return gtamd_fail(err, errlen, "option \"%s\" above 1 is not supported by the MI355X engine: one list, X.0.spm, is read",
                      "-spmfiles");

  if (!quiet) printf("# gt readjoiner assembly (version " ASM_VERSION ")\n");
  snprintf(path, sizeof path, "%s.esq", readset);
  if (access(path, R_OK) != 0) return gtamd_fail(err, errlen, "cannot open file '%s'", path);
  if (gtamd_read_esq_alpha(readset, &enc, &n, &alpha, &ss, err, errlen) != 0) return -1;
  if (!gtamd_alphabet_is_dna(&alpha)) {
    snprintf(err, errlen, "mirroring can only be enabled for DNA sequences, this encoded sequence has "
             "alphabet: %.*s", (int) alpha.numofchars, alpha.characters);
    goto done;
  }
  if (n == 0) { gtamd_fail(err, errlen, "readset '%s' holds no symbol", readset); goto done; }
  reads = 1;
  for (uint64_t k = 0; k < n; k++) reads += enc[k] == 255;
  if (n >= (1ull << 31) || reads > (1ull << 30)) {
    snprintf(err, errlen, "%llu symbols in %llu reads are beyond the limits of the string graph (2^31 symbols, 2^30 "
             "reads)", (unsigned long long) n, (unsigned long long) reads);
    goto done;
  }
  readlen = malloc(reads * sizeof *readlen);
  if (readlen == NULL) { gtamd_fail(err, errlen, "out of memory (%s)", "read lengths"); goto done; }
  for (uint64_t k = 0, r = 0, start = 0; k <= n; k++)
    if (k == n || enc[k] == 255) { readlen[r++] = (uint32_t) (k - start); start = k + 1; }
  if (!quiet) printf("# number of reads in filtered readset = %llu\n", (unsigned long long) reads);
  if (!quiet) printf("# calculate edges space for each vertex\n");
  snprintf(path, sizeof path, "%s.0.spm", readset);
  if (gtamd_spmlist_bin32_read(path, readlen, reads, &rec, &count, err, errlen) != 0) goto done;
  if (!quiet) printf("# build string graph\n");
  if ((sg = gtamd_strgraph_create(0)) == NULL || gtamd_strgraph_set_reads(sg, enc, n, 0) != 0 ||
      gtamd_strgraph_set_matches(sg, rec, count, 0) != 0 ||
      gtamd_strgraph_prepare(sg, minlen, depthcutoff, lengthcutoff, &info) != 0) {
    snprintf(err, errlen, "%s", gtamd_esa_last_error());
    goto done;
  }
  if (!quiet) printf("# save contig paths\n# pump encseq through cache\n# save contig sequences\n");

  contigs = malloc((info.contigs ? info.contigs : 1) * sizeof *contigs);
  lengths = malloc((info.contigs ? info.contigs : 1) * sizeof *lengths);
  sym = malloc(info.total_length ? info.total_length : 1);
  if (contigs == NULL || lengths == NULL || sym == NULL) { gtamd_fail(err, errlen, "out of memory (%s)", "contigs"); goto done; }
  do {
    if (gtamd_strgraph_emit(sg, &cursor, contigs + cursor, ASM_CAPACITY, 0, &written) != 0) {
      snprintf(err, errlen, "%s", gtamd_esa_last_error());
      goto done;
    }
  } while (written != 0);
  if (cursor != info.contigs) {
    snprintf(err, errlen, "%llu contigs counted, %llu given", (unsigned long long) info.contigs, (unsigned long long) cursor);
    goto done;
  }
  cursor = 0;
  do {
    if (gtamd_strgraph_emit_symbols(sg, &cursor, sym + cursor, ASM_CAPACITY, 0, &written) != 0) {
      snprintf(err, errlen, "%s", gtamd_esa_last_error());
      goto done;
    }
  } while (written != 0);
  if (cursor != info.total_length) {
    snprintf(err, errlen, "%llu symbols counted, %llu given", (unsigned long long) info.total_length,
             (unsigned long long) cursor);
    goto done;
  }
  snprintf(path, sizeof path, "%s.contigs.fas", readset);
  if ((fas = fopen(path, "wb")) == NULL) { gtamd_fail(err, errlen, "cannot open file '%s' for writing", path); goto done; }
  for (uint64_t c = 0; c < info.contigs; c++) {
    lengths[c] = contigs[c].length;
    if (write_contig(fas, c, &contigs[c], sym + contigs[c].offset) != 0) { gtamd_fail(err, errlen, "cannot write file '%s'", path); goto done; }
  }
  {
    const int closed = fclose(fas);
    fas = NULL;
    if (closed != 0) { gtamd_fail(err, errlen, "cannot close file '%s'", path); goto done; }
  }
  if (!quiet) {
    if (gtamd_assembly_statistics(lengths, info.contigs, stats, sizeof stats) != 0) {
      gtamd_fail(err, errlen, "out of memory (%s)", "statistics");
      goto done;
    }
    fputs(stats, stdout);
  }
  if (fflush(stdout) != 0) { gtamd_fail(err, errlen, "cannot write to %s", "stdout"); goto done; }
  rc = 0;
done:
  if (fas != NULL) fclose(fas);
  gtamd_strgraph_destroy(sg);
  gtamd_alphabet_free(&alpha);
  free(contigs); free(lengths); free(sym); free(rec); free(readlen); free(enc);
  return rc;
}
