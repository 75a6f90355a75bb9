/* locali_host.c -- `gt dev idxlocali -th T -esa INDEX -q FILES` for this path
   (tool src/tools/gt_idxlocali.c, gt_runidxlocali and idxlocali_showmatch
   src/match/idxlocali.c): every local alignment of the queries against an index
   whose score reaches the threshold, on the device through
   include/gtamd_locali.h.  The stdout is the reference's byte for byte but for
   the order of the match blocks of one query, which is the table's here and the
   reference's stack's there.

   The device gives (dbstart, dblen, score, qstart, qlen) and no edit script: for
   -s the alignment of a match is rebuilt here, from the columns 1 .. dblen of its
   start position with stored traces and the traceback from the row qstart +
   qlen, by the column rule of the header. */
#include "host_internal.h"
#include "gtamd_locali.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define IDXLOCALI_CAPACITY (1u << 20)            /* records of one gtamd_locali_emit */

typedef struct {
  uint8_t *symbols;      /* the queries' codes, one query after the other */
  uint64_t *offsets;     /* count + 1 */
  uint64_t count;
} querylist;

/* The sequences of FASTA files as codes of the index's alphabet, wildcards kept;
   a character the alphabet does not know ends the call with the reference's
   message (gt_seq_iterator_sequence_buffer_next). */
static int read_queries(const char *const *paths, size_t numfiles, const gtamd_alphabet *alpha, querylist *ql,
                        char *err, size_t errlen)
{
  uint64_t cap_sym = 1 << 16, cap_off = 1 << 10, used = 0;
  ql->symbols = malloc(cap_sym);
  ql->offsets = malloc(cap_off * sizeof *ql->offsets);
  ql->count = 0;
  if (ql->symbols == NULL || ql->offsets == NULL) return gtamd_fail(err, errlen, "out of memory (%s)", "queries");
  ql->offsets[0] = 0;
  for (size_t f = 0; f < numfiles; f++) {
    uint8_t *data = NULL;
    uint64_t len = 0, i = 0, line = 1;
    const int rc = gtamd_read_input_file(paths[f], &data, &len);
    if (rc != 0) {
      gtamd_read_input_error(rc, paths[f], err, errlen);
      return -1;
    }
    if (len > 0 && data[0] != '>') {
      free(data);
      return gtamd_fail(err, errlen, "the first character of fasta file \"%s\" has to be '>'", paths[f]);
    }
    while (i < len) {
      while (i < len && data[i] != '\n') i++;            /* the description */
      for (; i < len && data[i] != '>'; i++) {
        uint8_t code;
        if (data[i] == '\n') { line++; continue; }
        if (data[i] == '\r' || data[i] == ' ' || data[i] == '\t') continue;
        code = alpha->symbolmap[data[i]];
        if (code == 253) {
          snprintf(err, errlen, "illegal character '%c': file \"%s\", line %llu", data[i], paths[f],
                   (unsigned long long) line);
          free(data);
          return -1;
        }
        if (used == cap_sym) {
          uint8_t *grown = realloc(ql->symbols, cap_sym *= 2);
          if (grown == NULL) { free(data); return gtamd_fail(err, errlen, "out of memory (%s)", "queries"); }
          ql->symbols = grown;
        }
        ql->symbols[used++] = code;
      }
      if (ql->count + 1 == cap_off) {
        uint64_t *grown = realloc(ql->offsets, (cap_off *= 2) * sizeof *ql->offsets);
        if (grown == NULL) { free(data); return gtamd_fail(err, errlen, "out of memory (%s)", "queries"); }
        ql->offsets = grown;
      }
      ql->offsets[++ql->count] = used;
    }
    free(data);
  }
  return 0;
}

enum { TRACE_NONE = 0, TRACE_INSERT, TRACE_REPLACE, TRACE_DELETE };

/* The alignment of a match as gt_alignment_show_with_mapped_chars shows it
   (src/extended/alignment.c:528-643), `width` columns a block: the query
   substring on top, the subject substring below, '|' between equal letters and
   '-' for a gap.  0, or -1 when the columns do not lead from (e, dblen) to
   column 0 (a damaged index). */
static int show_alignment(FILE *fp, const gtamd_alphabet *alpha, const uint8_t *enc, uint64_t p, uint32_t dblen,
                          const uint8_t *q, uint32_t m, uint32_t e, int match, int mismatch, int gapextend,
                          unsigned width)
{
  const uint64_t rows = (uint64_t) m + 1;
  int64_t *col = malloc(2 * rows * sizeof *col);
  uint8_t *trace = malloc(rows * dblen), *ops = malloc((size_t) dblen + m + 1);
  char *buf = malloc(3 * ((size_t) width + 1));
  uint64_t count = 0, iu, iv = p;
  uint32_t d, i;
  unsigned pos = 0;
  int rc = -1;
  if (col == NULL || trace == NULL || ops == NULL || buf == NULL) goto done;
  for (d = 1; d <= dblen; d++) {
    int64_t *out = col + (d & 1) * rows;
    const int64_t *in = col + ((d - 1) & 1) * rows;
    const uint8_t c = enc[p + d - 1];
    uint8_t *tr = trace + (uint64_t) (d - 1) * rows;
    out[0] = -1;
    tr[0] = TRACE_NONE;
    for (i = 1; i <= m; i++) {
      const int64_t r = q[i - 1] == c && c < 254 ? match : mismatch;
      int64_t v = -1;
      uint8_t t = TRACE_NONE;
      if (out[i - 1] > 0 && out[i - 1] + gapextend > v) { v = out[i - 1] + gapextend; t = TRACE_DELETE; }
      if (d == 1) {
        if (r > v) { v = r; t = TRACE_REPLACE; }
        if (gapextend > v) { v = gapextend; t = TRACE_INSERT; }
      } else {
        if (in[i - 1] > 0 && in[i - 1] + r > v) { v = in[i - 1] + r; t = TRACE_REPLACE; }
        if (in[i] > 0 && in[i] + gapextend > v) { v = in[i] + gapextend; t = TRACE_INSERT; }
      }
      out[i] = v;
      tr[i] = t;
    }
  }
  for (d = dblen, i = e; d > 0; ) {
    const uint8_t t = trace[(uint64_t) (d - 1) * rows + i];
    if (t == TRACE_NONE || (t != TRACE_INSERT && i == 0)) goto done;
    ops[count++] = t;
    if (t != TRACE_DELETE) d--;
    if (t != TRACE_INSERT) i--;
  }
  iu = i;
  buf[width] = buf[2 * width + 1] = buf[3 * width + 2] = '\n';
  while (count-- > 0) {
    const uint8_t t = ops[count];
    const uint8_t a = t != TRACE_INSERT ? q[iu] : 0, b = t != TRACE_DELETE ? enc[iv] : 0;
    buf[pos] = t == TRACE_INSERT ? '-' : a >= 254 ? alpha->wildcardshow : alpha->characters[a];
    buf[width + 1 + pos] = t == TRACE_REPLACE && a == b && a < 254 ? '|' : ' ';
    buf[2 * width + 2 + pos] = t == TRACE_DELETE ? '-' : b >= 254 ? alpha->wildcardshow : alpha->characters[b];
    iu += t != TRACE_INSERT;
    iv += t != TRACE_DELETE;
    if (++pos == width) {
      fwrite(buf, 1, 3 * ((size_t) width + 1), fp);
      pos = 0;
    }
  }
  if (pos > 0) {
    for (int k = 0; k < 3; k++) {
      fwrite(buf + k * (width + 1), 1, pos, fp);
      fputc('\n', fp);
    }
  }
  rc = 0;
done:
  free(col); free(trace); free(ops); free(buf);
  return rc;
}

/* an integer argument of the reference's parser */
static int int_option(int argc, const char **argv, int *i, long *value, char *err, size_t errlen)
{
  char *end;
  if (*i + 1 >= argc) return gtamd_fail(err, errlen, "missing argument to option \"%s\"", argv[*i]);
  *value = strtol(argv[*i + 1], &end, 10);
  if (*end != 0 || end == argv[*i + 1]) {
    if (argv[*i + 1][0] == '-') return gtamd_fail(err, errlen, "missing argument to option \"%s\"", argv[*i]);
    return gtamd_fail(err, errlen, "argument to option \"%s\" must be an integer", argv[*i]);
  }
  (*i)++;
  return 0;
}

int gtamd_idxlocali(int argc, const char **argv, char *err, size_t errlen)
{
  static const char *const not_here[] = { "-pck", "-online", "-cmp", NULL };
  const char *index = NULL, *const *queryfiles = NULL;
  size_t numqueryfiles = 0;
  long match = 1, mismatch = -3, gapstart = -5, gapextend = -2, threshold = 0;
  int have_th = 0, showalignment = 0, verbose = 0, rc = -1;
  uint64_t next = 0;
  gtamd_project prj = { 0 };
  querylist ql = { NULL, NULL, 0 };
  gtamd_locali *lc = NULL;
  gtamd_locali_info info;
  gtamd_locali_record *rec = NULL;

  for (int i = 1; i < argc; i++) {
    const char *a = argv[i];
    if (!strcmp(a, "-esa")) { if (gtamd_opt_name(argc, argv, &i, &index, err, errlen) != 0) return -1; }
    else if (!strcmp(a, "-th")) {
      /* (an unsigned option of the reference's parser: "-3" is the next option, not a number) */
      if (i + 1 < argc && argv[i + 1][0] == '-') return gtamd_fail(err, errlen, "missing argument to option \"%s\"", a);
      if (int_option(argc, argv, &i, &threshold, err, errlen) != 0)
        return i + 1 < argc ? gtamd_fail(err, errlen, "argument to option \"%s\" is out of range", a) : -1;
      if (threshold < 1) return gtamd_fail(err, errlen, "argument to option \"%s\" must be an integer >= 1", a);
      have_th = 1;
    } else if (!strcmp(a, "-match")) { if (int_option(argc, argv, &i, &match, err, errlen) != 0) return -1; }
    else if (!strcmp(a, "-mismatch")) { if (int_option(argc, argv, &i, &mismatch, err, errlen) != 0) return -1; }
    else if (!strcmp(a, "-gapstart")) { if (int_option(argc, argv, &i, &gapstart, err, errlen) != 0) return -1; }
    else if (!strcmp(a, "-gapextend")) { if (int_option(argc, argv, &i, &gapextend, err, errlen) != 0) return -1; }
    else if (!strcmp(a, "-q")) {
      if (gtamd_opt_files(argc, argv, &i, &queryfiles, &numqueryfiles, err, errlen) != 0) return -1;
    } else if (!strcmp(a, "-s")) showalignment = gtamd_opt_switch(argc, argv, &i);
    else if (!strcmp(a, "-v")) verbose = gtamd_opt_switch(argc, argv, &i);
    else if (!strcmp(a, "-help")) {
      puts("Usage: gt-suffixerator-amd idxlocali [options] -q query-file-names -esa indexname\n"
           "Find all local alignments using the suffix table, on the device.\n\n"
           "-q         files containing the query sequences (FASTA, at most 16384 letters a query)\n"
           "-match     match score (default: 1)\n"
           "-mismatch  mismatch score (default: -3)\n"
           "-gapstart  gap start score (default: -5); parsed and without effect, as in the reference, whose affine\n"
           "           gap model is compiled out\n"
           "-gapextend gap extension score (default: -2)\n"
           "-th        the threshold: the smallest score of an alignment that is reported\n"
           "-esa       the index: INDEX.prj, .esq, .ssp and .suf, as written by `suffixerator -tis -suf -ssp`\n"
           "-s         show the alignment behind each match\n"
           "-v         figures of the search as a line that starts with '#', behind the matches\n\n"
           "The output is that of `gt dev idxlocali`; the matches of one query come in the order of the suffix\n"
           "table.  A match score that is not positive, and a mismatch or gap extension score that is not negative,\n"
           "are refused (the reference takes them, and need not end then).  -pck, -online and -cmp are refused.");
      return 0;
    } else return gtamd_opt_tail(a, not_here, GTAMD_UNKNOWN_TRY, GTAMD_SUPERFLUOUS_MORE, err, errlen);
  }
  (void) gapstart;
  if (queryfiles == NULL) return gtamd_fail(err, errlen, "option \"-%s\" is mandatory", "q");
  if (!have_th) return gtamd_fail(err, errlen, "option \"-%s\" is mandatory", "th");
  if (index == NULL) return gtamd_fail(err, errlen, "either option \"-esa\" or option \"-%s\" is mandatory", "pck");
  if (match <= 0 || mismatch >= 0 || gapextend >= 0 || match > 32767 || mismatch < -32767 || gapextend < -32767)
  {
    snprintf(err, errlen, "scores -match %ld -mismatch %ld -gapextend %ld: the match score must be in 1..32767, the "
             "mismatch and the gap extension score in -32767..-1", match, mismatch, gapextend);
    return -1;
  }
  if (threshold > 0xffffffffl) threshold = 0xffffffffl;      /* (no score reaches it) */

  /* gt_idxlocali_runner: these lines come before the index is read */
  printf("# indexname(esa)=%s\n", index);
  for (size_t f = 0; f < numqueryfiles; f++) printf("# queryfile=%s\n", queryfiles[f]);
  printf("# threshold=%ld\n", threshold);

  if (gtamd_project_open(&prj, index, "searched", GTAMD_PROJECT_FORWARD, "idxlocali", err, errlen) != 0 ||
      gtamd_project_map(&prj, index, GTAMD_TABLE_SUF, 1, err, errlen) != 0 ||
      read_queries(queryfiles, numqueryfiles, &prj.alpha, &ql, err, errlen) != 0)
    goto done;
  rec = malloc(IDXLOCALI_CAPACITY * sizeof *rec);
  if (gtamd_project_sequence_starts(&prj) != 0 || rec == NULL) {
    gtamd_fail(err, errlen, "out of memory (%s)", "records");
    goto done;
  }

  if (ql.count > 0) {
    if ((lc = gtamd_locali_create(0)) == NULL ||
        gtamd_locali_set_index_host(lc, prj.enc, prj.n, prj.suf.p, prj.suf_bytes, prj.alpha.numofchars) != 0 ||
        gtamd_locali_prepare(lc, ql.symbols, ql.offsets, ql.count, 0, (int32_t) match, (int32_t) mismatch,
                             (int32_t) gapextend, (uint32_t) threshold, &info) != 0) {
      snprintf(err, errlen, "%s", gtamd_esa_last_error());
      goto done;
    }
    for (uint64_t cursor = 0, written = 1; written != 0; ) {
      if (gtamd_locali_emit(lc, &cursor, rec, IDXLOCALI_CAPACITY, 0, &written) != 0) {
        snprintf(err, errlen, "%s", gtamd_esa_last_error());
        goto done;
      }
      for (uint64_t k = 0; k < written; k++) {
        const uint64_t t = rec[k].query, p = rec[k].dbstart;
        const uint32_t dblen = (uint32_t) rec[k].lenscore, score = (uint32_t) (rec[k].lenscore >> 32);
        const uint32_t qstart = (uint32_t) rec[k].qspan, qlen = (uint32_t) (rec[k].qspan >> 32);
        const uint64_t seq = gtamd_unit_of(prj.seqstart, prj.numseq, p);
        for (; next <= t; next++)                       /* the lines of the queries up to this one */
          printf("process sequence %llu of length %llu\n", (unsigned long long) next,
                 (unsigned long long) (ql.offsets[next + 1] - ql.offsets[next]));
        printf("%llu\t%llu\t%u\t\t%llu\t%u\t%u\t%u\n", (unsigned long long) seq,
               (unsigned long long) (p - prj.seqstart[seq]), dblen, (unsigned long long) t, qstart, qlen, score);
        if (showalignment &&
            (t >= ql.count || p + dblen > prj.n || (uint64_t) qstart + qlen > ql.offsets[t + 1] - ql.offsets[t] ||
             show_alignment(stdout, &prj.alpha, prj.enc, p, dblen, ql.symbols + ql.offsets[t],
                            (uint32_t) (ql.offsets[t + 1] - ql.offsets[t]), qstart + qlen, (int) match, (int) mismatch,
                            (int) gapextend, 70) != 0)) {
          snprintf(err, errlen, "the match at position %llu of query %llu has no alignment: the index is damaged, or "
                   "memory ran out", (unsigned long long) p, (unsigned long long) t);
          goto done;
        }
      }
    }
    for (; next < ql.count; next++)
      printf("process sequence %llu of length %llu\n", (unsigned long long) next,
             (unsigned long long) (ql.offsets[next + 1] - ql.offsets[next]));
    if (verbose && gtamd_locali_get_info(lc, &info) == 0)
      printf("# %llu jobs in %llu groups cut at depth %u, %llu matches, at most %llu of one job, %llu children "
             "examined, %llu levels, %llu single-suffix walks, %llu jobs with a child that found no room on the stack, "
             "%.3f ms on the device\n", (unsigned long long) info.jobs, (unsigned long long) info.groups, info.cut_depth,
             (unsigned long long) info.matches, (unsigned long long) info.max_matches_of_one_job,
             (unsigned long long) info.children_examined, (unsigned long long) info.levels_pushed,
             (unsigned long long) info.single_walks, (unsigned long long) info.jobs_finished_alone, info.device_ms);
  }
  if (fflush(stdout) != 0) { gtamd_fail(err, errlen, "cannot write to %s", "stdout"); goto done; }
  rc = 0;
done:
  fflush(stdout);
  gtamd_locali_destroy(lc);
  gtamd_project_close(&prj);
  free(rec); free(ql.offsets); free(ql.symbols);
  return rc;
}
