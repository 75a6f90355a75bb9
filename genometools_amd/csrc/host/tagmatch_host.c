/* tagmatch_host.c -- `gt tagerator -e K -esa INDEX -q TAGS` for this path (tool
   src/tools/gt_tagerator.c, gt_runtagerator src/match/tagerator.c:538-773): the
   approximate matches of short tags against an index, on the device through
   include/gtamd_tagmatch.h.  The stdout is the reference's byte for byte but for
   the order of the match lines of one tag and strand, which is the table's here
   and the reference's stack's there.  The project is read back through
   project_host.c, the options through cli_host.c. */
#include "host_internal.h"
#include "gtamd_tagmatch.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define TAGERATOR_CAPACITY (1u << 20)            /* records of one gtamd_tagmatch_emit */
#define MAXTAGSIZE 64

/* the keywords of -output in the order they are shown (gt_tagerator.c:36-52) */
enum { OUT_TAGNUM = 1, OUT_TAGSEQ = 2, OUT_DBLENGTH = 4, OUT_DBSTARTPOS = 8, OUT_DBABSPOS = 16,
       OUT_DBSEQUENCE = 32, OUT_STRAND = 64, OUT_EDIST = 128 };
static const char *const keywords[] = { "tagnum", "tagseq", "dblength", "dbstartpos", "abspos", "dbsequence",
                                        "strand", "edist", NULL };
/* those of the matching-statistics mode, which belongs to -maxocc */
static const char *const maxocc_keywords[] = { "tagstartpos", "taglength", "tagsuffixseq", NULL };

typedef struct { uint64_t start, len; } tagspan;   /* the raw characters of a tag in `text` */

typedef struct {
  char *text;            /* the tags' characters, one after the other */
  uint64_t textlen;
  tagspan *span;
  uint64_t count;
} taglist;

/* the sequences of FASTA files as they stand, white space dropped */
static int read_tags(const char *const *paths, size_t numfiles, taglist *tl, char *err, size_t errlen)
{
  uint64_t cap_text = 1 << 16, cap_span = 1 << 10;
  tl->text = malloc(cap_text);
  tl->span = malloc(cap_span * sizeof *tl->span);
  tl->textlen = tl->count = 0;
  if (tl->text == NULL || tl->span == NULL) return gtamd_fail(err, errlen, "out of memory (%s)", "tags");
  for (size_t f = 0; f < numfiles; f++) {
    uint8_t *data = NULL;
    uint64_t len = 0, i = 0;
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
      if (tl->count == cap_span) {
        tagspan *grown = realloc(tl->span, (cap_span *= 2) * sizeof *tl->span);
        if (grown == NULL) { free(data); return gtamd_fail(err, errlen, "out of memory (%s)", "tags"); }
        tl->span = grown;
      }
      tl->span[tl->count].start = tl->textlen;
      for (; i < len && data[i] != '>'; i++) {
        if (data[i] == '\n' || data[i] == '\r' || data[i] == ' ' || data[i] == '\t') continue;
        if (tl->textlen == cap_text) {
          char *grown = realloc(tl->text, cap_text *= 2);
          if (grown == NULL) { free(data); return gtamd_fail(err, errlen, "out of memory (%s)", "tags"); }
          tl->text = grown;
        }
        tl->text[tl->textlen++] = (char) data[i];
      }
      tl->span[tl->count].len = tl->textlen - tl->span[tl->count].start;
      tl->count++;
    }
    free(data);
  }
  return 0;
}

/* dotransformtag (tagerator.c:317-361) and the length rule of gt_runtagerator
   (:723-736) for tag t: 0, or -1 with the reference's message; *after_line: the
   error is raised behind the tag's `#` line */
static int transform_tag(const taglist *tl, uint64_t t, const gtamd_alphabet *alpha, long K, int replacewildcard,
                         uint8_t *out, int *after_line, char *err, size_t errlen)
{
  const char *tag = tl->text + tl->span[t].start;
  const uint64_t len = tl->span[t].len;
  *after_line = 0;
  if (len > MAXTAGSIZE) {
    snprintf(err, errlen, "tag \"%.*s\" of length %llu; tags must not be longer than %d", (int) len, tag,
             (unsigned long long) len, MAXTAGSIZE);
    return -1;
  }
  for (uint64_t i = 0; i < len; i++) {
    uint8_t code = alpha->symbolmap[(unsigned char) tag[i]];
    if (code == 253) {
      snprintf(err, errlen, "undefined character '%c' in tag number %llu", tag[i], (unsigned long long) t);
      return -1;
    }
    if (code == 254) {
      if (!replacewildcard) {
        snprintf(err, errlen, "wildcard in tag number %llu", (unsigned long long) t);
        return -1;
      }
      code = 0;
    }
    out[i] = code;
  }
  if ((K > 0 && len <= (uint64_t) K) || len == 0) {
    snprintf(err, errlen, "tag \"%.*s\" of length %llu; tags must be longer than the allowed number of errors "
             "(which is %ld)", (int) len, tag, (unsigned long long) len, K);
    *after_line = 1;
    return -1;
  }
  return 0;
}

static void show_tag_line(const gtamd_alphabet *alpha, unsigned mode, uint64_t t, const uint8_t *coded, uint64_t len)
{
  int first = 1;
  putchar('#');
  if (mode & OUT_TAGNUM) { printf("\t%llu", (unsigned long long) t); first = 0; }
  if (mode & OUT_TAGSEQ) {
    if (!first) putchar('\t');
    for (uint64_t i = 0; i < len; i++) putchar(alpha->characters[coded[i]]);
  }
  putchar('\n');
}

/* tgr_showmatch (tagerator.c:81-189) */
static void show_match(const gtamd_project *prj, unsigned mode, const gtamd_tagmatch_record *rec)
{
  const gtamd_alphabet *alpha = &prj->alpha;
  const uint8_t *enc = prj->enc;
  const uint64_t p = rec->dbstart, len = rec->lendist & 0xffffffffu, dist = rec->lendist >> 32;
  int first = 1;
#define TAB if (first) first = 0; else putchar('\t')
  if (mode & OUT_DBLENGTH) { printf("%llu", (unsigned long long) len); first = 0; }
  if (mode & OUT_DBSTARTPOS) {
    TAB;
    if (mode & OUT_DBABSPOS) printf("%llu", (unsigned long long) p);
    else {
      const uint64_t seq = gtamd_unit_of(prj->seqstart, prj->numseq, p);
      printf("%llu\t%llu", (unsigned long long) seq, (unsigned long long) (p - prj->seqstart[seq]));
    }
  }
  if (mode & OUT_DBSEQUENCE) {
    TAB;
    /* a match of a sound index ends at or in front of n; a damaged .suf may give one that does not */
    for (uint64_t i = 0; i < len && p + i < prj->n; i++) putchar(enc[p + i] < 254 ? alpha->characters[enc[p + i]] : alpha->wildcardshow);
  }
  if (mode & OUT_STRAND) { TAB; putchar(rec->tag & 1 ? '-' : '+'); }
  if (mode & OUT_EDIST) { TAB; printf("%llu", (unsigned long long) dist); }
#undef TAB
  if (!first) putchar('\n');
}

int gtamd_tagerator(int argc, const char **argv, char *err, size_t errlen)
{
  static const char *const not_here[] = { "-pck", "-online", "-cmp", "-maxocc", "-skpp", "-maxdepth", NULL };
  const char *index = NULL, *const *tagfiles = NULL;
  size_t numtagfiles = 0;
  long K = -1;
  int nofwd = 0, norc = 0, best = 0, nowildcards = 1, replacewildcard = 0, verbose = 0, rc = -1;
  int failed = 0, after_line = 0;
  unsigned mode = 0;
  char tagerr[1024] = "";
  uint8_t *symbols = NULL;
  uint64_t *offsets = NULL, stop, next = 0;
  uint32_t flags;
  gtamd_project prj = { 0 };
  taglist tl = { NULL, 0, NULL, 0 };
  gtamd_tagmatch *tm = NULL;
  gtamd_tagmatch_info info;
  gtamd_tagmatch_record *rec = NULL;

  for (int i = 1; i < argc; i++) {
    const char *a = argv[i];
    if (!strcmp(a, "-esa")) { if (gtamd_opt_name(argc, argv, &i, &index, err, errlen) != 0) return -1; }
    else if (!strcmp(a, "-e")) {
      char *end;
      if (i + 1 >= argc) return gtamd_fail(err, errlen, "missing argument to option \"%s\"", a);
      K = strtol(argv[i + 1], &end, 10);
      if (*end != 0 || end == argv[i + 1]) return gtamd_fail(err, errlen, "argument to option \"%s\" must be an integer", a);
      /* the reference takes a negative number as "no -e"; here it is refused by name */
      if (K < 0) return gtamd_fail(err, errlen, "argument to option \"%s\" must be a non-negative integer", a);
      i++;
    } else if (!strcmp(a, "-q")) {
      if (gtamd_opt_files(argc, argv, &i, &tagfiles, &numtagfiles, err, errlen) != 0) return -1;
    } else if (!strcmp(a, "-output")) {
      int given = 0;
      for (; i + 1 < argc && argv[i + 1][0] != '-'; i++, given++) {
        int k;
        for (k = 0; keywords[k] != NULL && strcmp(argv[i + 1], keywords[k]); k++) ;
        if (keywords[k] == NULL) {
          for (k = 0; maxocc_keywords[k] != NULL; k++)
            if (!strcmp(argv[i + 1], maxocc_keywords[k]))
              return gtamd_fail(err, errlen, "argument \"%s\" to option -output belongs to option -maxocc, which is not "
                          "supported by the MI355X engine", argv[i + 1]);
          return gtamd_fail(err, errlen, "illegal argument \"%s\" to option -output", argv[i + 1]);
        }
        if (mode & (1u << k)) return gtamd_fail(err, errlen, "argument \"%s\" to option -output already specified", argv[i + 1]);
        mode |= 1u << k;
      }
      if (!given) return gtamd_fail(err, errlen, "missing argument to option \"%s\"", a);
    } else if (!strcmp(a, "-nod")) nofwd = gtamd_opt_switch(argc, argv, &i);
    else if (!strcmp(a, "-nop")) norc = gtamd_opt_switch(argc, argv, &i);
    else if (!strcmp(a, "-best")) best = gtamd_opt_switch(argc, argv, &i);
    /* the reference stores this switch as "no wildcards" (gt_tagerator.c:170-174):
       only `-withwildcards no` lets wildcards of the subject pass */
    else if (!strcmp(a, "-withwildcards")) nowildcards = gtamd_opt_switch(argc, argv, &i);
    else if (!strcmp(a, "-rw")) replacewildcard = gtamd_opt_switch(argc, argv, &i);
    else if (!strcmp(a, "-v")) verbose = gtamd_opt_switch(argc, argv, &i);
    else if (!strcmp(a, "-help")) {
      puts("Usage: gt-suffixerator-amd tagerator [options] -q tagfile -esa indexname\n"
           "Map short sequence tags in given index, on the device.\n\n"
           "-q             files containing the short sequence tags (FASTA, at most 64 letters a tag)\n"
           "-e             the allowed number of differences (replacements/insertions/deletions)\n"
           "-esa           the index: INDEX.prj, .esq, .ssp and .suf, as written by `suffixerator -tis -suf -ssp`\n"
           "-nod           do not compute direct matches\n"
           "-nop           do not compute palindromic (reverse complemented) matches; needed for a protein index\n"
           "-best          only the matches of the smallest number of differences that gives a tag a match\n"
           "-withwildcards the reference's switch: `-withwildcards no` lets wildcards of the index be part of a\n"
           "               match (as symbols that equal nothing); only with -e 1 or more\n"
           "-rw            replace a wildcard in a tag by the first letter\n"
           "-output        tagnum tagseq dblength dbstartpos abspos dbsequence strand edist\n"
           "-v             figures of the search as lines that start with '#', behind the matches\n\n"
           "The output is that of `gt tagerator`; the match lines of one tag and strand come in the order of the\n"
           "suffix table.  -pck, -online, -cmp, -maxocc (and the matching statistics without -e), -skpp and\n"
           "-maxdepth are refused.");
      return 0;
    } else return gtamd_opt_tail(a, not_here, GTAMD_UNKNOWN_TRY, GTAMD_SUPERFLUOUS_MORE, err, errlen);
  }
  if (tagfiles == NULL) return gtamd_fail(err, errlen, "option \"-%s\" is mandatory", "q");
  if (index == NULL) return gtamd_fail(err, errlen, "either option \"-esa\" or option \"-%s\" is mandatory", "pck");
  if (K < 0 && best) return gtamd_fail(err, errlen, "option -best requires option %s", "-e");
  if (K < 0)
    return gtamd_fail(err, errlen, "option \"-e\" is needed: if option -e is not used then option -maxocc is required, and "
                "the matching statistics of %s are not supported by the MI355X engine", "-maxocc");
  if (K >= MAXTAGSIZE) return gtamd_fail(err, errlen, "argument to option \"%s\" must be smaller than 64, the longest tag", "-e");
  if (nofwd && norc) return gtamd_fail(err, errlen, "options -nod and -nop together leave %s to compute", "nothing");
  if (K == 0) nowildcards = 1;                          /* gt_tagerator_arguments_check */
  if (mode == 0) mode = OUT_TAGNUM | OUT_TAGSEQ | OUT_DBLENGTH | OUT_DBSTARTPOS | OUT_STRAND;

  /* gt_tagerator_runner: these lines come before the index is read */
  if (K == 0) printf("# computing complete matches without differences (exact matches)\n");
  else printf("# computing complete matches with up to %ld differences\n", K);
  printf("# indexname(esa)=%s\n", index);
  for (size_t f = 0; f < numtagfiles; f++) printf("# queryfile=%s\n", tagfiles[f]);

  if (gtamd_project_open(&prj, index, "searched", GTAMD_PROJECT_FORWARD, "tagerator", err, errlen) != 0) goto done;
  if (!norc && !gtamd_alphabet_is_dna(&prj.alpha)) {
    gtamd_fail(err, errlen, "reverse complemented matches need a DNA alphabet: the index has none, and its letters have no "
         "complement; use option \"%s\"", "-nop");
    goto done;
  }
  if (gtamd_project_map(&prj, index, GTAMD_TABLE_SUF, 1, err, errlen) != 0) goto done;
  printf("# for each match show: ");
  for (int k = 0; keywords[k] != NULL; k++)
    if (mode & (1u << k)) printf("%s ", keywords[k]);
  putchar('\n');

  /* the tags up to the first one the reference ends at: their blocks are printed,
     then its message */
  if (read_tags(tagfiles, numtagfiles, &tl, err, errlen) != 0) goto done;
  symbols = malloc(tl.textlen ? tl.textlen : 1);
  offsets = malloc((tl.count + 1) * sizeof *offsets);
  rec = malloc(TAGERATOR_CAPACITY * sizeof *rec);
  if (symbols == NULL || offsets == NULL || gtamd_project_sequence_starts(&prj) != 0 || rec == NULL) {
    gtamd_fail(err, errlen, "out of memory (%s)", "tags and records");
    goto done;
  }
  offsets[0] = 0;
  for (stop = 0; stop < tl.count; stop++) {
    if (transform_tag(&tl, stop, &prj.alpha, K, replacewildcard, symbols + offsets[stop], &after_line, tagerr,
                      sizeof tagerr) != 0) {
      failed = 1;
      break;
    }
    offsets[stop + 1] = offsets[stop] + tl.span[stop].len;
  }

  if (stop > 0) {
    flags = (nofwd ? 0 : GTAMD_TAGMATCH_FORWARD) | (norc ? 0 : GTAMD_TAGMATCH_REVCOMP) |
            (best ? GTAMD_TAGMATCH_BEST : 0) | (nowildcards ? 0 : GTAMD_TAGMATCH_WITH_WILDCARDS);
    if ((tm = gtamd_tagmatch_create(0)) == NULL ||
        gtamd_tagmatch_set_index_host(tm, prj.enc, prj.n, prj.suf.p, prj.suf_bytes, prj.alpha.numofchars) != 0 ||
        gtamd_tagmatch_prepare(tm, symbols, offsets, stop, 0, (uint32_t) K, flags, &info) != 0) {
      snprintf(err, errlen, "%s", gtamd_esa_last_error());
      goto done;
    }
    for (uint64_t cursor = 0, written = 1; written != 0; ) {
      if (gtamd_tagmatch_emit(tm, &cursor, rec, TAGERATOR_CAPACITY, 0, &written) != 0) {
        snprintf(err, errlen, "%s", gtamd_esa_last_error());
        goto done;
      }
      for (uint64_t k = 0; k < written; k++) {
        const uint64_t t = rec[k].tag >> 1;
        for (; next <= t; next++)          /* the lines of the tags up to this one */
          show_tag_line(&prj.alpha, mode, next, symbols + offsets[next], tl.span[next].len);
        show_match(&prj, mode, &rec[k]);
      }
    }
    for (; next < stop; next++) show_tag_line(&prj.alpha, mode, next, symbols + offsets[next], tl.span[next].len);
    if (verbose && gtamd_tagmatch_get_info(tm, &info) == 0)
      printf("# %llu jobs, %llu matches, at most %llu of one tag and strand, %llu children examined, %llu levels, "
             "%llu single-suffix walks, %.3f ms on the device\n", (unsigned long long) info.jobs,
             (unsigned long long) info.matches, (unsigned long long) info.max_matches_of_one_job,
             (unsigned long long) info.children_examined, (unsigned long long) info.levels_pushed,
             (unsigned long long) info.single_walks, info.device_ms);
  }
  if (failed) {
    /* (the characters of the tag as read: its code is not complete) */
    if (after_line) show_tag_line(&prj.alpha, mode, stop, symbols + offsets[stop], tl.span[stop].len);
    fflush(stdout);
    snprintf(err, errlen, "%s", tagerr);
    goto done;
  }
  if (fflush(stdout) != 0) { gtamd_fail(err, errlen, "cannot write to %s", "stdout"); goto done; }
  rc = 0;
done:
  fflush(stdout);
  gtamd_tagmatch_destroy(tm);
  gtamd_project_close(&prj);
  free(rec); free(offsets); free(symbols); free(tl.span); free(tl.text);
  return rc;
}
