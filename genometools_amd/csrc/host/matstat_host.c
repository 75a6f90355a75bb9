/* matstat_host.c -- `gt matstat` and `gt uniquesub` with -esa INDEX for this path
   (tool src/tools/gt_matstat.c): matching statistics and minimum unique
   prefixes of queries against an index, on the device through
   include/gtamd_mstat.h.  Option handling and messages of
   src/tools/gt_matstat.c:96-278, output of src/match/greedyfwdmat.c:168-211. */
#include "host_internal.h"
#include "gtamd_mstat.h"
#include <limits.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

enum { SHOW_SEQUENCE = 1, SHOW_QUERYPOS = 2, SHOW_SUBJECTPOS = 4 };

/* doms: matching statistics, else minimum unique prefixes */
static int greedy_forward_tool(int doms, int argc, const char **argv, char *err, size_t errlen)
{
  static const char *const refused[] = { "-fmi", "-pck", NULL };
  const char *index = NULL, *const *queries = NULL;
  size_t numqueries = 0;
  int have_min = 0, have_max = 0, have_output = 0, numflags = 0, rc = -1;
  unsigned show = 0;
  unsigned long long minlen = 0, maxlen = 0;
  uint8_t *query = NULL;
  uint64_t m = 0, desclen = 0;
  char *desc = NULL;
  uint32_t *length = NULL;
  uint64_t *subjectpos = NULL;
  gtamd_project prj = { 0 };
  gtamd_mstat *ms = NULL;

  for (int i = 1; i < argc; i++) {
    const char *a = argv[i];
    if (!strcmp(a, "-esa")) { if (gtamd_opt_name(argc, argv, &i, &index, err, errlen) != 0) return -1; }
    else if (!strcmp(a, "-query")) {
      if (gtamd_opt_files(argc, argv, &i, &queries, &numqueries, err, errlen) != 0) return -1;
    } else if (!strcmp(a, "-min")) {
      if (gtamd_opt_length(argc, argv, &i, ULLONG_MAX, &minlen, err, errlen) != 0) return -1;
      have_min = 1;
    } else if (!strcmp(a, "-max")) {
      if (gtamd_opt_length(argc, argv, &i, ULLONG_MAX, &maxlen, err, errlen) != 0) return -1;
      have_max = 1;
    } else if (!strcmp(a, "-output")) {
      have_output = 1;
      for (; i + 1 < argc && argv[i + 1][0] != '-'; i++, numflags++) {
        const char *f = argv[i + 1];
        if (!strcmp(f, "sequence")) show |= SHOW_SEQUENCE;
        else if (!strcmp(f, "querypos")) show |= SHOW_QUERYPOS;
        else if (doms && !strcmp(f, "subjectpos")) show |= SHOW_SUBJECTPOS;
        else return gtamd_fail(err, errlen, "illegal argument \"%s\" to option -output", f);
      }
    } else if (doms && !strcmp(a, "-verify")) (void) gtamd_opt_yesno(argc, argv, &i);   /* (no effect with -esa) */
    else return gtamd_opt_tail(a, refused, GTAMD_UNKNOWN_TRY, GTAMD_SUPERFLUOUS_ONE, err, errlen);
  }
  if (queries == NULL) return gtamd_fail(err, errlen, "option \"-%s\" is mandatory", "query");
  if (index == NULL) return gtamd_fail(err, errlen, "one of the options -esa, -pck must be %s", "used");
  if (!have_min && !have_max) return gtamd_fail(err, errlen, "one of the options -min or -max must be %s", "set");
  if (have_min && have_max && maxlen < minlen)
    return gtamd_fail(err, errlen, "minvalue must be smaller or equal than %s", "maxvalue");
  if (have_output && numflags == 0) return gtamd_fail(err, errlen, "missing arguments to option %s", "-output");

  if (gtamd_project_open(&prj, index, "searched", GTAMD_PROJECT_ANY, NULL, err, errlen) != 0) goto done;
  if (gtamd_project_map(&prj, index, GTAMD_TABLE_SUF, 0, err, errlen) != 0) goto done;
  /* the queries, with the index's alphabet: one sequence of symbols, a separator
     between two units */
  if (gtamd_encode_files_alpha(queries, numqueries, &prj.alpha, &query, &m, &desc, &desclen, NULL, err,
                               errlen) != 0)
    goto done;
  if (m > 0xffffffffull) {
    snprintf(err, errlen, "queries of %llu symbols, at most %llu in one call", (unsigned long long) m,
             0xffffffffull);
    goto done;
  }
  length = malloc((m ? m : 1) * sizeof *length);
  if (show & SHOW_SUBJECTPOS) subjectpos = malloc((m ? m : 1) * sizeof *subjectpos);
  if (length == NULL || ((show & SHOW_SUBJECTPOS) && subjectpos == NULL)) {
    gtamd_fail(err, errlen, "out of memory (%s)", "results");
    goto done;
  }
  {
    /* longer matches are not printed: the device stops looking there */
    const uint32_t cap = have_max && maxlen < 0xfffffffeull ? (uint32_t) maxlen : 0;
    if ((ms = gtamd_mstat_create(0)) == NULL ||
        gtamd_mstat_set_index_host(ms, prj.enc, prj.n, prj.suf.p, prj.suf_bytes, prj.alpha.numofchars) != 0 ||
        (doms ? gtamd_mstat_matstat(ms, query, m, 0, cap, length, subjectpos, 0)
              : gtamd_mstat_uniquesub(ms, query, m, 0, cap, length, 0)) != 0) {
      snprintf(err, errlen, "%s", gtamd_esa_last_error());
      goto done;
    }
  }
  {
    const char *d = desc;
    unsigned long long unit = 0;
    uint64_t end;
    for (uint64_t start = 0; start < m; start = end + 1, unit++) {
      for (end = start; end < m && query[end] != 255; end++) ;
      printf("unit %llu", unit);
      if (d != NULL && d < desc + desclen) {
        if (d[0] != 0) printf(" (%s)", d);
        d += strlen(d) + 1;
      }
      putchar('\n');
      for (uint64_t k = start; k < end; k++) {
        const uint32_t v = length[k];
        if (v == 0 || (have_min && v < minlen) || (have_max && v > maxlen)) continue;
        if (show & SHOW_QUERYPOS) printf("%llu ", (unsigned long long) (k - start));
        printf("%lu", (unsigned long) v);
        if (show & SHOW_SUBJECTPOS) printf(" %llu", (unsigned long long) subjectpos[k]);
        if (show & SHOW_SEQUENCE) {
          putchar(' ');
          for (uint32_t j = 0; j < v; j++) putchar(prj.alpha.characters[query[k + j]]);
        }
        putchar('\n');
      }
    }
  }
  if (fflush(stdout) != 0) { gtamd_fail(err, errlen, "cannot write to %s", "stdout"); goto done; }
  rc = 0;
done:
  gtamd_mstat_destroy(ms);
  gtamd_project_close(&prj);
  free(length); free(subjectpos); free(desc); free(query);
  return rc;
}

int gtamd_matstat(int argc, const char **argv, char *err, size_t errlen)
{
  return greedy_forward_tool(1, argc, argv, err, errlen);
}

int gtamd_uniquesub(int argc, const char **argv, char *err, size_t errlen)
{
  return greedy_forward_tool(0, argc, argv, err, errlen);
}
