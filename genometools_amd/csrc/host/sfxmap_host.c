/* sfxmap_host.c -- `gt dev sfxmap [-suf] [-lcp] [-bwt] [-v] -esa INDEX` for this
   path (tool function src/tools/gt_sfxmap.c; what it runs for these options:
   gt_suftab_lightweightcheck src/match/sfx-lwcheck.c:181-337,
   gt_lcptab_lightweightcheck src/match/sfx-linlcp.c:548): the tables of an
   existing index, written here or by GenomeTools, checked entry for entry on
   the device through include/gtamd_check.h. */
#include "host_internal.h"
#include "gtamd_check.h"
#include <stdio.h>
#include <string.h>

/* the reference's other modes (gt_sfxmap.c: the option list of the tool) */
static const char *const refused[] = {
  "-pck", "-stream-esq", "-sortmaxdepth", "-algbds", "-stream", "-bfcheck", "-delspranges", "-des",
  "-sds", "-bck", "-cmpsuf", "-cmplcp", "-diffcover", "-wholeleafcheck", "-enumlcpitvs",
  "-enumlcpitvtree", "-enumlcpitvtreeBU", "-scanesa", "-spmitv", "-ownencseq2file",
  "-compressedesa", "-compresslcp", NULL
};

int gtamd_sfxmap(int argc, const char **argv, char *err, size_t errlen)
{
  int want_suf = 0, want_lcp = 0, want_bwt = 0, verbose = 0, rc = -1;
  const char *index = NULL;
  char path[4096], msg[512];
  unsigned long long longest = 0, large = 0, depth = 0;
  uint64_t N;
  gtamd_project prj = { 0 };
  gtamd_check *chk = NULL;
  gtamd_check_report rep;

  for (int i = 1; i < argc; i++) {
    const char *a = argv[i];
    if (!strcmp(a, "-suf")) want_suf = 1;
    else if (!strcmp(a, "-lcp")) want_lcp = 1;
    else if (!strcmp(a, "-bwt")) want_bwt = 1;
    else if (!strcmp(a, "-v")) verbose = 1;
    else if (!strcmp(a, "-tis") || !strcmp(a, "-ssp")) continue;   /* (always read) */
    else if (!strcmp(a, "-esa")) { if (gtamd_opt_name(argc, argv, &i, &index, err, errlen) != 0) return -1; }
    else return gtamd_opt_tail(a, refused, GTAMD_UNKNOWN_TRY, GTAMD_SUPERFLUOUS_ONE, err, errlen);
  }
  if (index == NULL) return gtamd_fail(err, errlen, "option \"-%s\" is mandatory", "esa");
  if (!want_suf && (want_lcp || want_bwt))
    return gtamd_fail(err, errlen, "option \"-%s\" requires option \"-suf\": the table is checked through "
                      "the suffix array", want_lcp ? "lcp" : "bwt");

  if (gtamd_project_open(&prj, index, "checked", GTAMD_PROJECT_ANY, NULL, err, errlen) != 0) goto done;
  snprintf(path, sizeof path, "%s.prj", index);
  (void) gtamd_prj_value(path, "longest", &longest);
  (void) gtamd_prj_value(path, "largelcpvalues", &large);
  (void) gtamd_prj_value(path, "maxbranchdepth", &depth);
  N = prj.n + 1;

  if (want_suf && gtamd_project_map(&prj, index, GTAMD_TABLE_SUF, 0, err, errlen) != 0) goto done;
  if (want_lcp && (gtamd_project_map(&prj, index, GTAMD_TABLE_LCP, 0, err, errlen) != 0 ||
                   gtamd_project_map(&prj, index, GTAMD_TABLE_LLV, 0, err, errlen) != 0))
    goto done;
  if (want_bwt && gtamd_project_map(&prj, index, GTAMD_TABLE_BWT, 0, err, errlen) != 0) goto done;
  if (!want_suf) { rc = 0; goto done; }     /* the sequence and the project file agree */

  if ((chk = gtamd_check_create(0)) == NULL ||
      gtamd_check_tables_host(chk, prj.enc, prj.n, prj.suf.p, prj.suf_bytes, prj.lcp.p, prj.llv.p,
                              prj.llv.bytes / 16, prj.bwt.p, &rep) != 0) {
    snprintf(err, errlen, "%s", gtamd_esa_last_error());
    goto done;
  }
  if (verbose) {
    static const char *const phase[GTAMD_CHECK_PHASES] = {
      "suf: range and permutation", "suf: order", "bwt", "lcp/llv: structure", "lcp/llv: values" };
    for (int k = 0; k < GTAMD_CHECK_PHASES; k++)
      if (rep.phase_ms[k] > 0) printf("# %-27s %10.3f ms\n", phase[k], rep.phase_ms[k]);
    printf("# %-27s %10.3f ms on the device, %llu entries, %llu long ranges\n", "total", rep.check_ms,
           (unsigned long long) N, (unsigned long long) rep.long_claims);
  }
  if (!rep.ok) {
    gtamd_check_message(&rep, msg, sizeof msg);
    snprintf(err, errlen, "index '%s': %s", index, msg);
    goto done;
  }
  if (rep.longest != longest)
    snprintf(err, errlen, "file '%s' says longest=%llu, suffix 0 stands at table index %llu", path,
             longest, (unsigned long long) rep.longest);
  else if (want_lcp && rep.largelcpvalues != large)
    snprintf(err, errlen, "file '%s' says largelcpvalues=%llu, the .lcp table holds %llu", path, large,
             (unsigned long long) rep.largelcpvalues);
  else if (want_lcp && rep.maxbranchdepth != depth)
    snprintf(err, errlen, "file '%s' says maxbranchdepth=%llu, the largest value of the tables is %llu",
             path, depth, (unsigned long long) rep.maxbranchdepth);
  else rc = 0;
done:
  gtamd_check_destroy(chk);
  gtamd_project_close(&prj);
  return rc;
}
