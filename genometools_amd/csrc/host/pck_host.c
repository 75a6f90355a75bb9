/* pck_host.c -- `gt packedindex trsuftab [options] INDEX` for this path
   (tool function src/tools/gt_packedindex_trsuftab.c:44-79): INDEX.bdx from
   the project's INDEX.prj / .esq / .suf / .bwt, built on the device through
   include/gtamd_pck.h.  Options and defaults: src/match/eis-bwtseq-param.c:25-67,
   src/match/eis-blockcomp-param.c:21-36.

   And the other tool that reads a project back, with the same helpers:
   `gt dev sfxmap [-suf] [-lcp] [-bwt] [-v] -esa INDEX` (tool function
   src/tools/gt_sfxmap.c; what it runs for these options:
   gt_suftab_lightweightcheck src/match/sfx-lwcheck.c:181-337,
   gt_lcptab_lightweightcheck src/match/sfx-linlcp.c:548): the tables of an
   existing index, written here or by GenomeTools, checked entry for entry on
   the device through include/gtamd_check.h.

   And the first tools that ask an index a question: `gt matstat` and `gt
   uniquesub` with -esa INDEX (tool src/tools/gt_matstat.c), on the device
   through include/gtamd_mstat.h.

   And the tool that reads .suf and .lcp together: `gt repfind -l L -ii INDEX`
   (tool src/tools/gt_repfind.c), the maximal exact repeats, on the device
   through include/gtamd_maxpairs.h.

   And the one that needs no table on disk: `gt encseq2spm -l L -ii INDEX -spm
   show|count` (tool src/tools/gt_encseq2spm.c), all suffix-prefix matches of a
   read set on both strands; the engine builds .suf and .lcp of the mirrored
   reads in this process and hands them to include/gtamd_spm.h.  Its consumer,
   `gt readjoiner overlap`, the irreducible ones of them, is in rdj_host.c. */
#include "host_internal.h"
#include "gtamd_pck.h"
#include "gtamd_check.h"
#include "gtamd_mstat.h"
#include "gtamd_maxpairs.h"
#include "gtamd_qmatch.h"
#include "gtamd_spm.h"
#include <errno.h>
#include <fcntl.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

static int pfail(char *err, size_t errlen, const char *msg, const char *arg)
{
  snprintf(err, errlen, msg, arg);
  return -1;
}

/* one "key=value" line of INDEX.prj (src/match/esa-scanprj.c) */
static int prj_value(const char *path, const char *key, unsigned long long *value)
{
  char line[512];
  const size_t klen = strlen(key);
  FILE *fp = fopen(path, "r");
  int found = 0;
  if (fp == NULL) return -1;
  while (fgets(line, sizeof line, fp) != NULL)
    if (!strncmp(line, key, klen) && line[klen] == '=') {
      *value = strtoull(line + klen + 1, NULL, 10);
      found = 1;
    }
  fclose(fp);
  return found ? 0 : -1;
}

static void *read_whole(const char *path, uint64_t expect_bytes)
{
  FILE *fp = fopen(path, "rb");
  void *buf;
  if (fp == NULL) return NULL;
  buf = malloc(expect_bytes ? expect_bytes : 1);
  if (buf != NULL && (fread(buf, 1, expect_bytes, fp) != expect_bytes || fgetc(fp) != EOF)) {
    free(buf);
    buf = NULL;
  }
  fclose(fp);
  return buf;
}

/* INDEX.<ilog>cxm from the builder's context map image */
static int write_ctxmap(gtamd_pck *pck, const char *index, int ilog_used, char *err, size_t errlen)
{
  char path[4096];
  const uint64_t n = gtamd_pck_ctxmap_bytes(pck);
  uint8_t *buf = malloc(n ? n : 1);
  FILE *fp;
  int rc = -1;
  snprintf(path, sizeof path, "%s.%dcxm", index, ilog_used);
  if (buf == NULL) return pfail(err, errlen, "out of memory (%s)", "context map");
  if (gtamd_pck_ctxmap_copy(pck, buf, 0, n) != 0) snprintf(err, errlen, "%s", gtamd_esa_last_error());
  else if ((fp = fopen(path, "wb")) == NULL) pfail(err, errlen, "cannot open file '%s' for writing", path);
  else {
    rc = fwrite(buf, 1, n, fp) == n ? 0 : pfail(err, errlen, "cannot write file '%s'", path);
    if (fclose(fp) != 0 && rc == 0) rc = pfail(err, errlen, "cannot close file '%s'", path);
  }
  free(buf);
  return rc;
}

static int uint_option(int argc, const char **argv, int *i, uint32_t *out, char *err, size_t errlen)
{
  char *end;
  unsigned long v;
  if (*i + 1 >= argc) return pfail(err, errlen, "missing argument to option \"%s\"", argv[*i]);
  v = strtoul(argv[*i + 1], &end, 10);
  if (*end != 0 || argv[*i + 1][0] == '-')
    return pfail(err, errlen, "argument to option \"%s\" must be a non-negative integer", argv[*i]);
  *out = (uint32_t) v;
  (*i)++;
  return 0;
}

int gtamd_packedindex_trsuftab(int argc, const char **argv, char *err, size_t errlen)
{
  gtamd_pck_params pp = { 8, 8, 16, 0, 0 };
  int locbitmap = -1, verbose = 0, rc = -1, sprank = 0, ctxilog = -2;
  const char *index = NULL;
  char path[4096];
  unsigned long long totallength, longest, integersize = 64;
  uint8_t *enc = NULL, *bwt = NULL;
  uint64_t *suf = NULL, n = 0;
  gtamd_seqstats ss;
  gtamd_pck *pck = NULL;
  gtamd_pck_info info;
  FILE *fp = NULL;

  for (int i = 1; i < argc; i++) {
    const char *a = argv[i];
    if (!strcmp(a, "-bsize")) { if (uint_option(argc, argv, &i, &pp.block_size, err, errlen)) return -1; }
    else if (!strcmp(a, "-blbuck")) { if (uint_option(argc, argv, &i, &pp.bucket_blocks, err, errlen)) return -1; }
    else if (!strcmp(a, "-locfreq")) { if (uint_option(argc, argv, &i, &pp.locate_interval, err, errlen)) return -1; }
    else if (!strcmp(a, "-locbitmap")) {
      locbitmap = 1;
      if (i + 1 < argc && (!strcmp(argv[i + 1], "yes") || !strcmp(argv[i + 1], "no")))
        locbitmap = !strcmp(argv[++i], "yes");
    } else if (!strcmp(a, "-v")) verbose = 1;
    else if (!strcmp(a, "-sprank")) {
      sprank = 1;
      if (i + 1 < argc && (!strcmp(argv[i + 1], "yes") || !strcmp(argv[i + 1], "no")))
        sprank = !strcmp(argv[++i], "yes");
    } else if (!strcmp(a, "-sprankilog")) {
      /* the sampling interval of the reference's in-memory rank table: no effect on
         the file, but a value >= 0 switches the rank sort on (eis-bwtseq-param.c:98-100) */
      if (i + 1 >= argc) return pfail(err, errlen, "missing argument to option \"%s\"", a);
      if (atoi(argv[++i]) >= 0) sprank = 1;
    } else if (!strcmp(a, "-ctxilog")) {
      /* gt_registerCtxMapOptions, src/match/eis-bwtseq-context-param.c:20-32: -1 the
         automatic interval, -2 no map */
      if (i + 1 >= argc) return pfail(err, errlen, "missing argument to option \"%s\"", a);
      ctxilog = atoi(argv[++i]);
      if (ctxilog < -2 || ctxilog > 63) return pfail(err, errlen, "argument to option \"%s\" must be an integer between -2 and 63", a);
    }
    else if (a[0] == '-') return pfail(err, errlen, "unknown option: %s (try -help)", a);
    else if (index != NULL) return pfail(err, errlen, "superfluous argument \"%s\"", a);
    else index = a;
  }
  if (index == NULL) return pfail(err, errlen, "missing argument%s", "");
  /* the option parser's minima (gt_option_new_uint_min, eis-blockcomp-param.c) */
  if (pp.block_size < 1) return pfail(err, errlen, "argument to option \"-%s\" must be an integer >= 1", "bsize");
  if (pp.bucket_blocks < 1) return pfail(err, errlen, "argument to option \"-%s\" must be an integer >= 1", "blbuck");
  pp.feature_toggles = gtamd_pck_default_toggles(pp.block_size, pp.bucket_blocks, pp.locate_interval, locbitmap)
                       | (sprank ? GTAMD_PCK_REVERSIBLY_SORTED : 0);

  snprintf(path, sizeof path, "%s.prj", index);
  if (prj_value(path, "totallength", &totallength) != 0 || prj_value(path, "longest", &longest) != 0)
    return pfail(err, errlen, "cannot read totallength / longest from file '%s'", path);
  (void) prj_value(path, "integersize", &integersize);
  if (integersize != 64)
    return pfail(err, errlen, "file '%s' describes tables of another integer size", path);
  /* the alphabet comes with the encoded sequence (the reference maps INDEX.esq):
     DNA, protein or a symbol map, only its size matters here */
  {
    gtamd_alphabet alpha;
    if (gtamd_read_esq_alpha(index, &enc, &n, &alpha, &ss, err, errlen) != 0) return -1;
    gtamd_alphabet_free(&alpha);
  }
  free(enc);
  if (n != totallength) return pfail(err, errlen, "INDEX.esq and INDEX.prj of '%s' disagree on the total length", index);
  snprintf(path, sizeof path, "%s.bwt", index);
  if ((bwt = read_whole(path, totallength + 1)) == NULL) {
    /* the reference would derive the BWT from .suf and .esq; this tool asks for the table */
    pfail(err, errlen, "cannot read the %s table of the project (run suffixerator with -bwt)", path);
    goto done;
  }
  if (pp.locate_interval) {   /* (-sprank without locate information stores nothing either) */
    snprintf(path, sizeof path, "%s.suf", index);
    if ((suf = read_whole(path, 8 * (totallength + 1))) == NULL) {
      pfail(err, errlen, "suffix array project %s does not hold required suffix array (.suf) "
            "and encoded sequence (.esq) information!", index);
      goto done;
    }
  }
  if ((pck = gtamd_pck_create(0)) == NULL ||
      gtamd_pck_build_host(pck, bwt, suf, totallength + 1, ss.numofchars, longest, &pp) != 0 ||
      gtamd_pck_get_info(pck, &info) != 0) {
    snprintf(err, errlen, "%s", gtamd_esa_last_error());
    goto done;
  }
  /* the context map is made beside the locate marks (addLocateInfo,
     src/match/eis-bwtseq-extinfo.c:473-476): none without locate information */
  if (ctxilog >= -1 && pp.locate_interval) {
    int used = 0;
    if (gtamd_pck_ctxmap_build_host(pck, suf, totallength + 1, ctxilog, &used) != 0) {
      snprintf(err, errlen, "%s", gtamd_esa_last_error());
      goto done;
    }
    if (write_ctxmap(pck, index, used, err, errlen) != 0) goto done;
  }
  snprintf(path, sizeof path, "%s.bdx", index);
  if ((fp = fopen(path, "wb")) == NULL) { pfail(err, errlen, "cannot open file '%s' for writing", path); goto done; }
  {
    const uint64_t chunk = 64u << 20;
    uint8_t *buf = malloc(chunk);
    if (buf == NULL) { pfail(err, errlen, "out of memory (%s)", "packedindex"); goto done; }
    for (uint64_t off = 0; off < info.file_bytes; off += chunk) {
      const uint64_t cnt = info.file_bytes - off < chunk ? info.file_bytes - off : chunk;
      if (gtamd_pck_image_copy(pck, buf, off, cnt) != 0) { snprintf(err, errlen, "%s", gtamd_esa_last_error()); free(buf); goto done; }
      if (fwrite(buf, 1, cnt, fp) != cnt) { pfail(err, errlen, "cannot write file '%s'", path); free(buf); goto done; }
    }
    free(buf);
  }
  if (verbose)
    printf("# %llu buckets of %u bits + %llu variable bits, %llu regions, %llu bytes; %.2f ms on the device\n",
           (unsigned long long) info.num_buckets, info.cw_bits, (unsigned long long) info.var_bits,
           (unsigned long long) info.num_regions, (unsigned long long) info.file_bytes, info.build_ms);
  rc = 0;
done:
  if (fp != NULL && fclose(fp) != 0 && rc == 0) rc = pfail(err, errlen, "cannot close file '%s'", path);
  gtamd_pck_destroy(pck);
  free(bwt); free(suf);
  return rc;
}

/* `gt packedindex mkctxmap [-ctxilog I] [-v] INDEX` (src/tools/gt_packedindex_mkctxmap.c:40-139):
   the context map of an existing project from its INDEX.suf */
int gtamd_packedindex_mkctxmap(int argc, const char **argv, char *err, size_t errlen)
{
  int ctxilog = -1, rc = -1, used = 0;
  const char *index = NULL;
  char path[4096];
  unsigned long long totallength;
  uint64_t *suf = NULL;
  gtamd_pck *pck = NULL;
  for (int i = 1; i < argc; i++) {
    const char *a = argv[i];
    if (!strcmp(a, "-ctxilog")) {
      if (i + 1 >= argc) return pfail(err, errlen, "missing argument to option \"%s\"", a);
      ctxilog = atoi(argv[++i]);
    } else if (!strcmp(a, "-v")) continue;
    else if (a[0] == '-') return pfail(err, errlen, "unknown option: %s (try -help)", a);
    else if (index != NULL) return pfail(err, errlen, "superfluous argument \"%s\"", a);
    else index = a;
  }
  if (index == NULL) return pfail(err, errlen, "missing argument%s", "");
  if (ctxilog < -1) return pfail(err, errlen, "argument to option \"%s\" must be an integer >= -1", "-ctxilog");
  snprintf(path, sizeof path, "%s.prj", index);
  if (prj_value(path, "totallength", &totallength) != 0)
    return pfail(err, errlen, "cannot read totallength from file '%s'", path);
  snprintf(path, sizeof path, "%s.suf", index);
  if ((suf = read_whole(path, 8 * (totallength + 1))) == NULL)
    return pfail(err, errlen, "The project %s does not contain sufficient information to regenerate the suffix array.", index);
  if ((pck = gtamd_pck_create(0)) == NULL ||
      gtamd_pck_ctxmap_build_host(pck, suf, totallength + 1, ctxilog, &used) != 0)
    snprintf(err, errlen, "%s", gtamd_esa_last_error());
  else
    rc = write_ctxmap(pck, index, used, err, errlen);
  gtamd_pck_destroy(pck);
  free(suf);
  return rc;
}

/* ---- gt dev sfxmap ----
   The table files are mapped, not read: the upload takes them piece by piece,
   as the writer streamed them. */
/* the single-build limit of the engine: tables of more entries come in slices */
#define SFXMAP_MAX_ENTRIES ((1ull << 32) - 4096)

/* the reference's other modes (gt_sfxmap.c: the option list of the tool) */
static const char *const refused[] = {
  "-pck", "-stream-esq", "-sortmaxdepth", "-algbds", "-stream", "-bfcheck", "-delspranges", "-des",
  "-sds", "-bck", "-cmpsuf", "-cmplcp", "-diffcover", "-wholeleafcheck", "-enumlcpitvs",
  "-enumlcpitvtree", "-enumlcpitvtreeBU", "-scanesa", "-spmitv", "-ownencseq2file",
  "-compressedesa", "-compresslcp", NULL
};

typedef struct { void *p; uint64_t bytes; } mapped;

/* 0, -1 cannot open, -2 cannot map */
static int map_file(const char *path, mapped *m)
{
  struct stat sb;
  const int fd = open(path, O_RDONLY);
  m->p = NULL;
  m->bytes = 0;
  if (fd < 0) return -1;
  if (fstat(fd, &sb) != 0) { close(fd); return -2; }
  m->bytes = (uint64_t) sb.st_size;
  if (m->bytes) {
    m->p = mmap(NULL, m->bytes, PROT_READ, MAP_PRIVATE, fd, 0);
    if (m->p == MAP_FAILED) { m->p = NULL; close(fd); return -2; }
  }
  close(fd);
  return 0;
}

static void unmap_file(mapped *m)
{
  if (m->p != NULL) munmap(m->p, m->bytes);
  m->p = NULL;
}

static int map_table(const char *index, const char *suffix, mapped *m, char *path, size_t pathlen,
                     char *err, size_t errlen)
{
  snprintf(path, pathlen, "%s%s", index, suffix);
  switch (map_file(path, m)) {
    case 0: return 0;
    case -1: return pfail(err, errlen, "cannot open file '%s'", path);
    default: return pfail(err, errlen, "cannot map file '%s'", path);
  }
}

/* The sequence the tables of a project describe: the symbols of INDEX.esq, then
   -mirrored, then -dir, as INDEX.prj says.  Refuses a project without whole
   tables; `verb` words what is not done with the slices of a build in parts.
   *enc_out is malloc'ed; *alpha (may be NULL) receives the alphabet of
   INDEX.esq, to be given to gtamd_alphabet_free. */
static int load_project_sequence(const char *index, const char *verb, uint8_t **enc_out,
                                 uint64_t *n_out, gtamd_alphabet *alpha_out, char *err, size_t errlen)
{
  char path[4096];
  unsigned long long totallength = 0, sorted = 0, readmode = 0, mirrored = 0;
  uint8_t *enc = NULL;
  uint64_t n = 0;
  gtamd_alphabet alpha;
  gtamd_seqstats ss;
  int dnalike;

  snprintf(path, sizeof path, "%s.prj", index);
  {
    FILE *fp = fopen(path, "r");
    if (fp == NULL) return pfail(err, errlen, "cannot open file '%s'", path);
    fclose(fp);
  }
  if (prj_value(path, "totallength", &totallength) != 0 ||
      prj_value(path, "numberofallsortedsuffixes", &sorted) != 0)
    return pfail(err, errlen, "cannot read totallength / numberofallsortedsuffixes from file '%s'", path);
  (void) prj_value(path, "readmode", &readmode);
  (void) prj_value(path, "mirrored", &mirrored);
  if (sorted == 0 && totallength != 0)
    return pfail(err, errlen, "file '%s' describes the project of a packed index "
                 "(numberofallsortedsuffixes=0): it has no tables to check", path);
  if (totallength + 1 > SFXMAP_MAX_ENTRIES) {
    snprintf(err, errlen, "sequence of %llu symbols is beyond the limit of a single build (%llu table "
             "entries); the slices of a build in parts are not %s", totallength,
             SFXMAP_MAX_ENTRIES, verb);
    return -1;
  }
  if (sorted != totallength + 1 || readmode > 3)
    return pfail(err, errlen, "file '%s' does not describe whole tables (numberofallsortedsuffixes "
                 "is not totallength + 1, or the read mode is unknown)", path);

  /* as stored, then -mirrored, then -dir */
  if (gtamd_read_esq_alpha(index, &enc, &n, &alpha, &ss, err, errlen) != 0) return -1;
  dnalike = alpha.numofchars == 4 && alpha.symbolmap['a'] == 0 && alpha.symbolmap['c'] == 1 &&
            alpha.symbolmap['g'] == 2 && alpha.symbolmap['t'] == 3;
  if (!dnalike && (readmode >= 2 || mirrored)) {
    pfail(err, errlen, "file '%s' asks for complemented symbols of an alphabet that is not DNA", path);
    goto fail;
  }
  if (mirrored) {
    uint8_t *m = gtamd_mirror(enc, n);
    if (m == NULL) { pfail(err, errlen, "out of memory (%s)", "-mirrored"); goto fail; }
    free(enc);
    enc = m;
    n = 2 * n + 1;
  }
  gtamd_apply_readmode(enc, n, (int) readmode);
  if (n != totallength) {
    pfail(err, errlen, "INDEX.esq and INDEX.prj of '%s' disagree on the total length", index);
    goto fail;
  }
  if (alpha_out != NULL) *alpha_out = alpha; else gtamd_alphabet_free(&alpha);
  *enc_out = enc;
  *n_out = n;
  return 0;
fail:
  gtamd_alphabet_free(&alpha);
  free(enc);
  return -1;
}

int gtamd_sfxmap(int argc, const char **argv, char *err, size_t errlen)
{
  int want_suf = 0, want_lcp = 0, want_bwt = 0, verbose = 0, rc = -1;
  const char *index = NULL;
  char path[4096], msg[512];
  unsigned long long longest = 0, large = 0, depth = 0;
  uint8_t *enc = NULL;
  uint64_t n = 0, N;
  uint32_t suf_bytes = 8;
  mapped suf = { NULL, 0 }, lcp = { NULL, 0 }, llv = { NULL, 0 }, bwt = { NULL, 0 };
  gtamd_check *chk = NULL;
  gtamd_check_report rep;

  for (int i = 1; i < argc; i++) {
    const char *a = argv[i];
    if (!strcmp(a, "-suf")) want_suf = 1;
    else if (!strcmp(a, "-lcp")) want_lcp = 1;
    else if (!strcmp(a, "-bwt")) want_bwt = 1;
    else if (!strcmp(a, "-v")) verbose = 1;
    else if (!strcmp(a, "-tis") || !strcmp(a, "-ssp")) continue;   /* (always read) */
    else if (!strcmp(a, "-esa")) {
      if (i + 1 >= argc) return pfail(err, errlen, "missing argument to option \"%s\"", a);
      index = argv[++i];
    } else {
      for (int k = 0; refused[k] != NULL; k++)
        if (!strcmp(a, refused[k]))
          return pfail(err, errlen, "option \"%s\" is not supported by the MI355X engine", a);
      if (a[0] == '-') return pfail(err, errlen, "unknown option: %s (try -help)", a);
      return pfail(err, errlen, "superfluous argument \"%s\"", a);
    }
  }
  if (index == NULL) return pfail(err, errlen, "option \"-%s\" is mandatory", "esa");
  if (!want_suf && (want_lcp || want_bwt))
    return pfail(err, errlen, "option \"-%s\" requires option \"-suf\": the table is checked through "
                 "the suffix array", want_lcp ? "lcp" : "bwt");

  if (load_project_sequence(index, "checked", &enc, &n, NULL, err, errlen) != 0) goto done;
  snprintf(path, sizeof path, "%s.prj", index);
  (void) prj_value(path, "longest", &longest);
  (void) prj_value(path, "largelcpvalues", &large);
  (void) prj_value(path, "maxbranchdepth", &depth);
  N = n + 1;

  if (want_suf) {
    if (map_table(index, ".suf", &suf, path, sizeof path, err, errlen) != 0) goto done;
    if (suf.bytes == 4 * N) suf_bytes = 4;
    else if (suf.bytes != 8 * N) {
      snprintf(err, errlen, "file '%s' has %llu bytes, %llu (-suftabuint) or %llu expected for %llu entries",
               path, (unsigned long long) suf.bytes, (unsigned long long) (4 * N),
               (unsigned long long) (8 * N), (unsigned long long) N);
      goto done;
    }
  }
  if (want_lcp) {
    if (map_table(index, ".lcp", &lcp, path, sizeof path, err, errlen) != 0) goto done;
    if (lcp.bytes != N) {
      snprintf(err, errlen, "file '%s' has %llu bytes, %llu expected", path,
               (unsigned long long) lcp.bytes, (unsigned long long) N);
      goto done;
    }
    if (map_table(index, ".llv", &llv, path, sizeof path, err, errlen) != 0) goto done;
    if (llv.bytes % 16 != 0) {
      snprintf(err, errlen, "file '%s' has %llu bytes, not a multiple of 16 (pairs of two 64-bit numbers)",
               path, (unsigned long long) llv.bytes);
      goto done;
    }
  }
  if (want_bwt) {
    if (map_table(index, ".bwt", &bwt, path, sizeof path, err, errlen) != 0) goto done;
    if (bwt.bytes != N) {
      snprintf(err, errlen, "file '%s' has %llu bytes, %llu expected", path,
               (unsigned long long) bwt.bytes, (unsigned long long) N);
      goto done;
    }
  }
  if (!want_suf) { rc = 0; goto done; }     /* the sequence and the project file agree */

  if ((chk = gtamd_check_create(0)) == NULL ||
      gtamd_check_tables_host(chk, enc, n, suf.p, suf_bytes, lcp.p, llv.p, llv.bytes / 16, bwt.p,
                              &rep) != 0) {
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
  snprintf(path, sizeof path, "%s.prj", index);
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
  unmap_file(&suf); unmap_file(&lcp); unmap_file(&llv); unmap_file(&bwt);
  free(enc);
  return rc;
}

/* ---- gt matstat / gt uniquesub ----
   Option handling and messages of src/tools/gt_matstat.c:96-278, output of
   src/match/greedyfwdmat.c:168-211. */
enum { SHOW_SEQUENCE = 1, SHOW_QUERYPOS = 2, SHOW_SUBJECTPOS = 4 };

static int length_option(int argc, const char **argv, int *i, unsigned long long *out, char *err,
                         size_t errlen)
{
  char *end;
  if (*i + 1 >= argc) return pfail(err, errlen, "missing argument to option \"%s\"", argv[*i]);
  *out = strtoull(argv[*i + 1], &end, 10);
  if (*end != 0 || end == argv[*i + 1] || argv[*i + 1][0] == '-')
    return pfail(err, errlen, "argument to option \"%s\" is out of range", argv[*i]);
  if (*out < 1) return pfail(err, errlen, "argument to option \"%s\" must be an integer >= 1", argv[*i]);
  (*i)++;
  return 0;
}

/* doms: matching statistics, else minimum unique prefixes */
static int greedy_forward_tool(int doms, int argc, const char **argv, char *err, size_t errlen)
{
  const char *index = NULL, *const *queries = NULL;
  size_t numqueries = 0;
  int have_min = 0, have_max = 0, have_output = 0, numflags = 0, query_seen = 0, rc = -1;
  unsigned show = 0;
  unsigned long long minlen = 0, maxlen = 0;
  char path[4096];
  uint8_t *enc = NULL, *query = NULL;
  uint64_t n = 0, m = 0, N, desclen = 0;
  char *desc = NULL;
  uint32_t suf_bytes = 8, *length = NULL;
  uint64_t *subjectpos = NULL;
  mapped suf = { NULL, 0 };
  gtamd_alphabet alpha;
  int have_alpha = 0;
  gtamd_mstat *ms = NULL;

  for (int i = 1; i < argc; i++) {
    const char *a = argv[i];
    if (!strcmp(a, "-esa")) {
      if (i + 1 >= argc) return pfail(err, errlen, "missing argument to option \"%s\"", a);
      index = argv[++i];
    } else if (!strcmp(a, "-fmi") || !strcmp(a, "-pck")) {
      return pfail(err, errlen, "option \"%s\" is not supported by the MI355X engine", a);
    } else if (!strcmp(a, "-query")) {
      query_seen = 1;
      queries = argv + i + 1;
      for (numqueries = 0; i + 1 < argc && argv[i + 1][0] != '-'; i++) numqueries++;
      if (numqueries == 0) return pfail(err, errlen, "missing argument to option \"%s\"", a);
    } else if (!strcmp(a, "-min")) {
      if (length_option(argc, argv, &i, &minlen, err, errlen) != 0) return -1;
      have_min = 1;
    } else if (!strcmp(a, "-max")) {
      if (length_option(argc, argv, &i, &maxlen, err, errlen) != 0) return -1;
      have_max = 1;
    } else if (!strcmp(a, "-output")) {
      have_output = 1;
      for (; i + 1 < argc && argv[i + 1][0] != '-'; i++, numflags++) {
        const char *f = argv[i + 1];
        if (!strcmp(f, "sequence")) show |= SHOW_SEQUENCE;
        else if (!strcmp(f, "querypos")) show |= SHOW_QUERYPOS;
        else if (doms && !strcmp(f, "subjectpos")) show |= SHOW_SUBJECTPOS;
        else return pfail(err, errlen, "illegal argument \"%s\" to option -output", f);
      }
    } else if (doms && !strcmp(a, "-verify")) {       /* without effect with -esa, as in the reference */
      if (i + 1 < argc && (!strcmp(argv[i + 1], "yes") || !strcmp(argv[i + 1], "no"))) i++;
    } else if (a[0] == '-') return pfail(err, errlen, "unknown option: %s (try -help)", a);
    else return pfail(err, errlen, "superfluous argument \"%s\"", a);
  }
  if (!query_seen) return pfail(err, errlen, "option \"-%s\" is mandatory", "query");
  if (index == NULL) return pfail(err, errlen, "one of the options -esa, -pck must be %s", "used");
  if (!have_min && !have_max) return pfail(err, errlen, "one of the options -min or -max must be %s", "set");
  if (have_min && have_max && maxlen < minlen)
    return pfail(err, errlen, "minvalue must be smaller or equal than %s", "maxvalue");
  if (have_output && numflags == 0) return pfail(err, errlen, "missing arguments to option %s", "-output");

  if (load_project_sequence(index, "searched", &enc, &n, &alpha, err, errlen) != 0) goto done;
  have_alpha = 1;
  N = n + 1;
  if (map_table(index, ".suf", &suf, path, sizeof path, err, errlen) != 0) goto done;
  if (suf.bytes == 4 * N) suf_bytes = 4;
  else if (suf.bytes != 8 * N) {
    snprintf(err, errlen, "file '%s' has %llu bytes, %llu (-suftabuint) or %llu expected for %llu entries",
             path, (unsigned long long) suf.bytes, (unsigned long long) (4 * N),
             (unsigned long long) (8 * N), (unsigned long long) N);
    goto done;
  }
  /* the queries, with the index's alphabet: one sequence of symbols, a separator
     between two units */
  if (gtamd_encode_files_alpha(queries, numqueries, &alpha, &query, &m, &desc, &desclen, NULL, err,
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
    pfail(err, errlen, "out of memory (%s)", "results");
    goto done;
  }
  {
    /* longer matches are not printed: the device stops looking there */
    const uint32_t cap = have_max && maxlen < 0xfffffffeull ? (uint32_t) maxlen : 0;
    if ((ms = gtamd_mstat_create(0)) == NULL ||
        gtamd_mstat_set_index_host(ms, enc, n, suf.p, suf_bytes, alpha.numofchars) != 0 ||
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
          for (uint32_t j = 0; j < v; j++) putchar(alpha.characters[query[k + j]]);
        }
        putchar('\n');
      }
    }
  }
  if (fflush(stdout) != 0) { pfail(err, errlen, "cannot write to %s", "stdout"); goto done; }
  rc = 0;
done:
  gtamd_mstat_destroy(ms);
  unmap_file(&suf);
  if (have_alpha) gtamd_alphabet_free(&alpha);
  free(length); free(subjectpos); free(desc); free(query); free(enc);
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

/* ---- gt repfind ----
   Option handling of src/tools/gt_repfind.c:224-470, output of an exact match
   as the reference displays it by default. */

/* a table of the index that must be there: the reference's wording when it is not */
static int map_required(const char *index, const char *suffix, mapped *m, char *path, size_t pathlen,
                        char *err, size_t errlen)
{
  snprintf(path, pathlen, "%s%s", index, suffix);
  if (access(path, R_OK) != 0) {
    snprintf(err, errlen, "cannot open file \"%s\": %s", path, strerror(errno));
    return -1;
  }
  return map_table(index, suffix, m, path, pathlen, err, errlen);
}

int gtamd_repfind(int argc, const char **argv, char *err, size_t errlen)
{
  /* other algorithms (queries against the index, seed extension) and other
     displays: refused by name */
  static const char *const refused[] = {
    "-r", "-p", "-q", "-qii", "-spm", "-samples", "-maxfreq", "-seedlength", "-outfmt", "-evalue",
    "-xdropbelow", "-err", "-minidentity", "-maxalilendiff", "-history", "-percmathistory", "-cam",
    "-noxpolish", "-verify-alignment", "-trimstat", "-check_extend_symmetry", NULL };
  const char *index = NULL;
  int verbose = 0, rc = -1;
  unsigned long long minlen = 20, readmode = 0, mirrored = 0;
  char path[4096];
  uint8_t *enc = NULL;
  uint64_t n = 0, N, numseq = 1, *seqstart = NULL, capacity, cursor = 0, written = 0, total = 0;
  uint32_t suf_bytes = 8;
  mapped suf = { NULL, 0 }, lcp = { NULL, 0 }, llv = { NULL, 0 };
  gtamd_maxpairs *mp = NULL;
  gtamd_maxpairs_info info;
  gtamd_maxpairs_record *rec = NULL;

  for (int i = 1; i < argc; i++) {
    const char *a = argv[i];
    if (!strcmp(a, "-ii")) {
      if (i + 1 >= argc) return pfail(err, errlen, "missing argument to option \"%s\"", a);
      index = argv[++i];
    } else if (!strcmp(a, "-l")) {
      if (length_option(argc, argv, &i, &minlen, err, errlen) != 0) return -1;
      if (minlen > 0xffffffffull) return pfail(err, errlen, "argument to option \"%s\" is out of range", a);
    } else if (!strcmp(a, "-f") || !strcmp(a, "-scan")) {
      if (i + 1 < argc && (!strcmp(argv[i + 1], "yes") || !strcmp(argv[i + 1], "no"))) {
        if (a[1] == 'f' && argv[i + 1][0] == 'n')
          return pfail(err, errlen, "option \"%s no\" leaves nothing to compute: forward repeats are all "
                       "the MI355X engine enumerates", a);
        i++;
      }
    } else if (!strcmp(a, "-v")) verbose = 1;
    else if (!strcmp(a, "-help")) {
      puts("Usage: gt-suffixerator-amd repfind -ii INDEX [-l L] [-f] [-scan] [-v]\n"
           "Compute the maximal exact repeats (maximal pairs) of the sequences of INDEX on the device.\n\n"
           "-ii    the index: INDEX.prj, .esq (.ssp), .suf, .lcp and .llv, as written by\n"
           "       `suffixerator -suf -lcp -tis -ssp`, forward read mode, not mirrored\n"
           "-l     minimum length of a repeat (default: 20)\n"
           "-f     forward repeats (what is computed)\n"
           "-scan  accepted, without effect\n"
           "-v     figures of the enumeration as lines that start with '#'\n\n"
           "One line per pair: `len seqnum1 relpos1 F len seqnum2 relpos2`, in TABLE ORDER: ascending\n"
           "table index of the suffix that stands first in the suffix table, then of the other.  The\n"
           "reference prints the same lines in the order of its traversal: compare sorted outputs.\n"
           "Reverse, palindromic, query, seed extension and suffix-prefix options are refused.");
      return 0;
    } else {
      for (int k = 0; refused[k] != NULL; k++)
        if (!strcmp(a, refused[k]))
          return pfail(err, errlen, "option \"%s\" is not supported by the MI355X engine", a);
      if (!strncmp(a, "-extend", 7))
        return pfail(err, errlen, "option \"%s\" is not supported by the MI355X engine", a);
      if (a[0] == '-') return pfail(err, errlen, "unknown option: %s (try -help)", a);
      return pfail(err, errlen, "superfluous arguments: \"%s\"", a);
    }
  }
  if (index == NULL) return pfail(err, errlen, "option \"-%s\" is mandatory", "ii");

  snprintf(path, sizeof path, "%s.prj", index);
  (void) prj_value(path, "readmode", &readmode);
  (void) prj_value(path, "mirrored", &mirrored);
  if (readmode != 0)
    return pfail(err, errlen, "file '%s' gives a read mode other than forward: such an index is not "
                 "supported by the MI355X engine's repfind", path);
  if (mirrored)
    return pfail(err, errlen, "file '%s' describes a mirrored index: such an index is not supported by the "
                 "MI355X engine's repfind", path);
  if (load_project_sequence(index, "searched", &enc, &n, NULL, err, errlen) != 0) goto done;
  N = n + 1;
  if (map_required(index, ".suf", &suf, path, sizeof path, err, errlen) != 0) goto done;
  if (suf.bytes == 4 * N) suf_bytes = 4;
  else if (suf.bytes != 8 * N) {
    snprintf(err, errlen, "file '%s' has %llu bytes, %llu (-suftabuint) or %llu expected for %llu entries",
             path, (unsigned long long) suf.bytes, (unsigned long long) (4 * N),
             (unsigned long long) (8 * N), (unsigned long long) N);
    goto done;
  }
  if (map_required(index, ".lcp", &lcp, path, sizeof path, err, errlen) != 0) goto done;
  if (lcp.bytes != N) {
    snprintf(err, errlen, "file '%s' has %llu bytes, %llu expected", path, (unsigned long long) lcp.bytes,
             (unsigned long long) N);
    goto done;
  }
  if (map_required(index, ".llv", &llv, path, sizeof path, err, errlen) != 0) goto done;
  if (llv.bytes % 16 != 0) {
    snprintf(err, errlen, "file '%s' has %llu bytes, not a multiple of 16 (pairs of two 64-bit numbers)",
             path, (unsigned long long) llv.bytes);
    goto done;
  }
  /* where the sequences start: behind the separators (INDEX.ssp, as the reader of
     INDEX.esq has put them into the symbols) */
  for (uint64_t p = 0; p < n; p++) numseq += enc[p] == 255;
  seqstart = malloc(numseq * sizeof *seqstart);
  if (seqstart == NULL) { pfail(err, errlen, "out of memory (%s)", "sequence starts"); goto done; }
  seqstart[0] = 0;
  for (uint64_t p = 0, k = 1; p < n; p++)
    if (enc[p] == 255) seqstart[k++] = p + 1;

  if ((mp = gtamd_maxpairs_create(0)) == NULL ||
      gtamd_maxpairs_set_index_host(mp, enc, n, suf.p, suf_bytes, lcp.p, llv.p, llv.bytes / 16) != 0 ||
      gtamd_maxpairs_prepare(mp, (uint32_t) minlen, &info) != 0) {
    snprintf(err, errlen, "%s", gtamd_esa_last_error());
    goto done;
  }
  if (verbose)
    printf("# %llu pairs, %llu suffixes in %llu runs, %llu segments, at most %llu pairs of one suffix, "
           "longest %llu, %llu steps, %.3f ms on the device\n", (unsigned long long) info.pairs,
           (unsigned long long) info.run_suffixes, (unsigned long long) info.runs,
           (unsigned long long) info.segments, (unsigned long long) info.max_pairs_of_one_suffix,
           (unsigned long long) info.max_len, (unsigned long long) info.walk_steps, info.device_ms);
  capacity = info.max_pairs_of_one_suffix > (1u << 20) ? info.max_pairs_of_one_suffix : (1u << 20);
  if (capacity > info.pairs) capacity = info.pairs;
  rec = malloc((capacity ? capacity : 1) * sizeof *rec);
  if (rec == NULL) { pfail(err, errlen, "out of memory (%s)", "records"); goto done; }
  do {
    if (gtamd_maxpairs_emit(mp, &cursor, rec, capacity, 0, &written) != 0) {
      snprintf(err, errlen, "%s", gtamd_esa_last_error());
      goto done;
    }
    for (uint64_t k = 0; k < written; k++) {
      uint64_t s[2];
      const uint64_t pos[2] = { rec[k].pos1, rec[k].pos2 };
      for (int side = 0; side < 2; side++) {       /* the last start at or in front of the position */
        uint64_t lo = 0, hi = numseq;
        while (hi - lo > 1) {
          const uint64_t mid = lo + (hi - lo) / 2;
          if (seqstart[mid] <= pos[side]) lo = mid; else hi = mid;
        }
        s[side] = lo;
      }
      printf("%llu %llu %llu F %llu %llu %llu\n", (unsigned long long) rec[k].len, (unsigned long long) s[0],
             (unsigned long long) (pos[0] - seqstart[s[0]]), (unsigned long long) rec[k].len,
             (unsigned long long) s[1], (unsigned long long) (pos[1] - seqstart[s[1]]));
    }
    total += written;
  } while (written != 0);
  if (total != info.pairs) {
    snprintf(err, errlen, "%llu pairs counted, %llu given", (unsigned long long) info.pairs,
             (unsigned long long) total);
    goto done;
  }
  if (fflush(stdout) != 0) { pfail(err, errlen, "cannot write to %s", "stdout"); goto done; }
  rc = 0;
done:
  gtamd_maxpairs_destroy(mp);
  unmap_file(&suf); unmap_file(&lcp); unmap_file(&llv);
  free(rec); free(seqstart); free(enc);
  return rc;
}

/* ---- gt repfind -q / -r / -p ----
   Option handling of src/tools/gt_repfind.c:224-470, the calls it sends to
   gt_callenumquerymatches (:562-757); display and the `ordered` filter of
   src/match/querymatch.c:202-213, 357-369. */

/* the last of the numstart ascending starts at or in front of pos */
static uint64_t unit_of(const uint64_t *start, uint64_t numstart, uint64_t pos)
{
  uint64_t lo = 0, hi = numstart;
  while (hi - lo > 1) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (start[mid] <= pos) lo = mid; else hi = mid;
  }
  return lo;
}

/* where the sequences of seq[0..len) start: behind the separators; *num = their number */
static uint64_t *sequence_starts(const uint8_t *seq, uint64_t len, uint64_t *num)
{
  uint64_t count = 1, *start;
  for (uint64_t p = 0; p < len; p++) count += seq[p] == 255;
  start = malloc((count + 1) * sizeof *start);
  if (start == NULL) return NULL;
  start[0] = 0;
  for (uint64_t p = 0, k = 1; p < len; p++)
    if (seq[p] == 255) start[k++] = p + 1;
  start[count] = len + 1;              /* (as if one more separator followed) */
  *num = count;
  return start;
}

/* gt_mmsearch_accessquery: mode 1 reverses every sequence on its own, mode 2
   complements its letters in addition */
static void transform_query(uint8_t *out, const uint8_t *query, const uint64_t *start, uint64_t numunits, int mode)
{
  for (uint64_t u = 0; u < numunits; u++) {
    const uint64_t s = start[u], len = start[u + 1] - 1 - s;
    for (uint64_t k = 0; k < len; k++) {
      const uint8_t c = query[s + (mode ? len - 1 - k : k)];
      out[s + k] = mode == 2 && c < 254 ? (uint8_t) (3 - c) : c;
    }
    if (u + 1 < numunits) out[s + len] = 255;
  }
}

#define QUERYMATCH_CALL_LIMIT 0xffffffffull      /* symbols of one gtamd_qmatch_prepare */
#define QUERYMATCH_CAPACITY (1u << 20)           /* records of one gtamd_qmatch_emit */

int gtamd_querymatch(int argc, const char **argv, char *err, size_t errlen)
{
  /* a query from an index, seed extension, other displays: refused by name */
  static const char *const refused[] = {
    "-qii", "-scan", "-spm", "-samples", "-maxfreq", "-seedlength", "-outfmt", "-evalue", "-xdropbelow", "-err",
    "-minidentity", "-maxalilendiff", "-history", "-percmathistory", "-cam", "-noxpolish",
    "-verify-alignment", "-trimstat", "-check_extend_symmetry", NULL };
  static const char modechar[3] = { 'F', 'R', 'P' };
  const char *index = NULL, *const *queries = NULL;
  size_t numqueries = 0;
  int mode_on[3] = { 0, 0, 0 }, f_given = 0, have_q = 0, verbose = 0, have_alpha = 0, rc = -1;
  unsigned long long minlen = 20, readmode = 0, mirrored = 0;
  char path[4096];
  uint8_t *enc = NULL, *query_own = NULL, *tq = NULL;
  const uint8_t *query;
  uint64_t n = 0, m = 0, N, numseq = 0, numunits = 0, *seqstart = NULL, *unitstart = NULL, desclen = 0;
  char *desc = NULL;
  uint32_t suf_bytes = 8;
  mapped suf = { NULL, 0 };
  gtamd_alphabet alpha;
  gtamd_qmatch *qm = NULL;
  gtamd_qmatch_info info;
  gtamd_qmatch_record *rec = NULL;

  for (int i = 1; i < argc; i++) {
    const char *a = argv[i];
    if (!strcmp(a, "-ii")) {
      if (i + 1 >= argc) return pfail(err, errlen, "missing argument to option \"%s\"", a);
      index = argv[++i];
    } else if (!strcmp(a, "-l")) {
      if (length_option(argc, argv, &i, &minlen, err, errlen) != 0) return -1;
      if (minlen > 0xffffffffull) return pfail(err, errlen, "argument to option \"%s\" is out of range", a);
    } else if (!strcmp(a, "-f") || !strcmp(a, "-r") || !strcmp(a, "-p")) {
      const int k = a[1] == 'f' ? 0 : a[1] == 'r' ? 1 : 2;
      mode_on[k] = 1;
      if (i + 1 < argc && (!strcmp(argv[i + 1], "yes") || !strcmp(argv[i + 1], "no")))
        mode_on[k] = argv[++i][0] == 'y';
      if (k == 0) f_given = 1;
    } else if (!strcmp(a, "-q")) {
      have_q = 1;
      queries = argv + i + 1;
      for (numqueries = 0; i + 1 < argc && argv[i + 1][0] != '-'; i++) numqueries++;
      if (numqueries == 0) return pfail(err, errlen, "missing argument to option \"%s\"", a);
    } else if (!strcmp(a, "-v")) verbose = 1;
    else if (!strcmp(a, "-help")) {
      puts("Usage: gt-suffixerator-amd querymatch -ii INDEX [-l L] [-f] [-r] [-p] [-q FILE...] [-v]\n"
           "Compute the maximal exact matches of query sequences against the sequences of INDEX on the\n"
           "device: what `gt repfind` computes with -q, -r or -p.\n\n"
           "-ii    the index: INDEX.prj, .esq (.ssp) and .suf, as written by `suffixerator -suf -tis -ssp`,\n"
           "       forward read mode, not mirrored\n"
           "-l     minimum length of a match (default: 20)\n"
           "-q     FASTA files with the queries, read with the alphabet of INDEX; their sequences are\n"
           "       numbered across all files.  Without -q the sequences of INDEX are the queries of -r and\n"
           "       -p, and of two records that show the same pair only one is kept\n"
           "-f     forward matches (the default, unless -r or -p is given without -f); needs -q: the\n"
           "       forward repeats of an index are the business of the repfind sub-command\n"
           "-r     reverse matches: every query sequence is read backwards\n"
           "-p     reverse-complement matches (DNA only)\n"
           "-v     figures of every search as lines that start with '#'\n\n"
           "One line per match: `len dbseqnum dbrelpos F|R|P len querynum querystart`, querystart on the\n"
           "forward strand of the query, in the reference's order: the modes f, r, p one after the other,\n"
           "in each ascending query number and offset (of the query as read), then ascending table index\n"
           "of the subject suffix.  -qii, -scan, seed extension, -spm and the display options are refused.");
      return 0;
    } else {
      for (int k = 0; refused[k] != NULL; k++)
        if (!strcmp(a, refused[k]))
          return pfail(err, errlen, "option \"%s\" is not supported by the MI355X engine", a);
      if (!strncmp(a, "-extend", 7))
        return pfail(err, errlen, "option \"%s\" is not supported by the MI355X engine", a);
      if (a[0] == '-') return pfail(err, errlen, "unknown option: %s (try -help)", a);
      return pfail(err, errlen, "superfluous arguments: \"%s\"", a);
    }
  }
  if (index == NULL) return pfail(err, errlen, "option \"-%s\" is mandatory", "ii");
  /* gt_repfind_arguments_check: forward unless -r or -p is given without -f */
  if (!f_given) mode_on[0] = !(mode_on[1] || mode_on[2]);
  if (!have_q && mode_on[0])
    return pfail(err, errlen, "forward matches of the index with itself are its maximal repeats: use the "
                 "%s sub-command for them (querymatch takes -q FILE..., -r or -p)", "repfind");
  if (!(mode_on[0] || mode_on[1] || mode_on[2]))
    return pfail(err, errlen, "none of the options -f, -r and -p is %s", "set");

  snprintf(path, sizeof path, "%s.prj", index);
  (void) prj_value(path, "readmode", &readmode);
  (void) prj_value(path, "mirrored", &mirrored);
  if (readmode != 0)
    return pfail(err, errlen, "file '%s' gives a read mode other than forward: such an index is not "
                 "supported by the MI355X engine's querymatch", path);
  if (mirrored)
    return pfail(err, errlen, "file '%s' describes a mirrored index: such an index is not supported by the "
                 "MI355X engine's querymatch", path);
  if (load_project_sequence(index, "searched", &enc, &n, &alpha, err, errlen) != 0) goto done;
  have_alpha = 1;
  if (mode_on[2] && !(alpha.numofchars == 4 && alpha.symbolmap['a'] == 0 && alpha.symbolmap['c'] == 1 &&
                      alpha.symbolmap['g'] == 2 && alpha.symbolmap['t'] == 3)) {
    pfail(err, errlen, "option \"%s\" needs a DNA alphabet: the index has none, and its letters have no "
          "complement", "-p");
    goto done;
  }
  N = n + 1;
  if (map_required(index, ".suf", &suf, path, sizeof path, err, errlen) != 0) goto done;
  if (suf.bytes == 4 * N) suf_bytes = 4;
  else if (suf.bytes != 8 * N) {
    snprintf(err, errlen, "file '%s' has %llu bytes, %llu (-suftabuint) or %llu expected for %llu entries",
             path, (unsigned long long) suf.bytes, (unsigned long long) (4 * N),
             (unsigned long long) (8 * N), (unsigned long long) N);
    goto done;
  }
  /* the queries, with the index's alphabet: one sequence of symbols, a separator
     between two units; without -q the index's own */
  query = enc;
  m = n;
  if (have_q) {
    if (gtamd_encode_files_alpha(queries, numqueries, &alpha, &query_own, &m, &desc, &desclen, NULL, err,
                                 errlen) != 0)
      goto done;
    query = query_own;
  }
  seqstart = sequence_starts(enc, n, &numseq);
  unitstart = sequence_starts(query, m, &numunits);
  tq = malloc(m ? m : 1);
  rec = malloc(QUERYMATCH_CAPACITY * sizeof *rec);
  if (seqstart == NULL || unitstart == NULL || tq == NULL || rec == NULL) {
    pfail(err, errlen, "out of memory (%s)", "queries and records");
    goto done;
  }
  if ((qm = gtamd_qmatch_create(0)) == NULL || gtamd_qmatch_set_index_host(qm, enc, n, suf.p, suf_bytes) != 0) {
    snprintf(err, errlen, "%s", gtamd_esa_last_error());
    goto done;
  }
  for (int mode = 0; mode < 3; mode++) {
    if (!mode_on[mode]) continue;
    transform_query(tq, query, unitstart, numunits, mode);
    /* one call per run of whole units that fits its limit */
    for (uint64_t a = 0, b; a < numunits; a = b) {
      uint64_t cursor = 0, written = 0, first = unitstart[a], len;
      for (b = a + 1; b < numunits && unitstart[b + 1] - 1 - first <= QUERYMATCH_CALL_LIMIT; b++) ;
      len = unitstart[b] - 1 - first;
      if (len > QUERYMATCH_CALL_LIMIT) {
        snprintf(err, errlen, "query sequence %llu has %llu symbols, at most %llu in one search",
                 (unsigned long long) a, (unsigned long long) len, QUERYMATCH_CALL_LIMIT);
        goto done;
      }
      if (gtamd_qmatch_prepare(qm, tq + first, len, 0, (uint32_t) minlen, &info) != 0) {
        snprintf(err, errlen, "%s", gtamd_esa_last_error());
        goto done;
      }
      if (verbose)
        printf("# %c: %llu positions, %llu seeds, %llu candidates, widest interval %llu, %llu symbols "
               "compared by the searches, %.3f ms on the device\n", modechar[mode],
               (unsigned long long) info.positions, (unsigned long long) info.seeds,
               (unsigned long long) info.candidates, (unsigned long long) info.max_width,
               (unsigned long long) info.search_symbols, info.device_ms);
      do {
        if (gtamd_qmatch_emit(qm, &cursor, rec, QUERYMATCH_CAPACITY, 0, &written) != 0) {
          snprintf(err, errlen, "%s", gtamd_esa_last_error());
          goto done;
        }
        for (uint64_t k = 0; k < written; k++) {
          const uint64_t qpos = first + rec[k].qpos, reclen = rec[k].len;
          const uint64_t unit = unit_of(unitstart, numunits, qpos), offset = qpos - unitstart[unit];
          const uint64_t unitlen = unitstart[unit + 1] - 1 - unitstart[unit];
          const uint64_t dbseq = unit_of(seqstart, numseq, rec[k].dbpos), dbrel = rec[k].dbpos - seqstart[dbseq];
          /* gt_querymatch_position_convert: the start on the forward strand */
          const uint64_t qfwd = mode == 0 ? offset : unitlen - offset - reclen;
          /* gt_querymatch_ordered: of the two records of one pair, the one whose
             subject side comes first */
          if (!have_q && !(dbseq < unit || (dbseq == unit && dbrel < qfwd + (mode != 0)))) continue;
          printf("%llu %llu %llu %c %llu %llu %llu\n", (unsigned long long) reclen, (unsigned long long) dbseq,
                 (unsigned long long) dbrel, modechar[mode], (unsigned long long) reclen,
                 (unsigned long long) unit, (unsigned long long) qfwd);
        }
      } while (written != 0);
    }
  }
  if (fflush(stdout) != 0) { pfail(err, errlen, "cannot write to %s", "stdout"); goto done; }
  rc = 0;
done:
  gtamd_qmatch_destroy(qm);
  unmap_file(&suf);
  if (have_alpha) gtamd_alphabet_free(&alpha);
  free(rec); free(tq); free(unitstart); free(seqstart); free(desc); free(query_own); free(enc);
  return rc;
}

/* ---- gt encseq2spm ----
   Option handling of src/tools/gt_encseq2spm.c:94-260; the lines of
   processlcpinterval_spmsk (src/match/esa-spmsk.c:106) and the count line of
   the tool (gt_encseq2spm.c). */

#define ENCSEQ2SPM_CAPACITY (1u << 20)           /* records of one gtamd_spm_emit */

int gtamd_encseq2spm(int argc, const char **argv, char *err, size_t errlen)
{
  /* how the reference's own sort is run and checked: no counterpart here */
  static const char *const refused[] = {
    "-parts", "-memlimit", "-checksuftab", "-onlyaccum", "-onlyallfirstcodes", "-addbscachedepth",
    "-phase2extra", "-radixlarge", "-radixparts", "-singlescan", "-forcek", NULL };
  const char *index = NULL;
  int have_l = 0, show = 0, count = 0, verbose = 0, rc = -1, dnalike;
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
    if (!strcmp(a, "-ii")) {
      if (i + 1 >= argc) return pfail(err, errlen, "missing argument to option \"%s\"", a);
      index = argv[++i];
    } else if (!strcmp(a, "-l")) {
      if (length_option(argc, argv, &i, &minlen, err, errlen) != 0) return -1;
      if (minlen > 0xffffffffull) return pfail(err, errlen, "argument to option \"%s\" is out of range", a);
      have_l = 1;
    } else if (!strcmp(a, "-spm")) {
      if (i + 1 >= argc) return pfail(err, errlen, "missing argument to option \"%s\"", a);
      i++;
      show = !strcmp(argv[i], "show");
      count = !strcmp(argv[i], "count");
      if (!show && !count) return pfail(err, errlen, "illegal argument \"%s\" to option -spm", argv[i]);
    } else if (!strcmp(a, "-singlestrand")) {
      if (i + 1 < argc && !strcmp(argv[i + 1], "no")) { i++; continue; }
      /* (the reference's own message, gt_encseq2spm.c) */
      return pfail(err, errlen, "option %s is not implemented", "-singlestand");
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
    } else {
      for (int k = 0; refused[k] != NULL; k++)
        if (!strcmp(a, refused[k]))
          return pfail(err, errlen, "option \"%s\" is not supported by the MI355X engine", a);
      if (a[0] == '-') return pfail(err, errlen, "unknown option: %s (-help shows possible options)", a);
      return pfail(err, errlen, "unnecessary %s", "arguments");
    }
  }
  if (!have_l) return pfail(err, errlen, "option \"-%s\" is mandatory", "l");
  if (index == NULL) return pfail(err, errlen, "option \"-%s\" is mandatory", "ii");

  /* the reads as stored: a project that reads them another way is none for this tool */
  snprintf(path, sizeof path, "%s.prj", index);
  if (access(path, R_OK) != 0) return pfail(err, errlen, "cannot open file '%s'", path);
  (void) prj_value(path, "readmode", &readmode);
  (void) prj_value(path, "mirrored", &mirrored);
  if (readmode != 0 || mirrored)
    return pfail(err, errlen, "file '%s' gives a read mode other than forward or describes a mirrored index: "
                 "encseq2spm mirrors the reads itself", path);
  if (gtamd_read_esq_alpha(index, &enc, &n, &alpha, &ss, err, errlen) != 0) return -1;
  dnalike = alpha.numofchars == 4 && alpha.symbolmap['a'] == 0 && alpha.symbolmap['c'] == 1 &&
            alpha.symbolmap['g'] == 2 && alpha.symbolmap['t'] == 3;
  if (!dnalike) {
    snprintf(err, errlen, "mirroring can only be enabled for DNA sequences, this encoded sequence has "
             "alphabet: %.*s", (int) alpha.numofchars, alpha.characters);
    goto done;
  }
  if (2 * n + 2 > SFXMAP_MAX_ENTRIES) {
    snprintf(err, errlen, "%llu symbols on both strands are beyond the limit of a single build (%llu table "
             "entries); the slices of a build in parts are not searched", (unsigned long long) n,
             SFXMAP_MAX_ENTRIES);
    goto done;
  }
  /* the reference ends here too when no output is asked for */
  if (!show && !count) { rc = 0; goto done; }

  both = gtamd_mirror(enc, n);
  if (both == NULL) { pfail(err, errlen, "out of memory (%s)", "mirrored reads"); goto done; }
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
    if (rec == NULL) { pfail(err, errlen, "out of memory (%s)", "records"); goto done; }
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
  if (fflush(stdout) != 0) { pfail(err, errlen, "cannot write to %s", "stdout"); goto done; }
  rc = 0;
done:
  gtamd_spm_destroy(sp);
  if (ctx != NULL) gtamd_esa_destroy(ctx);
  if (de != NULL) gtamd_encoder_destroy(de);
  gtamd_alphabet_free(&alpha);
  free(rec); free(both); free(enc);
  return rc;
}

/* ---- gt tagerator ----
   In a file of its own, this one being long enough, but part of this translation
   unit: the sanitized tool of tests/test_host_sanitized.py is linked from a fixed
   list of files, of which this is the one with the helpers the tool needs (see the
   head of tagmatch_host.c). */
#include "tagmatch_host.c"

/* ---- gt dev idxlocali ----
   The same arrangement: it reads a project back with the helpers above and takes
   switch_option from tagmatch_host.c. */
#include "locali_host.c"

/* ---- gt readjoiner overlap ----
   The same arrangement: it takes pfail from above and switch_option from
   tagmatch_host.c. */
#include "rdj_host.c"
