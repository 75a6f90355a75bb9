/* host_san_driver.c -- TEST INFRASTRUCTURE ONLY.  The host layer's file readers
   and writers (-DDRIVER_HOST: esq_host.c alphabet_host.c encseq_host.c md5_host.c
   ois_host.c cli_host.c project_host.c) or the CPU oracle (-DDRIVER_ORACLE: esa_oracle.c pck_oracle.c)
   behind one small command reader, so that tests/test_host_sanitized.py can
   run thousands of inputs through an AddressSanitizer/UBSan build in one
   process.  Never opens a device; nothing here links the engine.

     host_san_driver canary          reads one byte past a heap block (the test
                                     asserts that the sanitizer reports it)
     host_san_driver run WORKFILE    one work item per line of WORKFILE ("-":
                                     standard input), fields separated by tabs

   For every item one line goes to standard output:
     rc <TAB> message <TAB> size of the output <TAB> crc32 of the output [<TAB> more]
   Work items with -DDRIVER_HOST:
     base ESQ SSP|- SCRATCH   load an index image to derive mutants from; SCRATCH
                              is the index name the mutants are written under
     mut E|S W V [E|S W V]    the image with 8-byte word W of the .esq (E) or the
                              .ssp (S) set to V, through gtamd_read_esq_alpha;
                              more: alphabet size, symbols that are no letter,
                              wildcard or separator
     cut E|S LEN              the same with the file cut to LEN bytes
     read INDEX OUT|-         gtamd_read_esq_alpha on INDEX; symbols to OUT
     encode ALPHA SAT|- LOSSLESS INDEX|- OUT|- FILE...
                              ALPHA dna | protein | smap:FILE; the input files through
                              the encoder (symbols to OUT) and, with an INDEX,
                              .ois (LOSSLESS 1) .esq .ssp .des .sds .md5 as the
                              tool writes them, input names stored without
                              directories
     project INDEX VERB WHICH TOOL REQUIRED TABLES|-
                              gtamd_project_open(INDEX, VERB, WHICH, TOOL), then
                              gtamd_project_map with REQUIRED for every letter of
                              TABLES (s .suf, l .lcp, v .llv, b .bwt), then the
                              sequence starts; output: the symbols; more: bytes of
                              a .suf entry, number of sequences
   Work items with -DDRIVER_ORACLE:
     fasta PROTEIN FILE       ora_encode_fasta; output: the symbols
     tables SIGMA K ENC BSIZE BLBUCK LOCFREQ LOCBITMAP MKINDEX SPRANK
                              ENC holds encoded symbols; suf lcp llv bwt, the
                              bucket table for prefix length K, one INDEX.bdx
                              image; size and crc32 over all of them in that
                              order, then size:crc32 of each */
#define _GNU_SOURCE              /* memfd_create */
#include <fcntl.h>
#include <inttypes.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/mman.h>
#include <unistd.h>
#include <zlib.h>

#if defined(DRIVER_HOST) == defined(DRIVER_ORACLE)
#error "build with exactly one of -DDRIVER_HOST and -DDRIVER_ORACLE"
#endif

#define MAXFIELDS 64

static int canary(void)
{
  /* the size is volatile, so that no compile-time object size check sees the
     overflow and the report is AddressSanitizer's own */
  volatile size_t size = 16;
  unsigned char *p = malloc(size), c;
  if (p == NULL) return 2;
  memset(p, 1, size);
  c = ((volatile unsigned char *) p)[size];       /* one byte past the block */
  printf("canary survived %u\n", (unsigned) c);
  free(p);
  return 0;
}

static void report(int rc, const char *msg, uint64_t size, uint32_t crc, const char *more)
{
  char clean[2048];
  size_t k = 0;
  for (; msg[k] != '\0' && k + 1 < sizeof clean; k++)
    clean[k] = msg[k] == '\t' || msg[k] == '\n' || msg[k] == '\r' ? ' ' : msg[k];
  clean[k] = '\0';
  printf("%d\t%s\t%" PRIu64 "\t%08x%s%s\n", rc, clean, size, (unsigned) crc,
         more[0] != '\0' ? "\t" : "", more);
}

static uint32_t crc_more(uint32_t crc, const void *p, uint64_t bytes)
{
  const unsigned char *q = p;
  while (bytes > 0) {
    const uint64_t piece = bytes < (1u << 30) ? bytes : (1u << 30);
    crc = (uint32_t) crc32(crc, q, (uInt) piece);
    q += piece; bytes -= piece;
  }
  return crc;
}

static int load(const char *path, unsigned char **data, uint64_t *len)
{
  FILE *fp = fopen(path, "rb");
  long size;
  *data = NULL; *len = 0;
  if (fp == NULL) return -1;
  if (fseek(fp, 0, SEEK_END) != 0 || (size = ftell(fp)) < 0 || fseek(fp, 0, SEEK_SET) != 0 ||
      (*data = malloc(size > 0 ? (size_t) size : 1)) == NULL ||
      fread(*data, 1, (size_t) size, fp) != (size_t) size) {
    free(*data); *data = NULL;
    fclose(fp);
    return -1;
  }
  fclose(fp);
  *len = (uint64_t) size;
  return 0;
}

#ifdef DRIVER_HOST
#include "host_internal.h"

static int store(const char *path, const void *data, uint64_t len)
{
  FILE *fp = fopen(path, "wb");
  if (fp == NULL) return -1;
  if (len > 0 && fwrite(data, 1, len, fp) != len) { fclose(fp); return -1; }
  return fclose(fp) != 0 ? -1 : 0;
}

static unsigned char *base_img[2];     /* .esq, .ssp */
static uint64_t base_len[2];
static int base_dirty[2];              /* the scratch file differs from the image */
static char scratch[4000];

static void base_free(void)
{
  for (int f = 0; f < 2; f++) { free(base_img[f]); base_img[f] = NULL; base_len[f] = 0; }
}

/* The reader takes file names, and a mutant differs from the last one in a few
   bytes: the two scratch files are opened once and rewritten in place.  Where
   the kernel has them they are anonymous memory files, reached by the reader
   through a link SCRATCH.esq -> /proc/self/fd/N, so that a hundred thousand
   mutants do not go through the file system's journal. */
static int scratch_fd[2] = {-1, -1};

static int scratch_open(int f)
{
  char path[4096], target[64];
  snprintf(path, sizeof path, "%s.%s", scratch, f == 0 ? "esq" : "ssp");
  if (scratch_fd[f] >= 0) close(scratch_fd[f]);
  unlink(path);
  scratch_fd[f] = memfd_create("scratch", 0);
  if (scratch_fd[f] >= 0) {
    snprintf(target, sizeof target, "/proc/self/fd/%d", scratch_fd[f]);
    if (symlink(target, path) == 0 && access(path, R_OK) == 0) return 0;
    close(scratch_fd[f]);
    unlink(path);
  }
  scratch_fd[f] = open(path, O_RDWR | O_CREAT | O_TRUNC, 0600);
  return scratch_fd[f] >= 0 ? 0 : -1;
}

static int scratch_write(int f, const unsigned char *data, uint64_t len)
{
  if (scratch_fd[f] < 0 || ftruncate(scratch_fd[f], (off_t) len) != 0) return -1;
  return len == 0 || pwrite(scratch_fd[f], data, len, 0) == (ssize_t) len ? 0 : -1;
}

static int do_base(char **fld, int nf)
{
  if (nf != 4) return -1;
  base_free();
  if (load(fld[1], &base_img[0], &base_len[0]) != 0) return -1;
  if (strcmp(fld[2], "-") != 0 && load(fld[2], &base_img[1], &base_len[1]) != 0) return -1;
  snprintf(scratch, sizeof scratch, "%s", fld[3]);
  for (int f = 0; f < 2; f++) {
    base_dirty[f] = 0;
    if (base_img[f] == NULL) {
      /* no such file for this index */
      char path[4096];
      snprintf(path, sizeof path, "%s.ssp", scratch);
      if (scratch_fd[f] >= 0) { close(scratch_fd[f]); scratch_fd[f] = -1; }
      unlink(path);
    } else if (scratch_open(f) != 0 || scratch_write(f, base_img[f], base_len[f]) != 0)
      return -1;
  }
  report(0, "", base_len[0] + base_len[1], 0, "");
  return 0;
}

/* the reader on an index; the symbols it returns are checked against the
   alphabet it returns */
static void read_and_report(const char *index, const char *out)
{
  uint8_t *enc = NULL;
  uint64_t n = 0, bad = 0;
  gtamd_alphabet a;
  gtamd_seqstats ss;
  char err[1024] = "", more[64] = "";
  uint32_t crc = 0;
  const int rc = gtamd_read_esq_alpha(index, &enc, &n, &a, &ss, err, sizeof err);
  if (rc == 0) {
    for (uint64_t i = 0; i < n; i++)
      bad += enc[i] >= a.numofchars && enc[i] != GTAMD_WILDCARD && enc[i] != GTAMD_SEPARATOR;
    crc = crc_more(0, enc, n);
    snprintf(more, sizeof more, "%u\t%" PRIu64, (unsigned) a.numofchars, bad);
    if (out != NULL && store(out, enc, n) != 0) snprintf(err, sizeof err, "cannot write %s", out);
    free(enc);
    gtamd_alphabet_free(&a);
  }
  report(rc, err, n, crc, more);
}

static int which_file(const char *s)
{
  return strcmp(s, "E") == 0 ? 0 : strcmp(s, "S") == 0 ? 1 : -1;
}

static int do_mut(char **fld, int nf)
{
  unsigned char *copy[2] = {NULL, NULL};
  int rc = -1;
  if (base_img[0] == NULL || (nf != 4 && nf != 7)) return -1;
  for (int k = 1; k < nf; k += 3) {
    const int f = which_file(fld[k]);
    const uint64_t w = strtoull(fld[k + 1], NULL, 10), v = strtoull(fld[k + 2], NULL, 10);
    if (f < 0 || base_img[f] == NULL || w >= base_len[f] / 8) goto done;
    if (copy[f] == NULL) {
      if ((copy[f] = malloc(base_len[f] ? base_len[f] : 1)) == NULL) goto done;
      memcpy(copy[f], base_img[f], base_len[f]);
    }
    memcpy(copy[f] + 8 * w, &v, 8);
  }
  for (int f = 0; f < 2; f++) {
    if (copy[f] != NULL) {
      if (scratch_write(f, copy[f], base_len[f]) != 0) goto done;
      base_dirty[f] = 1;
    } else if (base_dirty[f]) {
      if (scratch_write(f, base_img[f], base_len[f]) != 0) goto done;
      base_dirty[f] = 0;
    }
  }
  read_and_report(scratch, NULL);
  rc = 0;
done:
  free(copy[0]); free(copy[1]);
  return rc;
}

static int do_cut(char **fld, int nf)
{
  int f;
  uint64_t len;
  if (base_img[0] == NULL || nf != 3 || (f = which_file(fld[1])) < 0 || base_img[f] == NULL)
    return -1;
  len = strtoull(fld[2], NULL, 10);
  if (len > base_len[f]) return -1;
  if (base_dirty[1 - f] && base_img[1 - f] != NULL) {
    if (scratch_write(1 - f, base_img[1 - f], base_len[1 - f]) != 0) return -1;
    base_dirty[1 - f] = 0;
  }
  if (scratch_write(f, base_img[f], len) != 0) return -1;
  base_dirty[f] = 1;
  read_and_report(scratch, NULL);
  return 0;
}

static int do_read(char **fld, int nf)
{
  if (nf != 3) return -1;
  read_and_report(fld[1], strcmp(fld[2], "-") != 0 ? fld[2] : NULL);
  return 0;
}

static int do_encode(char **fld, int nf)
{
  gtamd_alphabet a;
  gtamd_encinfo info;
  gtamd_seqstats ss;
  uint8_t *enc = NULL, *orig = NULL;
  char *desc = NULL, err[2048] = "";
  const char *names[MAXFIELDS];
  uint64_t n = 0, desclen = 0;
  uint32_t crc = 0;
  int rc = -1;
  const int numfiles = nf - 6;
  if (numfiles < 1) return -1;
  {
    const char *sat = strcmp(fld[2], "-") != 0 ? fld[2] : NULL,
               *index = strcmp(fld[4], "-") != 0 ? fld[4] : NULL,
               *out = strcmp(fld[5], "-") != 0 ? fld[5] : NULL;
    const int lossless = atoi(fld[3]);
    const char *const *paths = (const char *const *) (fld + 6);
    memset(&info, 0, sizeof info);
    if (strncmp(fld[1], "smap:", 5) == 0) {
      if (gtamd_alphabet_from_file(fld[1] + 5, &a, err, sizeof err) != 0) goto said;
      if (a.numofchars > 28) {         /* the tool's own limit, suffixerator_tool.c */
        gtamd_alphabet_free(&a);
        snprintf(err, sizeof err, "symbol map '%s' defines more than 28 letters", fld[1] + 5);
        goto said;
      }
    } else if (strcmp(fld[1], "dna") == 0 || strcmp(fld[1], "protein") == 0)
      gtamd_alphabet_standard(&a, fld[1][0] == 'p');
    else return -1;
    for (int f = 0; f < numfiles; f++) {
      const char *slash = strrchr(paths[f], '/');
      names[f] = slash != NULL ? slash + 1 : paths[f];
    }
    if (gtamd_encode_files_orig(paths, (size_t) numfiles, &a, &enc, &n, lossless ? &orig : NULL,
                                &desc, &desclen, &info, err, sizeof err) != 0) goto freea;
    crc = crc_more(0, enc, n);
    if (out != NULL && store(out, enc, n) != 0) {
      snprintf(err, sizeof err, "cannot write %s", out);
      goto freeall;
    }
    if (index != NULL) {
      if (lossless && gtamd_write_ois(index, enc, orig, n, &a, &info, err, sizeof err) != 0)
        goto freeall;
      if (gtamd_write_esq_alpha(index, names, (size_t) numfiles, enc, n, &a, &info, 1, sat, &ss,
                                err, sizeof err) != 0) goto freeall;
      if (gtamd_write_des_sds(index, desc, desclen, 1, 1) != 0) {
        snprintf(err, sizeof err, "cannot write description files of index '%s'", index);
        goto freeall;
      }
      if ((lossless ? gtamd_write_md5_orig(index, enc, orig, n)
                    : gtamd_write_md5_alpha(index, enc, n, &a)) != 0) {
        snprintf(err, sizeof err, "cannot write md5 file of index '%s'", index);
        goto freeall;
      }
    }
    rc = 0;
freeall:
    free(enc); free(orig); free(desc);
    gtamd_encinfo_free(&info);
freea:
    gtamd_alphabet_free(&a);
  }
said:
  report(rc, err, rc == 0 ? n : 0, rc == 0 ? crc : 0, "");
  return 0;
}

/* a project through the reader of project_host.c, the calls in a tool's order */
static int do_project(char **fld, int nf)
{
  gtamd_project prj;
  char err[2048] = "", more[64] = "";
  uint32_t crc = 0;
  uint64_t n = 0;
  int rc;
  if (nf != 7) return -1;
  memset(&prj, 0, sizeof prj);
  gtamd_project_close(&prj);                       /* (a zeroed value: nothing to release) */
  rc = gtamd_project_open(&prj, fld[1], fld[2], atoi(fld[3]), fld[4], err, sizeof err);
  for (const char *t = fld[6]; rc == 0 && *t != '-' && *t != '\0'; t++) {
    const char *at = strchr("slvb", *t);
    if (at == NULL) return -1;
    rc = gtamd_project_map(&prj, fld[1], (int) (at - "slvb"), atoi(fld[5]), err, sizeof err);
  }
  if (rc == 0 && gtamd_project_sequence_starts(&prj) != 0) return -1;
  if (rc == 0) {
    /* the starts with their sentinel, and the sequence of the last position */
    if (prj.seqstart[0] != 0 || prj.seqstart[prj.numseq] != prj.n + 1 ||
        (prj.n > 0 && gtamd_unit_of(prj.seqstart, prj.numseq, prj.n - 1) != prj.numseq - 1))
      return -1;
    n = prj.n;
    crc = crc_more(0, prj.enc, prj.n);
    snprintf(more, sizeof more, "%u\t%" PRIu64, (unsigned) prj.suf_bytes, prj.numseq);
  }
  gtamd_project_close(&prj);
  gtamd_project_close(&prj);
  report(rc, err, n, crc, more);
  return 0;
}

static int dispatch(char **fld, int nf)
{
  if (strcmp(fld[0], "project") == 0) return do_project(fld, nf);
  if (strcmp(fld[0], "base") == 0) return do_base(fld, nf);
  if (strcmp(fld[0], "mut") == 0) return do_mut(fld, nf);
  if (strcmp(fld[0], "cut") == 0) return do_cut(fld, nf);
  if (strcmp(fld[0], "read") == 0) return do_read(fld, nf);
  if (strcmp(fld[0], "encode") == 0) return do_encode(fld, nf);
  return -1;
}

static void cleanup(void)
{
  base_free();
  for (int f = 0; f < 2; f++)
    if (scratch_fd[f] >= 0) close(scratch_fd[f]);
}
#endif

#ifdef DRIVER_ORACLE
#include "esa_oracle.h"
#include "pck_oracle.h"

static int do_fasta(char **fld, int nf)
{
  uint8_t *enc = NULL;
  uint64_t n = 0;
  char err[1024] = "";
  int rc;
  if (nf != 3) return -1;
  rc = ora_encode_fasta(fld[2], atoi(fld[1]), &enc, &n, err, sizeof err);
  if (rc == 0) {
    report(0, "", n, crc_more(0, enc, n), "");
    free(enc);
  } else report(rc, err, 0, 0, "");
  return 0;
}

static uint64_t ipow(uint64_t b, unsigned e)
{
  uint64_t r = 1;
  while (e-- > 0) r *= b;
  return r;
}

static int do_tables(char **fld, int nf)
{
  unsigned char *enc = NULL;
  uint8_t *lcpb = NULL, *bwt = NULL, *bdx = NULL;
  uint64_t n = 0, *sa = NULL, *lcpw = NULL, *llv = NULL, pairs, codes, special, dist = 0,
           longest = 0, total = 0;
  uint32_t *lb = NULL, *cs = NULL, *dp = NULL, crc = 0;
  size_t bdxlen = 0;
  ora_pck_params pp;
  char more[512] = "";
  int rc = -1, prc;
  if (nf != 10 || load(fld[3], &enc, &n) != 0) return -1;
  {
    const unsigned sigma = (unsigned) atoi(fld[1]), k = (unsigned) atoi(fld[2]);
    const int locbitmap = atoi(fld[7]), sprank = atoi(fld[9]);
    pp.block_size = (unsigned) atoi(fld[4]);
    pp.bucket_blocks = (unsigned) atoi(fld[5]);
    pp.locate_interval = (unsigned) atoi(fld[6]);
    pp.with_statistics = atoi(fld[8]);
    pp.feature_toggles = ora_pck_default_toggles(pp.block_size, pp.bucket_blocks,
                                                 pp.locate_interval, locbitmap) |
                         (sprank ? ORA_PCK_REVERSIBLY_SORTED : 0);
    /* sections of INDEX.bck, src/match/bcktab.c:240-287 */
    codes = ipow(sigma, k);
    special = k >= 1 ? ipow(sigma, k - 1) : 1;
    for (unsigned i = 1; i + 1 < k; i++) dist += ipow(sigma, i);
    sa = malloc(8 * (n + 1)); lcpw = malloc(8 * (n + 1));
    lcpb = malloc(n + 1); bwt = malloc(n + 1);
    lb = calloc(codes + 1, 4); cs = calloc(special, 4); dp = calloc(dist ? dist : 1, 4);
    if (sa == NULL || lcpw == NULL || lcpb == NULL || bwt == NULL || lb == NULL || cs == NULL ||
        dp == NULL) goto done;
    ora_suffix_array(enc, n, sa);
    ora_lcp_kasai(enc, n, sa, lcpw);
    pairs = ora_lcp_to_bytes(lcpw, n + 1, lcpb, NULL);
    if ((llv = malloc(16 * (pairs ? pairs : 1))) == NULL) goto done;
    ora_lcp_to_bytes(lcpw, n + 1, lcpb, llv);
    ora_bwt(enc, n, sa, bwt);
    ora_bcktab(enc, n, sigma, k, lb, cs, dp);
    for (uint64_t i = 0; i <= n; i++)
      if (sa[i] == 0) longest = i;
    prc = ora_pck_bdx(bwt, sa, enc, n + 1, sigma, longest, &pp, &bdx, &bdxlen);
    if (prc != 0) {
      snprintf(more, sizeof more, "ora_pck_bdx: %d", prc);
      report(prc, more, 0, 0, "");
      rc = 0;
      goto done;
    }
    {
      const void *part[8] = {sa, lcpb, llv, bwt, lb, cs, dp, bdx};
      const uint64_t bytes[8] = {8 * (n + 1), n + 1, 16 * pairs, n + 1, 4 * (codes + 1),
                                 4 * special, 4 * dist, bdxlen};
      size_t at = 0;
      for (int p = 0; p < 8; p++) {
        crc = crc_more(crc, part[p], bytes[p]);
        total += bytes[p];
        at += (size_t) snprintf(more + at, sizeof more - at, "%s%" PRIu64 ":%08x", p ? "\t" : "",
                                bytes[p], (unsigned) crc_more(0, part[p], bytes[p]));
      }
    }
    report(0, "", total, crc, more);
    rc = 0;
  }
done:
  if (bdx != NULL) ora_pck_free(bdx);
  free(enc); free(sa); free(lcpw); free(lcpb); free(bwt); free(llv); free(lb); free(cs); free(dp);
  return rc;
}

static int dispatch(char **fld, int nf)
{
  if (strcmp(fld[0], "fasta") == 0) return do_fasta(fld, nf);
  if (strcmp(fld[0], "tables") == 0) return do_tables(fld, nf);
  return -1;
}

static void cleanup(void) {}
#endif

int main(int argc, char **argv)
{
  FILE *in;
  char *line = NULL;
  size_t cap = 0;
  ssize_t got;
  unsigned long lineno = 0;
  int status = 0;
  if (argc == 2 && strcmp(argv[1], "canary") == 0) return canary();
  if (argc != 3 || strcmp(argv[1], "run") != 0) {
    fprintf(stderr, "usage: %s canary | run WORKFILE\n", argv[0]);
    return 2;
  }
  /* a line per finished item, at once: what is missing tells where a run ended */
  setvbuf(stdout, NULL, _IOLBF, 0);
  in = strcmp(argv[2], "-") == 0 ? stdin : fopen(argv[2], "r");
  if (in == NULL) { fprintf(stderr, "cannot open %s\n", argv[2]); return 2; }
  while ((got = getline(&line, &cap, in)) > 0) {
    char *fld[MAXFIELDS];
    int nf = 0;
    lineno++;
    if (line[got - 1] == '\n') line[--got] = '\0';
    if (got == 0) continue;
    for (char *p = line; nf < MAXFIELDS; ) {
      char *tab = strchr(p, '\t');
      fld[nf++] = p;
      if (tab == NULL) break;
      *tab = '\0';
      p = tab + 1;
    }
    if (dispatch(fld, nf) != 0) {
      fprintf(stderr, "work item %lu (%s) cannot be run\n", lineno, fld[0]);
      status = 3;
      break;
    }
  }
  free(line);
  if (in != stdin) fclose(in);
  cleanup();
  return status;
}
