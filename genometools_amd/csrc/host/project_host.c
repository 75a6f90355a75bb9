/* project_host.c -- what a tool reads back of an index written here or by
   GenomeTools: INDEX.prj (src/match/esa-scanprj.c), the sequence of INDEX.esq /
   .ssp as the tables see it, and the tables .suf / .lcp / .llv / .bwt, mapped,
   not read: an upload takes them piece by piece, as the writer streamed them.
   Every check of a file's size and its message is here once; each tool calls
   the pieces in the order in which it reports their errors.  Declared in
   host_internal.h.  Nothing here calls the engine. */
#include "host_internal.h"
#include <errno.h>
#include <fcntl.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

int gtamd_prj_value(const char *path, const char *key, unsigned long long *value)
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

/* the sequence of an accepted project; the alphabet stays in p */
static int load_sequence(gtamd_project *p, const char *index, const char *verb, char *err, size_t errlen)
{
  char path[4096];
  unsigned long long totallength = 0, sorted = 0, readmode = 0, mirrored = 0;
  gtamd_seqstats ss;

  snprintf(path, sizeof path, "%s.prj", index);
  {
    FILE *fp = fopen(path, "r");
    if (fp == NULL) return gtamd_fail(err, errlen, "cannot open file '%s'", path);
    fclose(fp);
  }
  if (gtamd_prj_value(path, "totallength", &totallength) != 0 ||
      gtamd_prj_value(path, "numberofallsortedsuffixes", &sorted) != 0)
    return gtamd_fail(err, errlen, "cannot read totallength / numberofallsortedsuffixes from file '%s'", path);
  (void) gtamd_prj_value(path, "readmode", &readmode);
  (void) gtamd_prj_value(path, "mirrored", &mirrored);
  if (sorted == 0 && totallength != 0)
    return gtamd_fail(err, errlen, "file '%s' describes the project of a packed index "
                      "(numberofallsortedsuffixes=0): it has no tables to check", path);
  if (totallength + 1 > GTAMD_MAX_ENTRIES)
    return gtamd_failf(err, errlen, "sequence of %llu symbols is beyond the limit of a single build (%llu table "
                       "entries); the slices of a build in parts are not %s", totallength, GTAMD_MAX_ENTRIES, verb);
  if (sorted != totallength + 1 || readmode > 3)
    return gtamd_fail(err, errlen, "file '%s' does not describe whole tables (numberofallsortedsuffixes "
                      "is not totallength + 1, or the read mode is unknown)", path);

  /* as stored, then -mirrored, then -dir */
  if (gtamd_read_esq_alpha(index, &p->enc, &p->n, &p->alpha, &ss, err, errlen) != 0) return -1;
  p->have_alpha = 1;
  if (!gtamd_alphabet_is_dna(&p->alpha) && (readmode >= 2 || mirrored))
    return gtamd_fail(err, errlen, "file '%s' asks for complemented symbols of an alphabet that is not DNA", path);
  if (mirrored) {
    uint8_t *m = gtamd_mirror(p->enc, p->n);
    if (m == NULL) return gtamd_fail(err, errlen, "out of memory (%s)", "-mirrored");
    free(p->enc);
    p->enc = m;
    p->n = 2 * p->n + 1;
  }
  gtamd_apply_readmode(p->enc, p->n, (int) readmode);
  if (p->n != totallength)
    return gtamd_fail(err, errlen, "INDEX.esq and INDEX.prj of '%s' disagree on the total length", index);
  return 0;
}

int gtamd_project_open(gtamd_project *p, const char *index, const char *verb, int which, const char *tool,
                       char *err, size_t errlen)
{
  if (which != GTAMD_PROJECT_ANY) {
    char path[4096];
    unsigned long long readmode = 0, mirrored = 0;
    snprintf(path, sizeof path, "%s.prj", index);
    (void) gtamd_prj_value(path, "readmode", &readmode);
    (void) gtamd_prj_value(path, "mirrored", &mirrored);
    if (which == GTAMD_PROJECT_FORWARD && (readmode != 0 || mirrored))
      return gtamd_failf(err, errlen, "file '%s' describes a mirrored index or one of a read mode other than "
                         "forward: such an index is not supported by the MI355X engine's %s", path, tool);
    if (readmode != 0)
      return gtamd_failf(err, errlen, "file '%s' gives a read mode other than forward: such an index is not "
                         "supported by the MI355X engine's %s", path, tool);
    if (mirrored)
      return gtamd_failf(err, errlen, "file '%s' describes a mirrored index: such an index is not supported by "
                         "the MI355X engine's %s", path, tool);
  }
  return load_sequence(p, index, verb, err, errlen);
}

/* 0, -1 cannot open, -2 cannot map */
static int map_file(const char *path, gtamd_mapped *m)
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

static void unmap_file(gtamd_mapped *m)
{
  if (m->p != NULL) munmap(m->p, m->bytes);
  m->p = NULL;
}

int gtamd_project_map(gtamd_project *p, const char *index, int table, int required, char *err, size_t errlen)
{
  static const char *const suffix[] = { ".suf", ".lcp", ".llv", ".bwt" };
  gtamd_mapped *const m = table == GTAMD_TABLE_SUF ? &p->suf : table == GTAMD_TABLE_LCP ? &p->lcp :
                          table == GTAMD_TABLE_LLV ? &p->llv : &p->bwt;
  const unsigned long long N = p->n + 1;
  char path[4096];
  snprintf(path, sizeof path, "%s%s", index, suffix[table]);
  if (required && access(path, R_OK) != 0)
    return gtamd_failf(err, errlen, "cannot open file \"%s\": %s", path, strerror(errno));
  unmap_file(m);
  switch (map_file(path, m)) {
    case 0: break;
    case -1: return gtamd_fail(err, errlen, "cannot open file '%s'", path);
    default: return gtamd_fail(err, errlen, "cannot map file '%s'", path);
  }
  switch (table) {
    case GTAMD_TABLE_SUF:
      p->suf_bytes = m->bytes == 4 * N ? 4 : 8;
      if (m->bytes != 4 * N && m->bytes != 8 * N)
        return gtamd_failf(err, errlen, "file '%s' has %llu bytes, %llu (-suftabuint) or %llu expected for %llu "
                           "entries", path, (unsigned long long) m->bytes, 4 * N, 8 * N, N);
      return 0;
    case GTAMD_TABLE_LLV:
      if (m->bytes % 16 != 0)
        return gtamd_failf(err, errlen, "file '%s' has %llu bytes, not a multiple of 16 (pairs of two 64-bit "
                           "numbers)", path, (unsigned long long) m->bytes);
      return 0;
    default:                              /* a byte an entry */
      if (m->bytes != N)
        return gtamd_failf(err, errlen, "file '%s' has %llu bytes, %llu expected", path,
                           (unsigned long long) m->bytes, N);
      return 0;
  }
}

uint64_t *gtamd_sequence_starts(const uint8_t *seq, uint64_t len, uint64_t *num)
{
  uint64_t count = 1, *start;
  for (uint64_t p = 0; p < len; p++) count += seq[p] == 255;
  start = malloc((count + 1) * sizeof *start);
  if (start == NULL) return NULL;
  start[0] = 0;
  for (uint64_t p = 0, k = 1; p < len; p++)
    if (seq[p] == 255) start[k++] = p + 1;
  start[count] = len + 1;
  *num = count;
  return start;
}

uint64_t gtamd_unit_of(const uint64_t *start, uint64_t numstart, uint64_t pos)
{
  uint64_t lo = 0, hi = numstart;
  while (hi - lo > 1) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (start[mid] <= pos) lo = mid; else hi = mid;
  }
  return lo;
}

int gtamd_project_sequence_starts(gtamd_project *p)
{
  if (p->seqstart == NULL) p->seqstart = gtamd_sequence_starts(p->enc, p->n, &p->numseq);
  return p->seqstart != NULL ? 0 : -1;
}

void gtamd_project_close(gtamd_project *p)
{
  unmap_file(&p->suf); unmap_file(&p->lcp); unmap_file(&p->llv); unmap_file(&p->bwt);
  if (p->have_alpha) gtamd_alphabet_free(&p->alpha);
  free(p->seqstart); free(p->enc);
  memset(p, 0, sizeof *p);
}
