/* Test driver (CPU, stand-alone): the host code of `gt-suffixerator-amd readjoiner
   correct` (genometools_amd/csrc/host/correct_host.c, and the section walk of
   esq_host.c) under AddressSanitizer and UBSan, as tests/test_correct_host.py
   builds it -- the option parser and what it refuses, and the in-place patch of
   an INDEX.esq.  No command line given to it reaches the device.

     correct_san_driver tool ARGS...             gtamd_readjoiner_correct(ARGS);
                                                 prints "rc<TAB>message"
     correct_san_driver patch INDEX POS:LETTER...   the edits, in order, into
                                                 INDEX.esq; "rc<TAB>message"
     correct_san_driver canary                   reads one byte past a heap block */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "gtamd_host.h"
#include "host_internal.h"

int main(int argc, char **argv)
{
  char err[2048] = "";
  int rc = 0;
  if (argc >= 2 && !strcmp(argv[1], "canary")) {
    volatile size_t n = 8;                 /* (a size the compiler does not see through) */
    char *p = malloc(n);
    printf("canary %d survived\n", p[n]);
    free(p);
    return 0;
  }
  if (argc >= 2 && !strcmp(argv[1], "tool")) {
    rc = gtamd_readjoiner_correct(argc - 1, (const char **) argv + 1, err, sizeof err);
    printf("%d\t%s\n", rc, err);
    return 0;
  }
  if (argc >= 3 && !strcmp(argv[1], "patch")) {
    const uint64_t count = (uint64_t) (argc - 3);
    uint64_t *pos = malloc((count ? count : 1) * sizeof *pos);
    uint8_t *letter = malloc(count ? count : 1);
    if (pos == NULL || letter == NULL) return 2;
    for (uint64_t r = 0; r < count; r++) {
      char *end;
      pos[r] = strtoull(argv[3 + r], &end, 10);
      letter[r] = (uint8_t) (*end == ':' ? strtoul(end + 1, NULL, 10) : 255);
    }
    rc = gtamd_correct_patch_esq(argv[2], pos, letter, count, err, sizeof err);
    free(pos);
    free(letter);
    printf("%d\t%s\n", rc, err);
    return 0;
  }
  fprintf(stderr, "usage: correct_san_driver tool|patch|canary ...\n");
  return 2;
}
