/* Test driver (CPU, stand-alone): the host code of `gt-suffixerator-amd assembly`
   (genometools_amd/csrc/host/assembly_host.c) under AddressSanitizer and UBSan,
   as tests/test_assembly_host.py builds it -- the option parser and what it
   refuses, the reader of Readjoiner's bin32 list, the statistics block.  No
   command line given to it reaches the device.

     assembly_san_driver tool ARGS...        gtamd_assembly(ARGS); prints
                                             "rc<TAB>message" as its last line
     assembly_san_driver list PATH LEN...    the list PATH over reads of the
                                             lengths LEN...: a line `suffix_read
                                             prefix_read len flags` per record,
                                             then "rc<TAB>message"
     assembly_san_driver stats LEN...        the statistics block of the contig
                                             lengths, then "rc<TAB>"
     assembly_san_driver canary              reads one byte past a heap block */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "gtamd_host.h"

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
    rc = gtamd_assembly(argc - 1, (const char **) argv + 1, err, sizeof err);
    printf("%d\t%s\n", rc, err);
    return 0;
  }
  if (argc >= 3 && !strcmp(argv[1], "list")) {
    const uint64_t reads = (uint64_t) (argc - 3);
    uint32_t *len = malloc((reads ? reads : 1) * sizeof *len);
    gtamd_spmred_record *rec = NULL;
    uint64_t count = 0;
    if (len == NULL) return 2;
    for (uint64_t r = 0; r < reads; r++) len[r] = (uint32_t) strtoul(argv[3 + r], NULL, 10);
    rc = gtamd_spmlist_bin32_read(argv[2], len, reads, &rec, &count, err, sizeof err);
    for (uint64_t k = 0; k < count; k++)
      printf("%llu %llu %llu %llu\n", (unsigned long long) rec[k].suffix_read, (unsigned long long) rec[k].prefix_read,
             (unsigned long long) rec[k].len, (unsigned long long) rec[k].flags);
    free(rec);
    free(len);
    printf("%d\t%s\n", rc, err);
    return 0;
  }
  if (argc >= 2 && !strcmp(argv[1], "stats")) {
    const uint64_t count = (uint64_t) (argc - 2);
    uint64_t *len = malloc((count ? count : 1) * sizeof *len);
    char out[4096];
    if (len == NULL) return 2;
    for (uint64_t c = 0; c < count; c++) len[c] = strtoull(argv[2 + c], NULL, 10);
    rc = gtamd_assembly_statistics(len, count, out, sizeof out);
    if (rc == 0) fputs(out, stdout);
    /* an output that is too small is refused, not overrun */
    if (rc == 0 && gtamd_assembly_statistics(len, count, out, 40) != -1) rc = 3;
    free(len);
    printf("%d\t\n", rc);
    return 0;
  }
  fprintf(stderr, "usage: assembly_san_driver tool|list|stats|canary ...\n");
  return 2;
}
