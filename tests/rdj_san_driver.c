/* Test driver (CPU, stand-alone): the host code of `gt readjoiner overlap`
   (genometools_amd/csrc/host/rdj_host.c) under AddressSanitizer and UBSan, as
   tests/test_rdjoverlap_host.py builds it -- the option parser and what it
   refuses, the readset reader up to the point where a device would be asked for,
   and the writer of Readjoiner's bin32 list.  No command line given to it reaches
   the device.

     rdj_san_driver tool ARGS...        gtamd_readjoiner_overlap(ARGS); prints
                                        "rc<TAB>message" as its last line
     rdj_san_driver list RECORDS OUT    RECORDS: lines `suffix_read prefix_read len
                                        flags`; writes the bin32 list OUT; prints
                                        "rc<TAB>message"
     rdj_san_driver canary              reads one byte past a heap block */
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
    rc = gtamd_readjoiner_overlap(argc - 1, (const char **) argv + 1, err, sizeof err);
    printf("%d\t%s\n", rc, err);
    return 0;
  }
  if (argc == 4 && !strcmp(argv[1], "list")) {
    gtamd_spmred_record *rec = malloc(sizeof *rec);
    uint64_t count = 0, cap = 1;
    unsigned long long a, b, c, d;
    FILE *in = fopen(argv[2], "r"), *out;
    if (in == NULL || rec == NULL) return 2;
    while (fscanf(in, "%llu %llu %llu %llu", &a, &b, &c, &d) == 4) {
      if (count == cap) {
        cap = 2 * cap;
        rec = realloc(rec, cap * sizeof *rec);
        if (rec == NULL) return 2;
      }
      rec[count].suffix_read = a; rec[count].prefix_read = b; rec[count].len = c; rec[count].flags = d;
      count++;
    }
    fclose(in);
    if ((out = fopen(argv[3], "wb")) == NULL) return 2;
    rc = gtamd_spmlist_bin32_header(out);
    /* in two calls, so that the second starts inside the list */
    if (rc == 0) rc = gtamd_spmlist_bin32_records(out, rec, count / 2, err, sizeof err);
    if (rc == 0) rc = gtamd_spmlist_bin32_records(out, rec + count / 2, count - count / 2, err, sizeof err);
    if (fclose(out) != 0) return 2;
    free(rec);
    printf("%d\t%s\n", rc, err);
    return 0;
  }
  return 2;
}
