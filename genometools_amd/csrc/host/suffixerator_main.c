/* gt-suffixerator-amd: command line entry, behaves like `gt suffixerator`
   (exit code 1 and "gt suffixerator: error: ..." on stderr, src/gt.c:48-52);
   `gt-suffixerator-amd mergeesa ...` is `gt dev mergeesa ...`,
   `gt-suffixerator-amd packedindex mkindex|trsuftab ...` is `gt packedindex ...`,
   `gt-suffixerator-amd sfxmap ...` is `gt dev sfxmap ...`,
   `gt-suffixerator-amd matstat|uniquesub ...` is `gt matstat|uniquesub ...`,
   `gt-suffixerator-amd repfind ...` is `gt repfind ...`,
   `gt-suffixerator-amd querymatch ...` is `gt repfind ...` with -q, -r or -p,
   `gt-suffixerator-amd encseq2spm ...` is `gt encseq2spm ...`,
   `gt-suffixerator-amd readjoiner overlap ...` is `gt readjoiner overlap ...`,
   `gt-suffixerator-amd readjoiner prefilter ...` is `gt readjoiner prefilter ...`,
   `gt-suffixerator-amd readjoiner correct ...` is `gt readjoiner correct ...`,
   `gt-suffixerator-amd assembly ...` is `gt readjoiner assembly ...` with default options,
   `gt-suffixerator-amd tagerator ...` is `gt tagerator ...`,
   `gt-suffixerator-amd idxlocali ...` is `gt dev idxlocali ...` */
#include <stdio.h>
#include <string.h>
#include "gtamd_host.h"

int main(int argc, char **argv)
{
  char err[2048] = "";
  if (argc > 1 && !strcmp(argv[1], "mergeesa")) {
    if (gtamd_mergeesa(argc - 1, (const char **) argv + 1, err, sizeof err) != 0) {
      fprintf(stderr, "gt dev mergeesa: error: %s\n", err);
      return 1;
    }
    return 0;
  }
  if (argc > 1 && !strcmp(argv[1], "sfxmap")) {
    if (gtamd_sfxmap(argc - 1, (const char **) argv + 1, err, sizeof err) != 0) {
      fprintf(stderr, "gt dev sfxmap: error: %s\n", err);
      return 1;
    }
    return 0;
  }
  if (argc > 1 && (!strcmp(argv[1], "matstat") || !strcmp(argv[1], "uniquesub"))) {
    if ((argv[1][0] == 'm' ? gtamd_matstat : gtamd_uniquesub)(argc - 1, (const char **) argv + 1, err,
                                                             sizeof err) != 0) {
      fprintf(stderr, "gt %s: error: %s\n", argv[1], err);
      return 1;
    }
    return 0;
  }
  if (argc > 1 && !strcmp(argv[1], "repfind")) {
    if (gtamd_repfind(argc - 1, (const char **) argv + 1, err, sizeof err) != 0) {
      fprintf(stderr, "gt repfind: error: %s\n", err);
      return 1;
    }
    return 0;
  }
  if (argc > 1 && !strcmp(argv[1], "querymatch")) {
    if (gtamd_querymatch(argc - 1, (const char **) argv + 1, err, sizeof err) != 0) {
      fprintf(stderr, "gt repfind: error: %s\n", err);
      return 1;
    }
    return 0;
  }
  if (argc > 1 && !strcmp(argv[1], "encseq2spm")) {
    if (gtamd_encseq2spm(argc - 1, (const char **) argv + 1, err, sizeof err) != 0) {
      fprintf(stderr, "gt encseq2spm: error: %s\n", err);
      return 1;
    }
    return 0;
  }
  if (argc > 1 && !strcmp(argv[1], "assembly")) {
    if (gtamd_assembly(argc - 1, (const char **) argv + 1, err, sizeof err) != 0) {
      fprintf(stderr, "gt readjoiner assembly: error: %s\n", err);
      return 1;
    }
    return 0;
  }
  /* (a bare `readjoiner prefilter`, without an option, is answered below as it always was) */
  if (argc > 3 && !strcmp(argv[1], "readjoiner") && !strcmp(argv[2], "prefilter")) {
    if (gtamd_readjoiner_prefilter(argc - 2, (const char **) argv + 2, err, sizeof err) != 0) {
      fprintf(stderr, "gt readjoiner prefilter: error: %s\n", err);
      return 1;
    }
    return 0;
  }
  if (argc > 3 && !strcmp(argv[1], "readjoiner") && !strcmp(argv[2], "correct")) {
    if (gtamd_readjoiner_correct(argc - 2, (const char **) argv + 2, err, sizeof err) != 0) {
      fprintf(stderr, "gt readjoiner correct: error: %s\n", err);
      return 1;
    }
    return 0;
  }
  if (argc > 1 && !strcmp(argv[1], "readjoiner")) {
    if (argc < 3 || strcmp(argv[2], "overlap")) {
      fprintf(stderr, "gt readjoiner: error: tool overlap expected\n");
      return 1;
    }
    if (gtamd_readjoiner_overlap(argc - 2, (const char **) argv + 2, err, sizeof err) != 0) {
      fprintf(stderr, "gt readjoiner overlap: error: %s\n", err);
      return 1;
    }
    return 0;
  }
  if (argc > 1 && !strcmp(argv[1], "tagerator")) {
    if (gtamd_tagerator(argc - 1, (const char **) argv + 1, err, sizeof err) != 0) {
      fprintf(stderr, "gt tagerator: error: %s\n", err);
      return 1;
    }
    return 0;
  }
  if (argc > 1 && !strcmp(argv[1], "idxlocali")) {
    if (gtamd_idxlocali(argc - 1, (const char **) argv + 1, err, sizeof err) != 0) {
      fprintf(stderr, "gt dev idxlocali: error: %s\n", err);
      return 1;
    }
    return 0;
  }
  if (argc > 1 && !strcmp(argv[1], "packedindex")) {
    if (argc > 2 && !strcmp(argv[2], "mkindex")) {
      if (gtamd_packedindex_mkindex(argc - 2, (const char **) argv + 2, err, sizeof err) != 0) {
        fprintf(stderr, "gt packedindex mkindex: error: %s\n", err);
        return 1;
      }
      return 0;
    }
    if (argc > 2 && !strcmp(argv[2], "mkctxmap")) {
      if (gtamd_packedindex_mkctxmap(argc - 2, (const char **) argv + 2, err, sizeof err) != 0) {
        fprintf(stderr, "gt packedindex mkctxmap: error: %s\n", err);
        return 1;
      }
      return 0;
    }
    if (argc < 3 || strcmp(argv[2], "trsuftab")) {
      fprintf(stderr, "gt packedindex: error: tool mkindex, trsuftab or mkctxmap expected\n");
      return 1;
    }
    if (gtamd_packedindex_trsuftab(argc - 2, (const char **) argv + 2, err, sizeof err) != 0) {
      fprintf(stderr, "gt packedindex trsuftab: error: %s\n", err);
      return 1;
    }
    return 0;
  }
  if (gtamd_suffixerator(argc, (const char **) argv, err, sizeof err) != 0) {
    fprintf(stderr, "gt suffixerator: error: %s\n", err);
    return 1;
  }
  return 0;
}
