/* repfind_host.c -- `gt repfind` for this path (tool src/tools/gt_repfind.c), as
   two sub-commands.  `repfind -l L -ii INDEX`: the maximal exact repeats of an
   index, from .suf and .lcp together, on the device through
   include/gtamd_maxpairs.h.  `querymatch`: what the reference computes with -q,
   -r or -p, the maximal exact matches of queries against an index, through
   include/gtamd_qmatch.h.  Option handling of src/tools/gt_repfind.c:224-470,
   output of an exact match as the reference displays it by default. */
#include "host_internal.h"
#include "gtamd_maxpairs.h"
#include "gtamd_qmatch.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

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
  unsigned long long minlen = 20;
  uint64_t capacity, cursor = 0, written = 0, total = 0;
  gtamd_project prj = { 0 };
  gtamd_maxpairs *mp = NULL;
  gtamd_maxpairs_info info;
  gtamd_maxpairs_record *rec = NULL;

  for (int i = 1; i < argc; i++) {
    const char *a = argv[i];
    if (!strcmp(a, "-ii")) { if (gtamd_opt_name(argc, argv, &i, &index, err, errlen) != 0) return -1; }
    else if (!strcmp(a, "-l")) {
      if (gtamd_opt_length(argc, argv, &i, 0xffffffffull, &minlen, err, errlen) != 0) return -1;
    } else if (!strcmp(a, "-f") || !strcmp(a, "-scan")) {
      if (!gtamd_opt_yesno(argc, argv, &i) && a[1] == 'f')
        return gtamd_fail(err, errlen, "option \"%s no\" leaves nothing to compute: forward repeats are all "
                          "the MI355X engine enumerates", a);
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
    } else if (!strncmp(a, "-extend", 7)) return gtamd_opt_unsupported(a, err, errlen);
    else return gtamd_opt_tail(a, refused, GTAMD_UNKNOWN_TRY, GTAMD_SUPERFLUOUS_MORE, err, errlen);
  }
  if (index == NULL) return gtamd_fail(err, errlen, "option \"-%s\" is mandatory", "ii");

  if (gtamd_project_open(&prj, index, "searched", GTAMD_PROJECT_FORWARD_TWO, "repfind", err, errlen) != 0 ||
      gtamd_project_map(&prj, index, GTAMD_TABLE_SUF, 1, err, errlen) != 0 ||
      gtamd_project_map(&prj, index, GTAMD_TABLE_LCP, 1, err, errlen) != 0 ||
      gtamd_project_map(&prj, index, GTAMD_TABLE_LLV, 1, err, errlen) != 0)
    goto done;
  /* where the sequences start: behind the separators (INDEX.ssp, as the reader of
     INDEX.esq has put them into the symbols) */
  if (gtamd_project_sequence_starts(&prj) != 0) {
    gtamd_fail(err, errlen, "out of memory (%s)", "sequence starts");
    goto done;
  }

  if ((mp = gtamd_maxpairs_create(0)) == NULL ||
      gtamd_maxpairs_set_index_host(mp, prj.enc, prj.n, prj.suf.p, prj.suf_bytes, prj.lcp.p, prj.llv.p,
                                    prj.llv.bytes / 16) != 0 ||
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
  if (rec == NULL) { gtamd_fail(err, errlen, "out of memory (%s)", "records"); goto done; }
  do {
    if (gtamd_maxpairs_emit(mp, &cursor, rec, capacity, 0, &written) != 0) {
      snprintf(err, errlen, "%s", gtamd_esa_last_error());
      goto done;
    }
    for (uint64_t k = 0; k < written; k++) {
      const uint64_t s1 = gtamd_unit_of(prj.seqstart, prj.numseq, rec[k].pos1),
                     s2 = gtamd_unit_of(prj.seqstart, prj.numseq, rec[k].pos2);
      printf("%llu %llu %llu F %llu %llu %llu\n", (unsigned long long) rec[k].len, (unsigned long long) s1,
             (unsigned long long) (rec[k].pos1 - prj.seqstart[s1]), (unsigned long long) rec[k].len,
             (unsigned long long) s2, (unsigned long long) (rec[k].pos2 - prj.seqstart[s2]));
    }
    total += written;
  } while (written != 0);
  if (total != info.pairs) {
    snprintf(err, errlen, "%llu pairs counted, %llu given", (unsigned long long) info.pairs,
             (unsigned long long) total);
    goto done;
  }
  if (fflush(stdout) != 0) { gtamd_fail(err, errlen, "cannot write to %s", "stdout"); goto done; }
  rc = 0;
done:
  gtamd_maxpairs_destroy(mp);
  gtamd_project_close(&prj);
  free(rec);
  return rc;
}

/* ---- gt repfind -q / -r / -p ----
   The calls the reference sends to gt_callenumquerymatches
   (gt_repfind.c:562-757); display and the `ordered` filter of
   src/match/querymatch.c:202-213, 357-369. */

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
  int mode_on[3] = { 0, 0, 0 }, f_given = 0, verbose = 0, rc = -1;
  unsigned long long minlen = 20;
  uint8_t *query_own = NULL, *tq = NULL;
  const uint8_t *query;
  uint64_t m = 0, numunits = 0, *unitstart = NULL, desclen = 0;
  char *desc = NULL;
  gtamd_project prj = { 0 };
  gtamd_qmatch *qm = NULL;
  gtamd_qmatch_info info;
  gtamd_qmatch_record *rec = NULL;

  for (int i = 1; i < argc; i++) {
    const char *a = argv[i];
    if (!strcmp(a, "-ii")) { if (gtamd_opt_name(argc, argv, &i, &index, err, errlen) != 0) return -1; }
    else if (!strcmp(a, "-l")) {
      if (gtamd_opt_length(argc, argv, &i, 0xffffffffull, &minlen, err, errlen) != 0) return -1;
    } else if (!strcmp(a, "-f") || !strcmp(a, "-r") || !strcmp(a, "-p")) {
      const int k = a[1] == 'f' ? 0 : a[1] == 'r' ? 1 : 2;
      mode_on[k] = gtamd_opt_yesno(argc, argv, &i);
      if (k == 0) f_given = 1;
    } else if (!strcmp(a, "-q")) {
      if (gtamd_opt_files(argc, argv, &i, &queries, &numqueries, err, errlen) != 0) return -1;
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
    } else if (!strncmp(a, "-extend", 7)) return gtamd_opt_unsupported(a, err, errlen);
    else return gtamd_opt_tail(a, refused, GTAMD_UNKNOWN_TRY, GTAMD_SUPERFLUOUS_MORE, err, errlen);
  }
  if (index == NULL) return gtamd_fail(err, errlen, "option \"-%s\" is mandatory", "ii");
  /* gt_repfind_arguments_check: forward unless -r or -p is given without -f */
  if (!f_given) mode_on[0] = !(mode_on[1] || mode_on[2]);
  if (queries == NULL && mode_on[0])
    return gtamd_fail(err, errlen, "forward matches of the index with itself are its maximal repeats: use the "
                      "%s sub-command for them (querymatch takes -q FILE..., -r or -p)", "repfind");
  if (!(mode_on[0] || mode_on[1] || mode_on[2]))
    return gtamd_fail(err, errlen, "none of the options -f, -r and -p is %s", "set");

  if (gtamd_project_open(&prj, index, "searched", GTAMD_PROJECT_FORWARD_TWO, "querymatch", err, errlen) != 0)
    goto done;
  if (mode_on[2] && !gtamd_alphabet_is_dna(&prj.alpha)) {
    gtamd_fail(err, errlen, "option \"%s\" needs a DNA alphabet: the index has none, and its letters have no "
               "complement", "-p");
    goto done;
  }
  if (gtamd_project_map(&prj, index, GTAMD_TABLE_SUF, 1, err, errlen) != 0) goto done;
  /* the queries, with the index's alphabet: one sequence of symbols, a separator
     between two units; without -q the index's own */
  query = prj.enc;
  m = prj.n;
  if (queries != NULL) {
    if (gtamd_encode_files_alpha(queries, numqueries, &prj.alpha, &query_own, &m, &desc, &desclen, NULL, err,
                                 errlen) != 0)
      goto done;
    query = query_own;
  }
  unitstart = gtamd_sequence_starts(query, m, &numunits);
  tq = malloc(m ? m : 1);
  rec = malloc(QUERYMATCH_CAPACITY * sizeof *rec);
  if (gtamd_project_sequence_starts(&prj) != 0 || unitstart == NULL || tq == NULL || rec == NULL) {
    gtamd_fail(err, errlen, "out of memory (%s)", "queries and records");
    goto done;
  }
  if ((qm = gtamd_qmatch_create(0)) == NULL ||
      gtamd_qmatch_set_index_host(qm, prj.enc, prj.n, prj.suf.p, prj.suf_bytes) != 0) {
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
          const uint64_t unit = gtamd_unit_of(unitstart, numunits, qpos), offset = qpos - unitstart[unit];
          const uint64_t unitlen = unitstart[unit + 1] - 1 - unitstart[unit];
          const uint64_t dbseq = gtamd_unit_of(prj.seqstart, prj.numseq, rec[k].dbpos),
                         dbrel = rec[k].dbpos - prj.seqstart[dbseq];
          /* gt_querymatch_position_convert: the start on the forward strand */
          const uint64_t qfwd = mode == 0 ? offset : unitlen - offset - reclen;
          /* gt_querymatch_ordered: of the two records of one pair, the one whose
             subject side comes first */
          if (queries == NULL && !(dbseq < unit || (dbseq == unit && dbrel < qfwd + (mode != 0)))) continue;
          printf("%llu %llu %llu %c %llu %llu %llu\n", (unsigned long long) reclen, (unsigned long long) dbseq,
                 (unsigned long long) dbrel, modechar[mode], (unsigned long long) reclen,
                 (unsigned long long) unit, (unsigned long long) qfwd);
        }
      } while (written != 0);
    }
  }
  if (fflush(stdout) != 0) { gtamd_fail(err, errlen, "cannot write to %s", "stdout"); goto done; }
  rc = 0;
done:
  gtamd_qmatch_destroy(qm);
  gtamd_project_close(&prj);
  free(rec); free(tq); free(unitstart); free(desc); free(query_own);
  return rc;
}
