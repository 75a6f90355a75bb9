/* host_internal.h -- shared between the files of the host layer, not part of
   the public interface */
#ifndef GTAMD_HOST_INTERNAL_H
#define GTAMD_HOST_INTERNAL_H
#include "gtamd_host.h"
#include "gtamd_encode.h"

/* GtEncseqAccessType, src/core/encseq_access_type.h:24-34 */
enum {
  GTAMD_SAT_DIRECTACCESS = 0, GTAMD_SAT_BYTECOMPRESS, GTAMD_SAT_EQUALLENGTH,
  GTAMD_SAT_BITACCESS, GTAMD_SAT_UCHARTABLES, GTAMD_SAT_USHORTTABLES,
  GTAMD_SAT_UINT32TABLES
};

typedef struct {
  gtamd_seqstats ss;
  uint64_t lengthoflongestnonspecial, minseqlen, maxseqlen;
  uint64_t chardist[32];          /* occurrences of every non-special code */
  int equallength;                /* all sequences equally long, no wildcard */
  uint64_t equallength_value;
  int sat;                        /* access type the reference would choose */
  uint64_t sat_wildcardranges;    /* stored wildcard ranges for that type */
  uint64_t sp_tab[3], wc_tab[3];  /* stored ranges per table width */
} gtamd_seqanalysis;

void gtamd_analyse_sequence(const uint8_t *enc, uint64_t n, uint32_t numofchars,
                            gtamd_seqanalysis *an);

/* the sections of INDEX.esq / INDEX.ssp behind the header, whichever the access
   type needs (gtamd_esq_needs): packed symbols, special bits, maximal
   wildcard runs, separator positions */
typedef struct {
  const uint64_t *twobit, *specialbits;
  const uint8_t *packed;
  const uint8_t *plain;           /* direct access: the symbols themselves */
  const uint64_t *wc_start, *wc_len;
  uint64_t wc_runs;
  const uint64_t *seppos;
} gtamd_esq_sections;

void gtamd_esq_needs(const gtamd_seqanalysis *an, int write_ssp, int *twobit,
                     int *specialbits, int *packed, int *wildcardruns,
                     int *separators);   /* direct access: none of the first three */
/* code that stands in for specials in the two-bit encoding of the equal-length
   and table access types (src/core/encseq.c:4468-4485) */
unsigned gtamd_least_probable(const gtamd_seqanalysis *an);
int gtamd_write_esq_sections(const char *indexname, const char *const *paths,
                             size_t numfiles, const gtamd_alphabet *a,
                             const gtamd_seqanalysis *an, const gtamd_encinfo *info,
                             int write_ssp, const gtamd_esq_sections *sec,
                             char *err, size_t errlen);

/* FASTQ: what the file length table needs of every record, and the table as the
   reference's FASTQ reader books it (encseq_host.c) */
typedef struct { uint64_t seqlen, desclen; size_t file; } gtamd_fastq_record;
void gtamd_fastq_filelengths(const gtamd_fastq_record *rec, size_t nrec, size_t lastfile,
                             gtamd_filelength *tab);

/* one input file, whole, decompressed when its name ends in ".gz"; 0 or a code
   for gtamd_read_input_error */
int gtamd_read_input_file(const char *path, uint8_t **data, uint64_t *len);
void gtamd_read_input_error(int code, const char *path, char *err, size_t errlen);

/* symbol map of the DNA / protein alphabet; 253 marks undefined characters */
void gtamd_symbolmap(uint8_t map[256], int protein);

/* stored-range counts and access type from the range counts per table width;
   needs ss.totallength/numofsequences/numofchars and equallength set */
int gtamd_choose_access_type(gtamd_seqanalysis *an, const uint64_t sp_tab[3],
                             const uint64_t wc_tab[3], int forced_sat);
/* -sat NAME -> access type number; the alphabet-dependent checks and messages
   of src/core/encseq.c:797-807, encseq_access_type.c:163-221 */
int gtamd_parse_sat(const char *name, int notdna, int *sat, char *err, size_t errlen);
/* apply a forced access type (-sat) to a finished analysis; -1 with the
   reference's message when "eqlen" does not fit the sequences */
int gtamd_force_sat(gtamd_seqanalysis *an, const char *satname, int notdna, char *err,
                    size_t errlen);
/* the same analysis from the device encoder's summary */
void gtamd_analysis_from_summary(const gtamd_encode_summary *s, uint32_t numofchars,
                                 gtamd_seqanalysis *an);

/* bytes of a range table of the given width (0 uchar, 1 ushort, 2 uint32),
   src/core/encseq.c:924-949 */
uint64_t gtamd_swtable_bytes(int width_kind, int withrangelengths, uint64_t n,
                             uint64_t items);

/* ---- prefilter_host.c: what `readjoiner prefilter` writes, from figures and
   symbols in host memory; nothing here calls the engine ---- */

/* an input file of `readjoiner prefilter`: its bytes, its reads with a wildcard
   and their symbols, the reads that are left and their letters */
typedef struct {
  uint64_t filesize, invalid_reads, invalid_letters, kept_reads, kept_letters;
} gtamd_prefilter_file;
/* The file table of X.esq as the reference computes it (src/match/reads2twobit.c:
   852-892, 1460-1482): the raw length is the file's without the symbols of its
   reads with a wildcard and three bytes for each of them, the effective length
   the letters of the reads that are left with a separator between two. */
void gtamd_prefilter_filetable(const gtamd_prefilter_file *f, size_t numfiles, gtamd_filelength *tab);
/* X.esq (and X.ssp where the access type has one) of the n kept symbols, with that
   table and the original file names */
int gtamd_prefilter_write_readset(const char *readset, const char *const *paths, size_t numfiles,
                                  const gtamd_prefilter_file *f, const uint8_t *kept, uint64_t n, char *err,
                                  size_t errlen);
/* X.cnt, Readjoiner's list of contained reads in its bit format
   (src/match/rdj-cntlist.c:49-58): removed[k] != 0 for read k of `reads` */
int gtamd_prefilter_write_cntlist(const char *path, const uint8_t *removed, uint64_t reads, char *err,
                                  size_t errlen);

/* ---- correct_host.c, esq_host.c: what `readjoiner correct` rewrites; nothing
   here calls the engine ---- */

/* The sections of the bytes of an INDEX.esq that an edit touches: the access
   type, the symbols, the offset of the character distribution with its entries
   and the offset of the 2-bit words.  -1 for bytes that are no such file. */
int gtamd_esq_locate(const uint8_t *data, uint64_t len, uint64_t *sat, uint64_t *n, uint64_t *chardist_off,
                     uint64_t *numofchars, uint64_t *twobit_off);
/* INDEX.esq edited IN PLACE as gt_twobitenc_editor_edit does it
   (src/match/rdj-twobitenc-editor.c:75-96), record by record in the order given:
   letters[r] (0..3) at positions[r].  Only the 2-bit words of those positions
   and the character distribution are written.  The distribution is kept as the
   reference keeps it: the letter an edit replaces is taken off its count only at
   the last four positions of a 2-bit word, elsewhere the count of letter 0 goes
   down (the reference casts the masked word to a byte before it shifts it).  A
   file whose access type is not the equal-length one is refused with the
   reference's sentence, and nothing is written. */
int gtamd_correct_patch_esq(const char *indexname, const uint64_t *positions, const uint8_t *letters,
                            uint64_t count, char *err, size_t errlen);

/* What follows is shared between the tools of this directory and stays inside
   libgtamd_host.so. */
#define GTAMD_INTERNAL __attribute__((visibility("hidden")))

/* acgt as codes 0..3 and nothing else: the alphabet whose letters have a
   complement (alphabet_host.c) */
GTAMD_INTERNAL int gtamd_alphabet_is_dna(const gtamd_alphabet *a);

/* ---- cli_host.c: the pieces of an option parser ---- */

/* -1, with msg (one %s at most, filled from arg) or a format in err */
GTAMD_INTERNAL int gtamd_fail(char *err, size_t errlen, const char *msg, const char *arg);
GTAMD_INTERNAL int gtamd_failf(char *err, size_t errlen, const char *fmt, ...)
  __attribute__((format(printf, 3, 4)));

/* The argument(s) of option argv[*i]; *i moves to the last one taken.  0, or -1
   with the message of the reference's parser. */
GTAMD_INTERNAL int gtamd_opt_name(int argc, const char **argv, int *i, const char **name, char *err,
                                  size_t errlen);
GTAMD_INTERNAL int gtamd_opt_uint32(int argc, const char **argv, int *i, uint32_t *out, char *err,
                                    size_t errlen);
/* a length: 1 .. max */
GTAMD_INTERNAL int gtamd_opt_length(int argc, const char **argv, int *i, unsigned long long max,
                                    unsigned long long *out, char *err, size_t errlen);
/* file names up to the next option, one at least */
GTAMD_INTERNAL int gtamd_opt_files(int argc, const char **argv, int *i, const char *const **files,
                                   size_t *numfiles, char *err, size_t errlen);
/* a switch: on, unless "no" follows (yes|no) or "no" / "false" (yes|true|no|false) */
GTAMD_INTERNAL int gtamd_opt_yesno(int argc, const char **argv, int *i);
GTAMD_INTERNAL int gtamd_opt_switch(int argc, const char **argv, int *i);

/* The end of a parser loop, for an argument `a` no clause has taken: -1 with
   "is not supported" for a name on the NULL-terminated list `refused` (may be
   NULL), with `unknown` for another option, with `superfluous` for a word.  The
   reference has two parsers and words both in several ways: */
#define GTAMD_UNKNOWN_TRY "unknown option: %s (try -help)"
#define GTAMD_UNKNOWN_SHOWS "unknown option: %s (-help shows possible options)"
#define GTAMD_SUPERFLUOUS_ONE "superfluous argument \"%s\""
#define GTAMD_SUPERFLUOUS_MORE "superfluous arguments: \"%s\""
#define GTAMD_UNNECESSARY "unnecessary arguments"
GTAMD_INTERNAL int gtamd_opt_unsupported(const char *a, char *err, size_t errlen);
GTAMD_INTERNAL int gtamd_opt_tail(const char *a, const char *const *refused, const char *unknown,
                                  const char *superfluous, char *err, size_t errlen);

/* ---- project_host.c: a project read back ----
   Nothing there calls the engine: it links into a program without it. */

/* the single-build limit of the engine: tables of more entries come in slices */
#define GTAMD_MAX_ENTRIES ((1ull << 32) - 4096)

/* one "key=value" line of INDEX.prj; -1 when the file or the key is not there */
GTAMD_INTERNAL int gtamd_prj_value(const char *path, const char *key, unsigned long long *value);

typedef struct { void *p; uint64_t bytes; } gtamd_mapped;

typedef struct {
  uint8_t *enc;                   /* the symbols the tables describe */
  uint64_t n;
  gtamd_alphabet alpha;           /* of INDEX.esq, once have_alpha is set */
  int have_alpha;
  gtamd_mapped suf, lcp, llv, bwt;
  uint32_t suf_bytes;             /* 8, or 4 with -suftabuint, once .suf is mapped */
  uint64_t *seqstart, numseq;     /* numseq starts and n + 1 behind them */
} gtamd_project;

/* Each call takes a zeroed or an opened value and leaves one that
   gtamd_project_close releases; -1 with a message in err. */

/* which projects a tool takes: any, or forward and not mirrored only, refused
   in one sentence or in one of two; both name `tool` */
enum { GTAMD_PROJECT_ANY = 0, GTAMD_PROJECT_FORWARD, GTAMD_PROJECT_FORWARD_TWO };
/* The sequence the tables of a project describe: the symbols of INDEX.esq, then
   -mirrored, then -dir, as INDEX.prj says.  Refuses a project without whole
   tables; `verb` words what is not done with the slices of a build in parts. */
GTAMD_INTERNAL int gtamd_project_open(gtamd_project *p, const char *index, const char *verb, int which,
                                      const char *tool, char *err, size_t errlen);
/* INDEX.suf / .lcp / .llv / .bwt into p->suf ..., its size checked against n.
   required: the reference's wording when the file is not there, with the reason. */
enum { GTAMD_TABLE_SUF = 0, GTAMD_TABLE_LCP, GTAMD_TABLE_LLV, GTAMD_TABLE_BWT };
GTAMD_INTERNAL int gtamd_project_map(gtamd_project *p, const char *index, int table, int required,
                                     char *err, size_t errlen);
/* p->seqstart and p->numseq; -1 when memory runs out, without a message */
GTAMD_INTERNAL int gtamd_project_sequence_starts(gtamd_project *p);
GTAMD_INTERNAL void gtamd_project_close(gtamd_project *p);

/* where the sequences of seq[0..len) start: behind the separators; *num = their
   number, and one more entry, len + 1, as if one more separator followed */
GTAMD_INTERNAL uint64_t *gtamd_sequence_starts(const uint8_t *seq, uint64_t len, uint64_t *num);
/* the last of the numstart ascending starts at or in front of pos */
GTAMD_INTERNAL uint64_t gtamd_unit_of(const uint64_t *start, uint64_t numstart, uint64_t pos);
#endif
