/*
  gtamd_host.h -- host-side C layer around the device engine: what the
  reference's driver (src/match/sfx-run.c:428-717) does before and after the
  Sfxiterator loop, reduced to the `gt suffixerator` surface of this path.

    gtamd_encode_files      GtEncseqEncoder read side: FASTA -> encoded symbols
                            (src/core/sequence_buffer_fasta.c:44-170,
                            src/core/alphabet.c:84-91,345-356,480-503)
    gtamd_sequence_stats    GtSpecialcharinfo (src/core/chardef.h:91-116,
                            src/core/encseq_charproc.gen, encseq.c:5061-5127)
    gtamd_write_prj         gt_outprjfile (src/match/sfx-outprj.c:38-118)
    gtamd_suffixerator      the tool function, GtToolfunc shape
                            (src/core/toolbox.h:32, src/tools/gt_suffixerator.c:22)
    gtamd_sfxmap            the checker of that path, `gt dev sfxmap -suf -lcp -bwt`
                            (src/tools/gt_sfxmap.c; src/match/sfx-lwcheck.c:181-337,
                            src/match/sfx-linlcp.c:548), on the device through
                            include/gtamd_check.h
    gtamd_matstat, gtamd_uniquesub
                            `gt matstat -esa` and `gt uniquesub -esa`
                            (src/tools/gt_matstat.c), on the device through
                            include/gtamd_mstat.h
    gtamd_querymatch        `gt repfind` with -q, -r or -p: maximal exact matches of
                            queries against the index
    gtamd_repfind           `gt repfind -l L -ii INDEX` (src/tools/gt_repfind.c),
                            on the device through include/gtamd_maxpairs.h
    gtamd_encseq2spm        `gt encseq2spm -l L -ii INDEX -spm show|count`
                            (src/tools/gt_encseq2spm.c), on the device through
                            the engine and include/gtamd_spm.h
    gtamd_readjoiner_overlap  `gt readjoiner overlap -readset X -l L`
                            (src/tools/gt_readjoiner_overlap.c), on the device
                            through the engine and include/gtamd_spmred.h
    gtamd_readjoiner_prefilter  `gt readjoiner prefilter -db FILE... -readset X`
                            (src/tools/gt_readjoiner_prefilter.c), on the device
                            through the encoder, the engine and
                            include/gtamd_contained.h
    gtamd_readjoiner_correct  `gt readjoiner correct -ii INDEX -k K -c C`
                            (src/tools/gt_readjoiner_correct.c), on the device
                            through the engine and include/gtamd_kcorrect.h
    gtamd_assembly          `gt readjoiner assembly -readset X` with default
                            options (src/tools/gt_readjoiner_assembly.c), on
                            the device through include/gtamd_strgraph.h
    gtamd_tagerator         `gt tagerator -e K -esa INDEX -q TAGS`
                            (src/tools/gt_tagerator.c), on the device through
                            include/gtamd_tagmatch.h
    gtamd_idxlocali         `gt dev idxlocali -th T -esa INDEX -q FILES`
                            (src/tools/gt_idxlocali.c), on the device through
                            include/gtamd_locali.h

  Pure C (gcc); links against libgtamd_esa.so for the hot path.
*/
#ifndef GTAMD_HOST_H
#define GTAMD_HOST_H

#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include "gtamd_esa.h"
#include "gtamd_encode.h"
#include "gtamd_spmred.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
  uint64_t totallength, specialcharacters, specialranges, realspecialranges,
           lengthofspecialprefix, lengthofspecialsuffix, wildcards,
           wildcardranges, realwildcardranges, lengthofwildcardprefix,
           lengthofwildcardsuffix, numofsequences;
  uint32_t numofchars;
} gtamd_seqstats;

/* An alphabet: the built-in DNA and protein ones (src/core/alphabet.c:84-91,
   345-356, 480-503) or one read from a symbol map file (-smap; format and
   parser src/core/alphabet.c:118-330: one line per symbol class, optionally a
   blank and the character shown for the class, leading '#' lines are comments,
   the last line holds the wildcards).  numofchars <= 28 for the engine. */
typedef struct {
  uint8_t symbolmap[256];      /* code per input byte; 254 wildcard, 253 undefined */
  uint32_t numofchars;
  char characters[64];         /* character shown for every code */
  char wildcardshow;
  int alphatype;               /* 0 DNA, 1 protein, 2 from a symbol map */
  unsigned bitspersymbol;      /* of the bit-packed access type */
  char *alphadef;              /* symbol map text as INDEX.esq stores it, or NULL */
  uint64_t lengthofalphadef;
} gtamd_alphabet;

void gtamd_alphabet_standard(gtamd_alphabet *a, int protein);
int gtamd_alphabet_from_file(const char *path, gtamd_alphabet *a, char *err, size_t errlen);
int gtamd_alphabet_from_text(const char *text, uint64_t len, const char *mapfile,
                             gtamd_alphabet *a, char *err, size_t errlen);
void gtamd_alphabet_free(gtamd_alphabet *a);

/* Read one or more (multi-)FASTA files into one encoded sequence; consecutive
   sequences are joined by one separator, also across files.  protein != 0
   selects the protein alphabet.  *enc is malloc'ed.  Returns 0, or -1 with the
   reference's error text in err ("illegal character 'X': file \"f\", line 2",
   "file 'f' contains an empty sequence"). */
int gtamd_encode_files(const char *const *paths, size_t numfiles, int protein,
                       uint8_t **enc, uint64_t *n, char *err, size_t errlen);

/* The same, also returning the sequence descriptions (header lines without
   the leading '>' / '@'), NUL-separated in one malloc'ed block of *desclen
   bytes, one per sequence.  desc may be NULL. */
int gtamd_encode_files_desc(const char *const *paths, size_t numfiles,
                            int protein, uint8_t **enc, uint64_t *n,
                            char **desc, uint64_t *desclen, char *err,
                            size_t errlen);

/* What the encoder saw besides the symbols: how often every original input
   byte occurred in the sequences, and per input file the bytes read and the
   symbols (with separators) it contributed -- GtFilelengthvalues,
   src/core/filelengthvalues.h:22-26, filled in
   src/core/sequence_buffer_fasta.c:56-94 / sequence_buffer_fastq.c:113-188. */
typedef struct { uint64_t length, effectivelength; } gtamd_filelength;
typedef struct {
  uint64_t originaldistribution[256];
  gtamd_filelength *filelengthtab;      /* numfiles entries, malloc'ed */
  size_t numfiles;
  uint64_t exceptioncharacters,         /* -lossless: set by gtamd_write_ois, go */
           realexceptionranges;         /* into the header of INDEX.esq          */
} gtamd_encinfo;

int gtamd_encode_files_info(const char *const *paths, size_t numfiles,
                            int protein, uint8_t **enc, uint64_t *n,
                            char **desc, uint64_t *desclen,
                            gtamd_encinfo *info, char *err, size_t errlen);
void gtamd_encinfo_free(gtamd_encinfo *info);

/* -lossless (src/core/encseq_api.h:276-286): the reader also returns the
   original character of every symbol (0 for separators; *orig malloc'ed);
   gtamd_write_ois writes INDEX.ois -- most frequent original character per
   symbol class, the classes' character lists, and the bit-packed list of
   "exceptions" with their runs (src/core/encseq.c:1018-1078, 5275-5419) -- and
   stores the exception counts in *info for INDEX.esq; the MD5 sums are taken
   over the original characters (encseq_charproc.gen:30-36). */
int gtamd_encode_files_orig(const char *const *paths, size_t numfiles,
                            const gtamd_alphabet *a, uint8_t **enc, uint64_t *n,
                            uint8_t **orig, char **desc, uint64_t *desclen,
                            gtamd_encinfo *info, char *err, size_t errlen);
int gtamd_write_ois(const char *indexname, const uint8_t *enc, const uint8_t *orig,
                    uint64_t n, const gtamd_alphabet *a, gtamd_encinfo *info,
                    char *err, size_t errlen);
int gtamd_write_md5_orig(const char *indexname, const uint8_t *enc,
                         const uint8_t *orig, uint64_t n);

/* The functions of this header that take `int protein` have a twin ending in
   _alpha that takes any alphabet instead. */
int gtamd_encode_files_alpha(const char *const *paths, size_t numfiles,
                             const gtamd_alphabet *a, uint8_t **enc, uint64_t *n,
                             char **desc, uint64_t *desclen,
                             gtamd_encinfo *info, char *err, size_t errlen);
int gtamd_write_md5_alpha(const char *indexname, const uint8_t *enc, uint64_t n,
                          const gtamd_alphabet *a);
int gtamd_write_esq_alpha(const char *indexname, const char *const *paths,
                          size_t numfiles, const uint8_t *enc, uint64_t n,
                          const gtamd_alphabet *a, const gtamd_encinfo *info,
                          int write_ssp, const char *sat, gtamd_seqstats *ss,
                          char *err, size_t errlen);
int gtamd_read_esq_alpha(const char *indexname, uint8_t **enc, uint64_t *n,
                         gtamd_alphabet *a, gtamd_seqstats *ss, char *err,
                         size_t errlen);
int gtamd_device_encode_files_alpha(const char *const *paths, size_t numfiles,
                                    const gtamd_alphabet *a, gtamd_encoder **enc,
                                    char **desc, uint64_t *desclen,
                                    gtamd_encinfo *info, char *err, size_t errlen);
int gtamd_write_esq_device_alpha(const char *indexname, const char *const *paths,
                                 size_t numfiles, const gtamd_encoder *enc,
                                 const gtamd_alphabet *a, const gtamd_encinfo *info,
                                 int write_ssp, const char *sat, gtamd_seqstats *ss,
                                 char *err, size_t errlen);

/* INDEX.esq -- the encoded sequence in the reference's own on-disk format, so
   that an index written here can be mapped by GenomeTools' tools
   (gt_encseq_loader_load) -- and INDEX.ssp, the separator positions, when the
   reference would write it: header and sequence sections of
   src/core/encseq.c:1195-1402 with the access type the reference chooses
   (src/core/encseq_access_type.c:96-162): "equallength", "bit", "uchar",
   "ushort", "uint32" for DNA, "bytecompress" for protein.  paths are stored as
   given.  write_ssp mirrors the -ssp option.  0, or -1 with a message. */
int gtamd_write_esq(const char *indexname, const char *const *paths,
                    size_t numfiles, const uint8_t *enc, uint64_t n,
                    int protein, const gtamd_encinfo *info, int write_ssp,
                    char *err, size_t errlen);

/* The same two steps with the device encoder (include/gtamd_encode.h) for
   FASTA input and FASTQ input in the four-line form: the files are read whole and encoded on the GPU; *enc (destroy
   with gtamd_encoder_destroy) holds the symbols in HBM, ready for
   gtamd_esa_set_sequence_bytes(ctx, gtamd_encoder_device_symbols(*enc), n, 1);
   descriptions and file information come back as from gtamd_encode_files_info.
   gtamd_write_esq_device writes INDEX.esq/.ssp from sections packed on the
   device, byte-identical to gtamd_write_esq; *ss (may be NULL) receives the
   sequence statistics.  gtamd_device_encode_files returns
   GTAMD_DEVICE_DECLINED (err says why) for FASTQ the device reader does not
   take: gtamd_encode_files_info then reads it.  gtamd_input_is_fastq: 1 if a
   file starts with '@'. */
#define GTAMD_DEVICE_DECLINED (-2)
int gtamd_input_is_fastq(const char *const *paths, size_t numfiles);
int gtamd_device_encode_files(const char *const *paths, size_t numfiles,
                              int protein, gtamd_encoder **enc,
                              char **desc, uint64_t *desclen,
                              gtamd_encinfo *info, char *err, size_t errlen);
int gtamd_write_esq_device(const char *indexname, const char *const *paths,
                           size_t numfiles, const gtamd_encoder *enc,
                           int protein, const gtamd_encinfo *info, int write_ssp,
                           const char *sat, gtamd_seqstats *ss, char *err, size_t errlen);

/* The way back (option -ii, src/match/sfx-run.c:454-493 /
   gt_encseq_loader_load): the symbols of an existing INDEX.esq, written by
   GenomeTools or by gtamd_write_esq, for every access type ("direct",
   "bytecompress", "equallength", "bit", "uchar", "ushort", "uint32"; the last
   three also need INDEX.ssp when there is more than one sequence).  DNA and
   protein alphabets only.  *enc is malloc'ed; ss (may be NULL) receives the
   sequence statistics stored in the header. */
int gtamd_read_esq(const char *indexname, uint8_t **enc, uint64_t *n,
                   int *protein, gtamd_seqstats *ss, char *err, size_t errlen);

/* The same with the access type forced (-sat direct|bytecompress|eqlen|bit|
   uchar|ushort|uint32; NULL: the reference's choice) and the sequence
   statistics -- whose stored-range counts follow the forced table type --
   returned in *ss (may be NULL).  Errors of src/core/encseq.c:797-807 and
   src/core/encseq_access_type.c:163-221 with their wording. */
int gtamd_write_esq_sat(const char *indexname, const char *const *paths,
                        size_t numfiles, const uint8_t *enc, uint64_t n,
                        int protein, const gtamd_encinfo *info, int write_ssp,
                        const char *sat, gtamd_seqstats *ss, char *err, size_t errlen);

void gtamd_sequence_stats(const uint8_t *enc, uint64_t n, uint32_t numofchars,
                          gtamd_seqstats *st);

/* INDEX.des (descriptions, each followed by '\n', then the length of the
   longest one and ~0 as two 8-byte words) and INDEX.sds (8-byte end offset of
   every description but the last), src/core/encseq_charproc.gen:118-130,
   src/core/encseq.c:5613-5624.  INDEX.md5: per sequence the MD5 of its decoded
   upper-case symbols as 32 hex digits + NUL (encseq_charproc.gen:52-92). */
/* -clipdesc (src/core/desc_buffer.c:63-80): cut every description of the
   NUL-separated block at its first white space, in place */
void gtamd_clip_descriptions(char *desc, uint64_t *desclen);
int gtamd_write_des_sds(const char *indexname, const char *desc,
                        uint64_t desclen, int write_des, int write_sds);
int gtamd_write_md5(const char *indexname, const uint8_t *enc, uint64_t n,
                    int protein);

/* The sequence as the reference reads it with -dir fwd|rev|cpl|rcl (readmode
   0..3, src/core/readmode_api.h:24-27), in place; complement (3 - code) is
   defined for DNA only, specials are their own complement. */
void gtamd_apply_readmode(uint8_t *enc, uint64_t n, int readmode);

/* -mirrored (src/core/encseq_api.h:190-198, encseq_options.c): sequence +
   separator + its reverse complement, 2n+1 symbols, malloc'ed; and the
   statistics a mirrored GtEncseq reports, from those of the original
   (src/core/encseq.c:4960-5054). */
uint8_t *gtamd_mirror(const uint8_t *enc, uint64_t n);
void gtamd_seqstats_mirror(gtamd_seqstats *st, int last_symbol_is_wildcard);

/* INDEX.prj; with_lcp == 0 writes the zero LCP statistics the reference
   writes when -lcp was not requested (src/match/sfx-run.c:664-670) */
int gtamd_write_prj(const char *path, const gtamd_seqstats *ss,
                    const gtamd_esa_stats *es, int with_lcp, int readmode,
                    int mirrored);

/* `gt suffixerator` for the option subset of this path:
     -db FILE... | -ii INDEX  -indexname NAME  -dna | -protein
     -suf -lcp -bwt -bck  -suftabuint  -sat TYPE  -smap FILE  -lossless
     -pl [K]  -v  -dir fwd|rev|cpl|rcl  -mirrored  -clipdesc  and, accepted
     without effect on the tables (strategy knobs of the CPU algorithm),
     -parts N  -memlimit X  -dc V  -algbds A B C  -maxwidthrealmedian W
     -cmpcharbychar -dccheck -iterscan -kmerswithencseqreader -noshortreadsort
     -samplewithprefixlengthnull -storespecialcodes -withradixsort
     -showprogress -tis [yes|no];
     -plain -kys -lcpdist -compressedoutput -genomediff
     -sortmaxdepth -spmopt -swallow-tail -onlybucketinsertion change what is
     written and are refused ("option \"-X\" is not supported ...").
   -des -sds -md5 -ssp [yes|no] select the sequence-side files; INDEX.esq is
   always written, as the reference does.
   argv[0] is the tool name.  Returns 0, or -1 with the message in err (the
   caller prints "gt suffixerator: error: <err>" and exits 1, src/gt.c:48-52). */
int gtamd_suffixerator(int argc, const char **argv, char *err, size_t errlen);

/* `gt dev mergeesa -indexname OUT -ii INDEX1 INDEX2 ...` (tool function
   src/tools/gt_mergeesa.c:61, engine src/match/esa-merge.c:136-200, output
   src/match/test-mergeesa.c:110-190): OUT.suf / OUT.lcp / OUT.llv of the
   concatenation of the indexes' sequence sets -- byte for byte what
   `gt suffixerator` writes for all their files at once, which is what the
   reference's own test compares the merge with
   (testsuite/gt_mergeesa_include.rb:17-19).  Here the merge is a build on the
   device from the input indexes' INDEX.esq. */
int gtamd_mergeesa(int argc, const char **argv, char *err, size_t errlen);

/* `gt packedindex trsuftab [-bsize B] [-blbuck K] [-locfreq F] [-locbitmap
   [yes|no]] [-sprank [yes|no]] [-sprankilog I] [-v] INDEX` (tool function src/tools/gt_packedindex_trsuftab.c:44-79,
   construction src/match/eis-bwtseq-construct.c:64-92): INDEX.bdx, the
   block-compressed BWT of the packed index, from the project's INDEX.prj / .esq /
   .bwt / .suf -- byte for byte the reference's file; built on
   the device through include/gtamd_pck.h; with -ctxilog I also INDEX.<I>cxm. */
int gtamd_packedindex_trsuftab(int argc, const char **argv, char *err, size_t errlen);

/* `gt packedindex mkindex` (src/tools/gt_packedindex.c:33-36:
   gt_parseargsandcallsuffixerator(false, ...)): the command line of
   gtamd_suffixerator without the table switches, plus -bsize -blbuck -locfreq
   -locbitmap -sprank -sprankilog; writes the sequence-side files, INDEX.bdx as the reference's
   run_packedindexconstruction does (src/match/sfx-run.c:369-425: with sequence
   statistics, block size 3 for alphabets of more than 10 letters) and INDEX.prj
   (no suffixes written, no `longest`). */
int gtamd_packedindex_mkindex(int argc, const char **argv, char *err, size_t errlen);
/* `gt packedindex mkctxmap [-ctxilog I] INDEX` (src/tools/gt_packedindex_mkctxmap.c:40-139):
   INDEX.<I>cxm from INDEX.prj / INDEX.suf; mkindex and trsuftab take -ctxilog too */
int gtamd_packedindex_mkctxmap(int argc, const char **argv, char *err, size_t errlen);
int gtamd_write_prj_packedindex(const char *path, const gtamd_seqstats *ss,
                                uint32_t prefixlength, int readmode, int mirrored);

/* `gt dev sfxmap [-suf] [-lcp] [-bwt] [-v] -esa INDEX` (tool function
   src/tools/gt_sfxmap.c): is INDEX the index of its sequence?  Reads INDEX.prj,
   INDEX.esq (+ .ssp) and the tables asked for (.suf of 4- or 8-byte entries, by
   its size; .lcp with .llv; .bwt), written here or by GenomeTools; applies
   `mirrored` and `readmode` of the project file to the symbols; checks EVERY
   table entry on the device (criteria: include/gtamd_check.h) and, against the
   tables, `longest` (-suf), `largelcpvalues` and `maxbranchdepth` (-lcp) of the
   project file (`averagelcp` is a rounded, masked figure and is not checked).
   -lcp and -bwt need -suf: both tables are checked through the suffix array
   (the reference's -bwt only prints a statistic).  Silent on success; -v prints
   the device time of every phase.  The reference's other modes (-pck, -stream,
   -bfcheck, -bck, -wholeleafcheck, -enumlcpitv*, -sortmaxdepth, -compressedesa
   ...) are refused by name; indexes beyond the single-build limit (2^32 - 4096
   entries) are refused too.  Returns 0, or -1 with the message in err (the
   caller prints "gt dev sfxmap: error: <err>" and exits 1). */
int gtamd_sfxmap(int argc, const char **argv, char *err, size_t errlen);

/* `gt matstat` and `gt uniquesub` with -esa INDEX (tool functions
   src/tools/gt_matstat.c, output src/match/greedyfwdmat.c:168-211): for every
   position of every query sequence the longest prefix that occurs in the index's
   sequence and where, or the shortest prefix that occurs exactly once, on the
   device (semantics: include/gtamd_mstat.h).
     -esa INDEX        reads INDEX.prj, INDEX.esq (+ .ssp) and INDEX.suf (4- or
                       8-byte entries, by its size) as gtamd_sfxmap does
     -query FILE...    FASTA, read with the alphabet of INDEX.esq
     -min L  -max L    print lengths in [L, L] only; one of them is required
     -output querypos sequence [subjectpos]    (subjectpos: matstat only)
     -verify           matstat only; accepted, without effect with -esa
     -fmi, -pck        refused ("option \"-X\" is not supported ...")
   Prints `unit U[ (DESCRIPTION)]` per query sequence, U counting across all
   files, then `[QUERYPOS ]LENGTH[ SUBJECTPOS][ SEQUENCE]` per position whose
   length is not 0 and within -min/-max.  Returns 0, or -1 with the message in
   err (the caller prints "gt matstat: error: <err>" and exits 1). */
int gtamd_matstat(int argc, const char **argv, char *err, size_t errlen);
int gtamd_uniquesub(int argc, const char **argv, char *err, size_t errlen);

/* `gt repfind -l L -ii INDEX` (tool function src/tools/gt_repfind.c): the
   maximal exact repeats of the index's sequences, enumerated on the device from
   .suf and .lcp together (semantics: include/gtamd_maxpairs.h).
     -ii INDEX   reads INDEX.prj, INDEX.esq (+ .ssp), INDEX.suf (4- or 8-byte
                 entries, by its size), INDEX.lcp and INDEX.llv, as written by
                 `suffixerator -suf -lcp -tis -ssp`; a read mode other than
                 forward and a mirrored index are refused
     -l L        minimum length, default 20 (gt_repfind_arguments_check); >= 1
     -f, -scan   accepted; -scan without effect
     -v          the figures of gtamd_maxpairs_info as one line starting with '#'
   Prints one line per pair, `len seqnum1 relpos1 F len seqnum2 relpos2` (the
   reference's default display of an exact match; its two '#' header lines are
   not printed), in TABLE ORDER: ascending table index of the suffix that stands
   first in the table, then of the other.  The reference prints in the order of
   its traversal; outputs are compared as sorted lines.
   -r -p -q -qii -spm -samples -maxfreq -seedlength -extend* (and the options
   those imply: -xdropbelow -err -minidentity -maxalilendiff -history
   -percmathistory -cam -noxpolish -verify-alignment -trimstat) -outfmt -evalue
   are refused ("option \"-X\" is not supported ..."): they are other
   algorithms or other displays.  A missing INDEX.suf / .lcp gives the
   reference's `cannot open file "INDEX.lcp": No such file or directory`.
   Returns 0, or -1 with the message in err (the caller prints "gt repfind:
   error: <err>" and exits 1). */
int gtamd_repfind(int argc, const char **argv, char *err, size_t errlen);

/* `gt repfind` with -q FILE..., -r or -p (the calls the tool function sends to
   gt_callenumquerymatches, src/tools/gt_repfind.c:562-757): the maximal exact
   matches of query sequences against the index's sequences, on the device from
   .suf and the sequence (semantics and order: include/gtamd_qmatch.h).  The
   sub-command `querymatch`; `repfind` keeps refusing these options.
     -ii INDEX    reads INDEX.prj, INDEX.esq (+ .ssp) and INDEX.suf (4- or 8-byte
                  entries, by its size); a read mode other than forward and a
                  mirrored index are refused
     -l L         minimum length, default 20; >= 1
     -q FILE...   FASTA, read with the alphabet of INDEX.esq; the sequences
                  (units) are numbered across all files, one shorter than L is
                  counted and gives nothing.  Files of more symbols than one
                  search takes (2^32 - 1) are searched in runs of whole units
     -f -r -p     forward, reverse, reverse-complement matches, in this order,
                  each a whole pass; -f is on unless -r or -p is given without
                  it (gt_repfind_arguments_check).  -p needs a DNA alphabet.
                  Without -q the index's own sequences are the queries of -r and
                  -p, and a record is kept only if gt_querymatch_ordered holds
                  (src/match/querymatch.c:357-369); forward matches without -q
                  are the maximal repeats: refused with a pointer to `repfind`
     -v           the figures of every search as a line starting with '#'
   Prints one line per match, `len dbseqnum dbrelpos F|R|P len unit querystart`,
   querystart on the forward strand (gt_querymatch_position_convert), in the
   reference's order; its two '#' header lines are not printed.
   -qii -scan -spm -samples -maxfreq -seedlength -extend* (and the options those
   imply) -outfmt -evalue are refused ("option \"-X\" is not supported ...").
   Returns 0, or -1 with the message in err (the caller prints "gt repfind:
   error: <err>" and exits 1). */
int gtamd_querymatch(int argc, const char **argv, char *err, size_t errlen);

/* `gt encseq2spm -l L -ii INDEX [-spm show|count]` (tool function
   src/tools/gt_encseq2spm.c; the traversal it replaces: src/match/esa-spmsk.c):
   all suffix-prefix matches of at least L letters of the reads of INDEX, on both
   strands (semantics and order: include/gtamd_spm.h).  The sub-command
   `encseq2spm`.
     -ii INDEX   reads INDEX.prj and INDEX.esq (+ .ssp) and no table: the reads
                 are mirrored (gtamd_mirror: R reads give 2R sequences, number
                 R + j the reverse complement of read R - 1 - j), .suf and .lcp of
                 the mirrored reads are built by the engine in this process and
                 handed to the matcher where they lie.  A protein index is
                 refused with the reference's message; so is a project with a
                 read mode other than forward or a mirrored one
     -l L        minimum length, >= 1; mandatory, as in the reference
     -spm show   one line `s t len` per match, in TABLE ORDER: ascending table
                 index of the matching suffix of sequence s, then of the start
                 of sequence t.  The reference prints in the order of its
                 traversal; outputs are compared as sorted lines
     -spm count  the line `number of suffix-prefix matches=Z`
                 without -spm nothing is computed and the exit code is 0, as
                 after the reference's sort
     -v          the build time and the figures of gtamd_spm_info as lines
                 starting with '#'
   -singlestrand is answered with the reference's own "option -singlestand is
   not implemented".  -parts -memlimit -checksuftab -onlyaccum
   -onlyallfirstcodes -addbscachedepth -phase2extra -radixlarge -radixparts
   -singlescan -forcek steer or check the reference's own sort and are refused
   ("option \"-X\" is not supported ...").
   Returns 0, or -1 with the message in err (the caller prints "gt encseq2spm:
   error: <err>" and exits 1). */
int gtamd_encseq2spm(int argc, const char **argv, char *err, size_t errlen);

/* `gt readjoiner overlap -readset X -l L [-elimtrans yes|no] [-showspm] [-q] [-v]`
   (tool function src/tools/gt_readjoiner_overlap.c; the traversal it replaces:
   src/match/rdj-spmfind.c): the irreducible suffix-prefix matches of at least L
   letters of the reads of X, on both strands (definition, filter and order:
   include/gtamd_spmred.h).  The sub-command `readjoiner overlap`.
     -readset X  reads X.esq (+ .ssp) and no table, as encseq2spm does; a protein
                 readset is refused with the reference's message
     -l L        2 or more, as the reference's parser has it
     -elimtrans  yes (default) or no: all matches, none tested
     -showspm    the lines `sn +|- pn +|- len`, in TABLE ORDER; the reference
                 prints the same lines in the order of its traversal.  Without it
                 no line is written and the matches go to X.0.spm in the bin32
                 list format (below), which `gt readjoiner assembly` opens
     -q          no '#' lines;  -v  '#' lines of the tool's own (the reference's
                 are the figures of its k-mer sort); the two exclude each other
   Stdout is the reference's byte for byte, the match lines sorted: the two
   opening '#' lines, the matches, then `number of irreducible suffix-prefix
   matches`, `average irreducible SPM/read`, `number of transitive suffix-prefix
   matches` (without reduction `number of suffix-prefix matches`, `average
   SPM/read`).
   A readset in which a read occurs whole at another place -- a duplicate, a
   contained read, a read equal to its own reverse complement -- is refused with
   their number and a pointer to `gt readjoiner prefilter`: there the reference's
   result depends on its traversal.  -singlestrand is answered "not implemented"
   (it aborts the reference).  -parts -memlimit -wmax -phase2extra -radixparts
   -radixsmall -onlyallfirstcodes steer the reference's own sort and its w sets
   and are refused ("option \"-X\" is not supported ...").
   Returns 0, or -1 with the message in err (the caller prints "gt readjoiner
   overlap: error: <err>" and exits 1). */
int gtamd_readjoiner_overlap(int argc, const char **argv, char *err, size_t errlen);

/* `gt readjoiner prefilter -db FILE... [-readset X] [-q] [-v] [-encodeonly]
   [-fasta] [-cnt] [-strict]` (tool function src/tools/gt_readjoiner_prefilter.c;
   what it replaces: src/match/reads2twobit.c, src/match/rdj-contfinder.c): the
   reads of FASTA or FASTQ files without those that hold a wildcard (the
   reference's "low-quality" reads), without the duplicates and without the reads
   that are a proper prefix or suffix of another read, on either strand
   (definition, tie rule and what -strict adds: include/gtamd_contained.h).  The
   sub-command `readjoiner prefilter`, followed by an option at least; the
   command answers the two words alone as it did before the tool was there.
     -db FILE...   unpaired libraries; a name with ':' (a paired library) is refused
     -readset X    the name of the output; default: the first file
     -encodeonly   nothing is decided: the reads without a wildcard are the output
     -fasta        X.p.fas: `>` and the read on a line each, lower case
     -cnt          X.cnt: the list of removed reads, bit format (rdj-cntlist.c)
     -strict       this tool's own: the reads that stand strictly inside another
                   and those equal to their own reverse complement go as well;
                   two more '#' lines behind the reference's give their numbers
     -q, -v        no '#' lines; the reference's verbose lines.  They exclude each other
   Writes X.esq, and X.ssp where its access type has one; no X.des, X.sds, X.md5,
   as the reference by default.  For reads of one length stdout, X.esq, X.p.fas
   and X.cnt are the reference's byte for byte: the file table of X.esq holds the
   original names, the effective lengths of the reads that are left and the raw
   lengths as src/match/reads2twobit.c:852-892 computes them (for a FASTA read over
   several lines whose wildcard is not on its last line the reference counts the
   letters up to the end of that line only; here the whole read counts).  For
   reads of several lengths the reference departs from its definition
   (include/gtamd_contained.h) and this tool does not.  X.rlt is not written and
   -libtable is refused: the reference's file holds an address of the process
   that wrote it.  -singlestrand -maxlow -lowqual -phred64 -des -clipdes -memdes
   -copynum -seqnums -encseq -testrs* are refused ("option \"-X\" is not supported
   ...").  A read set whose mirrored set is beyond one build is refused as in
   `readjoiner overlap`.
   Returns 0, or -1 with the message in err (the caller prints "gt readjoiner
   prefilter: error: <err>" and exits 1). */
int gtamd_readjoiner_prefilter(int argc, const char **argv, char *err, size_t errlen);

/* `gt readjoiner correct -ii INDEX [-k K] [-c C]` (tool function
   src/tools/gt_readjoiner_correct.c; what it replaces: src/match/rdj-errfind.c
   and the traversal under it): the k-mer based error correction of the reads of
   INDEX.esq, on both strands (definition and order rules:
   include/gtamd_kcorrect.h).  The sub-command `readjoiner correct`, followed by
   an option at least.
     -ii INDEX   INDEX.prj and INDEX.esq (and INDEX.ssp where the reader wants
                 it); no table is read: .suf and .lcp of the mirrored reads are
                 built on the device in this process
     -k K        k-mer length, 1 at least, default 31; above 255 refused in words
     -c C        minimal trusted count, 1 at least, default 3
   INDEX.esq is edited IN PLACE as the reference edits it: the 2-bit words of the
   changed positions and the character distribution.  Nothing is printed.
   INDEX.suf and INDEX.lcp, if present, are left alone.  A sequence file whose
   access type is not the equal-length one is refused with the reference's
   sentence.  The development options -encseq and -dbg are refused by name.
   Returns 0, or -1 with the message in err (the caller prints "gt readjoiner
   correct: error: <err>" and exits 1). */
int gtamd_readjoiner_correct(int argc, const char **argv, char *err, size_t errlen);

/* Readjoiner's bin32 list of matches (src/match/rdj-spmlist.c:45-124): one
   header byte, then three uint32 a match in host byte order: suffix_read,
   prefix_read, len << 2 | suffix_direct << 1 | prefix_direct.  A record that does
   not fit (a read number of 2^32 or more, a length of 2^30 or more) is refused by
   name: the bin64 format is not written.  0, or -1 (the second with a message). */
int gtamd_spmlist_bin32_header(FILE *fp);
int gtamd_spmlist_bin32_records(FILE *fp, const gtamd_spmred_record *rec, uint64_t count, char *err,
                                size_t errlen);

/* The reader of that list: the `*count` records of the file at `path`, in the
   order of the file, in memory the caller frees; readlen: the lengths of the
   `reads` reads the list numbers.  Each of these is refused with a message of
   its own: a file that cannot be opened or is empty, a format byte that is not
   bin32's, a TRUNCATED list (the bytes behind the format byte are no whole
   number of matches), a READ NUMBER beyond the set, a match LONGER than either
   of its reads, a match with both reads reversed.  0, or -1 with the message. */
int gtamd_spmlist_bin32_read(const char *path, const uint32_t *readlen, uint64_t reads,
                             gtamd_spmred_record **rec, uint64_t *count, char *err, size_t errlen);

/* `gt readjoiner assembly -readset X [-l L] [-depthcutoff D] [-lengthcutoff C]
   [-spmfiles 1] [-q]` (tool function src/tools/gt_readjoiner_assembly.c with
   default options): the string graph of the list X.0.spm -- the reference's or
   `readjoiner overlap`'s of this project -- over the reads of X.esq (+ .ssp),
   its unbranched paths and their contigs, on the device (semantics and order:
   include/gtamd_strgraph.h).  The sub-command `assembly`: the words `readjoiner
   assembly` keep the dispatcher's answer.  Writes X.contigs.fas (`>contig_N
   length=.. depth=.. <first>-->...--><last>`, lines of 60 letters) and prints the
   reference's lines, the progress lines, the statistics block or `# no contigs
   respect the given cutoff parameters`, both byte for byte; -q prints none.
   X.paths, the reference's intermediate file, is not written.  Every other
   option of the reference's tool is refused by name, and so is -spmfiles above
   1.  Returns 0, or -1 with the message in err (the caller prints "gt
   readjoiner assembly: error: <err>" and exits 1). */
int gtamd_assembly(int argc, const char **argv, char *err, size_t errlen);
/* The statistics block of the contig lengths as the lines the tool prints, "# "
   in front of each (gt_assembly_stats_calculator_show: quartiles, N50/L50,
   N80/L80), or the one line for no contig, into out; -1 when outlen is too small. */
int gtamd_assembly_statistics(const uint64_t *lengths, uint64_t count, char *out, size_t outlen);

/* `gt tagerator -e K -esa INDEX -q FILE...` (tool function
   src/tools/gt_tagerator.c, gt_runtagerator src/match/tagerator.c:538-773): the
   matches of short tags with up to K differences against the index's
   sequences, on the device from .suf and the sequence (semantics and order:
   include/gtamd_tagmatch.h).  The sub-command `tagerator`.
     -esa INDEX   reads INDEX.prj, INDEX.esq (+ .ssp) and INDEX.suf (4- or 8-byte
                  entries, by its size); a read mode other than forward and a
                  mirrored index are refused
     -q FILE...   FASTA; the tags are numbered across all files.  At most 64
                  letters a tag, more than K; no wildcard (but see -rw)
     -e K         the differences: replacements, insertions, deletions
     -nod -nop    without the forward, without the reverse-complement strand;
                  an index that is not DNA needs -nop
     -best        per tag the matches of the smallest k <= K that gives it one
     -withwildcards [yes|no]   the reference's switch, which it stores as "no
                  wildcards" (gt_tagerator.c:170-174): only `-withwildcards no`
                  lets wildcards of the index be part of a match, with K > 0
     -rw          a wildcard in a tag becomes the first letter
     -output tagnum tagseq dblength dbstartpos abspos dbsequence strand edist
     -v           the figures of gtamd_tagmatch_info as a line starting with
                  '#', behind the matches
   Stdout is the reference's byte for byte -- the four '#' lines in front, the
   `#\ttagnum\ttagseq` line of every tag, the columns and tab rules of
   tgr_showmatch -- except the order of the match lines of one tag and strand:
   ascending table index here, the reference's stack there.  The errors of the
   tags (longer than 64, not longer than K, wildcard, undefined character) come
   in the reference's words after the blocks of the tags before the failing one.
   -pck -online -cmp -maxocc -skpp -maxdepth are refused ("option \"-X\" is not
   supported ..."), and so is a call without -e: the matching statistics belong
   to -maxocc.
   Returns 0, or -1 with the message in err (the caller prints "gt tagerator:
   error: <err>" and exits 1). */
int gtamd_tagerator(int argc, const char **argv, char *err, size_t errlen);

/* `gt dev idxlocali -th T -esa INDEX -q FILE...` (tool function
   src/tools/gt_idxlocali.c, gt_runidxlocali src/match/idxlocali.c): every local
   alignment of the queries against the index whose score reaches T, from
   INDEX.prj, .esq, .ssp and .suf on the device (include/gtamd_locali.h).  The
   sub-command `idxlocali`.
     -th T        the threshold, an integer >= 1; mandatory
     -q FILE...   the queries (FASTA); characters the index's alphabet does not
                  know end the call with the reference's message, wildcards stay
                  and equal nothing
     -match -mismatch -gapextend   the scores (defaults 1, -3, -2); a match score
                  <= 0 and a mismatch or gap extension score >= 0 are refused,
                  which the reference does not do (its walk need not end then)
     -gapstart    parsed and without effect, as in the reference, whose affine
                  gap model is compiled out
     -s           the alignment behind each match, 70 columns a block, the query
                  on top (gt_alignment_show_with_mapped_chars); rebuilt on the
                  host from the columns of the match
     -v           the figures of gtamd_locali_info as a line starting with '#'
                  behind the matches
   stdout: `# indexname(esa)=`, one `# queryfile=` per file, `# threshold=`, then
   per query (numbered across the files) `process sequence Q of length m` and
   per match `seqnum\trelpos\tdblen\t\tQ\tqstart\tqlen\tscore`.  The matches
   of one query come in the order of the suffix table; the reference's come in
   the order of its stack.  -pck, -online and -cmp are refused by name.
   Returns 0, or -1 with the message in err (the caller prints "gt dev
   idxlocali: error: ..."). */
int gtamd_idxlocali(int argc, const char **argv, char *err, size_t errlen);

#ifdef __cplusplus
}
#endif
#endif
