/*
  gtamd_pcktag.h -- C ABI of the approximate matches of short tags through a
  packed index: what `gt tagerator -e K -pck INDEX -q TAGS` computes, on the
  device.  One call makes a reader of the packed index (include/gtamd_pckidx.h)
  the index of a gtamd_tagmatch; prepare, emit, best_k, the info struct, the
  record, the definition of a match, the strands, BEST and K', the limits on tags
  and the windows of any capacity from any cursor stay as
  include/gtamd_tagmatch.h states them.

  What it restates:

    gt_indexbasedapproxpatternmatching  src/match/idx-limdfs.c
      (pck_splitandprocess, processchildinterval, pck_overcontext,
       gen_pck_overinterval: the walk over the intervals of the BWT)
    gt_bwtrangesplitwithoutspecial      src/match/eis-voiditf.c
      (all children of an interval from the ranks of its two bounds)

  WHICH TEXT.  As for matstat (include/gtamd_pckidx.h): the matches are those of
  the text the index was built from, READ BACKWARDS.  An index of the reversed
  subject (-dir rev, the only read mode the reference accepts for -pck,
  idx-limdfs.c:130-136) answers for the subject: tag, strand, dbstart, len and
  dist are then what the -esa path gives for the subject read forward.

  DBSTART.  dbstart = (rows - 1) - (located + len), where `located` is the text
  position of the row the match was found at after len letters (totallength -
  (dbstartpos + offset) of the reference).  A located + len above rows - 1 is an
  inconsistent index: the call fails with a message, no wrapped number is given.

  ORDER.  Ascending tag, then the forward strand before the reverse complement.
  Inside one (tag, strand): the order of a depth-first walk that takes the
  children of an interval of rows in letter order and the rows of an interval in
  row order.  It is deterministic -- the same for every call on the same inputs,
  whatever the capacity and the cursor -- and it is NOT the order of the -esa
  path: matches with the same matched string come in the order of the rows of
  the index, which for an index of the reversed subject is the order of what
  stands in front of the match, read backwards.  Consumers that compare with
  the -esa path sort one (tag, strand) by dbstart.

  WILDCARDS.  gtamd_tagmatch_prepare with GTAMD_TAGMATCH_WITH_WILDCARDS is
  refused while a packed index is the index, with a message that names the flag.
  The reference's walk reads the rows of an interval as if its specials lay at
  its end (idx-limdfs.c:1096-1116), which holds for a suffix table and not for a
  column of the BWT, and walking on past a wildcard needs the stored ranks that
  only -sprank images have.  A wildcard and a separator of the
  text both end a match, as without the flag on the -esa path.

  NO LOCATE INFORMATION.  On an image with locate interval 0 prepare and its
  counts (matches, K') work; gtamd_tagmatch_emit is refused with a message.

  INFO.  children_examined counts the non-empty children whose column was
  stepped when their level was expanded for the first time; levels_pushed is as
  before; single_walks counts the rows that one lane finished alone.

  How it is computed (genometools_amd/csrc/esa_tagmatch.hip: k_tm_walk_pck,
  esa_pckidx_dec.h).  One wave a job, one level per depth in LDS:
  an interval of rows and the column.  Lane c computes the rank pair of letter c
  at the bounds of the level -- all lanes in the same one or two lines of the
  decoded form -- and steps the column with the Eq word of c: one round gives all
  children.  A child without a row <= K is dropped; one whose row m is <= K
  gives all its rows as matches (located 64 at a time, in emit only); one of at
  most 64 rows is finished by its lanes alone, one row a lane, by the BWT symbol
  of the row and LF; a wider one becomes the next level.  Every row that becomes
  an index is checked against the rows of the index: an inconsistent decoded
  form gives -1 and a message, never an endless loop or a read outside the
  arrays.

  Conventions as in gtamd_tagmatch.h: 0 / -1, message from
  gtamd_esa_last_error().  Plain C; no CPU fallback: -1 without a device.
*/
#ifndef GTAMD_PCKTAG_H
#define GTAMD_PCKTAG_H

#include "gtamd_pckidx.h"
#include "gtamd_tagmatch.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The reader as the index of a matcher; the call and gtamd_tagmatch_set_index*
   replace each other and what was prepared.  Refused with a message: a reader
   without an open image, one on another device.  The reader must outlive the
   calls and keep its image: after an open of the reader that failed, prepare and
   emit are refused with a message until the reader holds an image again.  A
   prepare is of the image the reader holds then; emit is refused with a message
   once the reader has been opened again since that prepare, gtamd_tagmatch_best_k
   is not: it reads only what the prepare left. */
int gtamd_tagmatch_set_index_pckidx(gtamd_tagmatch *tm, const gtamd_pckidx *px);

#ifdef __cplusplus
}
#endif
#endif
