/*
  gtamd_pcklocali.h -- C ABI of the local alignments of queries through a packed
  index: what `gt dev idxlocali -th T -pck INDEX -q FILES` computes, on the
  device.  One call makes a reader of the packed index (include/gtamd_pckidx.h)
  the index of a gtamd_locali; the column, the match, d_max, the record, the
  limits on queries and scores, set_limits, prepare, get_info and emit in windows
  of any capacity from any cursor stay as include/gtamd_locali.h states them.

  What it restates:

    gt_indexbasedlocali, runlimdfs          src/match/idx-limdfs.c
      (pck_splitandprocess, processchildinterval, pck_overcontext,
       gen_pck_overinterval: the walk over the intervals of the BWT)
    gt_bwtrangesplitwithoutspecial          src/match/eis-voiditf.c
      (all children of an interval from the ranks of its two bounds)

  WHICH TEXT.  As for tags (include/gtamd_pcktag.h): the matches are those of the
  text the index was built from, READ BACKWARDS.  An index of the reversed
  subject (-dir rev, the only read mode the reference accepts for -pck,
  idx-limdfs.c:130-136) answers for the subject: query, dbstart, dblen, score,
  qstart and qlen are then what the -esa path gives for the subject read
  forward.  A column depends only on the letters that follow a start position,
  and the walk spells exactly those.

  DBSTART.  dbstart = (rows - 1) - (located + dblen), where `located` is the text
  position of the row the match was found at after dblen letters
  (gen_pck_overinterval and pck_overcontext, idx-limdfs.c:439-460 and 703-802).
  A located + dblen above rows - 1 is an inconsistent index: the call fails with
  a message, no wrapped number is given.

  ORDER.  Ascending query.  Inside a query ascending job, which is ascending
  code (below); inside a job the order of a depth-first walk that takes the
  children of an interval of rows in letter order and the rows of an interval in
  row order.  It is deterministic -- the same for every call on the same inputs,
  whatever the capacity and the cursor -- and it is NOT the order of the -esa
  path.  Consumers that compare with the -esa path sort one query by dbstart.

  SPECIALS.  A wildcard or a separator of the text ends the columns of a start
  position, and so does the row of suffix 0: the children step yields letter
  children only, and a row that goes on alone ends at a BWT symbol >= sigma.  No
  stored ranks are needed, so images without -sprank work.  A wildcard in a query
  equals nothing, as before.

  THE JOBS.  A job is (query, code w of q letters c1 .. cq, c1 the highest digit
  of w in base sigma).  Every one of the sigma^q codes has a job, whether a
  string of the text spells it or not; info.groups = sigma^q, info.cut_depth = q,
  the smallest depth with Q * sigma^q >= 2^14 and sigma^q <= 2^16, or the
  cut_depth of gtamd_locali_set_limits (beyond what the alphabet allows: the
  largest it allows).  The job walks its own path: at depth d the rank pair of
  the letter cd and the column.  It ends when the interval becomes empty or the
  column has no cell > 0.  If the column reaches T at a depth d <= q the job ends
  too, and gives all rows of the interval of c1 .. cd if and only if c(d+1) .. cq
  are all letter 0: of the jobs that share the prefix, the first.  Otherwise the
  interval of w is the root of the walk.  A start position whose letters end
  before depth q has no match at that depth or deeper.  So every match is given
  once, and job order is query, then code.

  NO LOCATE INFORMATION.  On an image with locate interval 0 prepare and its
  counts work; gtamd_locali_emit is refused with a message.

  INFO.  children_examined counts the letters of the paths of the codes that had
  a non-empty interval, and the non-empty children of a level when it was
  expanded for the first time; levels_pushed, single_walks (rows finished alone)
  and jobs_finished_alone are as before.

  How it is computed (genometools_amd/csrc/esa_locali.hip: k_lc_walk_pck,
  esa_pckidx_dec.h).  One wave a job, the waves of the grid taking
  jobs in turn, the bands of the path on the wave's stack in global memory as on
  the -esa path.  Lane c computes the rank pair of letter c at the bounds of the
  level -- all lanes in the same one or two lines of the decoded form -- which
  gives all children; the whole wave then computes the column of each non-empty
  child in letter order.  A child whose column reaches T gives all its rows
  (located 64 at a time, in emit only, and only those of the window); one without
  a cell > 0 is dropped; a child of one row, or one for which the stack has no
  room, is finished row by row by the BWT symbol of the row and LF; a wider one
  is pushed.  When the walk comes back to a level the rank round runs again for
  the letters left.  Every row that becomes an index is checked against the rows
  of the index and no walk goes deeper than d_max(m): an inconsistent decoded
  form gives -1 and a message, never an endless loop or a read outside the arrays.

  LIMITS.  rows <= 2^32 - 4096; sigma <= 32; the others as in gtamd_locali.h.

  Conventions as in gtamd_locali.h: 0 / -1, message from gtamd_esa_last_error().
  Plain C; no CPU fallback: -1 without a device.
*/
#ifndef GTAMD_PCKLOCALI_H
#define GTAMD_PCKLOCALI_H

#include "gtamd_pckidx.h"
#include "gtamd_locali.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The reader as the index of an aligner; the call and gtamd_locali_set_index*
   replace each other and what was prepared.  Refused with a message: a reader
   without an open image, one on another device, an alphabet above 32 letters,
   rows above 2^32 - 4096.  The reader must outlive the calls and keep its image:
   after an open of the reader that failed, prepare and emit are refused with a
   message until the reader holds an image again.  A prepare is of the image the
   reader holds then; emit is refused with a message once the reader has been
   opened again since that prepare. */
int gtamd_locali_set_index_pckidx(gtamd_locali *lc, const gtamd_pckidx *px);

#ifdef __cplusplus
}
#endif
#endif
