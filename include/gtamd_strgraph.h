/*
  gtamd_strgraph.h -- C ABI of the CONTIGS of a read set from its irreducible
  suffix-prefix matches: the string graph, its unbranched paths and the
  sequences they spell, what `gt readjoiner assembly -readset X` computes with
  default options (tool src/tools/gt_readjoiner_assembly.c), on the device.

  What it restates:

    gt_spmproc_strgraph_add, gt_strgraph_add_edge   src/match/rdj-strgraph.c:769-824
    gt_strgraph_traverse and what it calls          src/match/rdj-strgraph.c:2366-2495
    the vertex macros                               src/match/rdj-strgraph-vertices-common-def.h
    gt_contigpaths_to_fasta                         src/match/rdj-contigpaths.c
    gt_contigs_writer_start, _append                src/match/rdj-contigs-writer.c

  INPUTS.  The read set: R reads as n symbols, letters 0..3, one separator (255)
  between two reads, NOT mirrored; what `gt readjoiner prefilter` leaves, no
  wildcards.  A list of Z matches { suffix_read, prefix_read, len, flags } in the
  layout of gtamd_spmred_record: the last len letters of read suffix_read are the
  first len of read prefix_read, each read taken as it is (its DIRECT bit of
  flags set) or as its reverse complement.  Both may be in host or in device
  memory; a device list is what gtamd_spmred_emit(..., out_on_device = 1, ...)
  gives, so reads become contigs without the list leaving the device.  A record
  with a read number beyond R, with flags of 0 or above 3, or longer than either
  of its reads, is refused (the prepare fails and names their number).

  GRAPH.  Read r has the vertices B = 2r and E = 2r + 1; other(v) = v ^ 1.  A
  record with len >= L (min_len) that is no match of a read with itself adds two
  edges, with (s, p) its two reads:

    suffix direct, prefix direct     E(s) -> E(p)   then   B(p) -> B(s)
    suffix direct, prefix reverse    E(s) -> B(p)   then   E(p) -> B(s)
    suffix reverse, prefix direct    B(s) -> E(p)   then   B(p) -> E(s)

  The reference states a fourth case, both reads reversed (B(s) -> B(p) then
  E(p) -> E(s)), and asserts that it never occurs: no list holds such a record.
  Here it is stated and refused: a record with flags 0 fails the prepare, as above.

  The two are mirror images: u -> w and other(w) -> other(u).  The LENGTH of an
  edge is the length of its destination read minus len.  The edges of a vertex
  stand in INSERTION ORDER: the order of the list, the first edge of a record
  before its second (the two never leave one vertex, as the record is no match
  of a read with itself).  Nothing sorts them by length or destination: the
  order decides which path a junction starts first and so the numbers of the
  contigs.  A vertex is INTERNAL when its out-degree and that of other(v) -- its
  in-degree -- are both 1.

  PATHS.  A path starts at (i, j): a vertex i that is not internal and has
  edges, and its j-th edge.  It runs over internal vertices to the first vertex t
  that is none.  The paths are written in ascending (i, j), and:

    - a path with at least one internal vertex is written once.  Its mirror image
      starts at (other(t), j'), j' the place of the mirror image of its last edge;
      the one with the smaller start is written.  A HAIRPIN ends at t = other(i):
      both orientations start at i, and the smaller j is written;
    - a path of a single edge i -> t follows the reference's elimination marks,
      which are not symmetric: a vertex that is not internal is marked when the
      scan over the vertices has passed it, so the edge is skipped when t < i and
      written when t > i -- whatever the out-degree of t, and although i -> t and
      its mirror image other(t) -> other(i) spell the same overlap, one of the two,
      both or neither may be written.  (i = t needs a match of a read with itself.)
      The rule is sometimes put as "skipped when t < i or t has no out-edge"; the
      second half is not what gt_strgraph_traverse does: a vertex without
      out-edges is marked only when the scan reaches it (rdj-strgraph.c:
      2465-2478), so an edge into a dead end with a higher number is written, as
      the overlap of two reads alone shows: one contig of depth 2, not none;
    - CYCLES of internal vertices come last, in the order of their lowest vertex
      taken over the cycle and its mirror image; the one of the two that holds
      this vertex is written, and starts and ends there.

  CONTIG.  A path i -> v_1 -> ... -> v_d spells the read of i as the path reads
  it, then of every v_k the last (length of the edge into v_k) letters of its
  read as the path reads it: an E vertex reads the read, a B vertex its reverse
  complement (GT_STRGRAPH_V_MIRROR_SEQNUM).  Its DEPTH is its number of
  vertices, d + 1, a cycle's lowest vertex counted twice.  It is KEPT when depth >=
  depthcutoff and length >= lengthcutoff (the tool's defaults: 3 and 100); the
  kept contigs are numbered in the order of the paths.

  RECORD.  { length, depth, first_vertex, last_vertex, offset }, five uint64;
  offset: where its symbols start among the symbols of all kept contigs, which
  stand side by side without separators.

  How it is computed (genometools_amd/csrc/esa_strgraph.hip,
  esa_strgraph_core.h), no lane ever walking a path:

    1 reads      the separators of the read set by a count, a scan and a scatter;
                 start and length of every read
    2 edges      one lane per record writes its two (source, slot) pairs; a
                 stable radix sort by source (esa_prims); destination, length and
                 the place of every slot's mirror image gathered behind it; the
                 first edge of every vertex by a search among the sorted sources
    3 classify   one lane per vertex: isolated, end, internal; junctions counted
    4 rank       pointer doubling over the internal vertices, carrying (vertex
                 ahead, edges, sum of their lengths, lowest and last internal
                 vertex passed), at most ceil(log2(2R)) + 1 rounds.  The
                 predecessor of v is other(successor(other(v))), so the one
                 ranking gives every vertex of a chain its end, and through
                 other(v) its start, its number from the start and the edge that
                 starts its path.  What has not reached an end lies on a cycle;
                 the written cycles are ranked once more from their lowest
                 vertex (at most ceil(log2(cycle vertices)) + 1 rounds)
    5 select     one lane per edge, which stand in (i, j) order already: is a
                 path written from here, and kept; a scan numbers the contigs,
                 two more place their elements and their symbols
    6 scatter    one lane per contig writes its first and last element, one per
                 internal vertex the element at offset + number
    7 spell      in the emit calls, one lane per symbol: its element by a search
                 among the elements' first symbols, then the letter

  Working memory: 8 bytes a read, 28 a slot (two a record) and the sort's
  workspace, 41 a vertex, 16 an element of a kept contig.

  LIMITS.  n < 2^31 symbols, R <= 2^30 reads, Z <= 2^30 records.  The contained
  reads a read set of several lengths may hold after the reference's prefilter
  (its X.0.cnt) are not looked for: the set is expected without them, as `gt
  readjoiner prefilter` of this project leaves it with -strict.

  Conventions as in gtamd_spm.h: 0 / -1, message from gtamd_esa_last_error().
  Plain C; no CPU fallback: -1 without a device.
*/
#ifndef GTAMD_STRGRAPH_H
#define GTAMD_STRGRAPH_H

#include <stddef.h>
#include <stdint.h>
#include "gtamd_spmred.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GTAMD_STRGRAPH_DEPTHCUTOFF 3u          /* the defaults of the reference's tool */
#define GTAMD_STRGRAPH_LENGTHCUTOFF 100u

typedef struct { uint64_t length, depth, first_vertex, last_vertex, offset; } gtamd_strgraph_contig;

typedef struct {
  uint64_t reads, vertices;
  uint64_t matches;                     /* records of the list */
  uint64_t edges;                       /* two for every record that counts */
  uint64_t internal_vertices, junctions;
  uint64_t paths;                       /* written paths that are no cycles, before the cutoffs */
  uint64_t cycles;                      /* written cycles, before the cutoffs */
  uint64_t cycle_vertices;              /* vertices on cycles, written or not */
  uint64_t contigs;                     /* kept: records the emit calls will give */
  uint64_t elements;                    /* vertices of the kept contigs */
  uint64_t total_length;                /* symbols the emit calls will give */
  uint64_t longest_contig;
  uint64_t device_bytes;                /* device memory the object holds */
  uint32_t doubling_rounds;             /* of the first ranking */
  uint32_t cycle_rounds;                /* of the ranking of the written cycles */
  float device_ms;                      /* device time of gtamd_strgraph_prepare (HIP events) */
  float build_ms;                       /* of which steps 1 to 3 */
  float rank_ms;                        /* step 4 */
  float select_ms;                      /* step 5 */
  float scatter_ms;                     /* step 6 */
  float spell_ms;                       /* step 7: the emit calls of symbols since the prepare */
} gtamd_strgraph_info;

typedef struct gtamd_strgraph gtamd_strgraph;

gtamd_strgraph *gtamd_strgraph_create(int device);
void gtamd_strgraph_destroy(gtamd_strgraph *sg);

/* Host only.  tile: the lanes of one workgroup (records, edges, vertices,
   contigs or symbols a lane); separator_tile: the symbols of one workgroup of
   step 1; min_capacity: the smallest capacity an emit call takes.  Any may be
   NULL. */
void gtamd_strgraph_geometry(uint32_t *tile, uint32_t *separator_tile, uint64_t *min_capacity);

/* the read set; on_device: enc is device memory, which must outlive the calls */
int gtamd_strgraph_set_reads(gtamd_strgraph *sg, const uint8_t *enc, uint64_t n, int on_device);
/* the list; on_device: rec is device memory, which must outlive the prepare */
int gtamd_strgraph_set_matches(gtamd_strgraph *sg, const gtamd_spmred_record *rec, uint64_t count, int on_device);

/* steps 1 to 6 for the minimum length min_len (0: every record) and the two
   cutoffs.  Fills *info (may be NULL).  Synchronous. */
int gtamd_strgraph_prepare(gtamd_strgraph *sg, uint32_t min_len, uint32_t depthcutoff, uint32_t lengthcutoff,
                           gtamd_strgraph_info *info);

/* The records of the kept contigs in pieces, as gtamd_spm_emit: *cursor counts
   contigs, 0 to `contigs` of the info. */
int gtamd_strgraph_emit(gtamd_strgraph *sg, uint64_t *cursor, gtamd_strgraph_contig *out, uint64_t capacity,
                        int out_on_device, uint64_t *written);
/* Step 7: the symbols of the kept contigs in pieces, one byte a symbol, 0..3:
   *cursor counts symbols, 0 to `total_length` of the info. */
int gtamd_strgraph_emit_symbols(gtamd_strgraph *sg, uint64_t *cursor, uint8_t *out, uint64_t capacity,
                                int out_on_device, uint64_t *written);

/* figures of the last prepare */
int gtamd_strgraph_get_info(const gtamd_strgraph *sg, gtamd_strgraph_info *info);

#ifdef __cplusplus
}
#endif
#endif
