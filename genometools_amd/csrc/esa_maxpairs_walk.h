// esa_maxpairs_walk.h -- the walk of one suffix over the segments of its run, of
// esa_maxpairs.hip (semantics and algorithm: include/gtamd_maxpairs.h), apart
// from the kernels so that a test can compile it for the CPU
// (tests/maxpairs_walk_shim.cpp) and run the very code the lanes run against the
// brute force without a device.
//
// What the walk is given: the M suffixes that lie in a run, in table order.
// Entry k has val[k], the LCP value of its table index (0 for the first entry of
// a run: the value there is below the minimum length and never used), and
// cls[k], its left character: a letter, or MP_UNIQUE.  Entries k of one run
// stand at consecutive table indices.  Segment s holds the entries
// [seg_first[s], seg_first[s + 1]): one class, one run; a unique entry alone.
#pragma once
#include <stdint.h>

typedef uint64_t u64;
typedef uint32_t u32;
typedef uint16_t u16;
typedef uint8_t u8;

#if defined(__HIPCC__)
#define MP_HD __device__ __forceinline__
#else
#define MP_HD inline
#endif

constexpr u32 MP_UNIQUE = 255;          // class of position 0 and of a suffix behind a special
constexpr u32 MP_RUN_START = 0x100;     // bit of seg_info: the segment is the first of its run
constexpr u32 MP_NO_MIN = 0xffffffffu;  // minimum of no value

struct MpRecord { u64 pos1, pos2, len; };   // gtamd_maxpairs_record

struct MpSegments {
  const u32 *val;        // [M]
  const u32 *tmin;       // [M] minimum of val over the entries behind k in its segment
  const u32 *seg_of;     // [M] segment of entry k
  const u32 *seg_first;  // [nseg + 1] first entry of the segment; seg_first[nseg] = M
  const u32 *seg_min;    // [nseg] minimum of val over the whole segment
  const u16 *seg_info;   // [nseg] class | MP_RUN_START
  u32 nseg;
};

MP_HD u32 mp_min(u32 a, u32 b) { return a < b ? a : b; }

// does a suffix of class `mine` form a pair with the suffixes of a segment of
// class `theirs`: left-maximality, a unique one never equals anything
MP_HD bool mp_reports(u32 mine, u32 theirs) { return theirs == MP_UNIQUE || theirs != mine; }

// segment s: tmin of its entries, its minimum and its info.  One backward pass.
MP_HD void mp_segment_fill(const u32 *val, const u8 *cls, const u32 *seg_first, u32 s, u32 *tmin,
                           u32 *seg_min, u16 *seg_info) {
  const u32 f = seg_first[s];
  u32 run = MP_NO_MIN;
  for (u32 k = seg_first[s + 1]; k-- > f;) {
    tmin[k] = run;
    run = mp_min(run, val[k]);
  }
  seg_min[s] = run;
  seg_info[s] = (u16) (cls[f] | (val[f] == 0 ? MP_RUN_START : 0));
}

// Pairs of entry k (class cls_k) with the entries behind it in its run: their
// number.  One step per segment behind k: a segment that reports adds its size,
// one of k's own class nothing; two of those never follow each other, so the
// steps are at most 2 * pairs + 1.  *longest: the length of the first pair, the
// longest of this entry (0 without a pair); *steps: the segments looked at.
MP_HD u32 mp_walk_count(const MpSegments &g, u32 k, u32 cls_k, u32 *longest, u32 *steps) {
  u32 run = g.tmin[k], cnt = 0, first = 0, st = 0;
  for (u32 s = g.seg_of[k] + 1; s < g.nseg; s++) {
    const u32 info = g.seg_info[s];
    if (info & MP_RUN_START) break;
    st++;
    const u32 f = g.seg_first[s];
    if (mp_reports(cls_k, info & 0xff)) {
      if (cnt == 0) first = mp_min(run, g.val[f]);
      cnt += g.seg_first[s + 1] - f;
    } else if (cnt == 0) {
      run = mp_min(run, g.seg_min[s]);
    }
  }
  *longest = first;
  *steps = st;
  return cnt;
}

// The same walk with the running minimum of the values: the pairs themselves,
// ascending in the table index of the second suffix, to out[0 .. count).  tab_k
// is the table index of entry k; entry j of the same run stands at tab_k + (j - k).
template <typename S>
MP_HD void mp_walk_emit(const MpSegments &g, u32 k, u32 cls_k, u64 tab_k, const S *suf, MpRecord *out) {
  const u64 pi = suf[tab_k];
  u32 run = g.tmin[k];
  for (u32 s = g.seg_of[k] + 1; s < g.nseg; s++) {
    const u32 info = g.seg_info[s];
    if (info & MP_RUN_START) break;
    if (!mp_reports(cls_k, info & 0xff)) {
      run = mp_min(run, g.seg_min[s]);
      continue;
    }
    const u32 l = g.seg_first[s + 1];
    for (u32 j = g.seg_first[s]; j < l; j++) {
      run = mp_min(run, g.val[j]);
      const u64 pj = suf[tab_k + (j - k)];
      out->pos1 = pi < pj ? pi : pj;
      out->pos2 = pi < pj ? pj : pi;
      out->len = run;
      out++;
    }
  }
}
