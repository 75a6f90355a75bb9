// esa_spm_state.h -- what a gtamd_spm holds after gtamd_spm_prepare (steps 1 to 4
// of include/gtamd_spm.h), for the two files that read it: esa_spm.hip, which
// fills it and emits every (terminal suffix, read start) pair, and
// esa_spmred.hip, which owns a gtamd_spm and decides pair by pair which of them
// it keeps.  Only .hip files include this header.
#pragma once
#include "esa_index.h"
#include "../../include/gtamd_spm.h"

// the three lists of steps 1 and 2
struct SpLists {
  u32 *idx, *len;        // terminal suffixes: table index, letters
  u32 *starts;           // read starts: table index
  u32 *seps;             // separators: position
};

struct gtamd_spm : ConsumerBase<> {
  ResidentIndex index;
  bool prepared = false;
  // what a prepare leaves for the emit calls
  Dev<u32> tiles, scanws, idx, len, starts, seps, first, cnt;
  Dev<u64> tsum, off;
  Dev<u8> out;                         // records on their way to host memory
  u32 M = 0, R = 0, nseps = 0;
  gtamd_spm_info info = gtamd_spm_info();
};
