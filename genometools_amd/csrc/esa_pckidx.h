// esa_pckidx.h -- what the consumers that take a reader of the packed index
// (esa_pckidx.hip) as their index need of it: esa_mstat.hip, esa_tagmatch.hip and
// esa_locali.hip, through the IndexSlot of esa_index.h, which includes this.  What
// a reader holds, and the search through its decoded form.  A kernel of another
// file that walks the decoded form itself takes it from pckidx_dec
// (esa_pckidx_dec.h, which has the lane functions too).
#pragma once
#include "esa_common.h"

struct gtamd_pckidx;

// device of the reader, does it hold an open image, can it locate
int pckidx_device(const gtamd_pckidx *px);
bool pckidx_is_open(const gtamd_pckidx *px);
// the open calls of the reader so far, failed ones included: two values that differ are two images
u64 pckidx_opens(const gtamd_pckidx *px);
bool pckidx_can_locate(const gtamd_pckidx *px);
u64 pckidx_decoded_bytes(const gtamd_pckidx *px);

// Launches the search of the m query positions at q on stream st: lengths to len,
// witnesses to pos (matstat, may be nullptr).  limit: letters of a query suffix
// that count, max_len + 1 or 2^32 - 1.  *pairs gets the rank pairs, *error is set
// to the error word (esa_pckidx_core.h) of a lane that met one; both are device
// memory the caller zeroed.
int pckidx_search(const gtamd_pckidx *px, hipStream_t st, bool matstat, const u8 *q, u64 m, u32 limit, u32 *len,
                  u64 *pos, u64 *pairs, u64 *error);
// the message for an error word a search left
void pckidx_set_search_error(u64 error);
