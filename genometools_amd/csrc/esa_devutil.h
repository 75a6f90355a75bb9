// esa_devutil.h -- wave / block level scan helpers shared by the kernels
// (wave64, 256-thread blocks).
#pragma once
#include "esa_prims.h"

constexpr int SC_THREADS = 256;

// v of the first active lane, in a scalar register: for what every lane of the wave has alike
__device__ __forceinline__ u32 uni(u32 v) { return __builtin_amdgcn_readfirstlane(v); }

// the lanes of `mask` (a __ballot) below this one
__device__ __forceinline__ u32 lanes_before(u64 mask) {
  return __builtin_amdgcn_mbcnt_hi((u32) (mask >> 32), __builtin_amdgcn_mbcnt_lo((u32) mask, 0u));
}

template <int OP> __device__ __forceinline__ u32 sc_op(u32 a, u32 b) {
  return OP == SCAN_SUM ? a + b : (a > b ? a : b);
}

// inclusive scan across the 64 lanes of a wave: four shifts inside the rows of
// 16 lanes and two row broadcasts, all as DPP operands of the VALU (a
// __shfl_up goes through the LDS crossbar: six dependent round trips of ~100
// cycles each, which was most of the latency of a block scan).  0 is the
// identity of both operations; a lane without a source reads it.
template <int OP> __device__ __forceinline__ u32 wave_scan_incl(u32 v) {
  v = sc_op<OP>(v, (u32) __builtin_amdgcn_update_dpp(0, (int) v, 0x111, 0xf, 0xf, false));  // row_shr:1
  v = sc_op<OP>(v, (u32) __builtin_amdgcn_update_dpp(0, (int) v, 0x112, 0xf, 0xf, false));  // row_shr:2
  v = sc_op<OP>(v, (u32) __builtin_amdgcn_update_dpp(0, (int) v, 0x114, 0xf, 0xf, false));  // row_shr:4
  v = sc_op<OP>(v, (u32) __builtin_amdgcn_update_dpp(0, (int) v, 0x118, 0xf, 0xf, false));  // row_shr:8
  v = sc_op<OP>(v, (u32) __builtin_amdgcn_update_dpp(0, (int) v, 0x142, 0xa, 0xf, false));  // row_bcast:15
  v = sc_op<OP>(v, (u32) __builtin_amdgcn_update_dpp(0, (int) v, 0x143, 0xc, 0xf, false));  // row_bcast:31
  return v;
}

// block-wide exclusive scan of one value per thread (256 threads);
// returns the exclusive prefix, *total gets the block total
template <int OP, int THREADS = SC_THREADS>
__device__ __forceinline__ u32 block_scan_excl(u32 v, u32 *total, u32 *lds4) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  u32 inc = wave_scan_incl<OP>(v);
  if (lane == 63) lds4[w] = inc;
  __syncthreads();
  u32 carry = 0, tot = 0;
#pragma unroll
  for (int i = 0; i < THREADS / 64; i++) {
    u32 s = lds4[i];
    if (i < w) carry = sc_op<OP>(carry, s);
    tot = sc_op<OP>(tot, s);
  }
  __syncthreads();
  *total = tot;
  // the inclusive value of the lane below (wave_shr:1; lane 0 reads 0)
  const u32 prev = (u32) __builtin_amdgcn_update_dpp(0, (int) inc, 0x138, 0xf, 0xf, false);
  return sc_op<OP>(carry, prev);
}


__device__ __forceinline__ u32 block_scan_excl_sum(u32 v, u32 *total, u32 *lds4) {
  return block_scan_excl<SCAN_SUM>(v, total, lds4);
}
__device__ __forceinline__ u32 block_scan_excl_max(u32 v, u32 *total, u32 *lds4) {
  return block_scan_excl<SCAN_MAX>(v, total, lds4);
}

// inclusive sum over the SC_THREADS values of a workgroup, 64 bits (s: SC_THREADS words)
__device__ __forceinline__ u64 block_scan_incl_u64(u64 v, u64 *s) {
  const u32 t = threadIdx.x;
  s[t] = v;
  __syncthreads();
  for (u32 d = 1; d < SC_THREADS; d <<= 1) {
    const u64 x = t >= d ? s[t - d] : 0;
    __syncthreads();
    s[t] += x;
    __syncthreads();
  }
  const u64 r = s[t];
  __syncthreads();
  return r;
}

// the last entry of [a, b) whose first record is not behind record g, from the
// ascending offsets of offsets_u64 (esa_prims.h); off[a] <= g, and off[b] is not read
__device__ __forceinline__ u64 entry_of(const u64 *off, u64 a, u64 b, u64 g) {
  while (b - a > 1) {
    const u64 mid = a + (b - a) / 2;
    if (off[mid] <= g) a = mid; else b = mid;
  }
  return a;
}

// the .llv pair (table index, value) of table index r among m ascending pairs:
// its number, or where it would stand
__device__ __forceinline__ u64 llv_lower_bound(const u64 *llv, u64 m, u64 r) {
  u64 lo = 0, hi = m;
  while (lo < hi) {
    const u64 mid = (lo + hi) >> 1;
    if (llv[2 * mid] < r) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// one workgroup of SC_THREADS lanes: a[i] = sum of a[0..i), *total = the sum of all
__device__ __forceinline__ void block_scan_excl_array_u64(u64 *a, u64 count, u64 *total, u64 *s) {
  u64 carry = 0;
  for (u64 base = 0; base < count; base += SC_THREADS) {
    const u64 i = base + threadIdx.x;
    const u64 v = i < count ? a[i] : 0;
    const u64 incl = block_scan_incl_u64(v, s);
    if (i < count) a[i] = carry + incl - v;
    carry += s[SC_THREADS - 1];
    __syncthreads();
  }
  if (threadIdx.x == 0) *total = carry;
}
