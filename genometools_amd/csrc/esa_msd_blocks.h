// esa_msd_blocks.h -- the position bits level A of the MSD first sort does not
// store, and how level B brings them back (esa_msd.h).  Host and device: the CPU
// tests run the same functions (tests/test_msd_blocks.py).
//
// A level-A entry of a whole-table build is one u64, K1 << 32 | X << 24 | the low
// 24 bits of its position.  The positions are cut into blocks of 2^L (L =
// msd_block_bits(N): at most 256 blocks, each a whole number of level-A tiles).
// Level A is a stable partition of text order, so inside parent range d the
// entries of block k follow those of block k - 1, and the scanned histogram row
// of block k's first tile holds where they start: bnd[d][k].  An entry at index i
// of parent d lies in block  max { k : bnd[d][k] <= i }  -- equal boundaries are
// blocks without an entry of d, which the maximum passes over.  Level B takes
// the boundaries at or before its tile's first entry as the tile's first block
// and the few inside the tile (at most 255, nearly always none or one) from LDS.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define MSD_HD __host__ __device__ __forceinline__
#else
#define MSD_HD inline
#endif

constexpr int MSD_BLOCKS = 256;      // boundaries per parent range (row of bnd)

// L: ceil(log2 N) - 8, clamped to [12, 24].  It follows N so that every build
// crosses block boundaries, small ones (the tests) included.
MSD_HD int msd_block_bits(uint64_t N) {
  int c = 0;
  while (c < 40 && (1ull << c) < N) c++;
  c -= 8;
  return c < 12 ? 12 : (c > 24 ? 24 : c);
}

// boundary b = bnd[d][k], k >= 1, against a level-B tile [start, start + valid) of
// parent d: 1 = at or before the tile's first entry (counted in its first block),
// 2 = inside the tile, 0 = behind it.  (Rows are nondecreasing in k, so the ones
// form a prefix of the row and the twos follow it.)
MSD_HD uint32_t msd_bound_class(uint32_t b, uint32_t start, uint32_t valid) {
  return b <= start ? 1u : (b - start < valid ? 2u : 0u);
}

// block of the entry e entries into the tile: kb0 = number of boundaries of class
// 1, in[0 .. m) = the boundaries of class 2 as offsets from the tile's first entry
template <typename P>
MSD_HD uint32_t msd_block_in_tile(uint32_t kb0, P in, uint32_t m, uint32_t e) {
  uint32_t lo = 0, hi = m;           // number of in[j] <= e: the first j with in[j] > e
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (in[mid] <= e) lo = mid + 1; else hi = mid;
  }
  return kb0 + lo;
}

MSD_HD uint32_t msd_position(uint32_t block, uint32_t low24, int L) {
  return (block << L) | (low24 & ((1u << L) - 1u));
}

// what a level-B tile does with the boundaries of its parent, one after the other
// (the kernel does it with one thread per boundary); returns kb0
inline uint32_t msd_tile_bounds(const uint32_t *row, uint32_t start, uint32_t valid,
                                uint32_t *in, uint32_t *m) {
  uint32_t kb0 = 0;
  *m = 0;
  for (int k = 1; k < MSD_BLOCKS; k++) {
    const uint32_t c = msd_bound_class(row[k], start, valid);
    if (c == 1u) kb0++;
    if (c == 2u) in[(*m)++] = row[k] - start;
  }
  return kb0;
}
