// Test shim (CPU): the block-number recovery of the MSD first sort's level B
// (genometools_amd/csrc/esa_msd_blocks.h) over one level-B tile.
#include "../genometools_amd/csrc/esa_msd_blocks.h"

extern "C" int msd_shim_block_bits(uint64_t N) { return msd_block_bits(N); }

// row: the parent's 256 boundaries; low: the stored low 24 bits of the tile's
// entries in index order; out: their positions.  Returns the tile's first block.
extern "C" uint32_t msd_shim_recover(const uint32_t *row, uint32_t start, uint32_t valid,
                                     const uint32_t *low, int L, uint32_t *out) {
  uint32_t in[MSD_BLOCKS], m = 0;
  const uint32_t kb0 = msd_tile_bounds(row, start, valid, in, &m);
  for (uint32_t e = 0; e < valid; e++)
    out[e] = msd_position(msd_block_in_tile(kb0, in, m, e), low[e], L);
  return kb0;
}
