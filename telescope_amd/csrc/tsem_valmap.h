// Where the fp64 value of an entry lives inside its sub-block on the layouts the fused kernel reads (h->valmap): the ONE definition
// the fill kernels, the fused kernel's loads and the host read-back share.
//
// A data wave of the fused kernel holds 64 consecutive quads of a sub-block, four consecutive entries per lane, and reads a lane's
// four values with two 16-byte loads.  Stored entry by entry, each of the two instructions covers 2 KB and uses half of every 128-byte
// line of it.  Here the values of every GROUP of 64 consecutive quads (the last group of a sub-block: the gq quads that are left) are
// stored as the first value pair of all its quads, then the second pair of all of them:
//
//   entry e of a sub-block of nq quads (nq a multiple of 16):   q = e >> 2, k = e & 3, g = q >> 6, gq = min(64, nq - 64 g)
//   its value is the double at index   g * 256 + (k >> 1) * gq * 2 + (q & 63) * 2 + (k & 1)      (byte = 8 x that)
//
// so each load of a wave covers gq * 16 contiguous bytes: whole lines.  The last group uses its own width: a sub-block occupies exactly
// the doubles [0, 4 nq) it occupied before, a lane holds the same four entries in the same registers, and nothing but the addresses
// differs.  The index stream (tsem_idx24.h, or 4-byte words on the split layout) stays entry by entry.
#pragma once
#include <cstdint>

constexpr int TS_VALMAP_GROUP = 64;                        // quads per group: one wave's share of a sub-block

// quads in group g of a sub-block of nq quads (0 behind the sub-block's end)
__host__ __device__ inline uint32_t ts_valmap_gq(uint32_t nq, uint32_t g) {
  const uint32_t first = g * (uint32_t)TS_VALMAP_GROUP;
  return nq <= first ? 0u : (nq - first < (uint32_t)TS_VALMAP_GROUP ? nq - first : (uint32_t)TS_VALMAP_GROUP);
}
// index (in doubles, from the sub-block's first value) of entry e of a sub-block of nq quads
__host__ __device__ inline uint32_t ts_valmap_pos(uint32_t e, uint32_t nq) {
  const uint32_t q = e >> 2, k = e & 3u, g = q / (uint32_t)TS_VALMAP_GROUP;
  return g * (4u * TS_VALMAP_GROUP) + (k >> 1) * ts_valmap_gq(nq, g) * 2u + (q % (uint32_t)TS_VALMAP_GROUP) * 2u + (k & 1u);
}
// ... or e itself on the layouts that keep the values entry by entry (the two-pass kernels').  `mapped` is a kernel argument: wave-uniform
__host__ __device__ inline uint32_t ts_valmap_slot(uint32_t e, uint32_t nq, int mapped) { return mapped ? ts_valmap_pos(e, nq) : e; }
