// The 8-byte quad index of the fused layouts with fp64 entries (2 B of index per entry, 10 B per entry in all): the ONE definition the
// pack kernel, the fused kernel and the host decoder share.
//
// A quad of four consecutive entries of a ROW-ORDERED sub-block is one little-endian 64-bit word:
//
//   bits  0-12   column slot of entry 0          13 bits each, as in tsem_idx24.h (Kp <= TS_MAX_KP = 7680)
//   bits 13-25   column slot of entry 1
//   bits 26-38   column slot of entry 2
//   bits 39-51   column slot of entry 3
//   bits 52-54   steps d1, d2, d3, each 0 or 1
//   bits 55-63   row slot r0 of entry 0          9 bits: R <= 512 (geometries 0 and 1)
//
// The row slot of entry k is r0 + d1 + ... + dk.  Every quad carries its own absolute row: no prefix over lanes, no side table per
// sub-block; quad t of a sub-block sits at byte 8 t.  A quad is representable when its rows step by 0 or 1 from entry to entry, which
// the layout build guarantees by construction (every row slot of a block appears in every part's sub-block: tsem_setup.hip,
// k_pc_raise and the dummies of k_sb_fill_sorted).  Column slot 8191 never occurs, so a low word of 0xFFFFFFFF — the fused kernel's
// idle mark — names no stored quad.
#pragma once
#include <cstdint>

constexpr int TS_QUAD64_COL_BITS = 13, TS_QUAD64_ROW_BITS = 9;
constexpr int TS_QUAD64_MAX_KP = 1 << TS_QUAD64_COL_BITS, TS_QUAD64_MAX_R = 1 << TS_QUAD64_ROW_BITS;
constexpr uint32_t TS_QUAD64_COL_MASK = (1u << TS_QUAD64_COL_BITS) - 1u;

// can the four (row slot, column slot) pairs be one quad?
__host__ __device__ inline bool ts_quad64_fits(const uint32_t row[4], const uint32_t col[4]) {
  bool ok = row[0] < (uint32_t)TS_QUAD64_MAX_R;
  for (int k = 0; k < 4; ++k) ok = ok && col[k] < (uint32_t)TS_QUAD64_MAX_KP - 1u;
  for (int k = 1; k < 4; ++k) ok = ok && (row[k] - row[k - 1]) <= 1u;   // (unsigned: a step down is refused too)
  return ok;
}
// the word of a quad that fits
__host__ __device__ inline uint64_t ts_quad64_pack(const uint32_t row[4], const uint32_t col[4]) {
  uint64_t w = 0;
  for (int k = 0; k < 4; ++k) w |= (uint64_t)col[k] << (TS_QUAD64_COL_BITS * k);
  for (int k = 1; k < 4; ++k) w |= (uint64_t)(row[k] - row[k - 1]) << (51 + k);
  return w | ((uint64_t)row[0] << 55);
}
// column / row slot of entry K (0..3) from the low and high half of the word
template <int K> __host__ __device__ inline uint32_t ts_quad64_col(uint32_t lo, uint32_t hi) {
  static_assert(K >= 0 && K < 4, "a quad has four entries");
  return K == 0 ? lo & TS_QUAD64_COL_MASK
       : K == 1 ? (lo >> 13) & TS_QUAD64_COL_MASK
       : K == 2 ? ((lo >> 26) | (hi << 6)) & TS_QUAD64_COL_MASK
                : (hi >> 7) & TS_QUAD64_COL_MASK;
}
template <int K> __host__ __device__ inline uint32_t ts_quad64_row(uint32_t lo, uint32_t hi) {
  static_assert(K >= 0 && K < 4, "a quad has four entries");
  (void)lo;
  uint32_t r = hi >> 23;
  if (K >= 1) r += (hi >> 20) & 1u;
  if (K >= 2) r += (hi >> 21) & 1u;
  if (K >= 3) r += (hi >> 22) & 1u;
  return r;
}
// does the word hold a stored quad?  (the idle mark of the fused kernel does not)
__host__ __device__ inline bool ts_quad64_stored(uint64_t w) { return (uint32_t)w != 0xFFFFFFFFu; }

// host side: four lrow << 16 | lcol words <-> the word
inline bool ts_quad64_pack_words(const uint32_t rc[4], uint64_t* out) {
  uint32_t row[4], col[4];
  for (int k = 0; k < 4; ++k) { row[k] = rc[k] >> 16; col[k] = rc[k] & 0xFFFFu; }
  if (!ts_quad64_fits(row, col)) return false;
  *out = ts_quad64_pack(row, col);
  return true;
}
inline void ts_quad64_unpack_words(uint64_t w, uint32_t rc[4]) {
  const uint32_t lo = (uint32_t)w, hi = (uint32_t)(w >> 32);
  rc[0] = (ts_quad64_row<0>(lo, hi) << 16) | ts_quad64_col<0>(lo, hi);
  rc[1] = (ts_quad64_row<1>(lo, hi) << 16) | ts_quad64_col<1>(lo, hi);
  rc[2] = (ts_quad64_row<2>(lo, hi) << 16) | ts_quad64_col<2>(lo, hi);
  rc[3] = (ts_quad64_row<3>(lo, hi) << 16) | ts_quad64_col<3>(lo, hi);
}
