// The 3-byte entry index of the fused layouts with fp64 entries: the ONE definition the fill kernels, the fused kernel and the
// host decoder share.
//
//   entry   e = lrow << 13 | lcol          13 bits of column slot (Kp <= TS_MAX_KP = 7680, hot-column spare slots included),
//                                          11 bits of row slot    (R <= fz_rmax <= 1152): no layout-dependent coding, no fallback
//   stream  entry t of the layout occupies bytes 3t .. 3t+2, little-endian; a quad of four entries is 12 bytes = three dwords
//
//     w0 = e0 | e1 << 24        w1 = e1 >> 8 | e2 << 16        w2 = e2 >> 16 | e3 << 8
//
// Every entry owns whole bytes, so the fill kernels — which place entries one at a time, from many threads — store an index without
// touching its neighbours' (any arrangement that lets two entries share a byte would need an atomic per entry there).  A quad whose
// first word is 0xFFFFFFFF decodes to row slot 2047 in its first entry, which no layout has: the fused kernel's idle mark stays
// unambiguous.  The 32-bit index of every other layout is lrow << 16 | lcol (TS_RC32_*).
#pragma once
#include <cstdint>

constexpr int TS_IDX24_COL_BITS = 13, TS_IDX24_ROW_BITS = 11;
constexpr int TS_IDX24_MAX_KP = 1 << TS_IDX24_COL_BITS, TS_IDX24_MAX_R = 1 << TS_IDX24_ROW_BITS;

__host__ __device__ inline uint32_t ts_idx24_entry(uint32_t lrow, uint32_t lcol) { return (lrow << TS_IDX24_COL_BITS) | lcol; }

// store the index of entry `pos` (two stores: the entry starts on an even or an odd byte)
__host__ __device__ inline void ts_idx24_store(uint8_t* base, int64_t pos, uint32_t lrow, uint32_t lcol) {
  const uint32_t e = ts_idx24_entry(lrow, lcol);
  uint8_t* const q = base + 3 * pos;
  if (pos & 1) {
    q[0] = (uint8_t)e;
    *reinterpret_cast<uint16_t*>(q + 1) = (uint16_t)(e >> 8);
  } else {
    *reinterpret_cast<uint16_t*>(q) = (uint16_t)e;
    q[2] = (uint8_t)(e >> 16);
  }
}

// entry K (0..3) of the quad (w0, w1, w2), in the low 24 bits; the top 8 bits are whatever lies next to it
template <int K>
__host__ __device__ inline uint32_t ts_idx24_raw(uint32_t w0, uint32_t w1, uint32_t w2) {
  static_assert(K >= 0 && K < 4, "a quad has four entries");
  return K == 0 ? w0 : (K == 1 ? (w0 >> 24) | (w1 << 8) : (K == 2 ? (w1 >> 16) | (w2 << 16) : w2 >> 8));
}
template <int K> __host__ __device__ inline uint32_t ts_idx24_row(uint32_t w0, uint32_t w1, uint32_t w2) {
  return (ts_idx24_raw<K>(w0, w1, w2) >> TS_IDX24_COL_BITS) & (uint32_t)(TS_IDX24_MAX_R - 1);
}
template <int K> __host__ __device__ inline uint32_t ts_idx24_col(uint32_t w0, uint32_t w1, uint32_t w2) {
  return ts_idx24_raw<K>(w0, w1, w2) & (uint32_t)(TS_IDX24_MAX_KP - 1);
}
// the row slots and the column slots of the quad's four entries
__host__ __device__ inline void ts_idx24_quad(uint32_t w0, uint32_t w1, uint32_t w2, uint32_t row[4], uint32_t col[4]) {
  row[0] = ts_idx24_row<0>(w0, w1, w2); row[1] = ts_idx24_row<1>(w0, w1, w2); row[2] = ts_idx24_row<2>(w0, w1, w2); row[3] = ts_idx24_row<3>(w0, w1, w2);
  col[0] = ts_idx24_col<0>(w0, w1, w2); col[1] = ts_idx24_col<1>(w0, w1, w2); col[2] = ts_idx24_col<2>(w0, w1, w2); col[3] = ts_idx24_col<3>(w0, w1, w2);
}

// host side: four lrow << 16 | lcol words <-> the 12 bytes of a quad
inline void ts_idx24_pack_quad(const uint32_t rc[4], uint8_t out[12]) {
  for (int k = 0; k < 4; ++k) {
    const uint32_t e = ts_idx24_entry(rc[k] >> 16, rc[k] & 0xFFFFu);
    out[3 * k] = (uint8_t)e; out[3 * k + 1] = (uint8_t)(e >> 8); out[3 * k + 2] = (uint8_t)(e >> 16);
  }
}
inline void ts_idx24_unpack_quad(const uint8_t in[12], uint32_t rc[4]) {
  uint32_t w[3];
  for (int j = 0; j < 3; ++j)
    w[j] = (uint32_t)in[4 * j] | ((uint32_t)in[4 * j + 1] << 8) | ((uint32_t)in[4 * j + 2] << 16) | ((uint32_t)in[4 * j + 3] << 24);
  uint32_t row[4], col[4];
  ts_idx24_quad(w[0], w[1], w[2], row, col);
  for (int k = 0; k < 4; ++k) rc[k] = (row[k] << 16) | col[k];
}
