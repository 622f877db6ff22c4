// Conflict-aware order of the entries INSIDE a quad of the row-ordered fused layouts with fp64 entries: the ONE definition the set-up
// kernel (k_quad_order, tsem_setup.hip), the host entry tsem_quad_order_host and the tests share.
//
// The column scatter of the fused kernel is four ds_add_f64 per data wave and step; instruction j covers entry j of every lane's quad
// and is served in four groups of 16 lanes, each at 2 clk x the largest number of lanes whose column slots agree modulo 16.  Which of
// a lane's four entries goes to which instruction is free wherever they share a row: the row fields of the index, the row-sum runs and
// the idle test do not change, a quad's values stay in its two 16-byte pieces.
//
//   window   64 consecutive entries of a sub-block = the 16 quads of one 16-lane group (sub-blocks are padded to 64 entries)
//   h[j]     for slot j = 0..3: how often each class (column slot & 15) was placed in slot j by the quads 0 .. l-1 of the window
//   rule     quads in order l = 0 .. 15.  Of the permutations p of the quad's entries with row[p[j]] == row[j] for every j, take the one
//            with the SMALLEST SUM over j of h[j][class of entry p[j]]; ties go to the first in lexicographic order of (p[0], p[1],
//            p[2], p[3]) — the identity is first.  Then count the placed classes in h.
//
// Padding and dummy entries (column slot 0, value 0) take part like any entry of their row.  ("Smallest maximum, then sum" models
// at 2.15 lanes per class against 2.18 for the sum alone and costs a second compare per permutation: the sum it is.)
#pragma once
#include <cstdint>

constexpr int TS_QO_QUADS = 16;                             // quads per window
constexpr uint32_t TS_QO_IDENTITY = 0xE4u;                 // permutation code: entry (code >> 2 j) & 3 goes to position j
constexpr uint32_t TS_QO_BARRED = 64u;                     // cost of a placement across rows: above any sum of four counts (<= 4 x 15)

// what the rule needs of a quad: bits 4k..4k+3 the class of entry k; bit 16 + t, t = 0..5: entries (0,1), (0,2), (0,3), (1,2), (1,3),
// (2,3) share a row
__host__ __device__ inline uint32_t ts_qo_word(const uint32_t row[4], const uint32_t col[4]) {
  uint32_t w = 0;
  for (int k = 0; k < 4; ++k) w |= (col[k] & 15u) << (4 * k);
  int t = 0;
  for (int a = 0; a < 4; ++a)
    for (int b = a + 1; b < 4; ++b, ++t) w |= (row[a] == row[b] ? 1u : 0u) << (16 + t);
  return w;
}
__host__ __device__ inline bool ts_qo_same_row(uint32_t w, int a, int b) {
  if (a == b) return true;
  const int lo = a < b ? a : b, hi = a < b ? b : a;
  const int t = lo == 0 ? hi - 1 : (lo == 1 ? hi + 1 : 5);
  return (w >> (16 + t)) & 1u;
}

// one quad: the permutation code the rule picks for word w given the window's counts so far, which are updated.  A count has four
// bits: a window places 16 quads, and the count a slot reaches with the last of them is never read.
__host__ __device__ inline uint32_t ts_qo_step(uint32_t w, unsigned long long (&h)[4]) {
  uint32_t code = TS_QO_IDENTITY;
  if (w >> 16) {                                           // (four different rows: nothing may move)
    uint32_t c[4][4];                                      // c[j][k]: cost of entry k at position j
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int k = 0; k < 4; ++k)
        c[j][k] = ts_qo_same_row(w, j, k) ? (uint32_t)(h[j] >> (4u * ((w >> (4 * k)) & 15u))) & 15u : TS_QO_BARRED;
    uint32_t best = 0xFFFFFFFFu;                           // sum << 13 | place in the enumeration << 8 | code: the minimum is the rule's choice
#pragma unroll
    for (int i = 0; i < 24; ++i) {
      int r[4] = {0, 1, 2, 3}, p[4];
      int d = i;
      const int f[3] = {6, 2, 1};
      for (int j = 0; j < 3; ++j) {                        // (constants once unrolled: the i-th permutation in lexicographic order)
        const int s = d / f[j];
        d -= s * f[j];
        p[j] = r[s];
        for (int m = s; m < 3; ++m) r[m] = r[m + 1];
      }
      p[3] = r[0];
      const uint32_t key = ((c[0][p[0]] + c[1][p[1]] + c[2][p[2]] + c[3][p[3]]) << 13) | ((uint32_t)i << 8) |
                           (uint32_t)(p[0] | (p[1] << 2) | (p[2] << 4) | (p[3] << 6));
      best = key < best ? key : best;
    }
    code = best & 0xFFu;
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) h[j] += 1ull << (4u * ((w >> (4u * ((code >> (2 * j)) & 3u))) & 15u));
  return code;
}

// a window: 16 words in, 16 permutation codes out
__host__ __device__ inline void ts_qo_window(const uint32_t* words, uint8_t* codes) {
  unsigned long long h[4] = {0ull, 0ull, 0ull, 0ull};
  for (int l = 0; l < TS_QO_QUADS; ++l) codes[l] = (uint8_t)ts_qo_step(words[l], h);
}
