// The index formats of the blocked layout's entries: the one list the context (tsem_ctx::index_fmt), the layout build, the table of
// the fused kernel's instantiations (fz_exists, tsem_fused.h) and layout_info() share.
#pragma once

constexpr int FZ_IX32 = 0;   // one lrow << 16 | lcol word per entry: score codes, the split layout, the two-pass kernels
constexpr int FZ_IX24 = 1;   // 3 bytes per entry (tsem_idx24.h): fp64 entries of a non-split fused layout
constexpr int FZ_IXQ = 2;    // one 8-byte word per four entries (tsem_quad64.h): where the layout build chose it over FZ_IX24
constexpr int fz_index_bytes(int ix) { return ix == FZ_IXQ ? 2 : (ix == FZ_IX24 ? 3 : 4); }   // bytes of index per stored entry
// The enumerated ranges of the table of instantiations (team size 1..8 x mode 0..9 x entry format 0..2 x geometry 0..3 x timeline x
// index format) in row-major order: the cell order of the launch census (tsem_ctx::fz_census); -1 outside the ranges.
constexpr int TS_FZ_CENSUS_CELLS = 8 * 10 * 3 * 4 * 2 * 3;
constexpr int fz_census_cell(int P, int mode, int fmt, int geo, bool prof, int ix) {
  return (P < 1 || P > 8 || mode < 0 || mode > 9 || fmt < 0 || fmt > 2 || geo < 0 || geo > 3 || ix < 0 || ix > 2)
             ? -1 : ((((((P - 1) * 10 + mode) * 3 + fmt) * 4 + geo) * 2 + (prof ? 1 : 0)) * 3 + ix);
}
