// The index formats of the blocked layout's entries: the one list the context (tsem_ctx::index_fmt), the layout build, the table of
// the fused kernel's instantiations (fz_exists, tsem_fused.h) and layout_info() share.
#pragma once

constexpr int FZ_IX32 = 0;   // one lrow << 16 | lcol word per entry: score codes, the split layout, the two-pass kernels
constexpr int FZ_IX24 = 1;   // 3 bytes per entry (tsem_idx24.h): fp64 entries of a non-split fused layout
constexpr int FZ_IXQ = 2;    // one 8-byte word per four entries (tsem_quad64.h): where the layout build chose it over FZ_IX24
constexpr int fz_index_bytes(int ix) { return ix == FZ_IXQ ? 2 : (ix == FZ_IX24 ? 3 : 4); }   // bytes of index per stored entry
