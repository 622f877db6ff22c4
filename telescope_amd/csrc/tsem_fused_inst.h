// Instantiation of the fused kernel for the team sizes one translation unit is responsible for (included by tsem_fz_*.hip only).
// Which kernels exist is fz_exists (tsem_fused.h) and nothing else: the look-up below is generated from it, cell by cell.
#pragma once
#include <cstdint>
#include <utility>
#include "tsem_common.h"
#include "tsem_device.h"
#include "tsem_fused.h"

typedef void (*fz_fn)(FusedArgs);
constexpr int FZ_MODES[] = {0, 1, 2, 3, 4, 5, 7, 8, 9};     // the modes k_em_fused knows (FusedArgs)
constexpr int FZ_N_MODES = sizeof(FZ_MODES) / sizeof(FZ_MODES[0]), FZ_MODE_CELLS = 3 * 2 * 3;   // per mode: format x timeline x index format
template <int P, int MODE, int FMT, int GEO, bool PROF, int IX> static fz_fn fz_cell() {
  if constexpr (fz_exists(P, MODE, FMT, GEO, PROF, IX)) return k_em_fused<P, MODE, FMT, GEO, PROF, IX>;
  else return nullptr;
}
template <int P, int GEO, size_t... C> static fz_fn fz_cells(size_t cell, std::index_sequence<C...>) {
  static const fz_fn tab[] = {fz_cell<P, FZ_MODES[C / FZ_MODE_CELLS], (C / 6) % 3, GEO, (C / 3) % 2 != 0, C % 3>()...};
  return tab[cell];
}
// the kernel of team size P that reads index format `ix` (tsem_index.h); nullptr: no such kernel
template <int P> static fz_fn fz_pick(int mode, int fmt, int geo, bool prof, int ix) {
  int m = 0;
  while (m < FZ_N_MODES && FZ_MODES[m] != mode) ++m;
  if (m == FZ_N_MODES || fmt < 0 || fmt > 2 || ix < 0 || ix > 2) return nullptr;
  const size_t cell = ((size_t)(m * 3 + fmt) * 2 + (prof ? 1 : 0)) * 3 + ix;
  constexpr std::make_index_sequence<FZ_N_MODES * FZ_MODE_CELLS> all{};
  switch (geo) {
    case 0: return fz_cells<P, 0>(cell, all);
    case 1: return fz_cells<P, 1>(cell, all);
    case 2: return fz_cells<P, 2>(cell, all);
    case 3: return fz_cells<P, 3>(cell, all);
    default: return nullptr;
  }
}
