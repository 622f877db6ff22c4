// Fused-kernel instantiations for teams of 3 members (one of eight such translation units compiled in parallel, telescope_amd/_lib.py).
#include "tsem_fused_inst.h"

fz_fn tsem_fz_kernel_p3(int P, int mode, int fmt, int geo, bool prof, int ix) {
  return P == 3 ? fz_pick<3>(mode, fmt, geo, prof, ix) : nullptr;
}
