// The mixture model's scalar arithmetic (model.py:631-806), once, for every unit that evaluates it per entry or per column: the pooled
// update (tsem_em.hip), the per-group fits (tsem_cellem.hip) and the bootstrap (tsem_boot.hip).  Those units are compiled with
// -ffp-contract=off, so the grouping of the operations written here IS the result: two callers of one function get the same bits.
#pragma once
#include <hip/hip_runtime.h>

// model.py:718-720 for one entry, both terms as the reference forms them: (Q Y)(pi theta) + (Q (1 - Y)) pi.  tm_numer_qq takes the two
// factors Q Y and Q (1 - Y) from a caller that forms them once per entry for several parameter pairs (the bootstrap's replicates).
__device__ __forceinline__ double tm_numer_qq(double qa, double qu, double pt, double p) { return qa * pt + qu * p; }
__device__ __forceinline__ double tm_numer(double q, double y, double pt, double p) { return tm_numer_qq(q * y, q * (1.0 - y), pt, p); }

// M-step closed forms (model.py:733-740) from a column's thetasum `ts` and pisum0 `ps0`
__device__ __forceinline__ double tm_theta(double ts, double tpw, double den_th) { return (ts + tpw) / den_th; }
__device__ __forceinline__ double tm_pi(double ps0, double ts, double ppw, double den_pi) { return ((ps0 + ts) + ppw) / den_pi; }

// exact twin columns share one accumulation while their sums agree to rounding: the representative's sum, or the column's own
__device__ __forceinline__ double tm_twin(double own, double rep) {
  if (fabs(own - rep) <= 1e-12 * fmax(fabs(own), fabs(rep))) own = rep;
  return own;
}

// prior weights and the closed forms' denominators (model.py:690-697) from the weights' total, their total over the ambiguous rows
// and the largest weight
struct TmPrior { double tpw, den_th, ppw, den_pi; };
__device__ __forceinline__ TmPrior tm_prior(double pi_prior, double theta_prior, int K, double w_tot, double w_amb, double w_max) {
  const double ppw = pi_prior * w_max, tpw = theta_prior * w_max;
  return TmPrior{tpw, w_amb + tpw * K, ppw, w_tot + ppw * K};
}
