// libtelescope_em.so, bootstrap unit: the reference's mixture model (model.py:631-806) refitted on RESAMPLED fragments — replicate b
// gives every row i a multiplicity m_i in 0..255 and is, by definition, the fit of the matrix in which row i appears m_i times, with
// the score scale of the whole matrix (the per-cell fits' convention, tsem_cellem.hip).  Nothing is resampled in memory: the weighted
// closed form is evaluated over the resident CSR.
//
//   W_tot = sum m w,  W_amb = sum m w Y,  w_max = max of w over the rows with m > 0,  prior weights = prior x w_max,
//   pisum0[j] = sum over unique rows of m Q[i, j];  per iteration thetasum[j] = sum m w z[i, j] over the ambiguous rows.
//
// A BATCH of R <= 8 replicates shares every sweep over the matrix: a row's scores and column ids are read once per phase for the whole
// batch, only the gathers of the parameters and the column sums are per replicate.  The state is dense: per column and replicate
// (pi theta, pi) in one 16-byte pair (the batch's pairs of a column are adjacent: one 128-byte line at R = 8), theta, the sums.
//
// Column sums are fp64 atomics: the H most popular columns (by the stored entries tsem_set_model was given) have workgroup-private
// LDS accumulators for all R replicates, flushed with global atomics when the workgroup's row range ends (every workgroup starts its
// flush at another slot); every other column is added in global memory.  The order of the additions is not fixed: results agree from
// run to run to rounding, not bit for bit — a handle with option "reproducible" is refused.
//
// No workgroup waits for another: a replicate's stop test is taken by the update kernel (the last workgroup to arrive adds the
// per-block parts of diff in block order), which freezes the replicate's parameters and iteration count from then on; the host looks
// at the number of running replicates every few iterations only to stop enqueueing.
//
// Twin columns (tsem_set_model: same rows, same scores in the whole matrix) are twins in every replicate and share one accumulation,
// as in k_update.  Columns that are twins only inside one replicate (the rows that tell them apart drew 0) are not recognised: their
// sums may differ in the last bit, and a tie between them can fall differently from the reference's.
//
// tsem_bootstrap_groups runs the same body (bt_run) with a GROUP SINK: the final sweep's fourth instantiation also adds every value
// m A[i, j] of a row in a group into the slot of (group, j) in the pattern P of the group map (tsem_cells.hip builds it, once per map),
// one fp64 global atomic each, slots x R accumulators per batch; after k_boot_finish a thread per slot folds the batch's replicates, in
// replicate order, into mean and M2 (Welford) and clears the accumulators.  tsem_bootstrap passes no sink and launches what it did.
#include "tsem_internal.h"

namespace {

constexpr int BT_RMAX = 8;                                 // replicates per batch at most: one lane of a row's 8 draws each
constexpr int BT_W = 8;                                    // lanes per row
constexpr int BT_T = 256;                                  // threads per workgroup: 32 rows at a time
constexpr int BT_LDS_SLOTS = 5120;                         // LDS accumulators (hot columns x R) per workgroup at most: 40 KiB
constexpr int BT_LDS_AUTO = 4096;                          // ... by default: 32 KiB, four workgroups per CU
constexpr int BT_SCAL = 12;                                // doubles per replicate of the batch's scalars, see BtScal
constexpr int BT_POLL = 8;                                 // iterations enqueued per look at the number of running replicates
static_assert(BT_W >= BT_RMAX, "lane r of a row draws replicate r's multiplicity");

enum BtScal { S_WTOT = 0, S_WAMB, S_WMAX /* bits */, S_NFRAG /* u64 */, S_TPW, S_DEN_TH, S_PPW, S_DEN_PI, S_LNL };
// ctl: [r] done, [8 + r] iterations, [16 + r] converged, [24] replicates still running, [25] the update kernel's block counter
constexpr int C_DONE = 0, C_ITER = BT_RMAX, C_CONV = 2 * BT_RMAX, C_LIVE = 3 * BT_RMAX, C_BLOCKS = 3 * BT_RMAX + 1, C_WORDS = 32;

struct BtDraw {                                            // the default multiplicities: Poisson(1) by the counter hash
  uint64_t seed;                                           // seed ^ TS_SALT_BOOT
  int64_t row_offset;
  int n_thr;
  uint32_t thr[32];                                        // floor(2^32 P(X <= n)), telescope_amd/synthetic.py poisson_cdf_u32(1.0)
};

struct BtArgs {
  int64_t N;
  int32_t K, R, rep0, H, method;
  double thresh;
  const int64_t* indptr;
  const int32_t* indices;
  const uint16_t* raw;
  const uint8_t* cls;              // [N] 0 empty, 1 unique, 2 ambiguous
  const uint16_t* wcode;           // [N] the row's largest score
  const double* lut;
  const uint8_t* mult;             // explicit multiplicities [n_rep x N], or null
  const int32_t* hot_slot;         // [K] LDS slot of a hot column, -1
  const int32_t* hot_col;          // [H] the hot columns, most popular first
  const double2* tab;              // [K x R] (pi theta, pi): the E-step's parameters
  const double2* tab2;             // [K x R] final sweep: the parameters after the last M-step
  double* acc;                     // [K x R] column sums of the sweep
  double* scal;                    // [R x BT_SCAL]
  const uint32_t* ctl;
  int64_t rows_per_block;
  BtDraw draw;
  // the group sink of the final sweep (MODE 3): the row -> group map, the pattern P and the batch's accumulators, one per slot and replicate
  const int32_t* grp;              // [N] -1 = none
  int32_t G;
  const int64_t* gptr;             // [G + 1] first slot of every group
  const int32_t* gcols;            // [slots] the slots' columns, ascending within a group
  double* gacc;                    // [slots x R]
};

__device__ __forceinline__ uint32_t bt_draw(const BtDraw& D, int64_t row, int rep) {
  const uint32_t hsh = (uint32_t)(ts_hash3(D.seed, (uint64_t)(D.row_offset + row), (uint64_t)rep) >> 32);
  uint32_t m = 0;
  for (int n = 0; n < D.n_thr; ++n) m += D.thr[n] <= hsh ? 1u : 0u;
  return m;
}
// one value into column `col` of replicate r: LDS for a hot column, global otherwise
__device__ __forceinline__ void bt_add(const BtArgs& A, double* hot, int col, int slot, int r, double v) {
  if (slot >= 0) atomicAdd(&hot[slot * A.R + r], v);
  else atomicAdd(&A.acc[(int64_t)col * A.R + r], v);
}

// The sweep over the CSR rows for one batch.  MODE 0: the replicates' statistics and pisum0 (into acc); 1: one E-step and the column
// sums of the M-step for the replicates still running; 2: the last E-step again, the log-likelihood and the counts of one method;
// 3: what 2 does and, for every value m v != 0 of a row in a group, one fp64 atomic into the slot of (group, column) in the pattern P —
// the group and its slots' range are read once per row and shared by the row's 8 lanes, the slot is found by a binary search in the
// group's columns.  A workgroup takes a contiguous range of rows, 8 lanes a row.
template <int MODE>
__global__ __launch_bounds__(BT_T) void k_boot_sweep(BtArgs A) {
  extern __shared__ double bt_hot[];                       // [H x R]
  __shared__ double red[BT_T / 64];
  __shared__ double st_sum[BT_RMAX][2];
  __shared__ unsigned long long st_bits[BT_RMAX][2];
  const int tid = threadIdx.x, sub = tid & (BT_W - 1), R = A.R;
  const int n_hot = A.H * R;
  uint64_t live = 0;                                       // 0xFF per replicate the sweep works for
  for (int r = 0; r < R; ++r)
    if (MODE != 1 || !A.ctl[C_DONE + r]) live |= 0xFFull << (8 * r);
  if (!live) return;
  for (int i = tid; i < n_hot; i += BT_T) bt_hot[i] = 0.0;
  if (MODE == 0 && tid < BT_RMAX) { st_sum[tid][0] = st_sum[tid][1] = 0.0; st_bits[tid][0] = st_bits[tid][1] = 0ull; }
  __syncthreads();
  const int64_t row0 = (int64_t)blockIdx.x * A.rows_per_block, row1 = min(A.N, row0 + A.rows_per_block);
  double tw = 0.0, aw = 0.0, wm = 0.0;                     // MODE 0: lane r's sums of replicate r
  unsigned long long nf = 0;
  double lnl[BT_RMAX];
#pragma unroll
  for (int r = 0; r < BT_RMAX; ++r) lnl[r] = 0.0;

  for (int64_t row = row0 + (tid >> 3); row < row1; row += BT_T / BT_W) {
    // ---- the row's multiplicities: lane r takes replicate r's, the 8 lanes then share them as the bytes of one word ----
    uint64_t mm = 0;
    if (sub < R) mm = (uint64_t)(A.mult ? A.mult[(int64_t)(A.rep0 + sub) * A.N + row] : bt_draw(A.draw, row, A.rep0 + sub)) << (8 * sub);
    const int cls = A.cls[row];
    const double w = cls ? A.lut[A.wcode[row]] : 0.0, y = cls == 2 ? 1.0 : 0.0;
    if constexpr (MODE == 0) {
      const double m = (double)(mm >> (8 * sub));
      tw += m * w; aw += (m * w) * y; nf += mm >> (8 * sub);
      if (mm) wm = fmax(wm, w);
    }
#pragma unroll
    for (int o = BT_W / 2; o > 0; o >>= 1) mm |= __shfl_xor(mm, o, BT_W);
    mm &= live;
    if (!mm || !cls) continue;
    const int64_t a = A.indptr[row], b = A.indptr[row + 1];
    [[maybe_unused]] int64_t glo = 0, ghi = 0;             // MODE 3: the slots of the row's group (none: the row is in no group)
    if constexpr (MODE == 3) {
      const int32_t g = __shfl(sub == 0 ? A.grp[row] : 0, 0, BT_W);
      if ((uint32_t)g < (uint32_t)A.G) {
        const int64_t p = sub < 2 ? A.gptr[g + sub] : 0;
        glo = __shfl(p, 0, BT_W); ghi = __shfl(p, 1, BT_W);
      }
    }

    if constexpr (MODE == 0) {                             // pisum0 (model.py:699): the unique rows' Q
      if (cls == 1) {
        for (int64_t e = a + sub; e < b; e += BT_W) {
          const int col = A.indices[e];
          const int slot = A.H ? A.hot_slot[col] : -1;
          const double q = A.lut[A.raw[e]];
          for (int r = 0; r < R; ++r) {
            const double m = (double)((mm >> (8 * r)) & 0xFFu);
            if (m != 0.0 && q != 0.0) bt_add(A, bt_hot, col, slot, r, m * q);
          }
        }
      }
    } else if constexpr (MODE == 1) {
      // ---- E-step (model.py:702-722): row sums of the numerators (Q Y)(pi theta) + (Q (1 - Y)) pi, all replicates per entry ----
      double s[BT_RMAX];
#pragma unroll
      for (int r = 0; r < BT_RMAX; ++r) s[r] = 0.0;
      for (int64_t e = a + sub; e < b; e += BT_W) {
        const double q = A.lut[A.raw[e]], qa = q * y, qu = q * (1.0 - y);
        const double2* t = A.tab + (int64_t)A.indices[e] * R;
#pragma unroll
        for (int r = 0; r < BT_RMAX; ++r)
          if (r < R && ((mm >> (8 * r)) & 0xFFu)) { const double2 cp = t[r]; s[r] += tm_numer_qq(qa, qu, cp.x, cp.y); }
      }
#pragma unroll
      for (int r = 0; r < BT_RMAX; ++r)
        if (r < R) s[r] = recip0(sg_sum<BT_W>(s[r]));
      // ---- the M-step's sums (model.py:724-729): m w z Y per entry; products that are exactly zero are not in z's pattern ----
      for (int64_t e = a + sub; e < b; e += BT_W) {
        const int col = A.indices[e];
        const int slot = A.H ? A.hot_slot[col] : -1;
        const double q = A.lut[A.raw[e]], qa = q * y, qu = q * (1.0 - y);
        const double2* t = A.tab + (int64_t)col * R;
#pragma unroll
        for (int r = 0; r < BT_RMAX; ++r) {
          const uint32_t mr = (uint32_t)(mm >> (8 * r)) & 0xFFu;
          if (r < R && mr) {
            const double2 cp = t[r];
            const double n = tm_numer_qq(qa, qu, cp.x, cp.y);
            const double v = n != 0.0 ? (((n * s[r]) * w) * y) * (double)mr : 0.0;
            if (v != 0.0) bt_add(A, bt_hot, col, slot, r, v);      // (a unique row adds nothing — unless its z is NaN, which spreads)
          }
        }
      }
    } else {
      // ---- the last E-step's z (model.py:795) from tab, calculate_lnl against tab2 (model.py:744-760, 800-801), reassign (:837-862) ----
#pragma unroll
      for (int r = 0; r < BT_RMAX; ++r) {
        const uint32_t mr = (uint32_t)(mm >> (8 * r)) & 0xFFu;
        if (r >= R || !mr) continue;
        const double m = (double)mr;
        double sum = 0.0;
        for (int64_t e = a + sub; e < b; e += BT_W) {
          const double q = A.lut[A.raw[e]];
          const double2 cp = A.tab[(int64_t)A.indices[e] * R + r];
          sum += tm_numer(q, y, cp.x, cp.y);
        }
        const double rinv = recip0(sg_sum<BT_W>(sum));
        double zmax = -INFINITY, cs = 0.0;
        int hole = (b - a) < A.K ? 1 : 0;                    // the row maximum counts the zeros that are not stored (sparse_plus.py:117-129)
        for (int64_t e = a + sub; e < b; e += BT_W) {
          const double q = A.lut[A.raw[e]], qa = q * y, qu = q * (1.0 - y);
          const int64_t ix = (int64_t)A.indices[e] * R + r;
          const double2 cp = A.tab[ix], cq = A.tab2[ix];
          const double n = tm_numer_qq(qa, qu, cp.x, cp.y);
          if (n != 0.0) {
            const double z = n * rinv, n2 = tm_numer_qq(qa, qu, cq.x, cq.y);
            zmax = fmax(zmax, z);
            if (z >= A.thresh) cs += z;
            if (n2 != 0.0) lnl[r] += m * (z * log1p(n2));
          } else {
            hole = 1;
          }
        }
        zmax = sg_max<BT_W>(zmax); cs = sg_sum<BT_W>(cs); hole = sg_max_i<BT_W>(hole);
        if (hole) zmax = fmax(zmax, 0.0);
        int best = 0;
        if (A.method == TSEM_RA_EXCLUDE || A.method == TSEM_RA_AVERAGE) {
          for (int64_t e = a + sub; e < b; e += BT_W) {
            const double q = A.lut[A.raw[e]];
            const double2 cp = A.tab[(int64_t)A.indices[e] * R + r];
            const double n = tm_numer(q, y, cp.x, cp.y);
            if (n != 0.0 && n * rinv == zmax) ++best;
          }
          best = sg_sum_i<BT_W>(best);
        }
        const double share = A.method == TSEM_RA_AVERAGE ? recip0((double)best) : recip0(cs);
        for (int64_t e = a + sub; e < b; e += BT_W) {
          const int col = A.indices[e];
          const double q = A.lut[A.raw[e]];
          const double2 cp = A.tab[(int64_t)col * R + r];
          const double n = tm_numer(q, y, cp.x, cp.y);
          if (n == 0.0) continue;
          const double z = n * rinv;
          double v;
          switch (A.method) {
            case TSEM_RA_EXCLUDE: v = (z == zmax && best == 1) ? 1.0 : 0.0; break;
            case TSEM_RA_AVERAGE: v = z == zmax ? 1.0 * share : 0.0; break;
            case TSEM_RA_CONF: v = z >= A.thresh ? z * share : 0.0; break;
            case TSEM_RA_UNIQUE: v = ceil(z * (1.0 - y)); break;
            default: v = z > 0.0 ? 1.0 : 0.0; break;         // all
          }
          if (v != 0.0) bt_add(A, bt_hot, col, A.H ? A.hot_slot[col] : -1, r, m * v);
          if constexpr (MODE == 3) {
            if (v != 0.0 && glo < ghi) {
              int64_t lo = glo, hi = ghi;
              while (lo < hi) {
                const int64_t mid = lo + (hi - lo) / 2;
                if (A.gcols[mid] < col) lo = mid + 1; else hi = mid;
              }
              if (lo < ghi && A.gcols[lo] == col) atomicAdd(&A.gacc[lo * R + r], m * v);   // (P holds every stored (group, column))
            }
          }
        }
      }
    }
  }

  // ---- the workgroup's scalars ----
  if constexpr (MODE == 0) {
    if (sub < R) {
      atomicAdd(&st_sum[sub][0], tw); atomicAdd(&st_sum[sub][1], aw);
      atomicMax(&st_bits[sub][0], (unsigned long long)__double_as_longlong(wm));   // (w >= 0: the bit patterns order like the values)
      atomicAdd(&st_bits[sub][1], nf);
    }
    __syncthreads();
    if (tid < R) {
      double* sc = A.scal + tid * BT_SCAL;
      atomicAdd(&sc[S_WTOT], st_sum[tid][0]); atomicAdd(&sc[S_WAMB], st_sum[tid][1]);
      atomicMax((unsigned long long*)&sc[S_WMAX], st_bits[tid][0]);
      atomicAdd((unsigned long long*)&sc[S_NFRAG], st_bits[tid][1]);
    }
  }
  if constexpr (MODE >= 2) {
#pragma unroll
    for (int r = 0; r < BT_RMAX; ++r) {
      if (r >= R) continue;                                  // (uniform)
      double v = sg_sum<64>(lnl[r]);
      __syncthreads();
      if ((tid & 63) == 0) red[tid >> 6] = v;
      __syncthreads();
      if (tid == 0) {
        v = 0.0;
        for (int i = 0; i < BT_T / 64; ++i) v += red[i];
        if (v != 0.0) atomicAdd(&A.scal[r * BT_SCAL + S_LNL], v);
      }
    }
  }
  // ---- flush the hot columns' accumulators: every workgroup starts at another slot ----
  __syncthreads();
  if (n_hot) {
    const int start = (int)(((int64_t)blockIdx.x * 67 * R) % n_hot);
    for (int i = tid; i < n_hot; i += BT_T) {
      int k = i + start;
      if (k >= n_hot) k -= n_hot;
      const double v = bt_hot[k];
      if (v != 0.0) atomicAdd(&A.acc[(int64_t)A.hot_col[k / R] * R + k % R], v);
    }
  }
}

// the batch's start: prior weights and denominators (model.py:690-697) from the statistics, pi = theta = 1 / K (model.py:667, 673);
// a replicate without fragments is not fitted: done from the start, NaN parameters
__global__ __launch_bounds__(256) void k_boot_init(int K, int R, double pi_prior, double theta_prior, double* __restrict__ scal,
                                                   uint32_t* __restrict__ ctl, double2* __restrict__ tab, double2* __restrict__ tab_prev,
                                                   double* __restrict__ theta) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  const double nan = __longlong_as_double(0x7FF8000000000000ll);
  if (j < K)
    for (int r = 0; r < R; ++r) {
      const double v = __double_as_longlong(scal[r * BT_SCAL + S_NFRAG]) ? 1.0 / K : nan;
      tab[(int64_t)j * R + r] = tab_prev[(int64_t)j * R + r] = make_double2(v * v, v);
      theta[(int64_t)j * R + r] = v;
    }
  if (blockIdx.x == 0 && threadIdx.x < C_WORDS) {
    const int t = threadIdx.x;
    int live = 0;
    for (int r = 0; r < R; ++r) live += __double_as_longlong(scal[r * BT_SCAL + S_NFRAG]) ? 1 : 0;
    uint32_t v = 0;
    if (t < BT_RMAX) v = (t < R && __double_as_longlong(scal[t * BT_SCAL + S_NFRAG])) ? 0u : 1u;
    else if (t == C_LIVE) v = (uint32_t)live;
    ctl[t] = v;
    if (t < R) {
      double* sc = scal + t * BT_SCAL;
      const double wmax = sc[S_WMAX];                      // (the bits of the largest weight are the value)
      const TmPrior P = tm_prior(pi_prior, theta_prior, K, sc[S_WTOT], sc[S_WAMB], wmax);
      sc[S_TPW] = P.tpw; sc[S_DEN_TH] = P.den_th; sc[S_PPW] = P.ppw; sc[S_DEN_PI] = P.den_pi;
    }
  }
}

// M-step closed forms (model.py:733-740) of every running replicate of the batch, diff_est (model.py:781) and the stop test
// (model.py:792): a thread per column.  The last workgroup to arrive adds the per-block parts of diff in block order and ends a
// replicate on diff < eps or at max_iter; an ended replicate is left alone by every later launch.
__global__ __launch_bounds__(256) void k_boot_update(int K, int R, double eps, int max_iter, const double* __restrict__ acc,
                                                     const double* __restrict__ ps0, const double* __restrict__ scal,
                                                     const int32_t* __restrict__ twin_rep, double2* __restrict__ tab,
                                                     double2* __restrict__ tab_prev, double* __restrict__ theta,
                                                     double* __restrict__ diff_part, uint32_t* __restrict__ ctl) {
  __shared__ double scratch[16];
  __shared__ bool last;
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  uint32_t done = 0;
  for (int r = 0; r < R; ++r) done |= (ctl[C_DONE + r] ? 1u : 0u) << r;
  if (done == (1u << R) - 1u) return;                      // nothing is running
  double d[BT_RMAX];
#pragma unroll
  for (int r = 0; r < BT_RMAX; ++r) {
    d[r] = 0.0;
    if (r >= R || j >= K || ((done >> r) & 1u)) continue;
    const int64_t ix = (int64_t)j * R + r;
    const int jr = twin_rep[j];
    double ts = acc[ix], ps = ps0[ix];
    if (jr != j) { ts = tm_twin(ts, acc[(int64_t)jr * R + r]); ps = tm_twin(ps, ps0[(int64_t)jr * R + r]); }   // (tsem_model.h)
    const double* sc = scal + r * BT_SCAL;
    const double th = tm_theta(ts, sc[S_TPW], sc[S_DEN_TH]);
    const double ph = tm_pi(ps, ts, sc[S_PPW], sc[S_DEN_PI]);
    const double2 old = tab[ix];
    d[r] = fabs(ph - old.y);
    tab_prev[ix] = old;
    tab[ix] = make_double2(ph * th, ph);
    theta[ix] = th;
  }
#pragma unroll
  for (int r = 0; r < BT_RMAX; ++r) {
    if (r >= R) continue;
    const double t = block_sum(d[r], scratch);
    if (threadIdx.x == 0) diff_part[(int64_t)blockIdx.x * BT_RMAX + r] = t;
  }
  if (threadIdx.x == 0) {
    __threadfence();
    last = atomicAdd(&ctl[C_BLOCKS], 1u) == gridDim.x - 1;
  }
  __syncthreads();
  if (!last) return;
  __threadfence();
#pragma unroll
  for (int r = 0; r < BT_RMAX; ++r) {
    if (r >= R) continue;
    double v = 0.0;
    for (int i = threadIdx.x; i < (int)gridDim.x; i += blockDim.x)
      v += __hip_atomic_load(&diff_part[(int64_t)i * BT_RMAX + r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const double diff = block_sum(v, scratch);
    if (threadIdx.x == 0 && !((done >> r) & 1u)) {
      const uint32_t it = ctl[C_ITER + r] + 1u;
      const bool conv = diff < eps;                        // (NaN: never)
      ctl[C_ITER + r] = it;
      if (conv || it >= (uint32_t)max_iter) { ctl[C_DONE + r] = 1u; ctl[C_CONV + r] = conv ? 1u : 0u; ctl[C_LIVE] -= 1u; }
    }
  }
  if (threadIdx.x == 0) ctl[C_BLOCKS] = 0u;
}

// the batch's results into the call's arrays (replicate-major).  A replicate without fragments, or whose log-likelihood is NaN
// (NaN parameters), has NaN counts and NaN lnl.
__global__ __launch_bounds__(256) void k_boot_finish(int K, int R, int rep0, const double* __restrict__ scal, const uint32_t* __restrict__ ctl,
                                                     const double2* __restrict__ tab, const double* __restrict__ theta,
                                                     const double* __restrict__ acc, double* __restrict__ pi_out,
                                                     double* __restrict__ theta_out, double* __restrict__ counts_out,
                                                     unsigned long long* __restrict__ nfrags, int32_t* __restrict__ n_iter,
                                                     int32_t* __restrict__ conv, double* __restrict__ lnl) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  const double nan = __longlong_as_double(0x7FF8000000000000ll);
  for (int r = 0; r < R; ++r) {
    const unsigned long long nf = (unsigned long long)__double_as_longlong(scal[r * BT_SCAL + S_NFRAG]);
    const double l = scal[r * BT_SCAL + S_LNL];
    const bool bad = nf == 0ull || isnan(l);
    if (j < K) {
      const int64_t ix = (int64_t)j * R + r, ox = (int64_t)(rep0 + r) * K + j;
      pi_out[ox] = tab[ix].y; theta_out[ox] = theta[ix]; counts_out[ox] = bad ? nan : acc[ix];
    }
    if (j == 0) {
      nfrags[rep0 + r] = nf; n_iter[rep0 + r] = (int32_t)ctl[C_ITER + r]; conv[rep0 + r] = (int32_t)ctl[C_CONV + r];
      lnl[rep0 + r] = bad ? nan : l;
    }
  }
}

// The group sink's fold, after k_boot_finish of the batch: a thread per slot of P takes the batch's replicates in replicate order —
// a good one (fragments, and a log-likelihood that is not NaN: k_boot_finish's test, the same words) by Welford's update, d = x - mean;
// mean += d / k; M2 += d (x - mean) — keeps the values where asked (NaN for a bad replicate) and clears the accumulators.
__global__ __launch_bounds__(256) void k_boot_fold(int64_t n_slots, int R, int rep0, const double* __restrict__ scal,
                                                   const int32_t* __restrict__ used, double* __restrict__ gacc, double* __restrict__ mean,
                                                   double* __restrict__ m2, double* __restrict__ values) {
  const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n_slots) return;
  const double nan = __longlong_as_double(0x7FF8000000000000ll);
  int k = used[0];
  double mu = mean[s], q = m2[s];
  for (int r = 0; r < R; ++r) {
    const bool good = __double_as_longlong(scal[r * BT_SCAL + S_NFRAG]) != 0ll && !isnan(scal[r * BT_SCAL + S_LNL]);
    const double x = gacc[s * R + r];
    if (good) {
      ++k;
      const double d = x - mu;
      mu += d / (double)k;
      q += d * (x - mu);
    }
    if (values) values[(int64_t)(rep0 + r) * n_slots + s] = good ? x : nan;
    gacc[s * R + r] = 0.0;
  }
  mean[s] = mu; m2[s] = q;
}
// ... the good replicates so far (after the fold that read the count)
__global__ void k_boot_fold_count(int R, const double* __restrict__ scal, int32_t* __restrict__ used) {
  if (blockIdx.x || threadIdx.x) return;
  int k = used[0];
  for (int r = 0; r < R; ++r)
    k += (__double_as_longlong(scal[r * BT_SCAL + S_NFRAG]) != 0ll && !isnan(scal[r * BT_SCAL + S_LNL])) ? 1 : 0;
  used[0] = k;
}
// ... and after the last batch: NaN means without a good replicate, M2 into sd (ddof 1; NaN below two good replicates)
__global__ __launch_bounds__(256) void k_boot_fold_end(int64_t n_slots, const int32_t* __restrict__ used, double* __restrict__ mean,
                                                       double* __restrict__ m2) {
  const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n_slots) return;
  const double nan = __longlong_as_double(0x7FF8000000000000ll);
  const int k = used[0];
  if (k < 1) mean[s] = nan;
  m2[s] = k < 2 ? nan : sqrt(m2[s] / (double)(k - 1));
}

__global__ void k_boot_mult(BtDraw D, int rep, int64_t row_begin, int64_t n, uint8_t* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = (uint8_t)bt_draw(D, row_begin + i, rep);
}

BtDraw bt_make_draw(const tsem_ctx* h, uint64_t seed) {
  BtDraw D{};
  D.seed = seed ^ TS_SALT_BOOT;
  D.row_offset = h->row_offset;
  // synthetic.py poisson_cdf_u32(1.0), the same operations in the same order
  const double mean = 1.0;
  double p = std::exp(-mean), cdf = p;
  int n = 0;
  while (cdf < 1.0 - 1e-12 && n < 4 * (int)mean + 64 && D.n_thr < 32) {
    D.thr[D.n_thr++] = (uint32_t)std::min<long long>((long long)(cdf * 4294967296.0), 4294967295ll);
    ++n;
    p *= mean / n;
    cdf += p;
  }
  return D;
}

void bt_free(tsem_ctx* h) {
  dfree(h->d_bt_pi); dfree(h->d_bt_theta); dfree(h->d_bt_counts); dfree(h->d_bt_lnl); dfree(h->d_bt_nfrags); dfree(h->d_bt_niter);
  dfree(h->d_bt_conv);
  dfree(h->d_bg_mean); dfree(h->d_bg_sd); dfree(h->d_bg_vals);
  h->bt_nrep = 0; h->bt_R = h->bt_H = 0;
  h->bg_nrep = h->bg_used = h->bg_kept = h->bg_groups = 0; h->bg_nnz = 0;
}

template <int MODE>
int bt_sweep(tsem_ctx* h, const BtArgs& A, int grid) {
  k_boot_sweep<MODE><<<grid, BT_T, 8 * (size_t)A.H * A.R, h->stream>>>(A);
  TSEM_HIP(hipGetLastError());
  return TSEM_OK;
}

struct BtSink { int keep_values; };                        // tsem_bootstrap_groups: per-group statistics beside the plain results

// the body of tsem_bootstrap and tsem_bootstrap_groups: the latter passes a sink, which changes the final sweep's instantiation (the
// pattern's accumulators), adds the fold after every batch and may lower the batch; without one nothing differs from before
int bt_run(tsem_ctx* h, int32_t n_rep, uint64_t seed, const uint8_t* mult, int32_t method, double thresh, double epsilon, int32_t max_iter,
           const BtSink* sink) {
  if (!h || !h->d_indptr) return TSEM_ERR_ARG;
  if (int rc = ensure_device(h)) return rc;
  const std::string who = sink ? "tsem_bootstrap_groups" : "tsem_bootstrap";
  if (tsem_comm_on(h)) TSEM_FAIL(TSEM_ERR_ARG, who + ": row-sharded handles are not supported (one GPU per run)");
  if (h->opt_reproducible)
    TSEM_FAIL(TSEM_ERR_ARG, who + ": option \"reproducible\" is set, and the bootstrap's column sums are unordered fp64 atomics: not supported");
  if (!h->have_rowstats || !h->d_row_cls || !h->d_row_code) TSEM_FAIL(TSEM_ERR_ARG, who + ": no row statistics (tsem_rowstats)");
  if (!h->d_lut || h->lut_len <= 0) TSEM_FAIL(TSEM_ERR_ARG, who + ": no score table (tsem_set_lut)");
  if (!h->have_model || !h->d_twin_rep) TSEM_FAIL(TSEM_ERR_ARG, who + ": no model (tsem_set_model gives the priors and the twin classes)");
  if (h->K <= 0) TSEM_FAIL(TSEM_ERR_ARG, who + ": the matrix has no columns");
  if (n_rep < 1) TSEM_FAIL(TSEM_ERR_ARG, who + ": n_rep must be at least 1");
  if (max_iter < 1) TSEM_FAIL(TSEM_ERR_ARG, who + ": max_iter must be at least 1");
  if (method != TSEM_RA_EXCLUDE && method != TSEM_RA_AVERAGE && method != TSEM_RA_CONF && method != TSEM_RA_UNIQUE && method != TSEM_RA_ALL)
    TSEM_FAIL(TSEM_ERR_ARG, who + ": method must be exclude, average, conf, unique or all (choose draws per row from numpy's stream: not offered)");
  if (sink && !h->d_group && h->N) TSEM_FAIL(TSEM_ERR_ARG, who + ": no group map (tsem_set_groups)");
  bt_free(h);
  const int K = h->K;
  const int64_t N = h->N;
  if (sink) if (int rc = tsem_build_group_pattern(h)) return rc;
  const int64_t n_slots = sink ? h->bp_nnz : 0;
  const int64_t stat_bytes = sink ? 16 * n_slots + (sink->keep_values ? 8 * (int64_t)n_rep * n_slots : 0) : 0;
  const int64_t mult_bytes = mult ? (int64_t)n_rep * N : 0;
  const int64_t res_bytes = 3 * 8 * (int64_t)n_rep * K + 32 * (int64_t)n_rep + stat_bytes;
  auto ws_of = [&](int r) { return (int64_t)K * r * (16 + 16 + 8 + 8 + 8) + 8 * (int64_t)K + (1 << 20); };
  size_t free_b = 0, total_b = 0;
  TSEM_HIP(hipMemGetInfo(&free_b, &total_b));
  // batch and hot columns: options "boot_batch" / "boot_hot_columns", else the LDS budget
  int R = (int)std::min<int64_t>(n_rep, h->opt_boot_batch > 0 ? std::min<int64_t>(h->opt_boot_batch, BT_RMAX) : BT_RMAX);
  if (n_slots > 0) {
    // the sink's accumulators, slots x batch doubles: within option "boot_group_bytes" and what is free beside everything else; a
    // smaller batch where the batch asked for does not fit
    auto room = [&](int r) {
      const int64_t avail = (int64_t)free_b - res_bytes - ws_of(r) - mult_bytes - (64ll << 20);
      return h->opt_boot_group > 0 ? std::min<int64_t>(h->opt_boot_group, avail) : avail;
    };
    while (R > 1 && 8 * n_slots * R > room(R)) --R;
    if (8 * n_slots > room(1))
      TSEM_FAIL(TSEM_ERR_NOMEM, who + ": the accumulators of " + std::to_string(n_slots) + " (group, column) slots need " + std::to_string(8 * n_slots) +
                " B per replicate of a batch; " + std::to_string(std::max<int64_t>(0, room(1))) + " B are allowed (option \"boot_group_bytes\" " +
                std::to_string(h->opt_boot_group) + ", " + std::to_string(free_b) + " B free, " + std::to_string(res_bytes + ws_of(1) + mult_bytes) +
                " B of results, workspace and multiplicities)");
  }
  const int64_t acc_bytes = 8 * n_slots * R;
  std::vector<int32_t> hot_col;
  {
    const int64_t want = h->opt_boot_hot < 0 ? BT_LDS_AUTO / R : std::min<int64_t>(h->opt_boot_hot, BT_LDS_SLOTS / R);
    std::vector<int32_t> ord;
    for (int j = 0; j < K && want > 0; ++j)
      if ((size_t)j < h->col_count.size() && h->col_count[j] > 0) ord.push_back(j);
    const size_t H = (size_t)std::min<int64_t>(want, (int64_t)ord.size());
    std::partial_sort(ord.begin(), ord.begin() + H, ord.end(), [&](int32_t a, int32_t b) {
      return h->col_count[a] != h->col_count[b] ? h->col_count[a] > h->col_count[b] : a < b;
    });
    hot_col.assign(ord.begin(), ord.begin() + H);
  }
  const int H = (int)hot_col.size();
  const int64_t ws_bytes = ws_of(R) + acc_bytes;
  if ((int64_t)free_b < res_bytes + ws_bytes + mult_bytes + (64ll << 20))
    TSEM_FAIL(TSEM_ERR_NOMEM, who + ": " + std::to_string(n_rep) + " replicates need " + std::to_string(res_bytes + ws_bytes + mult_bytes) +
              " B of device memory (" + std::to_string(mult_bytes) + " B of them the multiplicities given); " + std::to_string(free_b) + " B are free");
  CsrIds ids(h);
  if (int rc = ids.acquire()) return rc;
  PhaseTimer pt(h->stream);
  TSEM_ALLOC(h->d_bt_pi, (int64_t)n_rep * K); TSEM_ALLOC(h->d_bt_theta, (int64_t)n_rep * K); TSEM_ALLOC(h->d_bt_counts, (int64_t)n_rep * K);
  TSEM_ALLOC(h->d_bt_lnl, n_rep); TSEM_ALLOC(h->d_bt_nfrags, n_rep); TSEM_ALLOC(h->d_bt_niter, n_rep); TSEM_ALLOC(h->d_bt_conv, n_rep);
  DevTmp t_mult, t_slot, t_hcol, t_tab, t_prev, t_theta, t_acc, t_ps0, t_scal, t_ctl, t_diff, t_gacc, t_used;
  if (sink) {
    TSEM_ALLOC(h->d_bg_mean, n_slots); TSEM_ALLOC(h->d_bg_sd, n_slots);
    if (sink->keep_values) TSEM_ALLOC(h->d_bg_vals, (int64_t)n_rep * n_slots);
    TSEM_TMP(t_used, 4);
    TSEM_HIP(hipMemsetAsync(t_used.p, 0, 4, h->stream));
    if (n_slots > 0) {
      TSEM_TMP(t_gacc, acc_bytes);
      TSEM_HIP(hipMemsetAsync(t_gacc.p, 0, (size_t)acc_bytes, h->stream));
      TSEM_HIP(hipMemsetAsync(h->d_bg_mean, 0, 8 * (size_t)n_slots, h->stream));
      TSEM_HIP(hipMemsetAsync(h->d_bg_sd, 0, 8 * (size_t)n_slots, h->stream));
    }
  }
  const int ugrid = cdiv64(K, 256);
  TSEM_TMP(t_slot, 4 * (int64_t)K); TSEM_TMP(t_hcol, 4 * (int64_t)std::max(1, H));
  TSEM_TMP(t_tab, 16 * (int64_t)K * R); TSEM_TMP(t_prev, 16 * (int64_t)K * R); TSEM_TMP(t_theta, 8 * (int64_t)K * R);
  TSEM_TMP(t_acc, 8 * (int64_t)K * R); TSEM_TMP(t_ps0, 8 * (int64_t)K * R);
  TSEM_TMP(t_scal, 8 * BT_RMAX * BT_SCAL); TSEM_TMP(t_ctl, 4 * C_WORDS); TSEM_TMP(t_diff, 8 * (int64_t)ugrid * BT_RMAX);
  if (mult) {
    TSEM_TMP(t_mult, mult_bytes);
    TSEM_HIP(hipMemcpyAsync(t_mult.p, mult, (size_t)mult_bytes, hipMemcpyHostToDevice, h->stream));
  }
  {
    std::vector<int32_t> slot((size_t)K, -1);
    for (int s = 0; s < H; ++s) slot[hot_col[s]] = s;
    TSEM_HIP(hipMemcpyAsync(t_slot.p, slot.data(), 4 * (size_t)K, hipMemcpyHostToDevice, h->stream));
    if (H) TSEM_HIP(hipMemcpyAsync(t_hcol.p, hot_col.data(), 4 * (size_t)H, hipMemcpyHostToDevice, h->stream));
    TSEM_HIP(hipStreamSynchronize(h->stream));               // (the host vectors go out of scope)
  }
  BtArgs A{};
  A.N = N; A.K = K; A.H = H; A.method = method; A.thresh = thresh;
  A.indptr = h->d_indptr; A.indices = h->d_indices; A.raw = h->d_raw; A.cls = h->d_row_cls; A.wcode = h->d_row_code; A.lut = h->d_lut;
  A.mult = t_mult.as<uint8_t>(); A.hot_slot = t_slot.as<int32_t>(); A.hot_col = t_hcol.as<int32_t>();
  A.scal = t_scal.as<double>(); A.ctl = t_ctl.as<uint32_t>();
  A.draw = bt_make_draw(h, seed);
  A.grp = h->d_group; A.G = h->n_groups; A.gptr = h->d_bp_gptr; A.gcols = h->d_bp_cols; A.gacc = t_gacc.as<double>();
  const int fgrid = cdiv64(n_slots, 256);
  // a contiguous range of rows per workgroup (its LDS accumulators are flushed once), four workgroups per CU
  const int rows_at_once = BT_T / BT_W;
  A.rows_per_block = std::max<int64_t>(rows_at_once, ((N + 4ll * h->n_cu - 1) / (4ll * h->n_cu) + rows_at_once - 1) / rows_at_once * rows_at_once);
  if (h->opt_boot_rows > 0)                                  // option "boot_rows_per_block": a test and timing hook
    A.rows_per_block = (std::min<int64_t>(h->opt_boot_rows, 1ll << 40) + rows_at_once - 1) / rows_at_once * rows_at_once;
  const int grid = cdiv64(N, A.rows_per_block);
  double2 *tab = t_tab.as<double2>(), *prev = t_prev.as<double2>();
  for (int rep0 = 0; rep0 < n_rep; rep0 += R) {
    const int Rb = std::min(R, n_rep - rep0);
    A.R = Rb; A.rep0 = rep0;
    // ---- statistics and pisum0 ----
    TSEM_HIP(hipMemsetAsync(t_scal.p, 0, 8 * BT_RMAX * BT_SCAL, h->stream));
    TSEM_HIP(hipMemsetAsync(t_ps0.p, 0, 8 * (size_t)K * Rb, h->stream));
    A.acc = t_ps0.as<double>(); A.tab = tab; A.tab2 = tab;
    if (grid > 0) if (int rc = bt_sweep<0>(h, A, grid)) return rc;
    k_boot_init<<<ugrid, 256, 0, h->stream>>>(K, Rb, h->pi_prior, h->theta_prior, t_scal.as<double>(), t_ctl.as<uint32_t>(), tab, prev,
                                             t_theta.as<double>());
    TSEM_HIP(hipGetLastError());
    // ---- the iterations: E-step and column sums, update; the host looks every BT_POLL iterations whether anything still runs ----
    A.acc = t_acc.as<double>();
    for (int it = 0; it < max_iter;) {
      const int n = std::min(BT_POLL, max_iter - it);
      for (int k = 0; k < n; ++k) {
        TSEM_HIP(hipMemsetAsync(t_acc.p, 0, 8 * (size_t)K * Rb, h->stream));
        if (grid > 0) if (int rc = bt_sweep<1>(h, A, grid)) return rc;
        k_boot_update<<<ugrid, 256, 0, h->stream>>>(K, Rb, epsilon, max_iter, t_acc.as<double>(), t_ps0.as<double>(), t_scal.as<double>(),
                                                   h->d_twin_rep, tab, prev, t_theta.as<double>(), t_diff.as<double>(), t_ctl.as<uint32_t>());
        TSEM_HIP(hipGetLastError());
      }
      it += n;
      uint32_t live = 0;
      TSEM_HIP(hipMemcpyAsync(&live, t_ctl.as<uint32_t>() + C_LIVE, 4, hipMemcpyDeviceToHost, h->stream));
      TSEM_HIP(hipStreamSynchronize(h->stream));
      if (!live) break;
    }
    // ---- the last E-step again: lnl and counts ----
    TSEM_HIP(hipMemsetAsync(t_acc.p, 0, 8 * (size_t)K * Rb, h->stream));
    A.tab = prev; A.tab2 = tab;
    if (grid > 0) if (int rc = n_slots > 0 ? bt_sweep<3>(h, A, grid) : bt_sweep<2>(h, A, grid)) return rc;
    k_boot_finish<<<ugrid, 256, 0, h->stream>>>(K, Rb, rep0, t_scal.as<double>(), t_ctl.as<uint32_t>(), tab, t_theta.as<double>(),
                                               t_acc.as<double>(), h->d_bt_pi, h->d_bt_theta, h->d_bt_counts, h->d_bt_nfrags, h->d_bt_niter,
                                               h->d_bt_conv, h->d_bt_lnl);
    TSEM_HIP(hipGetLastError());
    if (sink) {                                              // the batch's values into the statistics (the good marks: the same scal words)
      if (n_slots > 0) {
        k_boot_fold<<<fgrid, 256, 0, h->stream>>>(n_slots, Rb, rep0, t_scal.as<double>(), t_used.as<int32_t>(), t_gacc.as<double>(),
                                                  h->d_bg_mean, h->d_bg_sd, h->d_bg_vals);
        TSEM_HIP(hipGetLastError());
      }
      k_boot_fold_count<<<1, 64, 0, h->stream>>>(Rb, t_scal.as<double>(), t_used.as<int32_t>());
      TSEM_HIP(hipGetLastError());
    }
  }
  if (sink) {
    if (n_slots > 0) {
      k_boot_fold_end<<<fgrid, 256, 0, h->stream>>>(n_slots, t_used.as<int32_t>(), h->d_bg_mean, h->d_bg_sd);
      TSEM_HIP(hipGetLastError());
    }
    TSEM_HIP(hipMemcpyAsync(&h->bg_used, t_used.p, 4, hipMemcpyDeviceToHost, h->stream));
  }
  TSEM_HIP(hipStreamSynchronize(h->stream));
  h->bt_nrep = n_rep; h->bt_R = R; h->bt_H = H;
  if (sink) { h->bg_nrep = n_rep; h->bg_kept = sink->keep_values ? 1 : 0; h->bg_groups = h->n_groups; h->bg_nnz = n_slots; }
  pt.lap(sink ? "bootstrap_groups" : "bootstrap");
  return TSEM_OK;
}

}  // namespace

extern "C" {

void tsem_boot_free(tsem_ctx* h) { bt_free(h); }

int tsem_bootstrap(tsem_ctx* h, int32_t n_rep, uint64_t seed, const uint8_t* mult, int32_t method, double thresh, double epsilon,
                   int32_t max_iter) {
  return bt_run(h, n_rep, seed, mult, method, thresh, epsilon, max_iter, nullptr);
}

int tsem_bootstrap_groups(tsem_ctx* h, int32_t n_rep, uint64_t seed, const uint8_t* mult, int32_t method, double thresh, double epsilon,
                          int32_t max_iter, int32_t keep_values, int64_t* nnz) {
  if (!h || !nnz) return TSEM_ERR_ARG;
  *nnz = 0;
  const BtSink sink{keep_values ? 1 : 0};
  if (int rc = bt_run(h, n_rep, seed, mult, method, thresh, epsilon, max_iter, &sink)) return rc;
  *nnz = h->bg_nnz;
  return TSEM_OK;
}

int tsem_bootstrap_groups_shape(tsem_ctx* h, int32_t* n_groups, int64_t* nnz, int32_t* n_rep, int32_t* n_used, int32_t* kept) {
  if (!h) return TSEM_ERR_ARG;
  if (h->bg_nrep <= 0) TSEM_FAIL(TSEM_ERR_ARG, "tsem_bootstrap_groups_shape: no result (tsem_bootstrap_groups)");
  if (n_groups) *n_groups = h->bg_groups;
  if (nnz) *nnz = h->bg_nnz;
  if (n_rep) *n_rep = h->bg_nrep;
  if (n_used) *n_used = h->bg_used;
  if (kept) *kept = h->bg_kept;
  return TSEM_OK;
}

int tsem_bootstrap_groups_copy(tsem_ctx* h, int64_t* group_ptr, int32_t* cols, double* mean, double* sd, double* values) {
  if (!h) return TSEM_ERR_ARG;
  if (h->bg_nrep <= 0) TSEM_FAIL(TSEM_ERR_ARG, "tsem_bootstrap_groups_copy: no result (tsem_bootstrap_groups)");
  if (h->bp_version != h->groups_version || !h->d_bp_gptr)
    TSEM_FAIL(TSEM_ERR_ARG, "tsem_bootstrap_groups_copy: the group map was set again since the call (its pattern is gone)");
  if (values && !h->bg_kept) TSEM_FAIL(TSEM_ERR_ARG, "tsem_bootstrap_groups_copy: the call kept no values (keep_values)");
  if (int rc = ensure_device(h)) return rc;
  const size_t S = (size_t)h->bg_nnz;
  if (group_ptr) TSEM_HIP(hipMemcpyAsync(group_ptr, h->d_bp_gptr, 8 * ((size_t)h->bg_groups + 1), hipMemcpyDeviceToHost, h->stream));
  if (S) {
    if (cols) TSEM_HIP(hipMemcpyAsync(cols, h->d_bp_cols, 4 * S, hipMemcpyDeviceToHost, h->stream));
    if (mean) TSEM_HIP(hipMemcpyAsync(mean, h->d_bg_mean, 8 * S, hipMemcpyDeviceToHost, h->stream));
    if (sd) TSEM_HIP(hipMemcpyAsync(sd, h->d_bg_sd, 8 * S, hipMemcpyDeviceToHost, h->stream));
    if (values) TSEM_HIP(hipMemcpyAsync(values, h->d_bg_vals, 8 * S * (size_t)h->bg_nrep, hipMemcpyDeviceToHost, h->stream));
  }
  TSEM_HIP(hipStreamSynchronize(h->stream));
  return TSEM_OK;
}

int tsem_bootstrap_copy(tsem_ctx* h, double* pi, double* theta, double* counts, int64_t* n_frags, int32_t* n_iter, int32_t* converged,
                        double* lnl, int32_t* info2) {
  if (!h) return TSEM_ERR_ARG;
  if (h->bt_nrep <= 0) TSEM_FAIL(TSEM_ERR_ARG, "tsem_bootstrap_copy: no result (tsem_bootstrap)");
  if (int rc = ensure_device(h)) return rc;
  const size_t B = (size_t)h->bt_nrep, BK = B * (size_t)h->K;
  if (pi) TSEM_HIP(hipMemcpyAsync(pi, h->d_bt_pi, 8 * BK, hipMemcpyDeviceToHost, h->stream));
  if (theta) TSEM_HIP(hipMemcpyAsync(theta, h->d_bt_theta, 8 * BK, hipMemcpyDeviceToHost, h->stream));
  if (counts) TSEM_HIP(hipMemcpyAsync(counts, h->d_bt_counts, 8 * BK, hipMemcpyDeviceToHost, h->stream));
  if (n_frags) TSEM_HIP(hipMemcpyAsync(n_frags, h->d_bt_nfrags, 8 * B, hipMemcpyDeviceToHost, h->stream));
  if (n_iter) TSEM_HIP(hipMemcpyAsync(n_iter, h->d_bt_niter, 4 * B, hipMemcpyDeviceToHost, h->stream));
  if (converged) TSEM_HIP(hipMemcpyAsync(converged, h->d_bt_conv, 4 * B, hipMemcpyDeviceToHost, h->stream));
  if (lnl) TSEM_HIP(hipMemcpyAsync(lnl, h->d_bt_lnl, 8 * B, hipMemcpyDeviceToHost, h->stream));
  TSEM_HIP(hipStreamSynchronize(h->stream));
  if (info2) { info2[0] = h->bt_R; info2[1] = h->bt_H; }
  return TSEM_OK;
}

int tsem_bootstrap_mult(tsem_ctx* h, uint64_t seed, int32_t rep, int64_t row_begin, int64_t row_end, uint8_t* out) {
  if (!h) return TSEM_ERR_ARG;
  if (rep < 0 || row_begin < 0 || row_end < row_begin || row_end > h->N || (row_end > row_begin && !out))
    TSEM_FAIL(TSEM_ERR_ARG, "tsem_bootstrap_mult: rep >= 0 and 0 <= row_begin <= row_end <= the handle's rows");
  if (int rc = ensure_device(h)) return rc;
  const int64_t n = row_end - row_begin;
  if (!n) return TSEM_OK;
  DevTmp d;
  TSEM_TMP(d, n);
  k_boot_mult<<<cdiv64(n, 256), 256, 0, h->stream>>>(bt_make_draw(h, seed), rep, row_begin, n, d.as<uint8_t>());
  TSEM_HIP(hipGetLastError());
  TSEM_HIP(hipMemcpyAsync(out, d.p, (size_t)n, hipMemcpyDeviceToHost, h->stream));
  TSEM_HIP(hipStreamSynchronize(h->stream));
  return TSEM_OK;
}

}  // extern "C"
