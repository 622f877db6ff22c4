// libtelescope_em.so, per-cell EM unit: the reference's mixture model (model.py:631-806) fitted once PER GROUP of rows — one fit per
// barcode of a single-cell run — for every group of the map set with tsem_set_groups, in one go.
//
// The fit of cell c is `TelescopeLikelihood(raw[rows_c])` with the score scale of the whole matrix: the cell's own weights, totals,
// prior weights and pisum0, the full K columns.  Thousands of small, independent problems: every cell is fitted by ONE workgroup
// (or one wave) from its first iteration to its last.  No workgroup ever waits for another: no flags, no grid barriers, the only
// loops are over rows, entries, columns and — bounded by max_iter — iterations.
//
// Layout (set-up, once per group map; tsem_cells.hip's cached grouping gives every cell's rows in ascending order):
//   row-ordered view     the entries of the cells' rows in group order: per entry its CELL-LOCAL column number (4 B) and score code
//                        (2 B), per row its class and weight code (4 B);
//   compacted columns    the sorted distinct columns of every cell (cols, col_ptr): only these Kc columns have state; the K - Kc
//                        columns a cell never touches share one closed-form value per parameter (`rest`);
//   column-ordered view  the entries stably radix-sorted by (cell, column): per compacted column the positions of its entries in the
//                        row-ordered view, ascending row order (4 B per entry).
//   scratch              8 B per entry: what the row pass leaves for the column pass.
// Order of sums: a column's sum is taken by ONE lane over the column-ordered view, in ascending row order from 0 — scipy's order
// (model.py:729, `.sum(0)`) — so it depends on the column's entries alone: two runs give the same bits, and two columns of a cell
// with the same rows and scores (twins) get bit-identical pi and theta.  No atomics anywhere.  Block-wide scalars (weights' totals,
// diff, lnl) are reduced in a fixed tree.
//
// Numerators are formed as the reference forms them, both terms (model.py:718-720): (Q Y)(pi theta) + (Q (1 - Y)) pi — so that a NaN
// theta (a cell without ambiguous rows at theta_prior = 0) spreads exactly as it does there.
//
// The SPREAD class (option "cell_em_spread_entries"): a group with more stored entries than the option says — a cell TYPE of a
// single-cell run, 10^5 - 10^7 fragments — is not given to one workgroup.  All spread groups are fitted together by the whole grid,
// one set of short launches per iteration, on the layout above and the global per-column arrays of the global-workspace class (plus
// one per-column array for |pi - previous pi|):
//   row kernel     E-step over chunks of CE_SP_ROWS rows of the row-ordered view (a chunk never straddles two groups; a lane per
//                  row: ce_row_estep, the function k_cell_em calls); leaves every entry's value in the scratch
//   column kernel  M-step over batches of CE_SP_T compacted columns (a batch never straddles two groups)
//   lnl kernel     ce_row_lnl over the same chunks: a partial per chunk; after the last iteration once more, writing z
//   finish kernel  a workgroup per spread group: diff, the stop test, n_iter / converged / the done mark, current -> previous
// Chunks and batches of a group marked done by an EARLIER launch are skipped; nothing is polled, no workgroup waits for another:
// kernel boundaries are the only synchronisation.  The host enqueues CE_SP_LOOK iterations, then reads the done marks back only to
// stop enqueueing (a finished group's launches do nothing): how often it looks changes no result.
// Order of sums of the spread class — a function of the column's entry count n alone, so that twins stay bit-identical and a group's
// result does not depend on what else is in the call:
//   n <= CE_SP_LANE   one lane adds the entries ascending from 0 (scipy's order; ce_col_sum, as in k_cell_em)
//   n <= CE_SP_WAVE   a wave: lane l adds the contiguous ascending piece [l m, (l + 1) m) of m = ceil(n / 64) entries from 0, the 64
//                     partials go through the sg_sum tree
//   beyond            the workgroup: thread t adds the piece [t m, (t + 1) m) of m = ceil(n / CE_SP_T) entries, a wave's partials
//                     through the sg_sum tree, the waves' sums added in wave order
// Block-wide scalars (the weights' totals, diff, lnl) are sums of per-chunk / per-column parts taken in a fixed order that differs
// from k_cell_em's.  A group's BITS therefore depend on its class (spread or not); within a class they depend on the group alone.
// Everything else — a row's weights, E-step and lnl, a column's M-step, the untouched columns, diff — is one device function (ce_*,
// on the scalar forms of tsem_model.h) that both classes call.
#include "tsem_runs.h"

namespace {

// device memory of the set-up per stored entry of the grouped rows: kept — local column 4, code 2, column view 4, scratch 8 (18 B, +
// 4 B per row, + 60 B per compacted column); while it runs — two 8-byte keys and a second 4-byte position on top (38 B)
constexpr int64_t CE_BYTES_KEPT = 18, CE_BYTES_PEAK = 38;
// cell classes: tables of Kc columns x 5 (pi, theta, their previous values, pisum0) in LDS
constexpr int CE_KC_WAVE = 256, CE_ENT_WAVE = 4096;        // a wave per cell: 10 KiB of tables
constexpr int CE_KC_SMALL = 1024;                          // 256 threads, up to 40 KiB
constexpr int CE_KC_LARGE = 3840;                          // 512 threads, up to 150 KiB; beyond: the tables in a global workspace
constexpr int CE_RED = 16;                                 // doubles of LDS in front of the tables (block reductions)
// the spread class (see the top of this file; tests/_group_em_reference.py restates these four)
constexpr int CE_SP_T = 256;                               // threads of every spread kernel = columns per batch
constexpr int CE_SP_ROWS = 1024;                           // rows per chunk
constexpr int CE_SP_LANE = 32;                             // a column of up to this many entries is added by one lane
constexpr int CE_SP_WAVE = 4096;                           // ... of up to this many by a wave; beyond: by the workgroup
constexpr int CE_SP_LOOK = 8;                              // iterations enqueued per look at the done marks

struct CeArgs {
  int32_t K, max_iter, use_lnl;
  double eps, pi_prior, theta_prior;
  const int32_t* cells;            // the cells of this launch (largest first)
  const int64_t* rptr;             // [G + 1] first row of every cell in group order
  const int64_t* eoff;             // [M + 1] first entry of every row of the group order
  const int32_t* rows;             // [M] the CSR row of every row of the group order
  const uint32_t* rinfo;           // [M] row class << 16 | weight code
  const int64_t* indptr;
  const int32_t* lcol;             // [E] cell-local column of every entry (row-ordered view)
  const uint16_t* code;            // [E] its score code
  const double* lut;
  const int64_t* col_ptr;          // [G + 1] first compacted column of every cell
  const uint32_t* cptr;            // [n_cols + 1] first entry of every compacted column in the column-ordered view
  const uint32_t* cpos;            // [E] column-ordered view: positions in the row-ordered view
  double* scratch;                 // [E]
  double* user_z;                  // [nnz] the final z at every entry's own CSR position
  double *pi, *theta, *pi_init, *theta_init, *ws_pi_prev, *ws_theta_prev, *ws_pisum0;   // [n_cols]
  double* rest;                    // [G][4] pi, theta, pi_init, theta_init of the columns a cell never touches
  int32_t *n_iter, *converged;     // [G]
  double* lnl;                     // [G]
};

template <int T>
__device__ __forceinline__ double ce_sum(double v, double* red) {   // the same value in every thread, fixed order
  v = sg_sum<64>(v);
  if (T == 64) return v;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  double t = 0.0;
#pragma unroll
  for (int i = 0; i < T / 64; ++i) t += red[i];
  return t;
}
template <int T>
__device__ __forceinline__ double ce_max(double v, double* red) {
  v = sg_max<64>(v);
  if (T == 64) return v;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  double t = red[0];
#pragma unroll
  for (int i = 1; i < T / 64; ++i) t = fmax(t, red[i]);
  return t;
}

// ---- the steps of a fit, each once: k_cell_em and the spread kernels decide who owns a row or a column, where the group's parameter
// tables are (LDS or its slices of the global arrays: the pointers) and how block-wide scalars are reduced; the arithmetic is here ----
// row i's part of the weights (model.py:690-697); Q (1 - Y) of its entries into the scratch (pisum0, model.py:699)
__device__ __forceinline__ void ce_row_weights(const CeArgs& A, int64_t i, double& tw, double& aw, double& wm) {
  const uint32_t info = A.rinfo[i];
  const int cls = (int)(info >> 16);
  const double w = cls ? A.lut[info & 0xFFFFu] : 0.0, y = cls == 2 ? 1.0 : 0.0;
  tw += w; aw += w * y; wm = fmax(wm, w);
  for (int64_t e = A.eoff[i]; e < A.eoff[i + 1]; ++e) A.scratch[e] = A.lut[A.code[e]] * (1.0 - y);
}
// E-step (model.py:702-722) of row i from the previous parameters: every entry's z w Y into the scratch, for the column pass
__device__ __forceinline__ void ce_row_estep(const CeArgs& A, int64_t i, const double* pp, const double* tp) {
  const uint32_t info = A.rinfo[i];
  const int cls = (int)(info >> 16);
  const double w = cls ? A.lut[info & 0xFFFFu] : 0.0, y = cls == 2 ? 1.0 : 0.0;
  const int64_t a = A.eoff[i], b = A.eoff[i + 1];
  double sum = 0.0;
  for (int64_t e = a; e < b; ++e) { const int lc = A.lcol[e]; const double p = pp[lc]; sum += tm_numer(A.lut[A.code[e]], y, p * tp[lc], p); }
  const double rinv = recip0(sum);
  for (int64_t e = a; e < b; ++e) {
    const int lc = A.lcol[e];
    const double p = pp[lc], n = tm_numer(A.lut[A.code[e]], y, p * tp[lc], p);
    A.scratch[e] = n != 0.0 ? ((n * rinv) * w) * y : 0.0;              // products that are exactly zero leave z's pattern
  }
}
// calculate_lnl(z(previous parameters), current parameters) (model.py:744-760) of row i, added to `part` entry by entry; WRITE: z goes
// to its CSR positions as well
template <bool WRITE>
__device__ __forceinline__ void ce_row_lnl(const CeArgs& A, int64_t i, const double* pi, const double* th, const double* pp,
                                           const double* tp, double& part) {
  const double nan = __longlong_as_double(0x7FF8000000000000ll);
  const uint32_t info = A.rinfo[i];
  const double y = (info >> 16) == 2 ? 1.0 : 0.0;
  const int64_t a = A.eoff[i], b = A.eoff[i + 1];
  double sum = 0.0;
  for (int64_t e = a; e < b; ++e) { const int lc = A.lcol[e]; const double p = pp[lc]; sum += tm_numer(A.lut[A.code[e]], y, p * tp[lc], p); }
  const double rinv = recip0(sum);
  const int64_t zo = WRITE ? A.indptr[A.rows[i]] - a : 0;
  for (int64_t e = a; e < b; ++e) {
    const int lc = A.lcol[e];
    const double q = A.lut[A.code[e]], p = pp[lc], c = pi[lc];
    const double n = tm_numer(q, y, p * tp[lc], p);
    const bool inp = n != 0.0;
    const double z = n * rinv;
    if (WRITE) A.user_z[zo + e] = inp ? z : nan;
    const double m = tm_numer(q, y, c * th[lc], c);
    if (inp && m != 0.0) part += z * log1p(m);
  }
}
// one lane adds the entries [p0, p1) of the column-ordered view over the scratch, ascending from 0 (scipy's order)
__device__ __forceinline__ double ce_col_sum(const CeArgs& A, uint32_t p0, uint32_t p1) {
  double s = 0.0;
  for (uint32_t p = p0; p < p1; ++p) s += A.scratch[A.cpos[p]];
  return s;
}
// M-step closed forms (model.py:724-742) of compacted column `col` from its sum s; the first iteration's values are kept; returns
// |pi - previous pi|
__device__ __forceinline__ double ce_col_mstep(const CeArgs& A, const TmPrior& P, int64_t col, bool first, double s, double ps0,
                                               double pi_prev, double& pi, double& th) {
  const double thn = tm_theta(s, P.tpw, P.den_th);
  const double pin = tm_pi(ps0, s, P.ppw, P.den_pi);
  pi = pin; th = thn;
  if (first) { A.pi_init[col] = pin; A.theta_init[col] = thn; }
  return fabs(pin - pi_prev);
}
// the columns a group never touches: the closed forms of empty sums
__device__ __forceinline__ double ce_rest_pi(const TmPrior& P) { return tm_pi(0.0, 0.0, P.ppw, P.den_pi); }
__device__ __forceinline__ double ce_rest_th(const TmPrior& P) { return tm_theta(0.0, P.tpw, P.den_th); }
// diff over all K columns (model.py:781) from the sum d over the Kc touched ones
__device__ __forceinline__ double ce_diff(double d, int K, int Kc, double rest_pi, double rest_pi_prev) {
  return d + (K > Kc ? (double)(K - Kc) * fabs(rest_pi - rest_pi_prev) : 0.0);
}

__global__ void k_ce_fill_nan(int64_t n, double* __restrict__ z) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) z[i] = __longlong_as_double(0x7FF8000000000000ll);
}

// One cell per workgroup of T threads.  LDS: the five column tables sit in LDS; otherwise in the cell's slices of the global arrays.
template <int T, bool LDS>
__global__ __launch_bounds__(T) void k_cell_em(CeArgs A) {
  extern __shared__ double ce_sm[];
  const int c = A.cells[blockIdx.x];
  const int tid = threadIdx.x;
  const int64_t r0 = A.rptr[c], r1 = A.rptr[c + 1];
  const int64_t c0 = A.col_ptr[c];
  const int Kc = (int)(A.col_ptr[c + 1] - c0);
  const int K = A.K;
  double* red = ce_sm;
  double *pi, *th, *pp, *tp, *ps0;
  if constexpr (LDS) { pi = ce_sm + CE_RED; th = pi + Kc; pp = th + Kc; tp = pp + Kc; ps0 = tp + Kc; }
  else { pi = A.pi + c0; th = A.theta + c0; pp = A.ws_pi_prev + c0; tp = A.ws_theta_prev + c0; ps0 = A.ws_pisum0 + c0; }
  const double nan = __longlong_as_double(0x7FF8000000000000ll);
  if (r1 == r0) {                                           // a cell without rows is not fitted
    if (tid == 0) {
      A.n_iter[c] = 0; A.converged[c] = 0; A.lnl[c] = nan;
      A.rest[4 * (int64_t)c] = 1.0 / K; A.rest[4 * (int64_t)c + 1] = 1.0 / K; A.rest[4 * (int64_t)c + 2] = nan; A.rest[4 * (int64_t)c + 3] = nan;
    }
    return;
  }
  // ---- the cell's weights (model.py:690-697) and pisum0 (model.py:699) ----
  double tw = 0.0, aw = 0.0, wm = 0.0;
  for (int64_t i = r0 + tid; i < r1; i += T) ce_row_weights(A, i, tw, aw, wm);
  tw = ce_sum<T>(tw, red); aw = ce_sum<T>(aw, red); wm = ce_max<T>(wm, red);
  __syncthreads();
  const double inv_k = 1.0 / K;
  for (int lc = tid; lc < Kc; lc += T) { ps0[lc] = ce_col_sum(A, A.cptr[c0 + lc], A.cptr[c0 + lc + 1]); pi[lc] = inv_k; th[lc] = inv_k; }
  const TmPrior P = tm_prior(A.pi_prior, A.theta_prior, K, tw, aw, wm);
  double rest_pi = inv_k, rest_th = inv_k, rest_pi_prev = inv_k, rest_th_prev = inv_k, rest_pi_init = nan, rest_th_init = nan;
  int it = 0;
  bool conv = false;
  double lnl_prev = INFINITY;

  auto lnl_pass = [&](auto write) -> double {
    double part = 0.0;
    for (int64_t i = r0 + tid; i < r1; i += T) ce_row_lnl<decltype(write)::value>(A, i, pi, th, pp, tp, part);
    return ce_sum<T>(part, red);
  };

  do {
    // ---- previous <- current ----
    __syncthreads();
    for (int lc = tid; lc < Kc; lc += T) { pp[lc] = pi[lc]; tp[lc] = th[lc]; }
    rest_pi_prev = rest_pi; rest_th_prev = rest_th;
    __syncthreads();
    // ---- E-step, a lane per row ----
    for (int64_t i = r0 + tid; i < r1; i += T) ce_row_estep(A, i, pp, tp);
    __syncthreads();
    // ---- M-step, a lane per column of the cell, ascending row order ----
    double dpart = 0.0;
    for (int lc = tid; lc < Kc; lc += T)
      dpart += ce_col_mstep(A, P, c0 + lc, it == 0, ce_col_sum(A, A.cptr[c0 + lc], A.cptr[c0 + lc + 1]), ps0[lc], pp[lc], pi[lc], th[lc]);
    rest_th = ce_rest_th(P); rest_pi = ce_rest_pi(P);
    if (it == 0) { rest_pi_init = rest_pi; rest_th_init = rest_th; }
    ++it;
    const double diff = ce_diff(ce_sum<T>(dpart, red), K, Kc, rest_pi, rest_pi_prev);
    __syncthreads();
    if (A.use_lnl) {                                        // model.py:783-789
      const double lnl = lnl_pass(std::false_type());
      conv = fabs(lnl - lnl_prev) < A.eps;
      lnl_prev = lnl;
    } else {
      conv = diff < A.eps;
    }
  } while (!conv && it < A.max_iter);

  // ---- the final z — the last E-step's, from the parameters before the last M-step (model.py:795) — and the lnl (model.py:800-801;
  // under use_likelihood the same sum as the last iteration's) ----
  const double lnl = lnl_pass(std::true_type());
  if constexpr (LDS) {
    for (int lc = tid; lc < Kc; lc += T) { A.pi[c0 + lc] = pi[lc]; A.theta[c0 + lc] = th[lc]; }
  }
  if (tid == 0) {
    A.n_iter[c] = it; A.converged[c] = conv ? 1 : 0; A.lnl[c] = lnl;
    double* r = A.rest + 4 * (int64_t)c;
    r[0] = rest_pi; r[1] = rest_th; r[2] = rest_pi_init; r[3] = rest_th_init;
  }
  (void)rest_th_prev;
}

// ---- the spread class -------------------------------------------------------------------------------------------------------
struct SpRange { int32_t slot, pad; int64_t a, b; };       // rows [a, b) of the group order | compacted columns [a, b) of spread group `slot`
struct SpArgs {
  const int32_t* gid;              // [S] the group of every spread slot
  const SpRange* chunk;            // row chunks, slot by slot
  const SpRange* batch;            // column batches
  const int64_t* cfirst;           // [S + 1] first chunk of every slot
  double* cpart;                   // [3 chunks] per-chunk parts: tw, aw, wm at set-up; lnl afterwards ([3 k])
  double* dabs;                    // [n_cols] |pi - previous pi| of every column
  double* st;                      // [S][8] the prior scale (TmPrior's four numbers, in its order), previous lnl
  int32_t* ctl;                    // [S][2] iterations done, the done mark
};
__device__ __forceinline__ TmPrior sp_prior(const double* st) { return TmPrior{st[0], st[1], st[2], st[3]}; }

// set-up, a lane per row (ce_row_weights): the chunk's parts of the weights, Q (1 - Y) into the scratch
__global__ __launch_bounds__(CE_SP_T) void k_sp_weights(SpArgs S, CeArgs A) {
  __shared__ double red[CE_RED];
  const SpRange ch = S.chunk[blockIdx.x];
  double tw = 0.0, aw = 0.0, wm = 0.0;
  for (int64_t i = ch.a + threadIdx.x; i < ch.b; i += CE_SP_T) ce_row_weights(A, i, tw, aw, wm);
  tw = ce_sum<CE_SP_T>(tw, red); aw = ce_sum<CE_SP_T>(aw, red); wm = ce_max<CE_SP_T>(wm, red);
  if (threadIdx.x == 0) { S.cpart[3 * (int64_t)blockIdx.x] = tw; S.cpart[3 * (int64_t)blockIdx.x + 1] = aw; S.cpart[3 * (int64_t)blockIdx.x + 2] = wm; }
}
// set-up, a workgroup per spread group: its weights from the chunks' parts in chunk order, the prior scale (tm_prior)
__global__ __launch_bounds__(CE_SP_T) void k_sp_begin(SpArgs S, CeArgs A) {
  __shared__ double red[CE_RED];
  const int s = blockIdx.x;
  double tw = 0.0, aw = 0.0, wm = 0.0;
  for (int64_t k = S.cfirst[s] + threadIdx.x; k < S.cfirst[s + 1]; k += CE_SP_T) {
    tw += S.cpart[3 * k]; aw += S.cpart[3 * k + 1]; wm = fmax(wm, S.cpart[3 * k + 2]);
  }
  tw = ce_sum<CE_SP_T>(tw, red); aw = ce_sum<CE_SP_T>(aw, red); wm = ce_max<CE_SP_T>(wm, red);
  if (threadIdx.x == 0) {
    const TmPrior P = tm_prior(A.pi_prior, A.theta_prior, A.K, tw, aw, wm);
    double* st = S.st + 8 * (int64_t)s;
    st[0] = P.tpw; st[1] = P.den_th; st[2] = P.ppw; st[3] = P.den_pi; st[4] = INFINITY;
    S.ctl[2 * s] = 0; S.ctl[2 * s + 1] = 0;
  }
}

// E-step of one chunk of rows, a lane per row (ce_row_estep), from the group's previous parameters
__global__ __launch_bounds__(CE_SP_T) void k_sp_rows(SpArgs S, CeArgs A) {
  const SpRange ch = S.chunk[blockIdx.x];
  if (S.ctl[2 * ch.slot + 1]) return;                       // (marked by an earlier launch)
  const int64_t c0 = A.col_ptr[S.gid[ch.slot]];
  for (int64_t i = ch.a + threadIdx.x; i < ch.b; i += CE_SP_T) ce_row_estep(A, i, A.ws_pi_prev + c0, A.ws_theta_prev + c0);
}

// the lnl pass of one chunk of rows, a lane per row (ce_row_lnl): a partial per chunk; WRITE: the final pass — every group, z to its
// CSR positions
template <bool WRITE>
__global__ __launch_bounds__(CE_SP_T) void k_sp_lnl(SpArgs S, CeArgs A) {
  __shared__ double red[CE_RED];
  const SpRange ch = S.chunk[blockIdx.x];
  if (!WRITE && S.ctl[2 * ch.slot + 1]) return;
  const int64_t c0 = A.col_ptr[S.gid[ch.slot]];
  double part = 0.0;
  for (int64_t i = ch.a + threadIdx.x; i < ch.b; i += CE_SP_T)
    ce_row_lnl<WRITE>(A, i, A.pi + c0, A.theta + c0, A.ws_pi_prev + c0, A.ws_theta_prev + c0, part);
  part = ce_sum<CE_SP_T>(part, red);
  if (threadIdx.x == 0) S.cpart[3 * (int64_t)blockIdx.x] = part;
}

// The sums of one batch of compacted columns over the scratch, in the order the top of this file states (by the column's entry
// count alone).  MSTEP: the closed forms (ce_col_mstep) and |pi - previous pi|; otherwise pisum0 and the start values 1 / K.
template <bool MSTEP>
__global__ __launch_bounds__(CE_SP_T) void k_sp_cols(SpArgs S, CeArgs A) {
  __shared__ double red[CE_RED];
  __shared__ uint32_t big_p[CE_SP_T], big_n[CE_SP_T];
  const SpRange bt = S.batch[blockIdx.x];
  if (MSTEP && S.ctl[2 * bt.slot + 1]) return;
  const int tid = threadIdx.x, lane = tid & 63;
  const int64_t col = bt.a + tid;
  const bool live = col < bt.b;
  const uint32_t p0 = live ? A.cptr[col] : 0u, n = live ? A.cptr[col + 1] - p0 : 0u;
  double s = 0.0;
  if (n <= (uint32_t)CE_SP_LANE) s = ce_col_sum(A, p0, p0 + n);
  for (unsigned long long m = __ballot(n > (uint32_t)CE_SP_LANE && n <= (uint32_t)CE_SP_WAVE); m; m &= m - 1) {
    const int src = __ffsll((long long)m) - 1;
    const uint32_t q0 = (uint32_t)__shfl((int)p0, src, 64), qn = (uint32_t)__shfl((int)n, src, 64);
    const uint32_t piece = (qn + 63u) / 64u, lo = min(qn, (uint32_t)lane * piece), hi = min(qn, lo + piece);
    double t = 0.0;
    for (uint32_t j = lo; j < hi; ++j) t += A.scratch[A.cpos[q0 + j]];
    t = sg_sum<64>(t);
    if (lane == src) s = t;
  }
  const bool big = n > (uint32_t)CE_SP_WAVE;
  big_p[tid] = p0; big_n[tid] = big ? n : 0u;
  if (__syncthreads_or(big)) {
    for (int c = 0; c < CE_SP_T; ++c) {
      const uint32_t qn = big_n[c];
      if (!qn) continue;                                     // (the same in every thread)
      const uint32_t q0 = big_p[c], piece = (qn + CE_SP_T - 1u) / CE_SP_T, lo = min(qn, (uint32_t)tid * piece), hi = min(qn, lo + piece);
      double t = 0.0;
      for (uint32_t j = lo; j < hi; ++j) t += A.scratch[A.cpos[q0 + j]];
      t = ce_sum<CE_SP_T>(t, red);
      if (tid == c) s = t;
    }
  }
  if (!live) return;
  if (!MSTEP) {
    const double inv_k = 1.0 / A.K;
    A.ws_pisum0[col] = s; A.ws_pi_prev[col] = inv_k; A.ws_theta_prev[col] = inv_k; A.pi[col] = inv_k; A.theta[col] = inv_k;
  } else {
    S.dabs[col] = ce_col_mstep(A, sp_prior(S.st + 8 * (int64_t)bt.slot), col, S.ctl[2 * bt.slot] == 0, s, A.ws_pisum0[col], A.ws_pi_prev[col],
                               A.pi[col], A.theta[col]);
  }
}

// End of an iteration, a workgroup per spread group still running: diff over all K columns (model.py:781) from the columns' parts,
// the stop test (model.py:783-789), n_iter / converged, the done mark; current -> previous only if the group goes on — a group
// that stops keeps the parameter pair of its last iteration for the final pass.
__global__ __launch_bounds__(CE_SP_T) void k_sp_finish(SpArgs S, CeArgs A) {
  __shared__ double red[CE_RED];
  const int s = blockIdx.x, tid = threadIdx.x;
  if (S.ctl[2 * s + 1]) return;
  const int c = S.gid[s];
  const int64_t c0 = A.col_ptr[c];
  const int Kc = (int)(A.col_ptr[c + 1] - c0), K = A.K;
  double* st = S.st + 8 * (int64_t)s;
  const int it = S.ctl[2 * s];
  bool conv;
  if (A.use_lnl) {
    double l = 0.0;
    for (int64_t k = S.cfirst[s] + tid; k < S.cfirst[s + 1]; k += CE_SP_T) l += S.cpart[3 * k];
    l = ce_sum<CE_SP_T>(l, red);
    conv = fabs(l - st[4]) < A.eps;
    __syncthreads();
    if (tid == 0) st[4] = l;
  } else {
    double d = 0.0;
    for (int lc = tid; lc < Kc; lc += CE_SP_T) d += S.dabs[c0 + lc];
    d = ce_sum<CE_SP_T>(d, red);
    const double rest_pi = ce_rest_pi(sp_prior(st));
    conv = ce_diff(d, K, Kc, rest_pi, it == 0 ? 1.0 / K : rest_pi) < A.eps;
  }
  const bool stop = conv || it + 1 >= A.max_iter;
  if (!stop)
    for (int lc = tid; lc < Kc; lc += CE_SP_T) { A.ws_pi_prev[c0 + lc] = A.pi[c0 + lc]; A.ws_theta_prev[c0 + lc] = A.theta[c0 + lc]; }
  if (tid == 0) {
    S.ctl[2 * s] = it + 1; S.ctl[2 * s + 1] = stop ? 1 : 0;
    A.n_iter[c] = it + 1; A.converged[c] = conv ? 1 : 0;
  }
}
// after the final pass: the group's lnl from the chunks' parts in chunk order, and the columns it never touches
__global__ __launch_bounds__(CE_SP_T) void k_sp_end(SpArgs S, CeArgs A) {
  __shared__ double red[CE_RED];
  const int s = blockIdx.x, tid = threadIdx.x;
  double l = 0.0;
  for (int64_t k = S.cfirst[s] + tid; k < S.cfirst[s + 1]; k += CE_SP_T) l += S.cpart[3 * k];
  l = ce_sum<CE_SP_T>(l, red);
  if (tid == 0) {
    const int c = S.gid[s];
    const TmPrior P = sp_prior(S.st + 8 * (int64_t)s);
    const double rest_pi = ce_rest_pi(P), rest_th = ce_rest_th(P);
    A.lnl[c] = l;
    double* r = A.rest + 4 * (int64_t)c;
    r[0] = rest_pi; r[1] = rest_th; r[2] = rest_pi; r[3] = rest_th;
  }
}

// ---- set-up kernels -----------------------------------------------------------------------------------------------------------
// per row of the group order: class and weight code; per entry: key (cell << cbits | column) and score code (a lane per row)
__global__ void k_ce_rows(int64_t M, const int32_t* __restrict__ rows, const uint32_t* __restrict__ gkey, const int64_t* __restrict__ eoff,
                          const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices, const uint16_t* __restrict__ raw,
                          const uint8_t* __restrict__ cls, const uint16_t* __restrict__ wcode, int cbits, uint32_t* __restrict__ rinfo,
                          uint64_t* __restrict__ key, uint16_t* __restrict__ code) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= M) return;
  const int32_t row = rows[i];
  rinfo[i] = (uint32_t)cls[row] << 16 | wcode[row];
  const uint64_t hi = (uint64_t)gkey[i] << cbits;
  const int64_t s = indptr[row], len = indptr[row + 1] - s, o = eoff[i];
  for (int64_t k = 0; k < len; ++k) { key[o + k] = hi | (uint32_t)indices[s + k]; code[o + k] = raw[s + k]; }
}
// first compacted column of every cell: the runs before the cell's first entry (the entries are sorted by cell first)
__global__ void k_ce_colptr(int64_t G1, int64_t E, int64_t n_runs, const int64_t* __restrict__ gent, const uint32_t* __restrict__ hscan,
                            int64_t* __restrict__ col_ptr) {
  const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= G1) return;
  const int64_t e = gent[g];
  col_ptr[g] = e < E ? (int64_t)hscan[e] - 1 : n_runs;
}
// per entry of the column-ordered view: its run = compacted column; heads write the column's start and id; every entry's local column
__global__ void k_ce_columns(int64_t E, int64_t n_runs, const uint64_t* __restrict__ key, const uint32_t* __restrict__ hscan,
                             const uint32_t* __restrict__ cpos, const int64_t* __restrict__ col_ptr, int cbits, uint32_t* __restrict__ cptr,
                             int32_t* __restrict__ cols, int32_t* __restrict__ lcol) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p == 0) cptr[n_runs] = (uint32_t)E;
  if (p >= E) return;
  const uint64_t k = key[p];
  const int64_t r = (int64_t)hscan[p] - 1;
  if (p == 0 || k != key[p - 1]) { cptr[r] = (uint32_t)p; cols[r] = (int32_t)(k & ((1ull << cbits) - 1ull)); }
  lcol[cpos[p]] = (int32_t)(r - col_ptr[k >> cbits]);
}

void ce_free_layout(tsem_ctx* h) {
  dfree(h->d_ce_rptr); dfree(h->d_ce_rinfo); dfree(h->d_ce_lcol); dfree(h->d_ce_code); dfree(h->d_ce_cpos); dfree(h->d_ce_cptr);
  dfree(h->d_ce_colptr); dfree(h->d_ce_cols); dfree(h->d_ce_scratch);
  h->ce_colptr.clear(); h->ce_version = ~0ull; h->ce_ncols = 0; h->ce_cells = 0;
}
void ce_free_result(tsem_ctx* h) {
  dfree(h->d_ce_pi); dfree(h->d_ce_theta); dfree(h->d_ce_pi_init); dfree(h->d_ce_theta_init); dfree(h->d_ce_ws0); dfree(h->d_ce_ws1);
  dfree(h->d_ce_ws2); dfree(h->d_ce_ws3); dfree(h->d_ce_rest); dfree(h->d_ce_niter); dfree(h->d_ce_conv); dfree(h->d_ce_lnl); dfree(h->d_ce_list);
  h->ce_fitted = false;
  for (int k = 0; k < 4; ++k) h->ce_class_n[k] = 0;
  h->ce_spread_n = 0;
}

// the compacted, column-ordered copy of the grouped rows (see the top of this file), cached per group map
int ce_build_layout(tsem_ctx* h) {
  if (int rc = tsem_build_grouping(h)) return rc;
  if (h->ce_version == h->groups_version && h->d_ce_colptr) return TSEM_OK;
  ce_free_layout(h);
  ce_free_result(h);
  const int32_t G = h->n_groups;
  const int64_t M = G ? h->gc_rptr[G] : 0, E = G ? h->gc_gent[G] : 0;
  if (E >= ((int64_t)1 << 31))
    TSEM_FAIL(TSEM_ERR_NOMEM, "tsem_cell_em: " + std::to_string(E) + " stored entries in cells: the per-cell layout holds fewer than 2^31 (tiling it is not supported)");
  size_t free_b = 0, total_b = 0;
  TSEM_HIP(hipMemGetInfo(&free_b, &total_b));
  const int64_t need = CE_BYTES_PEAK * E + 4 * M + (64ll << 20);
  if ((int64_t)free_b < need)
    TSEM_FAIL(TSEM_ERR_NOMEM, "tsem_cell_em: the per-cell layout needs " + std::to_string(need) + " B of device memory (" +
              std::to_string(CE_BYTES_KEPT) + " B per stored entry kept, " + std::to_string(CE_BYTES_PEAK) + " while it is built); " +
              std::to_string(free_b) + " B are free (tiling it is not supported)");
  CsrIds ids(h);
  if (int rc = ids.acquire()) return rc;
  PhaseTimer pt(h->stream);
  const int cbits = bits_for((uint64_t)std::max(0, h->K - 1)), gbits = bits_for((uint64_t)G);
  TSEM_ALLOC(h->d_ce_rptr, 2 * ((int64_t)G + 1));           // row pointer | entry pointer of every cell
  TSEM_ALLOC(h->d_ce_rinfo, M);
  TSEM_ALLOC(h->d_ce_lcol, E);
  TSEM_ALLOC(h->d_ce_code, E);
  TSEM_ALLOC(h->d_ce_cpos, E);
  TSEM_ALLOC(h->d_ce_colptr, (int64_t)G + 1);
  TSEM_ALLOC(h->d_ce_scratch, E);
  int64_t* d_gent = h->d_ce_rptr + G + 1;
  TSEM_HIP(hipMemcpyAsync(h->d_ce_rptr, h->gc_rptr.data(), 8 * ((size_t)G + 1), hipMemcpyHostToDevice, h->stream));
  TSEM_HIP(hipMemcpyAsync(d_gent, h->gc_gent.data(), 8 * ((size_t)G + 1), hipMemcpyHostToDevice, h->stream));
  int64_t n_runs = 0;
  DevTmp key, key2, hscan, tmp;
  TSEM_TMP(key, 8 * E); TSEM_TMP(key2, 8 * E); TSEM_TMP(hscan, 4 * E);
  if (M > 0) {                                              // (rows without entries too: their class is what the fit reads)
    k_ce_rows<<<cdiv64(M, 256), 256, 0, h->stream>>>(M, h->d_gc_rows, h->d_gc_key, h->d_gc_eoff, h->d_indptr, h->d_indices, h->d_raw,
                                                    h->d_row_cls, h->d_row_code, cbits, h->d_ce_rinfo, key.as<uint64_t>(), h->d_ce_code);
    TSEM_HIP(hipGetLastError());
  }
  if (E > 0) {
    rocprim::counting_iterator<uint32_t> iota(0);
    const int kbits = std::min(64, cbits + gbits);
    size_t tb = 0;
    if (int rc = sorted_runs_tmp_bytes(h, iota, h->d_ce_cpos, E, kbits, &tb)) return rc;
    TSEM_TMP(tmp, tb);
    // stable: equal (cell, column) keys keep the row-ordered view's order — ascending rows; the heads reuse the unsorted keys' buffer
    uint32_t nr = 0;
    if (int rc = sorted_runs(h, tmp.p, tb, key.as<uint64_t>(), key2.as<uint64_t>(), iota, h->d_ce_cpos, E, kbits, key.as<uint32_t>(),
                             hscan.as<uint32_t>(), &nr)) return rc;
    TSEM_HIP(hipStreamSynchronize(h->stream));
    n_runs = nr;
    TSEM_ALLOC(h->d_ce_cptr, n_runs + 1);
    TSEM_ALLOC(h->d_ce_cols, n_runs);
    k_ce_colptr<<<cdiv64((int64_t)G + 1, 256), 256, 0, h->stream>>>((int64_t)G + 1, E, n_runs, d_gent, hscan.as<uint32_t>(), h->d_ce_colptr);
    TSEM_HIP(hipGetLastError());
    k_ce_columns<<<cdiv64(E, 256), 256, 0, h->stream>>>(E, n_runs, key2.as<uint64_t>(), hscan.as<uint32_t>(), h->d_ce_cpos, h->d_ce_colptr,
                                                       cbits, h->d_ce_cptr, h->d_ce_cols, h->d_ce_lcol);
    TSEM_HIP(hipGetLastError());
    h->ce_colptr.assign((size_t)G + 1, 0);
    TSEM_HIP(hipMemcpyAsync(h->ce_colptr.data(), h->d_ce_colptr, 8 * ((size_t)G + 1), hipMemcpyDeviceToHost, h->stream));
    TSEM_HIP(hipStreamSynchronize(h->stream));
  } else {
    TSEM_ALLOC(h->d_ce_cptr, 1);
    TSEM_ALLOC(h->d_ce_cols, 1);
    TSEM_HIP(hipMemsetAsync(h->d_ce_cptr, 0, 4, h->stream));
    TSEM_HIP(hipMemsetAsync(h->d_ce_colptr, 0, 8 * ((size_t)G + 1), h->stream));
    h->ce_colptr.assign((size_t)G + 1, 0);
    TSEM_HIP(hipStreamSynchronize(h->stream));
  }
  h->ce_ncols = n_runs;
  h->ce_cells = G;
  h->ce_version = h->groups_version;
  pt.lap("cell_em: layout");
  return TSEM_OK;
}

template <int T, bool LDS>
int ce_launch(tsem_ctx* h, CeArgs A, const int32_t* d_list, int n, int kc_max) {
  if (n <= 0) return TSEM_OK;
  const size_t lds = 8 * ((size_t)CE_RED + (LDS ? 5 * (size_t)kc_max : 0));
  if (lds > 48 * 1024)
    TSEM_HIP(hipFuncSetAttribute((const void*)k_cell_em<T, LDS>, hipFuncAttributeMaxDynamicSharedMemorySize, TS_LDS_DYN_MAX));
  A.cells = d_list;
  k_cell_em<T, LDS><<<n, T, lds, h->stream>>>(A);
  TSEM_HIP(hipGetLastError());
  return TSEM_OK;
}

// The spread groups of a fit (see the top of this file): set-up, then CE_SP_LOOK iterations enqueued per look at the done marks,
// bounded by max_iter; the final pass writes z and the lnl.
int ce_fit_spread(tsem_ctx* h, const CeArgs& A, const std::vector<int32_t>& groups) {
  const int S = (int)groups.size();
  if (S == 0) return TSEM_OK;
  std::vector<SpRange> chunk, batch;
  std::vector<int64_t> cfirst((size_t)S + 1, 0);
  for (int s = 0; s < S; ++s) {
    const int32_t c = groups[(size_t)s];
    cfirst[(size_t)s] = (int64_t)chunk.size();
    for (int64_t r = h->gc_rptr[c]; r < h->gc_rptr[c + 1]; r += CE_SP_ROWS)
      chunk.push_back(SpRange{s, 0, r, std::min<int64_t>(r + CE_SP_ROWS, h->gc_rptr[c + 1])});
    for (int64_t k = h->ce_colptr[c]; k < h->ce_colptr[c + 1]; k += CE_SP_T)
      batch.push_back(SpRange{s, 0, k, std::min<int64_t>(k + CE_SP_T, h->ce_colptr[c + 1])});
  }
  cfirst[(size_t)S] = (int64_t)chunk.size();
  const int n_chunk = (int)chunk.size(), n_batch = (int)batch.size();   // (a spread group has entries: rows and columns)
  DevTmp t_gid, t_chunk, t_batch, t_cfirst, t_cpart, t_st, t_ctl;
  TSEM_TMP(t_gid, 4 * (size_t)S); TSEM_TMP(t_chunk, sizeof(SpRange) * chunk.size()); TSEM_TMP(t_batch, sizeof(SpRange) * batch.size());
  TSEM_TMP(t_cfirst, 8 * ((size_t)S + 1)); TSEM_TMP(t_cpart, 24 * chunk.size()); TSEM_TMP(t_st, 64 * (size_t)S); TSEM_TMP(t_ctl, 8 * (size_t)S);
  TSEM_HIP(hipMemcpyAsync(t_gid.p, groups.data(), 4 * (size_t)S, hipMemcpyHostToDevice, h->stream));
  TSEM_HIP(hipMemcpyAsync(t_chunk.p, chunk.data(), sizeof(SpRange) * chunk.size(), hipMemcpyHostToDevice, h->stream));
  TSEM_HIP(hipMemcpyAsync(t_batch.p, batch.data(), sizeof(SpRange) * batch.size(), hipMemcpyHostToDevice, h->stream));
  TSEM_HIP(hipMemcpyAsync(t_cfirst.p, cfirst.data(), 8 * ((size_t)S + 1), hipMemcpyHostToDevice, h->stream));
  SpArgs P{};
  P.gid = t_gid.as<int32_t>(); P.chunk = t_chunk.as<SpRange>(); P.batch = t_batch.as<SpRange>(); P.cfirst = t_cfirst.as<int64_t>();
  P.cpart = t_cpart.as<double>(); P.dabs = h->d_ce_ws3; P.st = t_st.as<double>(); P.ctl = t_ctl.as<int32_t>();
  k_sp_weights<<<n_chunk, CE_SP_T, 0, h->stream>>>(P, A);
  TSEM_HIP(hipGetLastError());
  k_sp_begin<<<S, CE_SP_T, 0, h->stream>>>(P, A);
  TSEM_HIP(hipGetLastError());
  k_sp_cols<false><<<n_batch, CE_SP_T, 0, h->stream>>>(P, A);
  TSEM_HIP(hipGetLastError());
  std::vector<int32_t> ctl(2 * (size_t)S);
  const int iters = std::max(1, A.max_iter);                // (k_cell_em's do-while: one iteration at least)
  for (int it = 0; it < iters;) {
    const int n = std::min(CE_SP_LOOK, iters - it);
    for (int k = 0; k < n; ++k) {
      k_sp_rows<<<n_chunk, CE_SP_T, 0, h->stream>>>(P, A);
      TSEM_HIP(hipGetLastError());
      k_sp_cols<true><<<n_batch, CE_SP_T, 0, h->stream>>>(P, A);
      TSEM_HIP(hipGetLastError());
      if (A.use_lnl) {
        k_sp_lnl<false><<<n_chunk, CE_SP_T, 0, h->stream>>>(P, A);
        TSEM_HIP(hipGetLastError());
      }
      k_sp_finish<<<S, CE_SP_T, 0, h->stream>>>(P, A);
      TSEM_HIP(hipGetLastError());
    }
    it += n;
    if (it >= iters) break;
    TSEM_HIP(hipMemcpyAsync(ctl.data(), t_ctl.p, 8 * (size_t)S, hipMemcpyDeviceToHost, h->stream));
    TSEM_HIP(hipStreamSynchronize(h->stream));
    int running = 0;
    for (int s = 0; s < S; ++s) running += ctl[2 * (size_t)s + 1] ? 0 : 1;
    if (!running) break;
  }
  k_sp_lnl<true><<<n_chunk, CE_SP_T, 0, h->stream>>>(P, A);
  TSEM_HIP(hipGetLastError());
  k_sp_end<<<S, CE_SP_T, 0, h->stream>>>(P, A);
  TSEM_HIP(hipGetLastError());
  TSEM_HIP(hipStreamSynchronize(h->stream));                // (the tables above go out of scope)
  return TSEM_OK;
}

}  // namespace

extern "C" {

void tsem_cellem_free(tsem_ctx* h) { ce_free_layout(h); ce_free_result(h); }

// One EM fit per group of rows (model.py:762-806 on raw[rows of the group], max_score of the whole matrix): see the top of this file.
int tsem_cell_em(tsem_ctx* h, double epsilon, int32_t max_iter, int32_t use_likelihood) {
  if (!h || !h->d_indptr) return TSEM_ERR_ARG;
  if (int rc = ensure_device(h)) return rc;
  if (tsem_comm_on(h)) TSEM_FAIL(TSEM_ERR_ARG, "tsem_cell_em: row-sharded per-cell fits are not supported (one GPU per run)");
  if (!h->have_rowstats || !h->d_row_cls || !h->d_row_code) TSEM_FAIL(TSEM_ERR_ARG, "tsem_cell_em: no row statistics (tsem_rowstats)");
  if (!h->d_lut || h->lut_len <= 0) TSEM_FAIL(TSEM_ERR_ARG, "tsem_cell_em: no score table (tsem_set_lut)");
  if (!h->have_model) TSEM_FAIL(TSEM_ERR_ARG, "tsem_cell_em: no model (tsem_set_model gives the priors)");
  if (!h->d_group && h->N) TSEM_FAIL(TSEM_ERR_ARG, "tsem_cell_em: no group map (tsem_set_groups)");
  if (h->K <= 0) TSEM_FAIL(TSEM_ERR_ARG, "tsem_cell_em: the matrix has no columns");
  h->ce_fitted = false;
  if (int rc = ce_build_layout(h)) return rc;
  PhaseTimer pt(h->stream);
  const int32_t G = h->n_groups;
  const int64_t nc = h->ce_ncols;
  if (!h->d_ce_pi) {
    TSEM_ALLOC(h->d_ce_pi, nc); TSEM_ALLOC(h->d_ce_theta, nc); TSEM_ALLOC(h->d_ce_pi_init, nc); TSEM_ALLOC(h->d_ce_theta_init, nc);
    TSEM_ALLOC(h->d_ce_ws0, nc); TSEM_ALLOC(h->d_ce_ws1, nc); TSEM_ALLOC(h->d_ce_ws2, nc); TSEM_ALLOC(h->d_ce_ws3, nc);
    TSEM_ALLOC(h->d_ce_rest, 4 * (int64_t)G); TSEM_ALLOC(h->d_ce_niter, G); TSEM_ALLOC(h->d_ce_conv, G); TSEM_ALLOC(h->d_ce_lnl, G);
    TSEM_ALLOC(h->d_ce_list, G);
  }
  TSEM_ALLOC(h->d_user_z, h->nnz);
  if (h->nnz) {
    k_ce_fill_nan<<<cdiv64(h->nnz, 256), 256, 0, h->stream>>>(h->nnz, h->d_user_z);   // rows in no cell have no entries
    TSEM_HIP(hipGetLastError());
  }
  // the cells by class, each class largest first (by entries; ties in cell order); the spread groups in group order
  std::vector<int32_t> cls[4], spread;
  int kc_max[4] = {0, 0, 0, 0};
  for (int32_t c = 0; c < G; ++c) {
    const int64_t kc = h->ce_colptr[c + 1] - h->ce_colptr[c], ne = h->gc_gent[c + 1] - h->gc_gent[c];
    if (h->opt_ce_spread > 0 && ne > h->opt_ce_spread) { spread.push_back(c); continue; }
    const int k = (kc <= CE_KC_WAVE && ne <= CE_ENT_WAVE) ? 0 : kc <= CE_KC_SMALL ? 1 : kc <= CE_KC_LARGE ? 2 : 3;
    cls[k].push_back(c);
    kc_max[k] = std::max<int>(kc_max[k], (int)kc);
  }
  std::vector<int32_t> list;
  list.reserve((size_t)G);
  int first[5] = {0, 0, 0, 0, 0};
  for (int k = 0; k < 4; ++k) {
    std::stable_sort(cls[k].begin(), cls[k].end(), [&](int32_t a, int32_t b) {
      return h->gc_gent[a + 1] - h->gc_gent[a] > h->gc_gent[b + 1] - h->gc_gent[b];
    });
    list.insert(list.end(), cls[k].begin(), cls[k].end());
    first[k + 1] = (int)list.size();
  }
  if (!list.empty()) TSEM_HIP(hipMemcpyAsync(h->d_ce_list, list.data(), 4 * list.size(), hipMemcpyHostToDevice, h->stream));
  CeArgs A{};
  A.K = h->K; A.max_iter = max_iter; A.use_lnl = use_likelihood ? 1 : 0;
  A.eps = epsilon; A.pi_prior = h->pi_prior; A.theta_prior = h->theta_prior;
  A.rptr = h->d_ce_rptr; A.eoff = h->d_gc_eoff; A.rows = h->d_gc_rows; A.rinfo = h->d_ce_rinfo; A.indptr = h->d_indptr;
  A.lcol = h->d_ce_lcol; A.code = h->d_ce_code; A.lut = h->d_lut; A.col_ptr = h->d_ce_colptr; A.cptr = h->d_ce_cptr; A.cpos = h->d_ce_cpos;
  A.scratch = h->d_ce_scratch; A.user_z = h->d_user_z;
  A.pi = h->d_ce_pi; A.theta = h->d_ce_theta; A.pi_init = h->d_ce_pi_init; A.theta_init = h->d_ce_theta_init;
  A.ws_pi_prev = h->d_ce_ws0; A.ws_theta_prev = h->d_ce_ws1; A.ws_pisum0 = h->d_ce_ws2;
  A.rest = h->d_ce_rest; A.n_iter = h->d_ce_niter; A.converged = h->d_ce_conv; A.lnl = h->d_ce_lnl;
  if (int rc = ce_launch<64, true>(h, A, h->d_ce_list + first[0], first[1] - first[0], kc_max[0])) return rc;
  if (int rc = ce_launch<256, true>(h, A, h->d_ce_list + first[1], first[2] - first[1], kc_max[1])) return rc;
  if (int rc = ce_launch<512, true>(h, A, h->d_ce_list + first[2], first[3] - first[2], kc_max[2])) return rc;
  if (int rc = ce_launch<512, false>(h, A, h->d_ce_list + first[3], first[4] - first[3], kc_max[3])) return rc;
  if (int rc = ce_fit_spread(h, A, spread)) return rc;
  TSEM_HIP(hipStreamSynchronize(h->stream));
  for (int k = 0; k < 4; ++k) h->ce_class_n[k] = first[k + 1] - first[k];
  h->ce_spread_n = (int32_t)spread.size();
  h->ce_fitted = true;
  pt.lap("cell_em: fit");
  return TSEM_OK;
}

int tsem_cell_em_shape(tsem_ctx* h, int32_t* n_cells, int64_t* n_cols) {
  if (!h || !n_cells || !n_cols) return TSEM_ERR_ARG;
  if (!h->ce_fitted) TSEM_FAIL(TSEM_ERR_ARG, "tsem_cell_em_shape: no result (tsem_cell_em)");
  *n_cells = h->ce_cells;
  *n_cols = h->ce_ncols;
  return TSEM_OK;
}

int tsem_cell_em_copy(tsem_ctx* h, int64_t* col_ptr, int32_t* cols, double* pi, double* theta, double* pi_init, double* theta_init,
                      double* rest, int32_t* n_iter, int32_t* converged, double* lnl) {
  if (!h || !col_ptr) return TSEM_ERR_ARG;
  if (!h->ce_fitted) TSEM_FAIL(TSEM_ERR_ARG, "tsem_cell_em_copy: no result (tsem_cell_em)");
  const size_t nc = (size_t)h->ce_ncols, G = (size_t)h->ce_cells;
  if ((nc && (!cols || !pi || !theta || !pi_init || !theta_init)) || (G && (!rest || !n_iter || !converged || !lnl))) return TSEM_ERR_ARG;
  if (int rc = ensure_device(h)) return rc;
  std::copy(h->ce_colptr.begin(), h->ce_colptr.end(), col_ptr);
  if (nc) {
    TSEM_HIP(hipMemcpyAsync(cols, h->d_ce_cols, 4 * nc, hipMemcpyDeviceToHost, h->stream));
    TSEM_HIP(hipMemcpyAsync(pi, h->d_ce_pi, 8 * nc, hipMemcpyDeviceToHost, h->stream));
    TSEM_HIP(hipMemcpyAsync(theta, h->d_ce_theta, 8 * nc, hipMemcpyDeviceToHost, h->stream));
    TSEM_HIP(hipMemcpyAsync(pi_init, h->d_ce_pi_init, 8 * nc, hipMemcpyDeviceToHost, h->stream));
    TSEM_HIP(hipMemcpyAsync(theta_init, h->d_ce_theta_init, 8 * nc, hipMemcpyDeviceToHost, h->stream));
  }
  if (G) {
    TSEM_HIP(hipMemcpyAsync(rest, h->d_ce_rest, 32 * G, hipMemcpyDeviceToHost, h->stream));
    TSEM_HIP(hipMemcpyAsync(n_iter, h->d_ce_niter, 4 * G, hipMemcpyDeviceToHost, h->stream));
    TSEM_HIP(hipMemcpyAsync(converged, h->d_ce_conv, 4 * G, hipMemcpyDeviceToHost, h->stream));
    TSEM_HIP(hipMemcpyAsync(lnl, h->d_ce_lnl, 8 * G, hipMemcpyDeviceToHost, h->stream));
  }
  TSEM_HIP(hipStreamSynchronize(h->stream));
  return TSEM_OK;
}

}  // extern "C"
