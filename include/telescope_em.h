/*
 * telescope_em.h — C ABI of libtelescope_em.so, the MI355X (gfx950) engine for
 * Telescope's EM reassignment path.
 *
 * The reference has no FFI layer: its boundary is the Python class
 * `TelescopeLikelihood` (telescope/utils/model.py:631-865) on top of
 * `csr_matrix_plus` (telescope/utils/sparse_plus.py:24-174) and scipy.sparse.
 * Each entry point below names the reference code it replaces.  The Python
 * host mirror (telescope_amd/likelihood.py) binds these with ctypes; the
 * binding a reference maintainer would add is shown in INTEGRATION.md.
 *
 * Conventions
 *   - plain C, opaque handle, `int` status (0 = TSEM_OK, <0 = error; text via
 *     tsem_last_error).  No exceptions or abort() cross the boundary.
 *   - one handle == one GPU == one host thread (not thread-safe).  Multi-GPU is
 *     one process per GPU; the only per-iteration exchange is a sum all-reduce
 *     of the reduce buffer (K+2 doubles: the per-locus column sums and an error
 *     flag).  With a communicator attached (tsem_comm_*) the library issues it
 *     itself — ncclAllReduce (RCCL over xGMI) on the engine's stream between the
 *     EM pass and the parameter update, no host round trip (tsem_em_chunk).  A
 *     host may instead do it between tsem_em_pass() and tsem_em_update().
 *   - host pointers are borrowed for the duration of the call; the library owns
 *     all device memory except a reduce buffer bound with
 *     tsem_bind_reduce_buffer().
 *   - there is no CPU fallback: tsem_create fails if no HIP device is usable.
 */
#ifndef TELESCOPE_EM_H
#define TELESCOPE_EM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TSEM_OK            0
#define TSEM_ERR_ARG      -1   /* bad argument / wrong state              */
#define TSEM_ERR_HIP      -2   /* HIP runtime error (text in last_error)  */
#define TSEM_ERR_NOMEM    -3
#define TSEM_ERR_TIMEOUT  -4   /* in-kernel hand-off watchdog fired       */

/* reassign methods, model.py:808-865 */
#define TSEM_RA_EXCLUDE 0
#define TSEM_RA_CHOOSE  1
#define TSEM_RA_AVERAGE 2
#define TSEM_RA_CONF    3
#define TSEM_RA_UNIQUE  4
#define TSEM_RA_ALL     5

/* which parameters define z: */
#define TSEM_Z_PREV     0   /* params before the last M-step == reference self.z (model.py:795) */
#define TSEM_Z_CUR      1   /* current params */
#define TSEM_Z_INITIAL  2   /* Q.norm(1), model.py:837 (initial=True)      */
#define TSEM_Z_USER     4   /* the z installed with tsem_set_user_z, used as is (a caller assigned tl.z, model.py:837) */
#define TSEM_Z_FIRST    3   /* tsem_get_params only: params after the FIRST iteration of the last run
                               == pi_init / theta_init (model.py:776-778) */

/* EM kernel selection (tsem_set_option "em_kernel") */
#define TSEM_EMK_AUTO     0
#define TSEM_EMK_TWOPASS  1   /* phase kernels, entries read twice                 */
#define TSEM_EMK_FUSED    2   /* persistent single-pass kernel with row-sum exchange */

typedef struct tsem_ctx tsem_ctx;

/* ---- lifecycle ---------------------------------------------------------- */
int  tsem_create(tsem_ctx** out, int device);
void tsem_destroy(tsem_ctx* h);
const char* tsem_last_error(const tsem_ctx* h);      /* h may be NULL: last create error */
int  tsem_set_stream(tsem_ctx* h, void* hip_stream); /* launch on this hipStream_t (default: null stream) */
/* options, set before tsem_rowstats (the layout is built from them):
 *   "em_kernel"    TSEM_EMK_*                      "block_rows", "parts"  override the layout geometry
 *   "value_format" 0 auto (2-byte score codes + LDS score table when the fused kernel runs and the table
 *                  has <= 2048 entries), 1 fp64 Q values, 2 codes (error if not possible)
 *   "index_format" index of fp64 entries under the fused kernel: 0 auto, 1 three bytes per entry, 2 the quad index — one 64-bit
 *                  word per four entries, 10 B per entry in all (error where it cannot apply: score codes, the split layout,
 *                  the strand-transposed fill, "reproducible", more than 512 row slots per block).  Auto takes the quad index where
 *                  it can apply, the dummy entries it needs stay within 0.5 % of the entries, and 11 B x the entries of the
 *                  ambiguous rows reach "index_auto_min_bytes" (default 1 GiB); see tsem_layout_info_n [40]-[43]
 *   "hot_split"    1 (default): very popular columns get several accumulator slots
 *   "row_offset"   global index of this rank's first row (synthetic generator, column signatures)
 *   "report_shortcuts" 1 (default): tsem_reassign answers `all` (initial) and `unique` from counts taken at
 *                  setup instead of a pass over the matrix (the same numbers; 0 forces the pass)
 *   "report_kernel" which kernels serve tsem_report_colsums / tsem_reassign_rows / tsem_reassign_groups: 1 (default) the streaming
 *                  report kernels, incl. the passes over the INITIAL z that run on the 2-byte score codes alone (no `conf` column
 *                  wanted, a strictly increasing score table, no stored score of 0); 0 the generic 16-lanes-per-row pass for
 *                  everything (same results); other values are rejected
 *   "report_dbg"   the final z's report kernel (tests, timing): 8 k_report_rows instead of k_report_pack32, 128 / 256 the latter
 *                  with 8 / 16 entries per lane; other bits are rejected
 *   "kernel_timing" n: HIP events around every n-th EM pass for tsem_kernel_stats (default 1, 0 = off)
 *   "phase_timing" 1: HIP events at the phase boundaries of every chunked iteration (tsem_phase_times)
 *   "drop_csr_indices" free the CSR column ids (4 of the 14 B per stored entry the default layout keeps resident) once the
 *                  blocked layout and the 2-byte popularity ids exist; they are rebuilt on demand (col = col_of_id[id]) for
 *                  the generic row passes, z export, tsem_export_csr and a layout rebuild.  -1 (default): from 4e9 stored
 *                  entries on; 0 never; 1 always
 *   "deconflict"   conflict-aware entry order inside the rows of the row-ordered code layout (LDS bank conflicts of the
 *                  column scatter 3.2 -> 2.4 lanes per class: -6 % per EM pass for ~4 ms of setup at 2e9 entries);
 *                  default -1 = on, 0 = off.  fp64 entries under the fused kernel (a non-split, row-ordered layout read through the
 *                  value map, 3-byte or quad index, not "reproducible"): the entries INSIDE each quad of four are ordered the same
 *                  way, among positions of one row (3.1 -> 2.2 lanes per class); 0 off, 1 on, -1 (default) on where 11 B x the
 *                  entries of the ambiguous rows reach "deconflict_min_bytes" (default 1 GiB).  Every other layout is left as it
 *                  is; see tsem_layout_info_n [44], [45]
 *   "reproducible" 1: ORDER-INDEPENDENT column sums in the fused EM pass.  Every contribution w*z is cut into a high and a low piece on
 *                  a per-column power-of-two grid; sums of such pieces are exact in fp64, so the unordered LDS atomics add up to
 *                  the same bits whatever their order: pi, theta, lnl and the iteration count are bit-identical from run to run
 *                  (same build, same device type, same number of ranks).  Two passes per iteration, plus a repeated pass when a
 *                  column's grid has to move (tsem_layout_info[20] counts them); the rows keep their entry order ("deconflict"
 *                  is off), so that a row's partial sum is one run ending in at most two atomics.  That holds for rows of up to
 *                  256 entries; with longer rows tsem_layout_info[21] reports 2 instead of 1 and the last bit of such a row's
 *                  sum may depend on timing.  3: a pass gave up moving a column's grid after 84 repeats — its sums are not
 *                  guaranteed exact (never seen; reported instead of hidden).  A hand-off time-out in this mode redoes the pass on the
 *                  fused kernel (the two-pass kernels have no exact sums); repeated time-outs end the run with TSEM_ERR_TIMEOUT on every rank.  Needs the fused kernel and a score table of <= 2048 entries; column sums are
 *                  within (entries of the column) x 2^-41 of exact, typically one fp64 rounding — "exact" being the sum of the fp64
 *                  contributions w*z as the default mode forms them, the error relative to the sum; the grids stop at 2^-903, so on top
 *                  of that every contribution may lose up to 2^-964 absolute (a column sum below 1e-290 may come out as 0).  The float-valued sums of
 *                  tsem_reassign / _rows / _groups / tsem_report_colsums (conf, average) are accumulated exactly as well
 *                  (two atomics per value).  1: both pieces in ONE pass over THREE tables per part when they fit the LDS (score
 *                  codes, at most 4800 columns per part with at most 8 parts — i.e. K <= 19k with teams of 4, K <= 38k with
 *                  long rows) — ~1.65x the default mode's time per iteration instead of ~2.5x; 2: always the two-pass form
 *                  (tsem_layout_info[22] says which one runs).  Default 0.
 *   "split"        how many loci the layout takes.  K <= 61 440 (8 column parts of 7680): the fused single-pass kernel.  K <= 122 880:
 *                  the SPLIT layout of the fused kernel (-1, default: when K needs it) — parts of up to 15 360 columns, one LDS table
 *                  per pass: a row-sum pass and a scatter pass per iteration (every entry read twice), the log-likelihood over two
 *                  halves of every part's columns; ~1.4-1.5x the fused kernel's time per entry.  1 forces it on a smaller matrix
 *                  (tests; needs "parts" >= 5), 0 forbids it (the two-pass kernels then take over at K > 61 440).  K <= 491 520:
 *                  the two-pass kernels (64 column parts).  Beyond: plain CSR row passes with global fp64 atomics — any K, an order
 *                  of magnitude slower per entry (tsem_layout_info[24] / [26] say which form runs).
 *   "boot_hot_columns", "boot_batch"  tsem_bootstrap (below): how many of the most popular columns get workgroup-private LDS accumulators
 *                  (-1, default: as many as 32 KiB of LDS hold for the batch, 4096 / batch; 0 none: every sum is a global fp64 atomic;
 *                  at most 5120 / batch) and how many replicates share one sweep over the matrix (0, default: 8, the most)
 *   "boot_rows_per_block"  tsem_bootstrap (below): a test and timing hook.  0 (default): every workgroup of the sweeps takes
 *                  max(32, ceil(rows / (4 x compute units)) rounded up to 32) rows.  n > 0: n rounded up to a multiple of 32 instead.
 *                  Negative values are rejected.  The results do not depend on it beyond the order of the fp64 atomics.
 *   "boot_group_bytes"  tsem_bootstrap_groups (below): bytes of the per-batch accumulators of the (group, column) pattern at most; the
 *                  batch is lowered to fit.  0 (default): what is free.  Negative values are rejected.
 *   "cell_em_spread_entries"  tsem_cell_em (below): a group of the map with MORE stored entries than this is not fitted by one workgroup
 *                  but spread over the whole grid, one set of short kernel launches per iteration (a cell type of a single-cell run).
 *                  0: never spread; negative values are rejected.  May be set at any time; the next tsem_cell_em reads it.  Default
 *                  32768.  Measured with tools/time_group_em.py (profiles/r14_group_em.txt): one group of 2^14 ... 2^22 entries is
 *                  fitted 1.2 x ... 22 x faster spread than by one workgroup — no crossover inside the sweep; 2^15 (1.5-1.9 x) is
 *                  the smallest power of two above every group a droplet cell gives (and above every cell of the unit's older tests)
 *   "em_precision" 1: the EM pass in fp32 arithmetic (row sums, posteriors and column sums in fp32) — a
 *                  DIAGNOSTIC for the fp32-vs-fp64 tolerance sweep of BASELINE config 3, not a product path
 *   "fused_dbg"    test hooks, a sum of bits: 32 / 64 the fused EM / lnl pass behaves like a hand-off time-out; 8192 the lnl pass
 *                  takes a logarithm per entry, 16384 looks log Q up where the arithmetic form applies, 32768 takes the log
 *                  form whatever the parameters.  Any other bit: TSEM_ERR_ARG.
 *   "fused_dbg_skip"  n: bits 32 / 64 of "fused_dbg" reach the kernel only after n fused launches of the kind they aim at (EM passes
 *                  for 32, lnl passes for 64; a split or "reproducible" EM pass is several launches) have gone by since either
 *                  option was set — a time-out placed inside a chunk.  0 (default): at once.  The hook stays an early return that
 *                  leaves the error word behind.  Negative: TSEM_ERR_ARG.
 *   "fused_prof", "chunk_blocks"     timing experiments */
int  tsem_set_option(tsem_ctx* h, const char* key, int64_t value);
int  tsem_synchronize(tsem_ctx* h);

/* ---- score matrix (model.py:638-653; sparse_plus.py:89-91) ---------------
 * CSR of uint16 raw scores for the rows this rank owns.  `lut[r]` is
 * Q = expm1((r * (1/max_score)) * 100.) for r = 0..lut_len-1, computed by the
 * host with the reference's numpy expression so Q is bit-identical; max_score
 * is the GLOBAL maximum (all ranks).  The arrays are borrowed for the call, copied to HBM and validated there
 * (non-decreasing row pointers, column ids in [0, n_cols), scores < lut_len): TSEM_ERR_ARG and no matrix otherwise.
 * `lut` may be NULL: the table then follows with tsem_set_lut once the (global) maximum is known — tsem_max_score
 * takes it on the device, so the host never has to scan the entries. */
int  tsem_load_scores(tsem_ctx* h, int64_t n_rows, int32_t n_cols,
                      const int64_t* indptr, const int32_t* indices,
                      const uint16_t* raw, const double* lut, int32_t lut_len);
/* Generate rows [row_begin,row_end) of the synthetic matrix on the device
 * (telescope_amd/synthetic.py is the bit-exact CPU twin).  `len_cdf` is
 * synthetic.poisson_cdf_u32(mean).  dist: 0 uniform, 1 zipf, 2 family (every row inside one family of 256 consecutive loci).  */
int  tsem_generate(tsem_ctx* h, int64_t row_begin, int64_t row_end, int32_t n_cols,
                   const uint32_t* len_cdf, int32_t cdf_len, uint64_t seed,
                   int32_t dist, double uniq_frac);
/* largest raw score of the local rows; (re)install the Q lookup table once the
 * GLOBAL maximum is known (model.py:640,653).
 * What the set-up assumes of a caller's table: finite, non-negative and NON-DECREASING entries.  tsem_rowstats takes a row's weight
 * from the row's largest CODE (w_i = lut[max code] is max_j Q_ij only then), stats[2] from the largest code of all, and the top of
 * the grids of the exact pisum0 from the table's LAST entry; none of this is validated. */
int  tsem_max_score(tsem_ctx* h, int32_t* max_score);
int  tsem_set_lut(tsem_ctx* h, const double* lut, int32_t lut_len);
/* The table for a host without numpy (the C host of tests/c_host/): lut[r] = expm1((r * (1 / max_score)) * scale_factor), r = 0 ..
 * max_score, with the C library's expm1.  NOTE what this is not: numpy's `expm1` — what the reference evaluates (model.py:653) — is a
 * SIMD routine on AVX-512 hosts and differs from libm's in the last bit of ~10 % of the entries (measured: 23 of 213 for max_score
 * 212, 6493 of 65536).  Every result then agrees with the reference's to ~1e-15 relative instead of bit for bit; a host that needs the
 * reference's bits passes the table the reference's own numpy produced (telescope_amd/likelihood.py score_lut does).  No handle, no
 * device: host arithmetic only. */
int  tsem_score_lut(int32_t max_score, double scale_factor, double* lut /* max_score + 1 */);
int  tsem_dims(tsem_ctx* h, int64_t* n_rows, int32_t* n_cols, int64_t* nnz);
/* copy the CSR back to the host (tests of the generator) */
int  tsem_export_csr(tsem_ctx* h, int64_t* indptr, int32_t* indices, uint16_t* raw);

/* ---- model setup (model.py:679-699) --------------------------------------
 * tsem_rowstats: Y, weights w_i = max_j Q_ij, and the LOCAL sums
 *   stats[0]=sum w, stats[1]=sum w*Y, stats[2]=max w, pisum0[K] = sum of Q over
 *   unique rows per column; col_count[K] = stored entries per column and
 *   col_hash[K] = order-independent 64-bit signature sum_i hash(global row, score)
 *   (wrap-around).  Multi-GPU hosts all-reduce them (sum,sum,max,sum,sum,sum).
 *   pisum0 is EXACT — exact sums on 9 grids 26 bits apart, added in a fixed order: independent of the order of
 *   the rows, of the launch and of the run, within 8 x 2^-53 of the exact sum — while floor(log2(largest entry)) -
 *   floor(log2(smallest positive entry)) <= 9 x 26 - 53 = 181 (any table whose largest / smallest positive entry is below
 *   2^181; the reference's span 2^145 to 2^154), the last entry lies in [2^-841, 2^997) and a column has at most 2^26
 *   unique rows.  Past that range what the grids leave of a Q is added with an ordinary fp64 atomic: pisum0[j] stays within
 *   (n_j + 9) x 2^-53 relative of the exact sum (n_j unique rows in column j) and is 0 only where the exact sum is 0, but its
 *   last bits then depend on the order of those atomics.  (Of col_hash only the low 32 bits are a function of the matrix: the
 *   value is a sum over workgroups of sums modulo 2^32, so its high half depends on how the rows fell to the workgroups —
 *   alike for twin columns, whose entries every workgroup sees alike, which is all twin detection needs.)
 *   Columns with equal (count, hash) are exact twins (same fragments, same
 *   scores): the reference keeps their pi/theta bit-identical because scipy
 *   accumulates every column in row order, and `reassign` ties depend on it, so
 *   the update step gives twins one shared accumulation.
 * tsem_set_model: global stats + priors; builds the column-partitioned EM
 *   layout and resets pi = theta = 1/K (model.py:667,673).  */
int  tsem_rowstats(tsem_ctx* h, double* stats3, double* pisum0,
                   uint64_t* col_count, uint64_t* col_hash);
/* Y[N] (model.py:679) and weights[N] = w_i (model.py:690) of the local rows as tsem_rowstats left them on the
 * device (either pointer may be NULL): the reference's `tl.Y` / `tl._weights`. */
int  tsem_export_rowinfo(tsem_ctx* h, uint8_t* Y, double* weights);
int  tsem_set_model(tsem_ctx* h, const double* stats3, const double* pisum0,
                    const uint64_t* col_count, const uint64_t* col_hash,
                    double pi_prior, double theta_prior);

/* ---- parameters ---------------------------------------------------------- */
int  tsem_set_params(tsem_ctx* h, const double* pi, const double* theta);
int  tsem_get_params(tsem_ctx* h, int which /*TSEM_Z_PREV|TSEM_Z_CUR|TSEM_Z_FIRST*/, double* pi, double* theta);

/* ---- EM iteration (estep model.py:702-722 + mstep 724-742, fused) ---------
 * tsem_em_pass: local fused E+M over this rank's rows with the current
 *   params; leaves red[0..K) = local thetasum, red[K] = 0, red[K+1] = 0 in the
 *   reduce buffer (device).  Asynchronous.
 * tsem_em_update: consumes the (all-reduced) reduce buffer: theta_hat, pi_hat
 *   (model.py:733-740), diff_est = sum|pi_hat - pi| (model.py:781); current
 *   params become "prev".  Synchronous when diff_est != NULL.
 * tsem_lnl_pass: local part of calculate_lnl(z(prev), cur) (model.py:744-760)
 *   into red[K]; tsem_read_reduce fetches the buffer.  */
int  tsem_reduce_buffer(tsem_ctx* h, void** dptr, int64_t* count);
int  tsem_bind_reduce_buffer(tsem_ctx* h, void* dptr, int64_t count); /* count >= K+2 doubles */
int  tsem_em_pass(tsem_ctx* h);
int  tsem_em_update(tsem_ctx* h, double* diff_est);
int  tsem_lnl_pass(tsem_ctx* h);
int  tsem_read_reduce(tsem_ctx* h, double* out, int64_t offset, int64_t count);
/* n fixed iterations (pass [+ all-reduce] + update) with no host round trip; the
 * per-iteration diff_est values are left in a device ring and copied out at the
 * end.  == em() with em_epsilon=0, max_iter=n. */
int  tsem_em_steps(tsem_ctx* h, int32_t n, double* diffs_out /* n or NULL */);
/* The loop body of em() (model.py:771-797) for up to n_max iterations, enqueued
 * back to back: fused E+M pass, column reduce, all-reduce (communicator
 * attached), parameter update; with use_likelihood also the lnl pass, its
 * all-reduce and the |lnl - lnl_prev| test.  Convergence (diff_est < epsilon,
 * or the lnl test) is decided ON THE DEVICE: the update kernel raises a stop
 * flag and every kernel enqueued behind it returns at once, so the host
 * synchronises once per chunk, not once per iteration, and the state after the
 * call is exactly the reference's after its last iteration.  flags bit 0
 * starts a run (lnl_prev = inf or tsem_set_prev_lnl, the next update saves
 * pi_init / theta_init).
 * *n_done = iterations committed, *stopped = 1 when the convergence test fired.
 * use_likelihood on a layout built for it (option "use_likelihood" = 1 before
 * tsem_set_model, or tsem_prepare_likelihood): no lnl pass per iteration — the
 * EM pass of iteration t+1 also sums lnl_t = sum z_t log1p(Q c_t) (model.py:
 * 783-789: its numerators ARE Q c_t; pi*theta of the previous parameters is a
 * third LDS table, the previous row sums are kept per row), and that
 * iteration's update kernel tests |lnl_t - lnl_(t-1)| < epsilon BEFORE it
 * commits: a run that converges in iteration t ends in the state of iteration
 * t.  The lnl of the chunk's LAST iteration is then unknown when the chunk
 * returns (lnls_out[n_done - 1] = NaN): it arrives as *lnl_carry of the next
 * chunk — which may do nothing else: n_done = 0, stopped = 1 — or, with flags
 * bit 1 (last chunk of the run), from the dedicated lnl pass before the call
 * returns.  *lnl_carry is NaN when nothing was owed.
 * A hand-off time-out of the fused kernel on ANY rank (the flag travels in the
 * all-reduce) leaves the parameters untouched on every rank; the failing rank
 * rebuilds its layout for the two-pass kernels and the iteration is redone. */
int  tsem_em_chunk(tsem_ctx* h, int32_t n_max, double epsilon, int32_t use_likelihood, int32_t flags,
                   int32_t* n_done, int32_t* stopped, double* diffs_out /* n_max or NULL */,
                   double* lnls_out /* n_max or NULL */, double* lnl_carry /* 1 or NULL */);
/* em(use_likelihood=True) on a model laid out without option "use_likelihood": rebuild the blocked layout so that the EM
 * pass can carry the log-likelihood (above).  A no-op when the layout has it or cannot have it (two-pass kernels, fp64
 * entries, option "reproducible", K > 8 x 5056): tsem_em_chunk then runs the lnl pass every iteration. */
int  tsem_prepare_likelihood(tsem_ctx* h);
/* Switch this handle to the two-pass kernels (rebuilds the blocked layout, keeps the parameters): what
 * tsem_em_chunk does after a time-out; public for hosts that drive pass / update themselves. */
int  tsem_fallback_twopass(tsem_ctx* h);
/* After tsem_em_update returned TSEM_ERR_TIMEOUT (every rank does, the flag is all-reduced): the rank whose
 * own fused pass raised the error word switches to the two-pass kernels (*switched = 1), the others do
 * nothing; then every rank redoes the pass. */
int  tsem_recover_timeout(tsem_ctx* h, int32_t* switched);
/* calculate_lnl(z(prev params), current params) (model.py:800-801), summed over the ranks of an attached
 * communicator; synchronous.  Redone on the two-pass kernels after a time-out of the fused pass. */
int  tsem_final_lnl(tsem_ctx* h, double* lnl);
/* The log-likelihood the FIRST iteration of the next run (tsem_em_chunk with first != 0) is compared with under
 * use_likelihood: the reference compares with self.lnl as the previous em() left it (model.py:786; inf on a fresh
 * model, model.py:683).  tsem_set_model resets it to inf, tsem_em_run leaves its final value. */
int  tsem_set_prev_lnl(tsem_ctx* h, double lnl);
/* Full EM loop (model.py:762-806) on top of tsem_em_chunk. */
int  tsem_em_run(tsem_ctx* h, double epsilon, int32_t max_iter, int32_t use_likelihood,
                 int32_t* n_iter, int32_t* converged, double* lnl,
                 double* diffs /* max_iter */, double* lnls /* max_iter or NULL */,
                 double* pi_init, double* theta_init /* K each or NULL */);

/* ---- communicator (row-sharded runs) ---------------------------
 * One RCCL communicator per process / GPU, created from an id that rank 0
 * generates and the host ships to the other ranks by any means (the Python
 * host uses its torch.distributed group).  Attached to a handle, it makes
 * tsem_em_chunk / tsem_em_steps / tsem_em_run all-reduce the reduce buffer
 * (sum, fp64, K+2) and the log-likelihood scalar on the handle's stream.
 * tsem_comm_allreduce_host: in-place sum of a host fp64 / uint64 vector over the
 * communicator (setup sums, reassign column sums).  */
#define TSEM_COMM_ID_BYTES 128
typedef struct tsem_comm tsem_comm;
int  tsem_comm_unique_id(void* id128);
int  tsem_comm_create(tsem_comm** out, int device, const void* id128, int rank, int world);
void tsem_comm_destroy(tsem_comm* c);
const char* tsem_comm_last_error(void);
int  tsem_comm_attach(tsem_ctx* h, tsem_comm* c);             /* c == NULL detaches */
int  tsem_comm_allreduce(tsem_ctx* h, int64_t offset, int64_t count);   /* reduce buffer [offset, offset+count), async */
int  tsem_comm_allreduce_host(tsem_comm* c, void* data, int64_t count, int dtype /*0 f64 sum, 1 u64 sum, 2 f64 max, 3 i64 max*/);
/* RCCL is resolved at run time, not linked: the librccl already mapped into the process (a torch process carries
 * one) or else librccl.so.1 from the loader path — ONE copy, chosen deliberately; without RCCL the library still
 * loads and runs single-GPU.  Writes "rccl <version> (<path>)" (or why it is unavailable) into buf. */
int  tsem_comm_library_info(char* buf, int32_t cap);
/* In-process transport: `world` handles on ONE device, one host thread each (tests of the row-sharded protocol on
 * a one-GPU box; hosts that share a GPU between engines).  Same tsem_em_chunk, same reduce buffer, error slot and
 * device-side stop flag; the all-reduce is a copy into per-rank slots, a host rendezvous of the ranks' threads at
 * ENQUEUE time, stream waits on the peers' events and a sum in rank order (bit-identical on every rank). */
typedef struct tsem_local_group tsem_local_group;
int  tsem_comm_local_group(tsem_local_group** out, int device, int world /* <= 8 */);
void tsem_comm_local_group_destroy(tsem_local_group* g);      /* after every communicator of the group */
int  tsem_comm_create_local(tsem_comm** out, tsem_local_group* g, int rank);
/* How long a rank waits at the host rendezvous for its peers before its collective fails with TSEM_ERR_TIMEOUT and the
 * group counts as broken (default 120 s; seconds > 0).  Tests set a short one, so that a rank that raised ends them soon. */
int  tsem_comm_local_group_set_timeout(tsem_local_group* g, double seconds);

/* ---- results -------------------------------------------------------------- */
/* z aligned to the CSR pattern of the loaded scores (-1 where the reference
 * drops the entry from z's pattern, i.e. where Q_ij * pi_j[*theta_j] == 0).  model.py:795 / 837.  */
int  tsem_export_z(tsem_ctx* h, int which, double* z /* nnz */);
/* install (z != NULL) or drop (NULL) a caller-supplied z aligned to the CSR pattern, NaN where z has no
 * entry: `which` = TSEM_Z_USER then makes reassign / best_counts / reassign_groups read it as is, without
 * renormalising — what the reference does with whatever `self.z` holds (model.py:837) */
int  tsem_set_user_z(tsem_ctx* h, const double* z /* nnz or NULL */);
/* estep on explicit params (public estep(pi,theta), model.py:702-722) */
int  tsem_estep(tsem_ctx* h, const double* pi, const double* theta, double* z /* nnz */);
/* public mstep(z) (model.py:724-742) and calculate_lnl(z,pi,theta) (744-760) on a
 * caller-supplied z aligned to the CSR pattern (0 where z has no entry); with a communicator
 * attached both sum over the ranks' row shards before the closed forms / the return */
int  tsem_mstep(tsem_ctx* h, const double* z, double* pi_hat, double* theta_hat);
int  tsem_calc_lnl(tsem_ctx* h, const double* z, const double* pi, const double* theta, double* lnl);
/* rows' best-hit counts for `choose` (sparse_plus.py:117-129): nbest[i] */
int  tsem_best_counts(tsem_ctx* h, int which, int32_t* nbest /* n_rows */);
/* the same, compacted on the device: only the rows with SEVERAL best hits (the ones `choose` draws a random
 * number for, sparse_plus.py:147-149), in row order: rows[i] = local row index, counts[i] = its number of best hits.
 * *n = how many there are; if n > cap nothing is copied and TSEM_ERR_ARG is returned (call again with cap >= n). */
int  tsem_best_ties(tsem_ctx* h, int which, int64_t cap, int32_t* rows, int32_t* counts, int64_t* n);
/* reassign(method, thresh, initial).sum(0) (model.py:808-865,435-457) -> colsums[K]
 * (local rows); optional per-entry mask aligned to the CSR pattern (nnz doubles,
 * NULL to skip).  `picks[i]` (choose only) = ordinal of the chosen best hit. */
int  tsem_reassign(tsem_ctx* h, int method, double thresh, int which,
                   const int32_t* picks, double* colsums, double* mask);
/* The column sums `Telescope.output_report` takes from ONE z (model.py:432-457) in ONE pass over the rows:
 * out[0..K) = reassign('conf', thresh).sum(0), out[K..2K) = 'exclude', out[2K..3K) = 'average' (local rows).  The
 * rows with several best hits — the only rows `choose` treats differently from `exclude` (sparse_plus.py:140-154) —
 * are compacted on the device in row order: *n_ties of them; tsem_report_ties copies their indices and numbers of
 * best hits out (cap >= n_ties), and tsem_reassign_rows(TSEM_RA_CHOOSE, ..., rows = NULL, picks, n_ties, out) adds up
 * the picked entries of exactly those rows, so that  choose = exclude + that.  tsem_reassign_rows with a caller's
 * row list gives the contribution of those rows to any method (picks[i] belongs to rows[i]).
 * thresh < 0: the caller needs no `conf` column (out[0..K) is then not meaningful).  For the INITIAL z the pass then runs on
 * the 2-byte score codes alone — a row's best hits are its largest codes when the score table is strictly increasing and no
 * stored score is 0 — with no score-table look-up and no floating point (k_report_init_codes). */
int  tsem_report_colsums(tsem_ctx* h, int which, double thresh, double* out /* 3*K */, int64_t* n_ties);
int  tsem_report_ties(tsem_ctx* h, int64_t cap, int32_t* rows, int32_t* counts);
int  tsem_reassign_rows(tsem_ctx* h, int method, double thresh, int which, const int32_t* rows,
                        const int32_t* picks, int64_t n, double* colsums);
/* z[ridx, fidx] and reassign(method, thresh)[ridx, fidx] for the entries of a LIST of rows: what Telescope.update_sam reads per
 * alignment (model.py:483,508-511 — `prob = tl.z[ridx, fidx]`, `mat[ridx, fidx] > 0`), without the N x K matrices.  Row rows[i]'s
 * entries (CSR order) go to z_out / mask_out [out_off[i], out_off[i + 1]) (out_off[n] = total; the slices must have the rows'
 * lengths: TSEM_ERR_ARG otherwise).  z_out: -1 where the reference drops the entry from z's pattern.  picks[i] (choose) belongs to
 * list row i.  Either output may be NULL. */
int  tsem_rows_lookup(tsem_ctx* h, int which, int method, double thresh, int64_t n, const int32_t* rows, const int32_t* picks,
                      const int64_t* out_off, double* z_out, double* mask_out);
/* The tags Telescope.update_sam sets on a PRI alignment (model.py:479-521), for every stored entry of the rows [row_begin,
 * row_end) — a tile of consecutive rows — in ONE row pass: out[k - indptr[row_begin]] for entry k (CSR order) =
 *   mapq | XP << 8 | assigned << 16 | (z >= 0.2) << 17
 * with z = the entry's posterior in `which`'s z (0 where the reference drops it from z's pattern; formed like tsem_rows_lookup's
 * z_out), mapq = phred(z) (helpers.py:14-37: the number of phred_tab entries <= z, 255 for z >= 1), XP = int(round(z * 100)),
 * assigned = reassign(method, thresh)[row, col] > 0.  phred_tab: n_tab < 256 non-decreasing thresholds in [0, 1) (entry q - 1:
 * the least P where numpy's scalar expression reaches q, computed on the host).  picks[i] (choose) belongs to tile row i.
 * In a near-tie row (two different numerators within 2^-42 at the row's maximum, or a z that close to `thresh`: tsem_layout_info
 * [31] counts them) the two halves of the word use two row sums: mapq, XP and the 0.2 bit are taken from the pass's own z — the
 * numerator times the reciprocal of the row sum in the pass's order of additions, bit for bit what tsem_export_z and
 * tsem_rows_lookup's z_out give — while `assigned` is decided with the row sum added in the reference's order (np.add.reduceat),
 * as tsem_rows_lookup's mask_out is; the two z differ by summation order only, (len + 3) 2^-53 relative at most.
 * With option "drop_csr_indices" the column ids are rebuilt at the first tile and kept: call tsem_entry_tags_end after the last
 * tile. */
int  tsem_entry_tags(tsem_ctx* h, int which, int method, double thresh, const int32_t* picks, int64_t row_begin, int64_t row_end,
                     const double* phred_tab, int32_t n_tab, uint32_t* out);
/* end of a run of tsem_entry_tags tiles: column ids rebuilt for them go again where option "drop_csr_indices" drops them */
int  tsem_entry_tags_end(tsem_ctx* h);
/* The random picks of `choose` (sparse_plus.py:140-154: np.random.choice per row with several best hits) in numpy's
 * LEGACY stream, on the host: out[i] = the draw np.random.randint(0, counts[i]) would return, taken in order from the
 * MT19937 state (key624, *pos) = np.random.get_state()[1:3]; the state is advanced exactly as numpy advances it, so
 * the caller's stream continues unchanged after np.random.set_state.  counts[i] >= 1 (1 consumes nothing). */
int  tsem_legacy_randint(uint32_t* key624, int32_t* pos, const int32_t* counts, int64_t n, int32_t* out);
/* the same assignment summed per GROUP of rows: scTelescope.output_report's per-barcode count matrix
 * `_assignments[_rows, :].sum(0)` for every barcode (model.py:611-625).  group_of_row[i] in
 * [0, n_groups) or -1 (row in no group); out is row-major [n_groups][K], caller-allocated.
 * tsem_set_groups copies the map to the device once (range-checked there) — the six methods of a report
 * then pass group_of_row = NULL; a non-NULL map is set first.  The device computes the groups in tiles
 * of at most 1 GB of device scratch (option "group_tile_bytes": the tile by column plus, for the streaming
 * kernel, the same tile by id), one pass over the matrix per tile: n_groups x K
 * doubles only have to fit the caller's `out`.  exclude / average / conf (conf_prob > 0.5) stream the
 * 4-byte id + score-code arrays like tsem_report_colsums; the other methods take the generic row pass. */
int  tsem_set_groups(tsem_ctx* h, const int32_t* group_of_row /* N, or NULL to drop */, int32_t n_groups);
int  tsem_reassign_groups(tsem_ctx* h, int method, double thresh, int which, const int32_t* picks,
                          const int32_t* group_of_row /* N, or NULL: the map of tsem_set_groups */, int32_t n_groups, double* out);
/* Per-barcode counts at droplet scale (model.py:611-625), where the dense n_groups x K matrix above is almost all zeros:
 * reassign(method, thresh, which)[rows of group g, :].sum(0) for every group g of the row -> group map set with
 * tsem_set_groups (a partition: each row in at most one group, -1 = none), as a SPARSE matrix kept on the device;
 * *nnz = its stored entries.  Rows of a group are taken in ascending row order.  picks: as tsem_reassign_groups.
 * Every (group, column) is added in ascending row order starting from 0 — what scipy's csr[rows].sum(0) does — so the
 * result is bit-identical to summing tsem_reassign's matrix with scipy, for every method, and deterministic.  No global
 * atomics: the entries of a tile of groups (option "group_tile_bytes" of device scratch for the tile's buffers, default 1 GB; the
 * grouping cached per map, 16 B per row, the picks and the result are outside it) are sorted by
 * (group, column) and one lane adds each (group, column)'s values; a (group, column) that holds a large share of the
 * matrix's rows therefore runs at one lane's speed (real barcodes never do).  Single GPU only: a handle with a
 * communicator attached is refused. */
int  tsem_group_counts(tsem_ctx* h, int method, double thresh, int which, const int32_t* picks, int64_t* nnz);
/* copy the last result out: group_ptr[n_groups + 1] (int64), cols[nnz] ascending within a group, vals[nnz] (fp64) */
int  tsem_group_counts_copy(tsem_ctx* h, int64_t* group_ptr, int32_t* cols, double* vals);
/* the last result's number of groups and stored entries: what the arrays of tsem_group_counts_copy must hold */
int  tsem_group_counts_shape(tsem_ctx* h, int32_t* n_groups, int64_t* nnz);
/* Single-cell `individual` pooling: ONE EM fit per group (cell) of the map set with tsem_set_groups — a partition: each row in at
 * most one group, -1 = none — instead of one fit of the pool (model.py:762-806 per cell; the reference fits the pool only,
 * model.py:570-625).  The fit of cell c is TelescopeLikelihood(raw[rows of c]) with the score scale of the whole matrix: the cell's
 * own weights, total_wt / ambig_wt, prior weights prior x (the cell's largest weight) (model.py:690-697) and pisum0 (:699); all K
 * columns count: a column the cell never touches has the closed-form value prior_wt / (total + prior_wt K) and takes part in
 * diff_est (model.py:781).  Priors as given to tsem_set_model; needs tsem_rowstats and the score table.  A group of up to
 * "cell_em_spread_entries" stored entries is fitted by one workgroup from its first iteration to its last, all such groups in one
 * launch per class (by Kc: <= 256 columns and <= 4096 entries a wave | <= 1024 256 threads | <= 3840 512 threads, tables in LDS |
 * beyond, tables in a global workspace); column sums are taken in ascending row order (scipy's).  A group with more entries — one
 * enormous group, a cell type — is no longer served by one workgroup: the SPREAD class fits all such groups together with the whole
 * grid, a row kernel, a column kernel and a one-workgroup-per-group finish kernel per iteration (under use_likelihood the lnl kernel
 * as well), no workgroup waiting for another; the host enqueues 8 iterations per look at the groups' done marks, which changes no
 * result.  There a column of n entries is added by one lane ascending from 0 for n <= 32, by a wave for n <= 4096 (lane l the
 * ascending piece of ceil(n / 64) entries, the 64 partials through a fixed tree) and by a 256-thread workgroup beyond (pieces of
 * ceil(n / 256), a fixed tree); rows are handled in chunks of 1024 and the weights' totals and lnl are sums of the chunks' parts in
 * chunk order.  In every class the order of a sum depends on the group alone, so the result is deterministic, exact twins inside a
 * group keep bit-identical pi / theta, and a group stops after the same iteration and gets the same bits whatever else is in the
 * call; the spread class's orders differ from the one-workgroup classes', so a group's BITS depend on its class (spread or not).
 * A cell without rows is not fitted: n_iter 0, converged 0, lnl NaN.
 * Installs the per-cell final z — the last E-step's (model.py:795), NaN outside z's pattern and for rows in no cell — as the
 * TSEM_Z_USER buffer: every report entry point reads it with which = TSEM_Z_USER.  Leaves the pooled state (pi, theta,
 * TSEM_Z_PREV/CUR, lnl) untouched.  The compacted per-cell layout (18 B per stored entry of the cells' rows, 38 B while it is
 * built, cached per group map) must fit the device: TSEM_ERR_NOMEM with a message otherwise.  Single GPU only: a handle with a
 * communicator attached is refused. */
int  tsem_cell_em(tsem_ctx* h, double epsilon, int32_t max_iter, int32_t use_likelihood);
/* the last fit's number of cells and the sum of the cells' distinct columns Kc: what the arrays of tsem_cell_em_copy must hold */
int  tsem_cell_em_shape(tsem_ctx* h, int32_t* n_cells, int64_t* n_cols /* sum of Kc */);
/* copy the last fit out: cell c's distinct columns are cols[col_ptr[c] .. col_ptr[c + 1]) (ascending) with pi / theta (model.py:
 * 733-740) and pi_init / theta_init (model.py:776-778) beside them; rest[4 c ..] = pi, theta, pi_init, theta_init of every column the
 * cell does not touch; n_iter, converged, lnl (model.py:800-806) per cell */
int  tsem_cell_em_copy(tsem_ctx* h, int64_t* col_ptr /* n_cells+1 */, int32_t* cols,
                      double* pi, double* theta, double* pi_init, double* theta_init, /* n_cols each */
                      double* rest /* n_cells x 4: the four values of the untouched columns */,
                      int32_t* n_iter, int32_t* converged, double* lnl /* n_cells each */);

/* ---- bootstrap replicates of the EM fit ---------------------------------------------------------------------------------------
 * Replicate b gives every row i a multiplicity m_i in 0..255; its fit is, by definition, the reference's fit of the matrix in which
 * row i appears m_i times (model.py:762-806 on raw[np.repeat(arange(N), m_b)]) with the score scale of the whole matrix, as for the
 * per-cell fits: its own W_tot = sum m w, W_amb = sum m w Y, prior weights prior x (the largest w of a row with m > 0), pisum0 =
 * sum over unique rows of m Q; all K columns, dense, from pi = theta = 1 / K.  Only the parameter stop test (diff_est < epsilon,
 * model.py:792) is offered.  `mult` NULL: Poisson(1) draws of the counter hash, m = #{n : T[n] <= hash3(seed ^ SALT_BOOT, global
 * row, b) >> 32} with T = floor(2^32 P(X <= n)) (at most 14; telescope_amd/synthetic.py bootstrap_multiplicities gives the same
 * numbers on the host), evaluated on the fly; else a HOST array [n_rep x N] that is copied to the device (TSEM_ERR_NOMEM with a
 * message if results, workspace and multiplicities do not fit).  Priors as given to tsem_set_model, whose twin classes are used
 * as well: a call before it is TSEM_ERR_ARG.
 * Replicates are fitted in batches of up to 8 that share every sweep over the CSR (scores, column ids through the same scope as
 * every other row pass: option "drop_csr_indices" keeps working); each stops on its own — diff_est < epsilon or max_iter — and is
 * frozen by the update kernel from then on, whatever else is in the batch and however often the host looks.  After its last
 * iteration: lnl (model.py:795-801, the z of the parameters before the last M-step against those after it) and counts[j] =
 * sum_i m_i A[i, j] with A = reassign(method, thresh) of that z (model.py:837-862; TSEM_RA_CHOOSE is refused).  A replicate with
 * sum m = 0 is not fitted: n_iter 0, not converged, NaN pi / theta / counts / lnl.  One whose parameters turn NaN (no ambiguous
 * fragment at theta_prior = 0) runs to max_iter unconverged, like the reference, and has NaN counts and lnl.
 * Column sums are unordered fp64 atomics (LDS for the most popular columns, options "boot_hot_columns" / "boot_batch"): results
 * agree from run to run to rounding, not bit for bit, so a handle with option "reproducible" is refused, as is a row-sharded
 * one (TSEM_ERR_ARG with a message).  Columns that are twins only inside a replicate (the rows that tell them apart drew 0) are not
 * recognised; ties between them may fall differently from the reference's.  The pooled state, every z buffer, the per-cell fits and
 * the blocked layout are left untouched. */
int  tsem_bootstrap(tsem_ctx* h, int32_t n_rep, uint64_t seed, const uint8_t* mult /* NULL | n_rep x N */,
                    int32_t method, double thresh, double epsilon, int32_t max_iter);
/* copy the last call's results out (tsem_dims gives K, the caller knows n_rep) */
int  tsem_bootstrap_copy(tsem_ctx* h, double* pi, double* theta, double* counts /* n_rep x K each, any may be NULL */,
                         int64_t* n_frags /* sum of m_i */, int32_t* n_iter, int32_t* converged, double* lnl /* n_rep each, any may be NULL */,
                         int32_t* info2 /* replicates per batch and hot columns used; may be NULL */);
/* The same replicates with PER-GROUP counts (single-cell: per barcode): besides everything tsem_bootstrap leaves for
 * tsem_bootstrap_copy — same definitions, the same fits, fitted once — the call gives, for the row -> group map g(i) set with
 * tsem_set_groups (a partition, -1 = the row is in no group; G groups), statistics over the replicates of
 *   X_b[g, j] = sum over the rows i with g(i) = g of m_{b,i} A_b[i, j],   A_b = reassign(method, thresh) of replicate b's last z,
 * on the PATTERN P: the distinct (g, j) such that some row of group g stores an entry in column j, ordered by (g, j) — group_ptr
 * [G + 1], cols ascending within a group.  P is structural: it depends on the matrix and the map alone, not on any z or replicate; it
 * is built once per map (the grouping, entry keys and stable sort of tsem_group_counts, without values; tiles under option
 * "group_tile_bytes", 32 B per entry of a tile) and stays on the device, 8 B per group and 4 B per slot.  Rows in no group add to
 * counts[b, :] as before and to no X.  A replicate is GOOD if it has fragments and its lnl is not NaN (the replicates whose counts
 * are not NaN); n_used counts them.  Per slot, over the good replicates in replicate order, by Welford's update (d = x - mean;
 * mean += d / k; M2 += d (x - mean); one thread owns a slot): mean (NaN when n_used = 0) and sd with ddof 1 (NaN when n_used < 2;
 * equal values give exactly 0).  keep_values != 0 also keeps values[n_rep x nnz], X_b per replicate, the row of a bad replicate NaN.
 * X_b is summed with one fp64 atomic per non-zero m A[i, j]: for exclude, unique and all every addend is an integer and X_b, mean and
 * sd are exact and reproducible; for average and conf they agree from run to run to rounding.  If every row is in a group, sum_g
 * X_b[g, j] = counts[b, j] (exactly for the integer methods).
 * Memory: 16 B per slot (mean, sd), 8 B x n_rep per slot if values are kept, and the batch's accumulators, 8 B x batch per slot.
 * Option "boot_group_bytes" caps the accumulators (0, default: what is free after results and workspace, less a 64 MiB margin);
 * where they do not fit at the batch asked for the batch is lowered, down to 1 (tsem_bootstrap_copy's info2 reports the batch
 * used); if they do not fit at 1 the call is TSEM_ERR_NOMEM with the byte counts in the message.  Limits and refusals are
 * tsem_bootstrap's (TSEM_RA_CHOOSE, option "reproducible", a row-sharded handle, no model: TSEM_ERR_ARG with a message), and one
 * more: no group map set.  *nnz = the slots of P. */
int  tsem_bootstrap_groups(tsem_ctx* h, int32_t n_rep, uint64_t seed, const uint8_t* mult /* NULL | n_rep x N */, int32_t method,
                           double thresh, double epsilon, int32_t max_iter, int32_t keep_values, int64_t* nnz);
/* the last grouped call: groups, slots of P, replicates, good replicates, whether values were kept (any pointer may be NULL) */
int  tsem_bootstrap_groups_shape(tsem_ctx* h, int32_t* n_groups, int64_t* nnz, int32_t* n_rep, int32_t* n_used, int32_t* kept);
/* copy it out: group_ptr[n_groups + 1], cols[nnz], mean[nnz], sd[nnz], values[n_rep x nnz] (NULL, or the call kept them); any may be
 * NULL.  TSEM_ERR_ARG once tsem_set_groups was called again (the pattern belongs to the map). */
int  tsem_bootstrap_groups_copy(tsem_ctx* h, int64_t* group_ptr, int32_t* cols, double* mean, double* sd,
                                double* values /* n_rep x nnz, or NULL */);
/* the default multiplicities of replicate `rep` for the handle's rows [row_begin, row_end), computed on the device */
int  tsem_bootstrap_mult(tsem_ctx* h, uint64_t seed, int32_t rep, int64_t row_begin, int64_t row_end, uint8_t* out);

/* ---- single-cell mode: UMI duplicates (telescope_amd/csrc/tsem_umi.hip) ----
 * The copies of one molecule carry the same cell barcode and the same UMI.  cell_of_row[i] in [-1, n_cells) and umi_of_row[i] in
 * [-1, n_umis) are HOST arrays of the loaded matrix's N rows (-1: no barcode / no UMI); they are copied to the device and checked there.
 *   class           the rows with cell >= 0, umi >= 0 and equal (cell, umi)
 *   link            two rows of one class that both store an entry in the same column (whatever the scores; column ids in any order)
 *   component       a connected set of a class under the links (A-B, B-C: A and C belong together); a row in no class, and a row
 *                   without stored entries, is a component by itself
 *   representative  the row of a component whose largest stored raw score code is largest; the smallest row index among equals
 * rep_of_row[i] = the representative of i's component (row i is kept iff rep_of_row[i] == i), stats4 = { rows in classes, classes,
 * components among the rows in classes, rows dropped }.  Integer work: the result is the same whatever the launch order.
 * Needs only tsem_load_scores (no score table, no model) and changes nothing else the handle holds: parameters, z buffers, group map,
 * layout, per-cell fits and bootstrap results stay as they are (with option "drop_csr_indices" the column ids are rebuilt for the call).
 * The components settle in rounds driven by the host, at most as many as the longest class has rows; a call that would need more ends
 * with TSEM_ERR_TIMEOUT and a message (never seen: reported instead of going on).  Memory: up to 72 B per row and 32 B per stored entry of
 * the rows in multi-row classes plus the sort's storage, not tiled: TSEM_ERR_NOMEM with the byte counts in the message if that does not
 * fit.  TSEM_ERR_ARG with a message: a value out of range, a NULL pointer with N > 0, no matrix loaded, a handle with a communicator
 * attached (single GPU only, like tsem_group_counts).  N = 0 and "no row in any class" are valid calls. */
int  tsem_umi_dedup(tsem_ctx* h, const int32_t* cell_of_row, const int32_t* umi_of_row, int32_t n_cells, int32_t n_umis,
                    int32_t* rep_of_row /* N */, int64_t* stats4);

/* ---- device loader: BAM records to per-fragment (locus, alnscore, alnlen) lists (telescope_amd/csrc/tsem_bam.hip) ----
 * What telescope_amd/loader.py does between the inflated bytes of a BAM file and its list of mappings, per chunk of the byte stream.
 * A chunk begins on a record boundary; a record is an int32 block_size and block_size bytes behind it.  A BUNDLE is a run of records
 * with one query name (compared as the reader does: l_read_name and the l_read_name - 1 bytes in front of the terminator).
 *
 * tsem_bam_scan: HOST only, no device.  Walks the block_size chain of bytes[0, n_bytes): rec_off[i] = the offset of record i's size
 * field, for the *n_rec records that lie completely inside the chunk (at most `cap`; rec_off holds cap + 1 values), and
 * rec_off[*n_rec] = *consumed = the offset behind the last of them — the trailing partial record belongs to the next chunk.
 * TSEM_ERR_ARG with a message (tsem_last_error(NULL)): a block_size below 32 (the fixed fields; nothing behind it can be trusted),
 * a NULL pointer, a negative size. */
typedef struct tsem_bam tsem_bam;
#define TSEM_BAM_COLS 34
int  tsem_bam_scan(const uint8_t* bytes, int64_t n_bytes, int64_t* rec_off /* cap + 1 */, int64_t cap, int64_t* n_rec, int64_t* consumed);
/* The annotation, uploaded once per load, as loader.Annotation._sorted builds it: reference r of the BAM header (r in [0, n_ref)) owns
 * the intervals [ref_lo[r], ref_hi[r]) — an empty range for a reference the annotation does not have — and inside such a range
 *   starts[j]   the interval's first position, ascending, equal starts in the annotation's order
 *   maxend[j]   the running maximum of ends over the range up to j (so it ascends as well)
 *   ends[j]     one behind the interval's last position
 *   locus[j]    an id >= 0 of the interval's locus (the caller's numbering)
 *   strand[j]   0 '+', 1 '-', 2 anything else
 * All are HOST arrays and are checked on the host (ranges inside [0, n_intervals], starts and maxend ascending inside a range:
 * TSEM_ERR_ARG with a message otherwise) before the device is touched; TSEM_ERR_HIP / TSEM_ERR_NOMEM if the device refuses.
 * `device` is a device index, as for tsem_csr_*: no matrix and no tsem_ctx exist yet.  Errors: tsem_last_error(NULL). */
int  tsem_bam_open(tsem_bam** out, int device, int32_t n_ref, const int32_t* ref_lo, const int32_t* ref_hi, int64_t n_intervals,
                   const int64_t* starts, const int64_t* maxend, const int64_t* ends, const int32_t* locus, const int8_t* strand);
int  tsem_bam_close(tsem_bam* b);                      /* NULL is fine */
/* One chunk through k_bam_decode, k_bam_pair, k_bam_overlap, k_bam_fragment.  bytes / rec_off / n_rec: as tsem_bam_scan left them
 * (HOST arrays; checked on the host before the copy: offsets inside the chunk, every record 36 .. 2^31 - 1 bytes, fewer than 2^31 - 1
 * records — TSEM_ERR_ARG otherwise, so that no kernel sees offsets it cannot trust); the chunk must end on a bundle boundary, the
 * first record starts a bundle.  barcode_tag / umi_tag: the Z tag's two letters as first | second << 8, or -1.  run_stranded: apply the
 * strand filter; first_f / last_f: stranded_mode[0] == 'F' / stranded_mode[-1] == 'F'.  record_cap >= 1: a longer bundle is left to
 * the host.  out: int32 [TSEM_BAM_COLS][n_rec], row c at out + c * n_rec; i = a record's index in the chunk, s = the index of a
 * bundle's first record:
 *    0-15  per record i: ref_id, pos, next_ref, next_pos, |tlen| (uint32 bits), flag, l_read_name, n_cigar, l_seq, AS, bits (1: AS
 *          present, 2: the name differs from record i - 1's, i.e. i starts a bundle, 4: a value only the host reproduces), offset
 *          (from the record's size field) and length of the barcode tag's value and of the UMI tag's (-1, -1: none; the last such
 *          tag counts), status (0, or the code below)
 *   16-18  per record slot: r1 and r2 (record indices, r2 -1: none) of the bundle's k-th alignment pair at slot s + k (-1: no pair at
 *          this slot), in the order of loader._fragments; s itself
 *   19-21  per pair slot: the pair's locus (-1: none, i.e. `__no_feature`; -2: r1 unmapped; -3: not computed), alnscore, alnlen
 *   22-24  per map slot: locus, alnscore, alnlen of the bundle's k-th mapping at slot s + k, in the loader's order
 *   25-32  per bundle, at s: code (0 SU 1 SM 2 PU 3 PM 4 PX), pairs, mappings, class (0 unmapped 1 nofeat_U 2 nofeat_A 3 feat_U
 *          4 feat_A 5 left to the host), minimum and maximum alnscore over its mapped pairs, how many those are, flags (1: host)
 *      33  scratch
 * A bundle of class 5 has no valid pairs or mappings: the caller runs the host loader on its bytes.  status2[0] = 0, or the code of
 * the first record in file order that cannot be decoded, status2[1] = that record: 1 block_size against rec_off, 2 l_read_name,
 * 3 n_cigar past the record, 4 l_seq past the record, 5 an aux field's head past the record, 6 an aux value past the record, 7 a Z / H
 * value without NUL inside the record, 8 a B array past the record (or a negative count, an unknown element type), 9 an unknown aux
 * type, 10 a mapped alignment without AS.  The call itself then still returns TSEM_OK, and `out` is not to be used.  TSEM_ERR_HIP /
 * TSEM_ERR_NOMEM with a message (tsem_last_error(NULL)) if a copy, a launch or an allocation fails.  The handle keeps its device
 * buffers between calls and grows them as needed: 1 B per chunk byte and 144 B per record. */
int  tsem_bam_chunk(tsem_bam* b, const uint8_t* bytes, int64_t n_bytes, const int64_t* rec_off, int64_t n_rec, int32_t barcode_tag,
                    int32_t umi_tag, int32_t run_stranded, int32_t first_f, int32_t last_f, double overlap_threshold,
                    int32_t record_cap, int32_t* out, int64_t* status2);
/* HIP-event milliseconds summed over the calls so far: host-to-device, k_bam_decode, k_bam_pair, k_bam_overlap, k_bam_fragment,
 * device-to-host; *calls = how many; reset != 0 clears both. */
int  tsem_bam_times(tsem_bam* b, int reset, double* ms6, int64_t* calls);
/* ---- the BAMs of --updated_sam from records rewritten on the device (telescope_amd/csrc/tsem_bam_edit.h) ----
 * A rewritten record keeps every byte but its block_size, flag, MAPQ and the aux fields that are replaced: those are removed wherever
 * they stand and whatever their type, the new ones are appended (bam_out.set_tag).  Streams are FRAMED records (block_size and body),
 * ready for a BGZF writer.  An output SLOT is a record index of the chunk: a bundle writes into the slots of its own records, in
 * the order of loader._fragments' pairs, r1 then r2, and never more records than it holds.
 *
 * tsem_bam_names: the names the load stage writes, uploaded once per load: name j = bytes[off[j], off[j + 1]) for the locus of id j
 * (the ids of tsem_bam_open's `locus`), the last one (j = n_names - 1) the no_feature_key.  HOST arrays, checked on the host:
 * TSEM_ERR_ARG with a message when off[0] != 0, the offsets descend, or the annotation holds a locus id >= n_names - 1.
 * Device memory: the bytes and 8 B per name. */
int  tsem_bam_names(tsem_bam* b, const uint8_t* bytes, const int64_t* off /* n_names + 1 */, int32_t n_names);
/* Load stage, sizing: k_bam_rw_plan, k_bam_rw_size and an exclusive scan per stream over the chunk the last tsem_bam_chunk left on the
 * device (it must have returned status 0; TSEM_ERR_ARG otherwise, or without names).  Bundles of class 0 send their first pair's
 * records to `other`, of class 1 / 2 every pair's, unchanged; of class 3 / 4 every pair's to `tmp`: an unmapped pair unchanged, a
 * mapped one without its ZF / ZT / ZB and with ZF:Z:<locus name | no_feature_key>, ZT:Z:PRI (the first pair of its locus, in pair
 * order, that reaches the locus's largest alnscore + alnlen) or SEC, ZB:Z:<the names of the bundle's mappings whose alnscore is the
 * first mapping's, comma-joined> appended.  A bundle of class 5 writes nothing: the caller splices its records in.
 * pos_other / pos_tmp (int64 [n_rec + 1], HOST): slot i writes [pos[i], pos[i + 1]) of the stream; pos[n_rec] = the stream's length; at
 * a bundle's first slot: where the bundle's bytes begin.  status2 as for tsem_bam_chunk (a record the aux walk cannot follow; the
 * streams are then not to be fetched).  Device memory: 32 B per record on top of tsem_bam_chunk's. */
int  tsem_bam_rewrite_size(tsem_bam* b, int64_t* pos_other, int64_t* pos_tmp, int64_t* status2);
/* Update stage, sizing: a chunk of the tmp BAM's records (bytes / rec_off / n_rec as for tsem_bam_chunk, checked the same way on the
 * host before the copy) and one word per record: bits 30-31 the kind, 0 unchanged, 1 SEC (flag |= 0x100, MAPQ 0, YC:Z:248,248,248
 * replaces every YC), 2 PRI (bits 0-17 the tsem_entry_tags word of the pair's entry: MAPQ, XP:C and YC replace every XP / YC, 0x100
 * cleared when assigned and set otherwise) — bam_out.update_pair.  Every record is walked again, the file having been re-read:
 * status2 = (code, record) of the first one that cannot be, with the codes of tsem_bam_chunk (and 9 for a kind of 3).
 * pos (int64 [n_rec + 1], HOST): record i becomes [pos[i], pos[i + 1]) of the updated stream.  Needs no annotation (a handle opened
 * with n_ref = 0 will do) and no names.  Device memory: 1 B per chunk byte, 44 B per record. */
int  tsem_bam_update_size(tsem_bam* b, const uint8_t* bytes, int64_t n_bytes, const int64_t* rec_off, int64_t n_rec, const uint32_t* words,
                          int64_t* pos /* n_rec + 1 */, int64_t* status2);
/* Between a sizing call and its fetch: per slot the kind (0 nothing, 1 other, 2 tmp unchanged, 3 tmp PRI, 4 tmp SEC, 5 update stage)
 * and the pair slot (-1: none) — what the caller's table for the update stage is made from.  n = the sizing call's record count. */
int  tsem_bam_rewrite_slots(tsem_bam* b, int32_t* kind /* n */, int32_t* pair /* n */, int64_t n);
/* k_bam_rw_write for the last sizing call (status 0) and the streams to the host.  n_other / n_tmp must be that call's stream lengths
 * (the update stage: other = NULL, 0; tmp = the updated stream), TSEM_ERR_ARG otherwise; one fetch per sizing call.  Device memory:
 * 1 B per output byte. */
int  tsem_bam_rewrite_fetch(tsem_bam* b, uint8_t* other, int64_t n_other, uint8_t* tmp, int64_t n_tmp);
/* HIP-event milliseconds of the rewriting, summed: host-to-device (the update stage's chunk), k_bam_rw_plan, the size kernel with its
 * scans, k_bam_rw_write, device-to-host; *calls = sizing calls; reset != 0 clears both. */
int  tsem_bam_rewrite_times(tsem_bam* b, int reset, double* ms5, int64_t* calls);

/* ---- device loader: a BAM that is not name-collated (`--collate`; telescope_amd/csrc/tsem_bam_collate.hip, tsem_bam_collate.h) ----
 * tsem_bam_chunk wants every alignment of a query name in one run of records.  tsem_bam_collate brings the records of a whole stream
 * into that order.  bytes / rec_off / n_rec: the record part of an inflated BAM as tsem_bam_scan leaves it (HOST arrays; rec_off holds
 * n_rec + 1 offsets).  A record's NAME is the l_read_name bytes at offset 36 of the framed record (its block_size included), the
 * trailing NUL among them, compared as bytes; a GROUP is the set of records with equal names.  out[0, rec_off[n_rec] - rec_off[0]) gets
 * the same framed records, byte for byte: the groups in the order of their first records, the records of a group in their input order.
 * order[k] = the input index of output record k, *n_names = the number of groups.  A stream that is collated already comes back
 * unchanged; the result depends on nothing but the input.
 * status2[0] = 0, or why the first record in input order that cannot be collated was refused, status2[1] = that record: 1 shorter than
 * the 32 fixed bytes and one byte of a name, 2 l_read_name is 0, 3 the name runs past the record's end.  The call then still returns
 * TSEM_OK, and out / order / n_names are not to be used; no byte outside a record is read to find that out.
 * hash_bits: 0, or (tests) so many bits of the names' 64-bit hash are kept: distinct names then share hash values and probe chains.
 * On the device: k_collate_hash, k_collate_insert (open addressing in a table of the next power of two >= 2 n_rec slots),
 * k_collate_key, rocprim's radix sort and scan, k_collate_gather.  ms (5 values, or NULL): HIP-event milliseconds of host-to-device,
 * hash + insert + key, sort + scan, gather, device-to-host.  Device memory: twice the bytes and 44 to 60 B per record, all of it
 * released when the call returns; TSEM_ERR_NOMEM with a message (tsem_last_error(NULL)) and nothing left allocated when that does not
 * fit.  TSEM_ERR_ARG with a message, before the device is touched: a NULL pointer, a negative size, n_rec >= 2^32 - 1, hash_bits
 * outside 0 .. 64, offsets that descend or leave [0, n_bytes].  n_rec = 0 is a valid call.  TSEM_ERR_HIP if a copy or a launch fails.
 * tsem_bam_collate_host: the same contract and the same bodies on one CPU thread, no device; it gives the bytes and the order that the
 * kernels give. */
int  tsem_bam_collate(int device, const uint8_t* bytes, int64_t n_bytes, const int64_t* rec_off, int64_t n_rec, int32_t hash_bits,
                      uint8_t* out /* n_bytes */, int64_t* order /* n_rec */, int64_t* n_names, int64_t* status2, double* ms /* 5 */);
int  tsem_bam_collate_host(const uint8_t* bytes, int64_t n_bytes, const int64_t* rec_off, int64_t n_rec, int32_t hash_bits,
                           uint8_t* out /* n_bytes */, int64_t* order /* n_rec */, int64_t* n_names, int64_t* status2);

/* ---- device loader: the BGZF blocks of a BAM file inflated on the device (telescope_amd/csrc/tsem_bgzf.hip) ----
 * A BGZF file is a chain of gzip members ("blocks") of at most 64 KiB compressed and 64 KiB inflated bytes; each needs nothing from
 * its neighbours and carries the CRC-32 and the length (ISIZE) of its inflated bytes in its trailer.
 *
 * tsem_bgzf_scan: HOST only, no device.  Walks the chain of block headers of bytes[0, n_bytes), which begins on a block boundary.  A
 * header is 1f 8b 08 04 with the subfield 'B' 'C' (SLEN 2: the block's size - 1) among its extra fields, in any position.  Row k of
 * `blocks` (int64 [cap][5]) = { the block's offset, its payload's offset, the payload's length, ISIZE, CRC-32 } for the *n_blocks
 * blocks that lie completely inside the bytes (at most `cap`); *consumed = the offset behind the last of them — a trailing partial
 * block, header or payload or trailer, belongs to the next call.  *not_bgzf = 1 (and nothing consumed) when the first bytes are no BGZF
 * header: another magic, or a gzip header without the BC subfield, as plain gzip writes it.  TSEM_ERR_ARG with a message
 * (tsem_last_error(NULL)): such bytes behind the first block, a BSIZE smaller than header plus trailer, a NULL pointer, a negative size. */
typedef struct tsem_bgzf tsem_bgzf;
int  tsem_bgzf_scan(const uint8_t* bytes, int64_t n_bytes, int64_t* blocks /* cap x 5 */, int64_t cap, int64_t* n_blocks,
                    int64_t* consumed, int32_t* not_bgzf);
/* A handle on device `device` (an index, as for tsem_bam_open); it keeps its device buffers from call to call and grows them when a
 * batch is larger: 1 B per compressed and per inflated byte, 36 B per block.  Errors: tsem_last_error(NULL). */
int  tsem_bgzf_open(tsem_bgzf** out, int device);
int  tsem_bgzf_close(tsem_bgzf* z);                    /* NULL is fine */
/* One batch through k_bgzf_inflate (one wave per block).  bytes / blocks / n_blocks: as tsem_bgzf_scan left them (HOST arrays).  Block k
 * inflates into out[o_k, o_k + ISIZE_k), o_k = the sum of the ISIZEs of the blocks in front of it; *out_bytes = their total.  A block
 * whose ISIZE exceeds 65,536 (the format forbids it, a gzip member can claim it) takes no range and is not inflated: status 255, the
 * caller inflates it on the host.  status[k]: 0, 255, or
 *    1 block type 3                       2 stored block: LEN does not match NLEN     3 over-subscribed or incomplete code set
 *    4 no code for end-of-block           5 invalid symbol (286, 287, distance 30, 31) 6 distance before the start of the output
 *    7 output longer than ISIZE           8 input exhausted                           9 output shorter than ISIZE
 *   10 CRC-32 mismatch
 * first2[0] = 0, or the code of the first block in file order with a code in 1 .. 10, first2[1] = that block (else -1); the other
 * blocks' bytes are valid all the same.  The call itself then still returns TSEM_OK.  Checked on the host before the device is
 * touched, TSEM_ERR_ARG with a message: a NULL pointer, a negative size, 2^31 - 1 blocks or more, a payload range outside [0, n_bytes)
 * or longer than 65,536, an ISIZE or CRC-32 outside 32 bits, a total of the ISIZEs above out_cap, a NULL handle — so no kernel sees a
 * range it cannot trust.  TSEM_ERR_HIP / TSEM_ERR_NOMEM with a message if a copy, the launch or an allocation fails. */
int  tsem_bgzf_inflate(tsem_bgzf* z, const uint8_t* bytes, int64_t n_bytes, const int64_t* blocks /* n_blocks x 5 */, int64_t n_blocks,
                       uint8_t* out, int64_t out_cap, int32_t* status /* n_blocks */, int64_t* first2, int64_t* out_bytes);
/* HIP-event milliseconds summed over the calls so far: host-to-device, k_bgzf_inflate, device-to-host; *calls = how many; reset != 0
 * clears both. */
int  tsem_bgzf_times(tsem_bgzf* z, int reset, double* ms3, int64_t* calls);
/* The other direction (`--deflate device`): bytes[0, n_bytes), a HOST stream that begins on a block boundary, becomes the BGZF blocks
 * of a file, one behind the other in out[0, *out_bytes): the stream is cut every 0xff00 bytes (the last block may be shorter; n_bytes
 * = 0 gives no block), every block is 18 header bytes (1f 8b 08 04, MTIME 0, XFL 0, OS ff, XLEN 6, 'B' 'C' 2 0, BSIZE - 1), a raw
 * DEFLATE stream of at most len + 5 bytes, CRC-32 and ISIZE.  *n_blocks = how many.  The EOF block is NOT written: that is the file
 * writer's business.  One upload (the stream) and one download (the finished image; its size, 8 bytes, travels ahead of it); in
 * between k_bgzf_deflate (one wave per block: hash-table LZ77, greedy parse, the smaller of a stored, a fixed and a dynamic block;
 * telescope_amd/csrc/tsem_bgzf_deflate.h), k_bgzf_offsets and k_bgzf_pack.  The handle keeps 1 B per stream byte, 2 B per byte for
 * the slots and the image and 4 B per byte for the tokens.  Checked before the handle is looked at, TSEM_ERR_ARG with a message: a
 * NULL pointer, a negative size, 2^31 - 1 blocks or more, out_cap below the worst case n_bytes + 31 per block (a stored block: 5 bytes
 * of DEFLATE framing, 26 of BGZF); then a NULL handle.  TSEM_ERR_HIP / TSEM_ERR_NOMEM as for tsem_bgzf_inflate.
 * tsem_bgzf_deflate_host: the same contract and the same body with one lane on the CPU, no device and no handle; it gives the bytes
 * that the kernel gives (the body's result does not depend on the number of lanes). */
int  tsem_bgzf_deflate(tsem_bgzf* z, const uint8_t* bytes, int64_t n_bytes, uint8_t* out, int64_t out_cap, int64_t* out_bytes,
                       int64_t* n_blocks);
int  tsem_bgzf_deflate_host(const uint8_t* bytes, int64_t n_bytes, uint8_t* out, int64_t out_cap, int64_t* out_bytes, int64_t* n_blocks);
/* HIP-event milliseconds summed over the tsem_bgzf_deflate calls so far: host-to-device, k_bgzf_deflate, k_bgzf_offsets + k_bgzf_pack,
 * device-to-host; *calls = how many; reset != 0 clears both.  tsem_bgzf_times is not touched by them. */
int  tsem_bgzf_deflate_times(tsem_bgzf* z, int reset, double* ms4, int64_t* calls);

/* ---- csr_matrix_plus primitives on arbitrary fp64 CSR (sparse_plus.py) ---- */
/* All three: indptr[n_rows + 1] is a HOST array and is checked on the host before the device is touched. TSEM_ERR_ARG (text in
 * tsem_last_error(NULL)) for n_rows < 0, n_cols < 0, indptr NULL, indptr[0] != 0, any indptr[i + 1] < indptr[i], or data / out
 * NULL with indptr[n_rows] > 0: with or without a GPU, and no kernel ever sees such row pointers.  data and out hold
 * indptr[n_rows] values.  A failed launch or copy is TSEM_ERR_HIP; out is then not to be read. */
/* norm(1) :46-52: out = data * recip0(row sum); a NaN in a row makes the row NaN, as in scipy. */
int  tsem_csr_norm_rows(int device, int64_t n_rows, const int64_t* indptr,
                        const double* data, double* out);
/* binmax(1) :117-129: out = 1 where data equals the row maximum, else 0.  The maximum is numpy's: a row with fewer than n_cols
 * entries includes an implicit 0, and a row that holds a NaN has the maximum NaN and marks nothing. */
int  tsem_csr_binmax_rows(int device, int64_t n_rows, int32_t n_cols, const int64_t* indptr,
                          const double* data, int8_t* out);
/* mode 0: norm() :47-48   mode 1: scale() :94-95   mode 2: scale(1) :96-97; any other mode is TSEM_ERR_ARG.  The maxima of modes 1
 * and 2 are numpy's, as above: an implicit 0 where the matrix (1) or the row (2) is not full, and NaN once a NaN is seen, so
 * that the whole matrix (1) or row (2) comes out NaN. */
int  tsem_csr_scale(int device, int mode, int64_t n_rows, int32_t n_cols, const int64_t* indptr,
                    const double* data, double* out);

/* ---- instrumentation ------------------------------------------------------ */
/* HIP-event time (ms) and number of TIMED launches of the dominant EM kernel(s) since the
 * last call with reset=1 (option "kernel_timing" = n times every n-th pass, 0 none; default 1);
 * algorithmic bytes one EM pass reads, as stored: per entry 6 (score codes), 11 (fp64 values behind the 3-byte index) or 12, plus
 * 2 per row.  */
int  tsem_kernel_stats(tsem_ctx* h, int reset, double* em_ms, int64_t* em_launches,
                       int64_t* algo_bytes_per_pass);
/* The last tsem_report_colsums of the handle: HIP-event time (ms) of its dominant kernel — the pass over the stored entries — when
 * option "kernel_timing" is not 0 (else 0), the algorithmic bytes that pass reads and writes (4 B per stored entry: popularity id +
 * score code; 8 B row pointer + 4 B output per row), the rows it left to the exact row kernel (too long, tied, near-tied, on the
 * threshold), and which kernel it was: 0 none yet, 1 generic row pass, 2 capacity kernel (k_report_rows), 3 score codes only
 * (k_report_init_codes), 4 packed fp32 filter (k_report_pack32).  model.py:432-457 is what the pass computes. */
int  tsem_report_stats(tsem_ctx* h, double* kernel_ms, int64_t* algo_bytes, int64_t* deferred_rows, int32_t* kernel);
/* Which kernel INSTANCE served the last tsem_report_colsums (values [0 .. 16)) and the last tsem_reassign_groups ([16 .. 32)): the
 * first min(n, TSEM_REPORT_INFO_N) values (the Python binding names them: _lib.Engine.report_info).  Read-only: the report calls
 * note host values next to their launches and gain no copy, synchronisation or kernel; this query counts the deferred rows from the
 * list the launch left on the device and synchronises the handle's stream.  Per half:
 *   [0] kernel family, the codes of tsem_report_stats (0 none yet .. 4 k_report_pack32), and 5: k_group_unique (per-group `unique`);
 *   [1] lanes per row G and [2] entries per lane E of the instance (k_report_pack32: 64, the most lanes a row takes; the generic row
 *       pass: 16 and 0);  [3] 1 the initial z, 0 the model's;  [4] group mode (0 column sums, 1 exclude, 2 average, 3 conf, 4 all);
 *   [5] COLD of k_report_pack32 (its table of the ids does not fit LDS: [7] < the number of ids);
 *   [6] Hs, the ids with accumulator slots in LDS;  [7] HC, the ids whose pi*theta sits in LDS;  [8] lut_rep (log2 of the copies of the
 *       score table in LDS);  [9] grid and [10] block of the launch;
 *   [11] rows left to k_report_slow because they are longer than G * E entries, [12] rows left to it as near-ties (k_report_pack32:
 *       everything else its filter did not decide — ties, near-ties, rows on the threshold); both -1 where there is no such list
 *       (family 1 and 5) or the other of the two calls has reused it since.  Of a tsem_reassign_groups they are those of its LAST tile;
 *   [13] tiles of the last tsem_reassign_groups and [14] groups in its last tile (0 in the first half);  [15] 0. */
#define TSEM_REPORT_INFO_N 32
int  tsem_report_info_n(tsem_ctx* h, int64_t* info, int32_t n);
/* Option "phase_timing" = 1: tsem_em_chunk records a HIP event at every phase boundary of every iteration it enqueues (a
 * diagnostic: ~5 events per iteration on the engine's stream).  ms6 = summed milliseconds over *n_iter iterations of
 * { EM pass | column reduce | all-reduce of the K+2 sums (0 without a communicator) | update | gap to the next iteration's
 * pass | first mark to last mark }.  What bench.py prints as `phase_us`. */
int  tsem_phase_times(tsem_ctx* h, int reset, double* ms6, int64_t* n_iter);
/* Free / total bytes of the device's memory (hipMemGetInfo; h may be NULL, then `device` is asked) and, with a handle, the bytes its
 * matrix keeps resident: resident5 = { CSR row pointers + scores | CSR column ids (0 after option "drop_csr_indices") | popularity
 * ids | blocked layout (its index at 2, 3 or 4 B per padded entry, see tsem_layout_info_n [32]) | per-row arrays }.  What a capacity plan needs: 14 B per stored entry by default (score codes), 10 after
 * the drop, + ~20 B per row. */
int  tsem_device_memory(tsem_ctx* h, int device, int64_t* free_bytes, int64_t* total_bytes, int64_t* resident5);
/* Facts about the resident layout, 32 values (the Python binding names them: _lib.Engine.layout_info).  Of the later ones: [23] the
 * EM pass carries the previous iteration's lnl; [24] split layout; [26] plain CSR row passes; [27] entries of the lnl pass's log Q
 * table (0: none), [28] log Q is arithmetic (no table); [29] stored entries that k_log_tab counted for the exact branch of the log
 * form before the LAST lnl pass (-1: no choice armed) and [30] the count above which the per-entry logarithm runs instead — reading
 * [29] synchronises the handle's stream; [31] rows whose row sum the report / row passes recomputed in the reference's own order of
 * additions (scipy's `sum(axis=1)` = np.add.reduceat: a0 + pairwise(a1 ..)) since the matrix was loaded — the rows where two z values,
 * or a z value and conf_prob, are closer than the rounding of 1 / rowsum could decide (sparse_plus.py:99-129 compares with `==`). */
int  tsem_layout_info(tsem_ctx* h, int64_t* info32);
/* The same with the caller's buffer length: the first min(n, TSEM_LAYOUT_INFO_N) values.  Appended behind the 32 above: [32] bytes of
 * index per stored entry of the blocked layout — 3 where the fused kernel reads fp64 entries of a non-split layout (a 13-bit column
 * slot and an 11-bit row slot per entry, four entries in 12 bytes), 4 (local row << 16 | local column) everywhere else; [33]-[36] the
 * cells the last tsem_cell_em fitted per kernel class — a wave per cell | 256 threads | 512 threads, tables in LDS | 512 threads,
 * tables in a global workspace — all 0 before a fit; [37] the groups the last tsem_cell_em spread over the grid (option
 * "cell_em_spread_entries"): a spread group is counted here and in none of [33]-[36]; [38], [39] the lanes per row (1, 2, 4, 8 or
 * 16, sixteen entries per lane) of the last tsem_rowstats's row-statistics and column-signature kernels — from the mean row length,
 * and from the row-length histogram (the smallest group that takes 99.5 % of the rows in one step) —, 0 before one ran; [40] the
 * index format of the blocked layout (0: one 32-bit word per entry, 1: three bytes per entry, 2: the quad index — one 64-bit word per
 * four entries of a row-ordered sub-block, [32] == 2; option "index_format" 0 auto / 1 / 2); [41] the dummy entries (column slot 0,
 * value 0) a quad layout stores so that every row of a block has an entry in every part: counted in nnz_pad, not in nnz_amb; [42] the
 * quads the pack kernel could not represent (0 by construction: anything else is a fault of the set-up, and the layout then keeps the
 * 3-byte index); [43] option "index_auto_min_bytes": the smallest 3-byte stream (11 B x nnz_amb) for which auto takes the quad
 * index (default 1 GiB); [44] the conflict-aware entry order the layout got (0 none, 1 the walk over the rows of a score-code layout,
 * 2 the order inside the quads of fp64 entries) and [45] the quads the latter permuted. */
#define TSEM_LAYOUT_INFO_N 46
int  tsem_layout_info_n(tsem_ctx* h, int64_t* info, int32_t n);
/* per-block shader-clock stamps of team 0 / member 0 of the fused kernel (option "fused_prof") */
int  tsem_debug_fused_prof(tsem_ctx* h, uint64_t* out512);
/* the same option's start-up timeline: per workgroup b (up to 512), out[8 b ..] = 100 MHz wall clock at entry / tickets counted /
 * LDS zeroed / tables loaded / loop start / loop end / exit, and (team << 32 | member << 16 | blocks) */
int  tsem_debug_fused_startup(tsem_ctx* h, uint64_t* out4096);
/* the local row << 16 | local column words of one sub-block of the blocked layout (layout studies); a layout that stores the 3-byte
 * index (tsem_layout_info_n [32] == 3) is decoded on the host: the same words either way */
int64_t tsem_debug_subblock(tsem_ctx* h, int64_t block, int32_t part, uint32_t* out, int64_t cap);
/* the fp64 values of the same sub-block in the same (entry) order: out[e] belongs to word e of tsem_debug_subblock, wherever the layout
 * keeps it (a layout the fused kernel reads groups a sub-block's values by wave; the host applies the map the fill kernels used).
 * rows / cols (each may be null): the CSR row and the column that word e names (-1: an empty row slot; every slot of a hot column names it); the
 * padding of a sub-block has value 0.  TSEM_ERR_ARG on a layout of score codes; returns the number of values */
int64_t tsem_debug_subblock_values(tsem_ctx* h, int64_t block, int32_t part, double* out, int32_t* rows, int32_t* cols, int64_t cap);
/* host only, no device: pos[e] = the index (in doubles from the sub-block's first value) at which a layout read by the fused kernel
 * keeps the value of entry e of a sub-block of nq quads (nq a multiple of 16), e = 0 .. 4 nq - 1, by the inline function the fill
 * kernels and the read-back use */
int  tsem_debug_valmap(int32_t nq, uint32_t* pos);
/* host only, no device: four local row << 16 | local column words (rows < 2048, columns < 8192; TSEM_ERR_ARG otherwise) packed into
 * the 12 bytes of a quad of the 3-byte index — entry k is the 24-bit little-endian number row << 13 | column at bytes 3k .. 3k+2 —
 * and unpacked again into back4, both with the inline functions the fill kernels and the fused kernel use */
int  tsem_debug_idx24(const uint32_t* rc4, uint8_t* out12, uint32_t* back4);
/* host only, no device: four local row << 16 | local column words packed into the 64-bit word of the quad index — 13-bit column slots
 * at bits 0, 13, 26 and 39, the steps row[k] - row[k-1] (0 or 1) at bits 52-54, the first entry's row slot at bits 55-63 — and unpacked
 * again into back4, with the inline functions the pack kernel and the fused kernel use; TSEM_ERR_ARG for a quad the format cannot hold.
 * *stored (may be null): 1 when `probe` names a stored quad, 0 when its low half is the fused kernel's idle mark 0xFFFFFFFF */
int  tsem_debug_quad64(const uint32_t* rc4, uint64_t* word, uint32_t* back4, uint64_t probe, int32_t* stored);
/* host only, no device: one cell of the table of fused-kernel instantiations — team size P, kernel mode, entry format (0 fp64, 1 score
 * codes, 2 fp64 with the score table in LDS), geometry, timeline kernel (0 / 1), index format read (layout_info 'index_format': 0, 1, 2).
 * *found: 1 when the library's look-up returns a kernel for the cell; *listed: 1 when the table's predicate lists it.  The two agree. */
int  tsem_debug_fused_cell(int32_t P, int32_t mode, int32_t fmt, int32_t geo, int32_t prof, int32_t ix, int32_t* found, int32_t* listed);
/* host only: the fused kernel's dynamic LDS for one cell of that table and the sizes (Kp, R, lut_len, lq_n, lq_lin) — regions[26]: byte
 * offset and bytes of each of its 13 regions (may be null), *kernel_end where the last ends — and for a layout of these flags (1 split,
 * 2 exact_single, 4 lnl3, 8 reproducible, 16 score table in LDS): *launch_bytes the dynamic LDS the cell is launched with, *rmax the
 * most row slots per block the set-up chooses, *room the bytes left for the log-Q table */
int  tsem_debug_fused_lds(int32_t P, int32_t mode, int32_t fmt, int32_t geo, int32_t prof, int32_t ix, int32_t Kp, int32_t R, int32_t lut_len,
                          int32_t lq_n, int32_t lq_lin, int32_t flags, int32_t* regions, int32_t* kernel_end, int32_t* launch_bytes,
                          int32_t* rmax, int32_t* room);
/* host only, nothing on the device: the launch census of a handle.  Every launch of the fused kernel is counted under the cell it was
 * looked up by — the six values above, in the order team size 1..8 x mode 0..9 x entry format 0..2 x geometry 0..3 x timeline x index
 * format, row-major: 5760 cells.  out[2 c]: launches that run unconditionally; out[2 c + 1]: launches enqueued with the device's
 * choice between the two forms of the lnl pass armed (which of the two did the work the host cannot know).  cap: int64 slots of
 * `out`, at least 11520 (TSEM_ERR_ARG otherwise).  tsem_debug_fused_launches_clear zeroes the counters. */
int  tsem_debug_fused_launches(tsem_ctx* h, int64_t* out, int64_t cap);
int  tsem_debug_fused_launches_clear(tsem_ctx* h);
/* host only: the position c of a cell in that order, -1 outside the enumerated ranges (not an error code) */
int  tsem_debug_fused_census_index(int32_t P, int32_t mode, int32_t fmt, int32_t geo, int32_t prof, int32_t ix);
/* host only, no device: the conflict-aware order inside quads (option "deconflict" on fp64 entries) applied to n_win windows of 64
 * consecutive local row << 16 | local column words: codes[16 w + l] is the permutation of quad l of window w — entry (code >> 2 j) & 3
 * of the quad goes to position j, 0xE4 is the identity —, *moved (may be null) the quads that change; by the inline functions the
 * set-up kernel uses */
int  tsem_quad_order_host(int64_t n_win, const uint32_t* rc, uint8_t* codes, int64_t* moved);
/* y[i] = the device log1p the lnl passes use (finite x >= 0), for accuracy tests against libm */
int  tsem_debug_log1p(int device, int32_t n, const double* x, double* y);
/* out[i] = the PHRED lookup of tsem_entry_tags for p[i] (the table as there), for tests against numpy */
int  tsem_debug_phred(int device, int32_t n, const double* p, const double* phred_tab, int32_t n_tab, int32_t* out);
/* GB/s of a pure streaming read (16-byte non-temporal loads, 8 in flight per thread) over a scratch buffer of `bytes`,
 * best of `reps` launches: the measured-stream peak quoted beside the nominal HBM peak */
int  tsem_debug_stream_read(int device, int64_t bytes, int32_t reps, double* gbs);
/* the same for the table-driven log1p of the fused lnl pass (64-entry table in LDS, ~1e-16 absolute error per evaluation) */
int  tsem_debug_log1p_tab(int device, int32_t n, const double* x, double* y);
/* ... and of the log-table form of the lnl passes (round 5): log1p(q c) from lq = log q and lc = log c — L + exp(-L) for
 * L = lq + lc >= 18.715, 0 below -40, the table-driven log1p of the exact product q * c between */
int  tsem_debug_log1p_of_log(int device, int32_t n, const double* lq, const double* lc, const double* q, const double* c, double* y);

#ifdef __cplusplus
}
#endif
#endif /* TELESCOPE_EM_H */
