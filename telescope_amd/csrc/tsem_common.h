// Shared declarations for libtelescope_em.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <cmath>
#include <string>
#include <vector>

#include <rccl/rccl.h>   // types and enum values only: the library is resolved at run time (nccl_api, tsem.hip), never linked

#include "telescope_em.h"
#include "tsem_index.h"

#define TSEM_HIP(call)                                                           \
  do {                                                                           \
    hipError_t e_ = (call);                                                      \
    if (e_ != hipSuccess) {                                                      \
      h->err = std::string(#call) + ": " + hipGetErrorString(e_) + " (" +        \
               __FILE__ + ":" + std::to_string(__LINE__) + ")";                  \
      return TSEM_ERR_HIP;                                                       \
    }                                                                            \
  } while (0)

#define TSEM_FAIL(code, msg)                                                     \
  do {                                                                           \
    h->err = (msg);                                                              \
    return (code);                                                               \
  } while (0)

// ---- counter-based hash shared with telescope_amd/synthetic.py --------------
#define TS_GOLDEN 0x9E3779B97F4A7C15ull
#define TS_M1 0xBF58476D1CE4E5B9ull
#define TS_M2 0x94D049BB133111EBull
#define TS_SALT_LEN 0xA5A5A5A5A5A5A5A5ull
#define TS_SALT_UNIQ 0x5BD1E9955BD1E995ull
#define TS_SALT_COL0 0xC2B2AE3D27D4EB4Full
#define TS_SALT_SCORE 0x165667B19E3779F9ull
#define TS_SALT_FAM 0x27D4EB2F165667C5ull
#define TS_SALT_BOOT 0x94D049BB133111EBull   /* bootstrap multiplicities (tsem_boot.hip, synthetic.bootstrap_multiplicities) */
#define TS_FAMILY 256                 /* loci per family of the synthetic distribution 2 ('family', telescope_amd/synthetic.py) */

__host__ __device__ inline uint64_t ts_mix64(uint64_t z) {
  z += TS_GOLDEN;
  z = (z ^ (z >> 30)) * TS_M1;
  z = (z ^ (z >> 27)) * TS_M2;
  return z ^ (z >> 31);
}
__host__ __device__ inline uint64_t ts_hash3(uint64_t seed, uint64_t row, uint64_t k) {
  return ts_mix64(ts_mix64(seed ^ (row * TS_GOLDEN)) ^ (k * TS_M1));
}

// LDS budget for the per-part tables (c and acc, 8 B each per column).
constexpr int TS_LDS_TABLE_BYTES = 120 * 1024;
constexpr int TS_MAX_KP = TS_LDS_TABLE_BYTES / 16;   // 7680 columns per part
constexpr int TS_MAX_KP_LNL = 5120;                  // ... when a part keeps pi*theta of TWO parameter sets and the accumulators (option "use_likelihood")
constexpr int TS_MAX_KP3 = 4800;                     // ... when a part keeps THREE tables and the exponent table in LDS (option "reproducible", one pass)
// (what each of the three leaves of the LDS at 64 row slots and a 2048-entry score table: the static_asserts behind fz_lds_bytes, tsem_internal.h)
constexpr int TS_LDS_MAX = 160 * 1024;
constexpr int TS_LDS_DYN_MAX = TS_LDS_MAX - 1024;    // the dynamic LDS a kernel may ask for: what hipFuncSetAttribute is handed and launch sizes are held to
constexpr int TS_ENTRY_PAD = 320;   // entries of padding behind indices[] / raw[] (k_report_rows reads 16-entry lanes past a row's end)
constexpr int TS_STRANDS = 16;   // strand-transposed entry order inside a sub-block

struct tsem_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  std::string err;
  int n_cu = 256;

  // ---- CSR of raw scores (rows owned by this rank) ----
  int64_t N = 0, nnz = 0;
  int32_t K = 0;
  int64_t* d_indptr = nullptr;
  int32_t* d_indices = nullptr;
  uint16_t* d_raw = nullptr;
  int64_t opt_ce_spread = 32768;    // option "cell_em_spread_entries": a group with more stored entries is fitted by the whole grid (tsem_cellem.hip); 0 never.
                                    // Measured (profiles/r14_group_em.txt): spread wins from the smallest group timed, 2^14 entries (1.2-1.4 x), 1.5-1.9 x here
  int64_t opt_drop_indices = -1;    // option "drop_csr_indices": free the CSR column ids (4 B per entry) once the blocked layout and the 2-byte popularity ids
                                    // exist — col = col_of_id[rid16], rebuilt for the span of a call (CsrIds, tsem_internal.h) by the generic row passes, z export, a
                                    // layout rebuild.  -1 auto: from 4e9 stored entries on; 0 never; 1 always
  double* d_lut = nullptr;
  int lut_len = 0;
  std::vector<double> lut_host;
  bool lut0_zero = false;           // lut[0] == 0: a masked score code adds nothing (k_report_pack)
  bool lut_increasing = false;      // lut[1] > 0 and strictly increasing from there: a larger score code is a larger Q (k_report_init_codes)

  // ---- row classes ----
  int64_t N_amb = 0, N_uni = 0, nnz_amb = 0;
  int32_t* d_amb_row = nullptr;     // [N_amb]  compact ambiguous row -> CSR row
  uint16_t* d_amb_wcode = nullptr;  // [N_amb_pad] per row SLOT: max raw code of the row (w = lut[code]), 0 = hole
  uint16_t* d_amb_wcode_c = nullptr;  // [N_amb]   same, per compact ambiguous row
  int32_t* d_slot_row = nullptr;    // [N_amb_pad] row slot -> CSR row, -1 = hole
  int32_t* d_uni_col = nullptr;     // [N_uni]
  uint16_t* d_uni_code = nullptr;   // [N_uni]
  uint32_t* d_maxcode = nullptr;    // [1]
  uint16_t* d_row_code = nullptr;   // [N] per CSR row: its largest raw score (w_i = lut[code], model.py:690); tsem_rowstats, kept for tsem_export_rowinfo
  uint8_t* d_row_cls = nullptr;     // [N] 0 empty row, 1 unique (Y_i = 0), 2 ambiguous (Y_i = 1, model.py:679)
  int32_t max_code = -1;            // largest raw score of the resident matrix (-1: not taken yet); tsem_max_score
  int32_t min_code = -1;            // smallest stored score above 0 (taken by the same pass; -1: none / not taken yet)
  bool have_rowstats = false;
  bool bin_inexact = false;         // option "reproducible": a pass gave up moving a column's grid after 84 repeats (its sums are not exact)

  // ---- model scalars (GLOBAL after set_model) ----
  double W_tot = 0, W_amb = 0, w_max = 0, pi_prior = 0, theta_prior = 0;
  double* d_pisum0 = nullptr;  // [K]
  uint32_t* d_ucount = nullptr;            // [K+1] unique rows with a positive score per column (local); [K]: some stored score is 0
  bool has_zero_score = false;             // ... read back once by tsem_rowstats
  unsigned long long* d_colcount = nullptr;   // [K] stored entries per column (local rows)
  bool em_cur = false, em_prev = false;    // current / previous pi, theta come from tsem_set_model or the M-step, not from tsem_set_params
  int64_t opt_split = -1;                  // split layout: -1 when K needs it, 1 forced (tests), 0 never
  int64_t opt_issue = -1;                  // fused kernel, exchange wave: partner loads before the combine (1), after it (0), -1 auto
  int64_t opt_report_kernel = 1;           // the report passes run the streaming kernels (0: the generic k_rowpass)
  int64_t opt_report_dbg = 0;              // the final z's report kernel: 8 k_report_rows, 128 / 256 k_report_pack32 with 8 / 16 entries per lane
  unsigned long long len_gt[6] = {0, 0, 0, 0, 0, 0};   // rows with more than 8, 16, 32, 64, 128, 256 entries (tsem_rowstats)
  int rowstats_G = 0, colsig_G = 0;        // lanes per row of the last k_rowstats / k_colsig (0: not launched; tsem_layout_info_n [38], [39])
  int64_t opt_shortcuts = 1;               // tsem_reassign answers `all`(initial) and `unique` from the setup counts
  int32_t* d_twin_rep = nullptr;  // [K] representative column of each exact-twin class
  std::vector<uint64_t> col_count;  // global entries per column
  std::vector<int32_t> twin_rep_host;
  int64_t row_offset = 0;      // global index of this rank's first row
  int n_twin_cols = 0;
  bool have_model = false;

  // ---- column partition + blocked COO layout of ambiguous rows ----
  int P = 1, Kp = 0, Kpad = 0, R = 2048;
  int64_t nb = 0, N_amb_pad = 0, nnz_pad = 0;
  uint32_t* d_colmap = nullptr;     // [K]    col -> (part<<16 | lcol)
  int32_t* d_col_of_pc = nullptr;   // [Kpad] part*Kp+lcol -> col or -1
  uint16_t* d_rid16 = nullptr;      // [nnz + TS_ENTRY_PAD] popularity id (slot * P + part) of every stored entry's column: the report pass
  int32_t* d_col_of_id = nullptr;   // [Kpad] id -> col or -1
  int64_t* d_sb_off = nullptr;      // [nb*P+1] entry offsets (multiples of 4)
  double* d_pval = nullptr;         // [nnz_pad]  Q values (fp64 entry format)
  uint16_t* d_pcode = nullptr;      // [nnz_pad]  raw score codes (code16 entry format: Q = lut[code])
  int64_t opt_sorted = -1;          // -1 auto, 0: strand-transposed sub-blocks, 1: row-ordered sub-blocks (fused layout)
  int64_t opt_timing = 1;           // HIP events around every n-th EM pass (tsem_kernel_stats); 0 = none
  int64_t opt_precision = 0;        // 1: the EM pass in fp32 arithmetic (diagnostic for the config-3 tolerance sweep)
  float *d_c32 = nullptr, *d_cs32 = nullptr, *d_lut32 = nullptr;
  int64_t opt_reproducible = 0;     // 1: order-independent (exact, binned) column sums in the fused EM pass: pi / theta / lnl bit-identical from run to run,
                                    //    two passes per iteration (profiles/HISTORY.md 5.1)
  uint16_t* d_ebias = nullptr;      // [Kpad] per slot: biased exponent of the bound 2^E of its contributions
  uint8_t* d_ovf = nullptr;         // [Kpad] a contribution reached its slot's bound in the last pass
  double* d_red_hi = nullptr;       // [K+2] column sums of the high pieces
  int64_t opt_lnl_fused = 0;        // option "use_likelihood" = 1: lay the matrix out so that the EM pass can sum the previous iteration's log-likelihood
                                    //    as well (fused kernel MODE 4: three tables per part in LDS, tsem_fused.h); tsem_em_chunk then needs no lnl pass per iteration
  bool lnl3 = false;                // the current layout allows it
  bool lnl3_declined = false;       // tsem_prepare_likelihood asked once and the geometry said no (reset with the matrix)
  bool em_rows = false;             // K beyond 64 x 7680 columns: no blocked layout at all, the EM pass and the log-likelihood are plain CSR row passes
                                    // with global gathers and fp64 atomics (any K; slow: a completeness path, tsem_em.hip k_em_rows)
  int64_t n_single_part = 0;        // ambiguous rows with all their entries in one column part (layout statistic, tsem_layout_info[25])
  bool split = false;               // SPLIT layout (K > 8 x 7680 on the fused path): parts of up to 15 424 columns, one LDS table per pass — a row-sum pass and a
                                    // scatter pass per iteration (tsem_fused.h MODE 5 / 7), the log-likelihood over column halves (MODE 8)
  double* d_rinv = nullptr;         // [N_amb_pad] recip0(row sum) of the last MODE 4 pass (what the next one needs of its E-step)
  // log tables of the log-likelihood passes (round 5): log1p(Q c) = log Q + log c + 1 / (Q c) for Q c >= 2^27 — one add and a table
  // look-up instead of a logarithm per stored entry (tsem_fused.h, fz_lnl_term)
  double* d_lctab = nullptr;        // [Kpad] log(pi * theta), permuted like d_ctab; rebuilt before every pass that reads it
  double* d_lqtab = nullptr;        // [lq_n] log Q: per score code (code entries), or indexed by the top bits of Q (fp64 entries)
  int lq_n = 0, lq_shift = 0, lq_base = 0;   // fp64 entries: index = (high word of Q >> lq_shift) - lq_base
  bool lq_tab_fits = false;         // the log Q table fits the LDS the layout leaves
  int lq_lin = 0, lq_c0 = 0;        // code entries with the reference's own score table: log Q = (code * lq_a) * lq_b from lq_c0 on (no table at all)
  double lq_a = 0, lq_b = 0;
  bool lq_tried = false;            // the tables were attempted for this layout (lq_n == 0 afterwards: they do not fit / do not apply)
  double lq_lo = 0, lq_hi = 0;      // log Q of the smallest / largest stored score (> 0): which columns may reach the exact branch of the log form
  unsigned long long* d_lq_mid = nullptr;   // [1] stored entries of such columns, counted by k_log_tab before every lnl pass (the device picks the form)
  int64_t lq_choice[2] = {0, 0};    // lnl passes enqueued with the selection armed | (diagnostic) reserved
  // The launch census (host only; tsem_debug_fused_launches): per cell of the table of instantiations, in the order team size 1..8 x
  // mode 0..9 x entry format 0..2 x geometry 0..3 x timeline x index format, [2 c] the launches that run whatever the device finds and
  // [2 c + 1] those enqueued with the selection armed (the device decides which of the two forms works: never coverage).
  // Sized at the first fused launch of the handle (fz_count): a handle that never launches the fused kernel holds nothing.
  std::vector<int64_t> fz_census;
  bool lag_agreed = false;          // row-sharded runs: EVERY rank can run MODE 4 (decided once per run, dropped for good after a time-out anywhere)
  bool lag_valid = false;           // the iteration committed last still owes its lnl, and d_rinv / d_ctab_prev are what the next MODE 4 pass needs for it
  bool exact_single = false;        // reproducible: both pieces in ONE pass (three tables per part fit the LDS with <= 8 parts)
  double* d_fpartial2 = nullptr;    // [fz_teams][Kpad] the low pieces' team partials of that pass
  int16_t* d_ehist = nullptr;       // [2K] per column: exponent (+4) of its last sum, and by how many bits it fell in the last iteration
  uint32_t* d_binflag = nullptr;    // [1] some column wants the pass repeated with another exponent
  int64_t n_bin_repeats = 0;        // passes repeated because an exponent had to move
  int64_t opt_deconflict = -1;      // conflict-aware entry order inside the rows of the row-ordered code layout (k_sb_deconflict): -1 auto = on
                                    //    (round 3: 4 ms of setup at 2e9 entries for -6 % per EM pass; round 2's version cost 14 ms and was opt-in)
  // fp64 entries: the order inside the quads (k_quad_order, tsem_quadorder.h) on the layouts that qualify: 0 off, 1 on, -1 auto = from
  // 11 B x nnz_amb >= opt_deconflict_min_bytes on (option "deconflict_min_bytes", default 1 GiB: every smaller layout stays as it was)
  int64_t opt_deconflict_min_bytes = 1ll << 30;
  int order_kind = 0;               // conflict-aware order of this layout: 0 none, 1 the score-code walk, 2 the quad order
  int64_t n_quads_moved = 0;        // quads k_quad_order permuted
  int64_t opt_geo = -1;             // -1 auto; 0 / 2 force the geometry of teams of 1-4 (experiments)
  double run_len_est = 0.0;         // mean entries per ambiguous row and column part (set by tsem_rowstats)
  bool sorted_layout = false;       // sub-blocks stored in row order (k_sb_fill_sorted)
  int geo = 0;                      // fused kernel geometry (tsem_fused.h): exchange waves x row pairs per lane
  bool fmt_wcode = false;           // fp64 entries, but the score table sits in LDS for the row weights (kernel FMT 2)
  bool fmt_code = false;            // entry format of the blocked layout: false = fp64 values, true = 2-byte codes
  int64_t opt_hot_split = 1;        // 1: very popular columns get several accumulator slots (see build_layout)
  int hot_extra = 0;                // spare slots per part reserved for them
  int n_hot_cols = 0;               // columns that were split
  int64_t opt_format = 0;           // 0 auto (codes when the fused kernel runs and the table fits LDS), 1 fp64, 2 codes
  uint32_t* d_prc = nullptr;        // [nnz_pad]  the entries' index in the format index_fmt names
  bool valmap = false;              // d_pval holds every sub-block's values grouped by wave (tsem_valmap.h): fused kernel, fp64 entries (set by every layout build)
  // The format of d_prc (tsem_index.h): FZ_IX32 one lrow << 16 | lcol word per entry; FZ_IX24 3 bytes per entry (fused kernel, non-split
  // layout, fp64 entries); FZ_IXQ the quad index.  Every layout build writes the FINAL format in one place (layout_decide_format; the
  // quad pack's fall-back alone may demote FZ_IXQ to FZ_IX24), and the fused kernels are looked up by it (fz_kernel).
  int index_fmt = FZ_IX32;
  // The 8-byte quad index (tsem_quad64.h; 2 B of index per entry).  Option "index_format": 0 auto, 1 the 3-byte index, 2 the quad
  // index (an error where it cannot apply).  Auto takes it where the fused kernel reads fp64 entries of a non-split, row-ordered
  // layout outside option "reproducible", geometry 0 or 1, with dummies of at most 0.5 % of nnz_amb and a 3-byte stream of at least
  // opt_quad_min_bytes (option "index_auto_min_bytes"; default 1 GiB: four times the Infinity Cache, a stream HBM certainly serves).
  int64_t opt_index = 0;
  int64_t opt_quad_min_bytes = 1ll << 30;
  bool quad_slots = false;          // this build raised the per-row part counts: every row of a block has an entry (a real one or a dummy) in every part (a property of the block cut, not of index_fmt)
  int64_t n_dummies = 0;            // dummy entries (column slot 0, value 0) of this layout: in nnz_pad, not in nnz_amb
  int64_t n_quad_bad = 0;           // quads the pack kernel could not represent (0 by construction; otherwise the layout keeps the 3-byte index)
  double* d_ypart = nullptr;        // [P][N_amb_pad] partial row sums
  int G1 = 1, G2 = 1, T1 = 512, T2 = 1024;
  double* d_partial = nullptr;      // [G2][Kpad]
  double* d_lnl_part = nullptr;     // [4096]
  int em_kernel = TSEM_EMK_AUTO;
  int64_t opt_R = 0, opt_P = 0, opt_chunk = 0, opt_dbg = 0;
  int64_t opt_dbg_skip = 0;         // option "fused_dbg_skip": fused launches of the kind fused_dbg's bits 32 / 64 aim at that go by untouched first
  int64_t dbg_seen[2] = {0, 0};     // ... and how many went by since either option was set (0: EM passes, 1: lnl passes)
  bool use_fused = false;
  int64_t max_subblock = 0;
  int64_t last_slow_path = 0;       // exchange granules that missed their tag in the last checked pass
  int fz_grid = 0, fz_teams = 0;
  double* d_fpartial = nullptr;     // [fz_teams][Kpad]
  double* d_amb_w = nullptr;        // [N_amb_pad] fragment weights
  uint32_t* d_sb_q32 = nullptr;     // [nb*P+2] sub-block offsets / 4
  bool fused_launched = false;
  unsigned long long* d_prof = nullptr;
  int prof_steps = 64;

  // ---- parameters ----
  double *d_pi = nullptr, *d_theta = nullptr, *d_pi_prev = nullptr, *d_theta_prev = nullptr;
  double *d_ctab = nullptr, *d_ctab_prev = nullptr;  // [Kpad] permuted pi*theta
  double* d_user_z = nullptr;       // [nnz] caller-assigned z (TSEM_Z_USER), NaN = not in z's pattern
  int32_t* d_tie_rows = nullptr;    // rows with several best hits, in row order, and their counts: left by the last
  int32_t* d_tie_cnt = nullptr;     // tsem_report_colsums for tsem_report_ties / tsem_reassign_rows
  int64_t n_ties = 0;
  int32_t* d_group = nullptr;       // [N] row -> group of the per-group sums (tsem_set_groups), -1 = none
  int32_t n_groups = 0;
  void* d_gtile = nullptr; size_t gtile_bytes = 0;   // one tile of per-group sums (by column | by id), kept between calls
  int64_t opt_group_tile = 0;       // bytes of per-group output computed per pass over the matrix (0 = 1 GB)
  // sparse per-group counts (tsem_group_counts, tsem_cells.hip): the group map's rows in group order, cached per map, and the last result
  uint64_t groups_version = 0;      // bumped by every tsem_set_groups
  uint64_t gc_version = ~0ull;      // the map version the cached grouping below was built from
  uint32_t* d_gc_key = nullptr;     // [N] group of the i-th row in group order (n_groups: the rows in no group, last)
  int32_t* d_gc_rows = nullptr;     // [N] the rows in group order, ascending within a group
  int64_t* d_gc_eoff = nullptr;     // [N + 1] where the i-th row's entries start in group order
  std::vector<int64_t> gc_rptr;     // host [n_groups + 1]: first row of every group in d_gc_rows
  std::vector<int64_t> gc_gent;     // host [n_groups + 1]: first entry of every group (d_gc_eoff at gc_rptr)
  int32_t gc_groups = 0;            // groups of the last result
  int64_t gc_nnz = 0, gc_cap = 0;   // stored entries of the last result / capacity of its arrays
  int32_t *d_gc_ogrp = nullptr, *d_gc_ocol = nullptr;   // [gc_cap] the last result: group, column, value per stored entry
  double* d_gc_oval = nullptr;
  int64_t* d_gc_gptr = nullptr;     // [gc_groups + 1] the last result's group pointer
  // per-cell EM fits (tsem_cell_em, tsem_cellem.hip): the compacted, column-ordered copy of the grouped rows, cached per map, and the last fit
  uint64_t ce_version = ~0ull;      // the map version the layout below was built from
  int64_t* d_ce_rptr = nullptr;     // [2 (n_groups + 1)] first row | first entry of every cell in group order
  uint32_t* d_ce_rinfo = nullptr;   // [rows in cells] row class << 16 | weight code, group order
  int32_t* d_ce_lcol = nullptr;     // [entries in cells] cell-local column of every entry, row-ordered view
  uint16_t* d_ce_code = nullptr;    // [entries in cells] its score code
  uint32_t* d_ce_cpos = nullptr;    // [entries in cells] column-ordered view: positions in the row-ordered view
  uint32_t* d_ce_cptr = nullptr;    // [ce_ncols + 1] first entry of every compacted column in the column-ordered view
  int64_t* d_ce_colptr = nullptr;   // [n_groups + 1] first compacted column of every cell
  int32_t* d_ce_cols = nullptr;     // [ce_ncols] the compacted columns: sorted distinct columns of every cell
  double* d_ce_scratch = nullptr;   // [entries in cells] what the row pass leaves for the column pass
  std::vector<int64_t> ce_colptr;   // host copy of d_ce_colptr
  int64_t ce_ncols = 0;             // sum of the cells' distinct columns
  int32_t ce_cells = 0;             // cells of the layout
  double *d_ce_pi = nullptr, *d_ce_theta = nullptr, *d_ce_pi_init = nullptr, *d_ce_theta_init = nullptr;   // [ce_ncols] the last fit
  double *d_ce_ws0 = nullptr, *d_ce_ws1 = nullptr, *d_ce_ws2 = nullptr;   // [ce_ncols] previous pi / theta, pisum0 of the cells whose tables do not fit LDS
  double* d_ce_ws3 = nullptr;       // [ce_ncols] |pi - previous pi| per column of the spread groups
  double* d_ce_rest = nullptr;      // [ce_cells][4] pi, theta, pi_init, theta_init of the columns a cell never touches
  int32_t *d_ce_niter = nullptr, *d_ce_conv = nullptr, *d_ce_list = nullptr;   // [ce_cells] iterations, converged, launch order
  double* d_ce_lnl = nullptr;       // [ce_cells]
  int32_t ce_class_n[4] = {0, 0, 0, 0};   // cells per class of the last fit: wave | 256 threads | 512 threads | global workspace
  int32_t ce_spread_n = 0;          // groups the last fit spread over the grid (counted in none of the four classes)
  bool ce_fitted = false;
  // bootstrap replicates (tsem_bootstrap, tsem_boot.hip): the last call's results, replicate-major
  int64_t opt_boot_hot = -1;        // option "boot_hot_columns": columns with LDS accumulators; -1 auto (the LDS budget), 0 none
  int64_t opt_boot_batch = 0;       // option "boot_batch": replicates per sweep over the matrix; 0 auto (8)
  int64_t opt_boot_rows = 0;        // option "boot_rows_per_block": rows per workgroup of the sweeps, rounded up to 32; 0 the formula
  double *d_bt_pi = nullptr, *d_bt_theta = nullptr, *d_bt_counts = nullptr;   // [bt_nrep x K]
  double* d_bt_lnl = nullptr;       // [bt_nrep]
  unsigned long long* d_bt_nfrags = nullptr;   // [bt_nrep] sum of the multiplicities
  int32_t *d_bt_niter = nullptr, *d_bt_conv = nullptr;   // [bt_nrep]
  int32_t bt_nrep = 0, bt_R = 0, bt_H = 0;   // replicates of the last call (0: none), its batch size and hot columns
  // ... per group (tsem_bootstrap_groups): the pattern P of the group map — the distinct (group, column) of the grouped rows' stored
  // entries, built by tsem_cells.hip and cached per map — and the last call's statistics per slot of P
  int64_t opt_boot_group = 0;       // option "boot_group_bytes": bytes of the per-batch accumulators of P at most; 0 auto (what is free)
  uint64_t bp_version = ~0ull;      // the map version the pattern below was built from
  int64_t* d_bp_gptr = nullptr;     // [bp_groups + 1] first slot of every group
  int32_t* d_bp_cols = nullptr;     // [bp_cap] the slots' columns, ascending within a group
  int64_t bp_nnz = 0, bp_cap = 0;   // slots of P / capacity of d_bp_cols
  int32_t bp_groups = 0;
  double *d_bg_mean = nullptr, *d_bg_sd = nullptr, *d_bg_vals = nullptr;   // [bg_nnz] mean, M2 then sd | [bg_nrep x bg_nnz] kept values
  int64_t bg_nnz = 0;
  int32_t bg_nrep = 0, bg_used = 0, bg_kept = 0, bg_groups = 0;   // the last grouped call (bg_nrep 0: none): replicates, good ones, values kept
  int32_t *d_rep_nb = nullptr, *d_rep_rows = nullptr;   // [N] scratch of tsem_report_colsums, kept between calls
  unsigned long long* d_rep_n = nullptr;
  struct RpChunk* d_rep_chunks = nullptr; int64_t n_rep_chunks = 0; int rep_chunk_E = 0;   // k_report_pack's packing of the rows into wave-sized chunks (tsem_report_pack.h)
  uint32_t* d_flag_bits = nullptr; int64_t flag_words = 0;   // near-tie bitmap of the generic row passes (+ their counter), kept between calls
  unsigned long long* d_exact_n = nullptr;   // [1] rows whose sum a report / row pass redid in the reference's order of additions (near-ties, tsem_npsum.h)
                                             //     since the matrix was loaded; tsem_layout_info[31]
  void* d_rep_tmp = nullptr; size_t rep_tmp_bytes = 0;
  double* d_red = nullptr;          // reduce buffer (K+2), internal or bound
  double* d_red_own = nullptr;
  int64_t red_count = 0;
  double* d_diffs = nullptr;        // [TS_DIFF_RING]
  double *d_tmp_pi = nullptr, *d_tmp_theta = nullptr;
  double* d_cnat = nullptr;         // [K] pi*theta in column order for the CSR row passes

  // ---- fused-kernel exchange state ----
  double* d_xchg = nullptr;
  uint32_t* d_xflags = nullptr;
  uint32_t* d_fz_aux = nullptr;     // [0] k_update's block counter, [2..3] error word / miss counter saved by its cleanup
  bool fz_clean = false;            // sync words and exchange ring are zero (k_update cleaned them after the last pass)
  uint32_t* d_xerr = nullptr;

  // ---- device-side loop control (tsem_em_chunk) ----
  uint32_t* d_ctl = nullptr;        // [0] stop: 0 run, 1 converged, 2 a rank's EM pass timed out, 3 ... its lnl pass  [1] iterations committed
  double* d_ctld = nullptr;         // [0] lnl of the previous iteration  [1..2] lnl reduce slots (value, error flag)
  double* d_lnls = nullptr;         // [TS_DIFF_RING]
  double *d_pi_first = nullptr, *d_theta_first = nullptr;   // params after the first iteration of the run (model.py:776-778)
  bool first_pending = false;       // the next committed update saves them
  double lnl_prev_seed = INFINITY;  // lnl the first iteration of the next run is compared with (model.py:683,786)
  int64_t n_fallbacks = 0;          // time-outs answered by switching to the two-pass kernels

  // ---- communicator (row-sharded runs) ----
  tsem_comm* comm = nullptr;

  // ---- instrumentation ----
  int64_t opt_phase = 0;            // option "phase_timing": HIP events between the phases of every iteration of tsem_em_chunk (tsem_phase_times)
  std::vector<hipEvent_t> pev;      // TS_PHASE_MARKS events per iteration of the current chunk
  std::vector<uint8_t> pev_set;     // ... which of them were recorded
  int pev_iter = -1;                // iteration of the chunk being enqueued (-1: outside tsem_em_chunk, nothing is marked)
  double phase_ms[6] = {0, 0, 0, 0, 0, 0};   // pass | column reduce | all-reduce | update | gap to the next iteration | first mark to last mark
  int64_t phase_n = 0;              // iterations summed into phase_ms
  std::vector<hipEvent_t> ev;       // pairs
  hipEvent_t ev_rep[2] = {nullptr, nullptr};   // around the dominant kernel of the last tsem_report_colsums (tsem_report_stats)
  bool rep_timed = false; int rep_kernel = 0; int64_t rep_deferred = 0;
  // What the last tsem_report_colsums ([0]) and the last tsem_reassign_groups ([1]: its last tile) launched (tsem_report_info_n): host
  // values noted next to the launch.  `list`: d_rep_rows / d_rep_n still hold THIS launch's deferred rows (the two calls share them).
  struct ReportLaunch {
    int family = 0, G = 0, E = 0, init = 0, gm = 0, cold = 0, Hs = 0, HC = 0, lut_rep = 0, grid = 0, block = 0, tiles = 0, tile_groups = 0;
    bool list = false;
  } rep_launch[2];
  int32_t* d_rep_sel = nullptr; unsigned long long* d_rep_sel_n = nullptr;   // [N], [1] the tied rows as ties_of_counts selects them (the deferred list stays)
  size_t ev_used = 0;
  double em_ms_acc = 0;
  int64_t em_launches = 0, em_timed = 0;
};

constexpr int TS_DIFF_RING = 65536;
constexpr int TS_PHASE_MARKS = 5;   // before the pass | after it | after the column reduce | after the all-reduce | after the update
constexpr int TS_PROF_WORDS = 64 * 16 + 512 * 8;   // option "fused_prof": per-step slots of team 0 + start-up stamps of up to 512 workgroups

struct tsem_local_group;            // in-process transport: several handles on ONE device (tsem_comm_create_local)

struct tsem_comm {
  ncclComm_t nccl = nullptr;        // RCCL transport (one process per GPU)
  tsem_local_group* local = nullptr;   // in-process transport (tests, several engines sharing a GPU)
  int device = 0, rank = 0, world = 1;
  uint64_t epoch = 0;               // collectives issued so far (local transport: slot parity)
  void* d_stage = nullptr;          // staging buffer of tsem_comm_allreduce_host
  size_t stage_bytes = 0;
  bool active() const { return nccl != nullptr || local != nullptr; }
};
