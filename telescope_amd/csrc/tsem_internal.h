// Internal to libtelescope_em.so: what the translation units of the library share besides the context (tsem_common.h).
//
//   tsem_host.hip    handle, options, matrix load / synthetic generator, score table, instrumentation
//   tsem_setup.hip   row statistics, column signatures, the blocked layout (build_layout), model / parameter set-up
//   tsem_em.hip      EM pass (fused launch, two-pass kernels), column reduce, update, log-likelihood, the chunked loop
//   tsem_report.hip  CSR row passes: z export, best hits, reassign, the streaming report pass, per-barcode sums
//   tsem_comm.hip    collectives: RCCL resolved at run time, the in-process transport, the communicator ABI
//   tsem_csr.hip     csr_matrix_plus primitives on fp64 CSR, numpy's legacy random draw
//   tsem_cells.hip   sparse per-group counts of the assignment matrix; the grouping (rows of every group in order) and the pattern
//                    (distinct (group, column) of the grouped rows' entries) cached per map
//   tsem_cellem.hip  one EM fit per group of rows (single-cell `--pooling_mode individual` / `celltype`)
//   tsem_boot.hip    bootstrap replicates: the EM refitted with a multiplicity per row, batches of replicates per sweep;
//                    with a group sink also per-(group, column) statistics over the replicates (the pattern comes from tsem_cells.hip)
//   tsem_umi.hip     UMI duplicates of a single-cell run: classes, links, components, representatives (tsem_umi_dedup)
//   tsem_bam.hip     the device loader of `assign`: BAM records of a chunk to per-fragment (locus, alnscore, alnlen) lists (tsem_bam_*;
//                    the stages' bodies are host / device functions in tsem_bam_rec.h and tsem_bam_stages.h, the record chain in tsem_bam_scan.h)
//   tsem_bgzf.hip    the BGZF blocks of a BAM file inflated on the device (tsem_bgzf_*; the body is the host / device function of
//                    tsem_bgzf_inflate.h, the chain of block headers in tsem_bgzf_scan.h)
//   tsem_bam_collate.hip  the records of a BAM that is not name-collated brought together by name (tsem_bam_collate; the bodies are the
//                    host / device functions of tsem_bam_collate.h, which tsem_bam_collate_host runs on one CPU thread)
//   tsem_stage.h     the host side that these three units share (host code only, included by them alone): one failure function and
//                    HIP-call macro, the grow-only device buffer, the stage clock, the status word, the rec_off check and chunk upload
//   tsem_fz_p*.hip   instantiations of the fused kernel, one team size per unit: the look-up generated (tsem_fused_inst.h) from the one
//                    table of what exists, fz_exists (tsem_fused.h)
//   tsem_index.h     the index formats of the layout's entries: tsem_ctx::index_fmt, fz_exists' `ix`, layout_info()
//   tsem_model.h     the model's scalar arithmetic (numerator, closed forms, twin rule, prior scale) for tsem_em / _cellem / _boot
//
// A kernel is launched only from the unit that defines it; other units go through the host functions declared here.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <numeric>
#include <type_traits>

#include "tsem_common.h"
#include "tsem_device.h"
#include "tsem_fused.h"
#include "tsem_model.h"

constexpr int RS_SUB = 16, RP_SUB = 16;     // lanes per row of the 16-lane row passes (set-up / report)
extern std::string g_create_err;           // why the last tsem_create / stateless primitive failed (tsem_last_error(NULL))

// ---- small device helpers ---------------------------------------------------------------------------------------
template <int W>
__device__ __forceinline__ double sg_sum(double v) {
#pragma unroll
  for (int o = W / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, W);
  return v;
}
template <int W>
__device__ __forceinline__ double sg_max(double v) {
#pragma unroll
  for (int o = W / 2; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, W));
  return v;
}
template <int W>
__device__ __forceinline__ int sg_sum_i(int v) {
#pragma unroll
  for (int o = W / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, W);
  return v;
}
template <int W>
__device__ __forceinline__ int sg_max_i(int v) {
#pragma unroll
  for (int o = W / 2; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, W));
  return v;
}

// block-wide sum of one double per thread; result valid in thread 0
__device__ __forceinline__ double block_sum(double v, double* scratch /* >= 16 doubles */) {
  v = sg_sum<64>(v);
  int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  __syncthreads();
  if (lane == 0) scratch[wave] = v;
  __syncthreads();
  double t = 0.0;
  if (threadIdx.x == 0) {
    int nw = (blockDim.x + 63) >> 6;
    for (int i = 0; i < nw; ++i) t += scratch[i];
  }
  return t;
}

// ---- host helpers -----------------------------------------------------------------------------------------------
template <typename T>
static int dalloc(tsem_ctx* h, T** p, size_t n) {
  if (*p) { (void)hipFree(*p); *p = nullptr; }
  if (n == 0) n = 1;
  hipError_t e = hipMalloc((void**)p, n * sizeof(T));
  if (e != hipSuccess) {
    h->err = std::string("hipMalloc(") + std::to_string(n * sizeof(T)) + " B): " + hipGetErrorString(e);
    return TSEM_ERR_NOMEM;
  }
  return TSEM_OK;
}
#define TSEM_ALLOC(ptr, n) do { int rc_ = dalloc(h, &(ptr), (size_t)(n)); if (rc_) return rc_; } while (0)

template <typename T>
static void dfree(T*& p) { if (p) { (void)hipFree(p); p = nullptr; } }

// Device memory freed when the scope ends: the temporaries of a call, on every return path.
struct DevTmp {
  void* p = nullptr;
  ~DevTmp() { if (p) (void)hipFree(p); }
  template <typename T> T* as() const { return static_cast<T*>(p); }
};
// ... and the same for a plain local pointer filled by TSEM_ALLOC / hipMalloc:  T* d_x = nullptr; TSEM_SCOPED(d_x);  — freed at scope
// exit on every return path (the manual hipFree at the end of a function is skipped by every early `return rc`)
template <typename T> struct DevScope {
  T*& p;
  explicit DevScope(T*& r) : p(r) {}
  ~DevScope() { if (p) { (void)hipFree(p); p = nullptr; } }
};
#define TSEM_SCOPED(ptr) DevScope<std::remove_pointer<decltype(ptr)>::type> tsem_scope_##ptr(ptr)
#define TSEM_TMP(tmp, bytes) do { if (hipMalloc(&(tmp).p, std::max<size_t>(1, (size_t)(bytes))) != hipSuccess) { \
    (tmp).p = nullptr; TSEM_FAIL(TSEM_ERR_NOMEM, "hipMalloc(" + std::to_string((size_t)(bytes)) + " B) failed"); } } while (0)

static inline int cdiv64(int64_t a, int64_t b) { return (int)((a + b - 1) / b); }

// TSEM_TRACE=1: host wall clock of the set-up phases on stderr (each lap synchronises the stream; a diagnostic, not a product path)
struct PhaseTimer {
  bool on; hipStream_t s; std::chrono::steady_clock::time_point t;
  explicit PhaseTimer(hipStream_t st) : on(getenv("TSEM_TRACE") != nullptr), s(st), t(std::chrono::steady_clock::now()) {}
  void lap(const char* name) {
    if (!on) return;
    (void)hipStreamSynchronize(s);
    const auto n = std::chrono::steady_clock::now();
    fprintf(stderr, "[tsem] %-34s %8.3f ms\n", name, std::chrono::duration<double, std::milli>(n - t).count());
    t = n;
  }
};

static inline int ensure_device(tsem_ctx* h) {
  TSEM_HIP(hipSetDevice(h->device));
  return TSEM_OK;
}

// The fused kernel's instantiations (fz_exists, tsem_fused.h: 376 kernels, most of the library's build time) live in eight
// translation units compiled in parallel (tsem_fz_p1.hip ... tsem_fz_p8.hip, tsem_fused_inst.h); each exports one look-up function.
// The host launches through the pointer.  ix: the index format the kernel must read — callers pass the layout's, h->index_fmt, and a
// kernel that reads another format is not returned.  Host code that only asks whether a kernel exists calls fz_exists.
typedef void (*fz_fn)(FusedArgs);
fz_fn tsem_fz_kernel_p1(int P, int mode, int fmt, int geo, bool prof, int ix);
fz_fn tsem_fz_kernel_p2(int P, int mode, int fmt, int geo, bool prof, int ix);
fz_fn tsem_fz_kernel_p3(int P, int mode, int fmt, int geo, bool prof, int ix);
fz_fn tsem_fz_kernel_p4(int P, int mode, int fmt, int geo, bool prof, int ix);
fz_fn tsem_fz_kernel_p5(int P, int mode, int fmt, int geo, bool prof, int ix);
fz_fn tsem_fz_kernel_p6(int P, int mode, int fmt, int geo, bool prof, int ix);
fz_fn tsem_fz_kernel_p7(int P, int mode, int fmt, int geo, bool prof, int ix);
fz_fn tsem_fz_kernel_p8(int P, int mode, int fmt, int geo, bool prof, int ix);
static inline int fz_fmt(const tsem_ctx* h) { return h->fmt_code ? 1 : (h->fmt_wcode ? 2 : 0); }
static inline fz_fn fz_kernel(int P, int mode, int fmt, int geo, bool prof, int ix) {
  switch (P) {
    case 1: return tsem_fz_kernel_p1(P, mode, fmt, geo, prof, ix); case 2: return tsem_fz_kernel_p2(P, mode, fmt, geo, prof, ix);
    case 3: return tsem_fz_kernel_p3(P, mode, fmt, geo, prof, ix); case 4: return tsem_fz_kernel_p4(P, mode, fmt, geo, prof, ix);
    case 5: return tsem_fz_kernel_p5(P, mode, fmt, geo, prof, ix); case 6: return tsem_fz_kernel_p6(P, mode, fmt, geo, prof, ix);
    case 7: return tsem_fz_kernel_p7(P, mode, fmt, geo, prof, ix); case 8: return tsem_fz_kernel_p8(P, mode, fmt, geo, prof, ix);
    default: return nullptr;
  }
}

// code16 entry format: only with the fused kernel, and only while the score table is small enough to
// sit in LDS beside the column tables (uint16 scores allow 65536 entries; alignments give a few hundred).
// With the round-2 exchange (branch-free, partner loads after the combine for short rows) codes in row order win
// at every row length measured — 10 / 14 / 20 / 28 / 40 / 100 entries per row: 1.47 / 1.61 / 1.98 / 2.55 / 3.60 /
// 3.76 ms against 1.71 / 1.96 / 2.57 / 3.26 / 4.23 / 4.39 ms with fp64 entries (profiles/r02_sweep_short.txt).
constexpr bool fz_lut_fits(int lut_len) { return lut_len > 0 && lut_len <= 2048; }   // the score table goes into LDS beside the column tables
static inline bool fz_wants_codes(const tsem_ctx* h) {
  return h->opt_format != 1 && fz_lut_fits(h->lut_len);
}
// Dynamic LDS of the layout's fused launches, from the kernel's own map (tsem_fused_lds.h: the bound over the passes the layout can
// launch).  codes: the score table in LDS;  lq_n: entries of the log-Q table behind it (the lnl pass with log tables).
static inline size_t fz_lds_bytes(const tsem_ctx* h, bool codes, int lq_n = 0) {
  return (size_t)fz_lds_layout_bytes(h->Kp, h->R, fz_yr(h->geo), h->split, h->exact_single, h->lnl3, h->opt_reproducible != 0, codes ? h->lut_len : 0, lq_n);
}
// The most row slots the set-up gives a block of this layout: the geometry's, and the largest R for which the map — the score table in
// LDS wherever it may go there — stays FZ_RMAX_RESERVE below the limit.  The reserve is what the choice of R has always kept beyond the
// launch check; R hangs on it.
constexpr int FZ_RMAX_RESERVE = 832;
constexpr int fz_layout_rmax(int Kp, int geo, bool split, bool exact_single, bool lnl3, bool reproducible, int lut_len) {
  const int lut = fz_lut_fits(lut_len) ? lut_len : 0;
  const int fixed = fz_lds_layout_bytes(Kp, 0, fz_yr(geo), split, exact_single, lnl3, reproducible, lut, 0);
  const int per_row = fz_lds_layout_bytes(Kp, 1, fz_yr(geo), split, exact_single, lnl3, reproducible, lut, 0) - fixed;
  const int fit = (TS_LDS_DYN_MAX - FZ_RMAX_RESERVE - fixed) / per_row;
  return fz_rmax(geo) < fit ? fz_rmax(geo) : fit;
}
// The column limits of a part, through the map: at that many columns, 64 row slots (the smallest block), a 2048-entry score table and
// the class's tail, the layout fits the limit.  Per column: two tables 16 B; "use_likelihood" three tables 24 B; "reproducible" in one
// pass three tables and 2 B of exponent bound, 26 B.
static_assert(fz_lds_layout_bytes(TS_MAX_KP, 64, fz_yr(0), false, false, false, false, 2048, 0) <= TS_LDS_DYN_MAX, "TS_MAX_KP: two tables");
static_assert(fz_lds_layout_bytes(TS_MAX_KP, 64, fz_yr(0), false, false, false, true, 2048, 0) <= TS_LDS_DYN_MAX, "TS_MAX_KP: reproducible, two passes");
static_assert(fz_lds_layout_bytes(2 * TS_MAX_KP, 64, fz_yr(1), true, false, false, false, 2048, 0) <= TS_LDS_DYN_MAX, "2 * TS_MAX_KP: split layout");
static_assert(fz_lds_layout_bytes(TS_MAX_KP_LNL, 64, fz_yr(0), false, false, true, false, 2048, 0) <= TS_LDS_DYN_MAX, "TS_MAX_KP_LNL: use_likelihood");
static_assert(fz_lds_layout_bytes(TS_MAX_KP3, 64, fz_yr(0), false, true, false, true, 2048, 0) <= TS_LDS_DYN_MAX, "TS_MAX_KP3: reproducible, one pass");

// ---- host functions shared between the units (defined in the unit named) ---------------------------------------------
class CsrIds;
extern "C" {
// tsem_host.hip
void tsem_free_layout(tsem_ctx* h);
void tsem_free_matrix(tsem_ctx* h);
// tsem_setup.hip
int tsem_choose_geometry(tsem_ctx* h);
int tsem_build_layout(tsem_ctx* h);
int tsem_bin_reset(tsem_ctx* h);                           // option "reproducible": the slots' bounds as a run finds them
int tsem_make_ctabs(tsem_ctx* h);                          // after tsem_build_layout: the permuted pi * theta tables (current and previous), allocated and filled
void tsem_report_preload(void);                            // the same for the report unit (build_layout, behind the fill)
void tsem_setup_preload(void);                             // load the set-up unit's code object now (behind a kernel that is running anyway)
int tsem_ensure_indices(tsem_ctx* h);                      // the CSR column ids, rebuilt from the popularity ids if option "drop_csr_indices" freed
void tsem_redrop_indices(tsem_ctx* h);                     // them | dropped again where the option says so: both for CsrIds (below) alone
// tsem_em.hip
int tsem_take_fused_error(tsem_ctx* h, uint32_t* word);
int tsem_twopass_attributes(tsem_ctx* h);                 // dynamic-LDS limits of the two-pass kernels
int tsem_sum_parts(tsem_ctx* h, const double* a, int na, const double* b, int nb, double* out);   // out[0] = sum a + sum b, fixed order
// tsem_report.hip
int tsem_rowpass_grid(tsem_ctx* h);
// reassign(method)[row, :] of a DEVICE row list into mask[off[i] ...] (the row pass of tsem_rows_lookup, no host copies; d_picks[i]
// belongs to list row i).  The CSR column ids are acquired in the caller's scope `ids`, which reads them after the pass as well.
int tsem_rows_mask_dev(tsem_ctx* h, CsrIds& ids, int which, int method, double thresh, int64_t n, const int32_t* d_rows,
                       const int32_t* d_picks, const int64_t* d_off, double* d_mask);
// tsem_cells.hip
int tsem_build_grouping(tsem_ctx* h);                      // d_gc_rows / d_gc_key / d_gc_eoff, gc_rptr / gc_gent for the current group map (cached)
int tsem_build_group_pattern(tsem_ctx* h);                 // d_bp_gptr / d_bp_cols, bp_nnz: the distinct (group, column) of the current map's rows (cached)
// tsem_cellem.hip
void tsem_cellem_free(tsem_ctx* h);                        // the per-cell layout and the last fit
// tsem_boot.hip
void tsem_boot_free(tsem_ctx* h);                          // the last bootstrap's results
// tsem_comm.hip
bool tsem_comm_on(const tsem_ctx* h);
int tsem_comm_allreduce_dev(tsem_comm* c, void* buf, size_t count, int dtype, hipStream_t s, std::string& err);
int tsem_comm_allreduce_red(tsem_ctx* h, int64_t offset, int64_t count);
}  // extern "C"

// Option "drop_csr_indices" frees h->d_indices once the blocked layout exists (tsem_setup.hip).  A pass that reads them obtains them
// through a scope of this type only: the constructor notes whether they are resident, acquire() rebuilds them if not (a path that never
// acquires never rebuilds) and the destructor drops again what the scope had to bring back, the stream synchronised first, on every
// return path.  A scope that found them resident does nothing at its end: no synchronisation on such a matrix, and scopes nest.
class CsrIds {
  tsem_ctx* h; bool had;
 public:
  explicit CsrIds(tsem_ctx* c) : h(c), had(c && c->d_indices != nullptr) {}   // (a null handle: the entry point's argument check follows)
  ~CsrIds() { if (h && !had) tsem_redrop_indices(h); }
  int acquire() { return tsem_ensure_indices(h); }
  template <typename Args> int acquire(Args& A) { const int rc = acquire(); A.indices = h->d_indices; return rc; }   // (RowPassArgs)
  void keep() { had = true; }                                      // the ids are meant to outlive the scope: every use says why
  static void drop_kept(tsem_ctx* c) { tsem_redrop_indices(c); }   // ... and the end of that (tsem_entry_tags_end)
};
