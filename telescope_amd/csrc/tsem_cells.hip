// libtelescope_em.so, cells unit: per-group counts of the assignment matrix as a SPARSE matrix on the device — scTelescope.output_report's
// per-barcode count matrix `_assignments[_rows, :].sum(0)` for every barcode (model.py:611-625) — without global atomics.
//
// scipy's `csr[rows].sum(0)` adds every column's values in listing order, starting from 0 (the transposed matvec walks the selected rows
// in order), and the reference lists a barcode's rows in ascending order.  This unit reproduces that order exactly:
//   grouping (once per map)  a stable radix sort of (group, row) puts every group's rows in ascending row order;
//   per tile of groups       the row pass of tsem_rows_lookup writes reassign(method)[row, :] for every entry of the tile's rows, taken in
//                            group order (stage A); the entries are keyed (group, column) and stably radix-sorted, so every run of equal
//                            keys holds one (group, column)'s values in ascending row order; ONE lane adds each run's values in that
//                            order (k_run_sums, stage B) and the runs with a non-zero sum are compacted into the result.
// A group with more entries than a tile holds is cut into pieces of rows; its running totals are kept in a K-sized row of doubles
// between the pieces (the pieces' lanes continue from them) and compacted after its last piece.  The result is bit-identical to summing
// the device's own `reassign` matrix with scipy, for every method, and deterministic.  Limit: a (group, column) run is summed by one
// lane — a group that holds a large share of the matrix's rows in one column runs at one lane's speed.  Real barcodes never do.
#include "tsem_runs.h"

namespace {

// scratch per stored entry of a tile: keys x 2, values x 2, run heads, runs, sort storage.  Option "group_tile_bytes" bounds these tile
// buffers; outside it stay the grouping cached per map (16 B per row), the caller's picks (4 B per row, `choose`), the result (16 B per
// stored entry) and, after option "drop_csr_indices", the CSR column ids rebuilt for the call (4 B per entry of the matrix)
constexpr int64_t GC_BYTES_PER_ENTRY = 96;

__global__ void k_gc_keys(int64_t N, const int32_t* __restrict__ grp, int32_t n_groups, uint32_t* __restrict__ key) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < N) { const int32_t g = grp[i]; key[i] = (g < 0 || g >= n_groups) ? (uint32_t)n_groups : (uint32_t)g; }
}
// first position of every group g in [0, n_q) among n sorted keys: out[g] = min { i : key[i] >= g } (n if none) — one lane per group,
// a binary search each (most of the 10^5-10^6 barcodes of a droplet run may be empty in a result: no lane walks a gap of groups)
template <typename T>
__global__ void k_lower_bounds(int64_t n_q, int64_t n, const T* __restrict__ key, int64_t* __restrict__ out) {
  const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= n_q) return;
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = lo + (hi - lo) / 2;
    if ((int64_t)key[mid] < g) lo = mid + 1; else hi = mid;
  }
  out[g] = lo;
}
__global__ void k_gc_lens(int64_t M, const int32_t* __restrict__ rows, const int64_t* __restrict__ indptr, int64_t* __restrict__ len) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < M) len[i] = indptr[rows[i] + 1] - indptr[rows[i]];
  else if (i == M) len[i] = 0;
}
__global__ void k_gc_gather64(int64_t n, const int64_t* __restrict__ idx, const int64_t* __restrict__ src, int64_t* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = src[idx[i]];
}
// the rows [r0, r0 + n) of the group order: their entries' offsets relative to the tile and their picks (list order)
__global__ void k_gc_tile_rows(int64_t n, int64_t r0, const int32_t* __restrict__ rows, const int64_t* __restrict__ eoff,
                               const int32_t* __restrict__ picks, int64_t* __restrict__ off, int32_t* __restrict__ lpicks) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i <= n) off[i] = eoff[r0 + i] - eoff[r0];
  if (i < n && lpicks) lpicks[i] = picks ? picks[rows[r0 + i]] : 0;
}
// key of every entry of the tile: (group - g0) << cbits | column, in the tile's entry order (one lane per row: rows are short)
__global__ void k_gc_entry_keys(int64_t n, int64_t r0, const int32_t* __restrict__ rows, const uint32_t* __restrict__ gkey,
                                const int64_t* __restrict__ off, const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices,
                                int32_t g0, int cbits, uint64_t* __restrict__ key) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int32_t row = rows[r0 + i];
  const uint64_t hi = (uint64_t)(gkey[r0 + i] - (uint32_t)g0) << cbits;
  const int64_t s = indptr[row], len = indptr[row + 1] - s, o = off[i];
  for (int64_t k = 0; k < len; ++k) key[o + k] = hi | (uint32_t)indices[s + k];
}
// run r = the entries [start[r], start[r + 1]) — found from the inclusive scan of the heads: head i starts run hscan[i] - 1
__global__ void k_gc_starts(int64_t n, const uint32_t* __restrict__ head, const uint32_t* __restrict__ hscan, uint32_t* __restrict__ start) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n && head[i]) start[hscan[i] - 1] = (uint32_t)i;
}
// Stage B: one lane per (group, column) run adds its values in position order — ascending row order — onto 0, or, for the pieces of a
// group cut across tiles, onto the running total in carry[column] (written back; such runs are not kept).
__global__ void k_run_sums(int64_t n_runs, int64_t n, const uint32_t* __restrict__ start, const uint64_t* __restrict__ key,
                           const double* __restrict__ val, int cbits, int32_t g0, double* __restrict__ carry,
                           int32_t* __restrict__ rgrp, int32_t* __restrict__ rcol, double* __restrict__ rval, uint32_t* __restrict__ keep) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n_runs) return;
  const int64_t s = start[r], e = r + 1 < n_runs ? (int64_t)start[r + 1] : n;
  const uint64_t k = key[s];
  const int32_t col = (int32_t)(k & ((1ull << cbits) - 1ull));
  double sum = carry ? carry[col] : 0.0;
  for (int64_t p = s; p < e; ++p) sum += val[p];
  if (carry) { carry[col] = sum; keep[r] = 0u; return; }
  rgrp[r] = g0 + (int32_t)(k >> cbits); rcol[r] = col; rval[r] = sum;
  keep[r] = sum != 0.0 ? 1u : 0u;
}
// the running totals of a finished cut group as runs (one per column) — compacted like the tile's runs — and the row cleared
__global__ void k_carry_runs(int32_t K, int32_t g, double* __restrict__ carry, int32_t* __restrict__ rgrp, int32_t* __restrict__ rcol,
                             double* __restrict__ rval, uint32_t* __restrict__ keep) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= K) return;
  const double v = carry[j];
  rgrp[j] = g; rcol[j] = j; rval[j] = v; keep[j] = v != 0.0 ? 1u : 0u;
  carry[j] = 0.0;
}
__global__ void k_gc_scatter(int64_t n, const uint32_t* __restrict__ keep, const uint32_t* __restrict__ kscan, const int32_t* __restrict__ rgrp,
                             const int32_t* __restrict__ rcol, const double* __restrict__ rval, int64_t base, int32_t* __restrict__ ogrp,
                             int32_t* __restrict__ ocol, double* __restrict__ oval) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n || !keep[r]) return;
  const int64_t o = base + kscan[r] - 1;
  ogrp[o] = rgrp[r]; ocol[o] = rcol[r]; oval[o] = rval[r];
}

// the rows of every group in ascending order, their entry offsets, and per group its first row and entry (host copies)
int build_grouping(tsem_ctx* h) {
  if (h->gc_version == h->groups_version && h->d_gc_rows) return TSEM_OK;
  const int64_t N = h->N;
  const int32_t G = h->n_groups;
  TSEM_ALLOC(h->d_gc_key, N);
  TSEM_ALLOC(h->d_gc_rows, N);
  TSEM_ALLOC(h->d_gc_eoff, N + 1);
  DevTmp keys, rptr, lens, gent, tmp;
  TSEM_TMP(keys, 4 * N); TSEM_TMP(rptr, 8 * ((int64_t)G + 1)); TSEM_TMP(lens, 8 * (N + 1)); TSEM_TMP(gent, 8 * ((int64_t)G + 1));
  if (N) {
    k_gc_keys<<<cdiv64(N, 256), 256, 0, h->stream>>>(N, h->d_group, G, keys.as<uint32_t>());
    TSEM_HIP(hipGetLastError());
  }
  rocprim::counting_iterator<int32_t> iota(0);
  const int gbits = bits_for((uint64_t)G);
  size_t tb = 0;
  TSEM_HIP(rocprim::radix_sort_pairs(nullptr, tb, keys.as<uint32_t>(), h->d_gc_key, iota, h->d_gc_rows, (size_t)N, 0, gbits, h->stream));
  size_t tb2 = 0;
  TSEM_HIP(rocprim::exclusive_scan(nullptr, tb2, lens.as<int64_t>(), h->d_gc_eoff, (int64_t)0, (size_t)N + 1, rocprim::plus<int64_t>(), h->stream));
  TSEM_TMP(tmp, std::max(tb, tb2));
  if (N) TSEM_HIP(rocprim::radix_sort_pairs(tmp.p, tb, keys.as<uint32_t>(), h->d_gc_key, iota, h->d_gc_rows, (size_t)N, 0, gbits, h->stream));
  k_lower_bounds<uint32_t><<<cdiv64((int64_t)G + 1, 256), 256, 0, h->stream>>>((int64_t)G + 1, N, h->d_gc_key, rptr.as<int64_t>());
  TSEM_HIP(hipGetLastError());
  h->gc_rptr.assign((size_t)G + 1, 0);
  TSEM_HIP(hipMemcpyAsync(h->gc_rptr.data(), rptr.p, 8 * ((size_t)G + 1), hipMemcpyDeviceToHost, h->stream));
  TSEM_HIP(hipStreamSynchronize(h->stream));
  const int64_t M = h->gc_rptr[G];                         // rows that belong to a group
  k_gc_lens<<<cdiv64(M + 1, 256), 256, 0, h->stream>>>(M, h->d_gc_rows, h->d_indptr, lens.as<int64_t>());
  TSEM_HIP(hipGetLastError());
  TSEM_HIP(rocprim::exclusive_scan(tmp.p, tb2, lens.as<int64_t>(), h->d_gc_eoff, (int64_t)0, (size_t)M + 1, rocprim::plus<int64_t>(), h->stream));
  k_gc_gather64<<<cdiv64((int64_t)G + 1, 256), 256, 0, h->stream>>>((int64_t)G + 1, rptr.as<int64_t>(), h->d_gc_eoff, gent.as<int64_t>());
  TSEM_HIP(hipGetLastError());
  h->gc_gent.assign((size_t)G + 1, 0);
  TSEM_HIP(hipMemcpyAsync(h->gc_gent.data(), gent.p, 8 * ((size_t)G + 1), hipMemcpyDeviceToHost, h->stream));
  TSEM_HIP(hipStreamSynchronize(h->stream));
  h->gc_version = h->groups_version;
  return TSEM_OK;
}

// room for `need` stored entries in the result, the entries so far kept
int grow_result(tsem_ctx* h, int64_t need) {
  if (need <= h->gc_cap && h->d_gc_ogrp) return TSEM_OK;
  const int64_t cap = std::max<int64_t>(need, std::max<int64_t>(2 * h->gc_cap, 1 << 16));
  int32_t *g = nullptr, *c = nullptr;
  double* v = nullptr;
  TSEM_ALLOC(g, cap);
  if (int rc = dalloc(h, &c, (size_t)cap)) { dfree(g); return rc; }
  if (int rc = dalloc(h, &v, (size_t)cap)) { dfree(g); dfree(c); return rc; }
  if (h->gc_nnz) {
    (void)hipMemcpyAsync(g, h->d_gc_ogrp, 4 * (size_t)h->gc_nnz, hipMemcpyDeviceToDevice, h->stream);
    (void)hipMemcpyAsync(c, h->d_gc_ocol, 4 * (size_t)h->gc_nnz, hipMemcpyDeviceToDevice, h->stream);
    (void)hipMemcpyAsync(v, h->d_gc_oval, 8 * (size_t)h->gc_nnz, hipMemcpyDeviceToDevice, h->stream);
    const hipError_t e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) { dfree(g); dfree(c); dfree(v); TSEM_HIP(e); }
  }
  dfree(h->d_gc_ogrp); dfree(h->d_gc_ocol); dfree(h->d_gc_oval);
  h->d_gc_ogrp = g; h->d_gc_ocol = c; h->d_gc_oval = v; h->gc_cap = cap;
  return TSEM_OK;
}

// One tile: the rows [r0, r1) of the group order (entries [e0, e1)), groups from g0.  carry != nullptr: the tile is a piece of group g0
// alone, whose running totals carry[K] holds.
struct TileBufs {
  int64_t* off; int32_t* lpicks; double* val; double* val2; uint64_t* key; uint64_t* key2; uint32_t* head; uint32_t* hscan; uint32_t* start;
  int32_t* rgrp; int32_t* rcol; double* rval; void* sort_tmp; size_t sort_bytes;
};

int keep_runs(tsem_ctx* h, const TileBufs& B, int64_t n_runs) {
  if (n_runs <= 0) return TSEM_OK;
  size_t tb = B.sort_bytes;
  TSEM_HIP(rocprim::inclusive_scan(B.sort_tmp, tb, B.head, B.hscan, (size_t)n_runs, rocprim::plus<uint32_t>(), h->stream));
  uint32_t kept = 0;
  TSEM_HIP(hipMemcpyAsync(&kept, B.hscan + n_runs - 1, 4, hipMemcpyDeviceToHost, h->stream));
  TSEM_HIP(hipStreamSynchronize(h->stream));
  if (int rc = grow_result(h, h->gc_nnz + kept)) return rc;
  k_gc_scatter<<<cdiv64(n_runs, 256), 256, 0, h->stream>>>(n_runs, B.head, B.hscan, B.rgrp, B.rcol, B.rval, h->gc_nnz, h->d_gc_ogrp,
                                                          h->d_gc_ocol, h->d_gc_oval);
  TSEM_HIP(hipGetLastError());
  h->gc_nnz += kept;
  return TSEM_OK;
}

int run_tile(tsem_ctx* h, CsrIds& ids, const TileBufs& B, int method, double thresh, int which, const int32_t* d_picks, int64_t r0, int64_t r1,
             int64_t ne, int32_t g0, int32_t g1, double* carry) {
  const int64_t n = r1 - r0;
  if (n <= 0 || ne <= 0) return TSEM_OK;
  const int cbits = bits_for((uint64_t)std::max(0, h->K - 1));
  const int kbits = cbits + bits_for((uint64_t)(g1 - g0 - 1 > 0 ? g1 - g0 - 1 : 0));
  k_gc_tile_rows<<<cdiv64(n + 1, 256), 256, 0, h->stream>>>(n, r0, h->d_gc_rows, h->d_gc_eoff, d_picks, B.off,
                                                            method == TSEM_RA_CHOOSE ? B.lpicks : nullptr);
  TSEM_HIP(hipGetLastError());
  // stage A: reassign(method) of every entry, in the tile's entry order (acquires the CSR column ids)
  if (int rc = tsem_rows_mask_dev(h, ids, which, method, thresh, n, h->d_gc_rows + r0, method == TSEM_RA_CHOOSE ? B.lpicks : nullptr,
                                  B.off, B.val)) return rc;
  k_gc_entry_keys<<<cdiv64(n, 256), 256, 0, h->stream>>>(n, r0, h->d_gc_rows, h->d_gc_key, B.off, h->d_indptr, h->d_indices, g0,
                                                         cbits, B.key);
  TSEM_HIP(hipGetLastError());
  uint32_t n_runs = 0;
  if (int rc = sorted_runs(h, B.sort_tmp, B.sort_bytes, B.key, B.key2, B.val, B.val2, ne, kbits, B.head, B.hscan, &n_runs)) return rc;
  k_gc_starts<<<cdiv64(ne, 256), 256, 0, h->stream>>>(ne, B.head, B.hscan, B.start);
  TSEM_HIP(hipGetLastError());
  TSEM_HIP(hipStreamSynchronize(h->stream));
  // stage B (the run flags reuse the heads' array: the runs are at most the entries)
  k_run_sums<<<cdiv64(n_runs, 256), 256, 0, h->stream>>>(n_runs, ne, B.start, B.key2, B.val2, cbits, g0, carry, B.rgrp, B.rcol, B.rval, B.head);
  TSEM_HIP(hipGetLastError());
  if (carry) return TSEM_OK;
  return keep_runs(h, B, n_runs);
}

// ---- the pattern P of the group map (tsem_bootstrap_groups): the distinct (group, column) of the grouped rows' stored entries, ordered
// by (group, column).  The same tiles of groups, entry keys and stable sort as the counts above, without values: the heads of the runs
// of equal keys ARE the pattern.  Structural: no z is read.
// scratch per stored entry of a pattern tile: keys x 2, run heads, their scan, the rows' entry offsets; the sort's storage beside them
constexpr int64_t BP_BYTES_PER_ENTRY = 32;

__global__ void k_bp_compact(int64_t n, const uint32_t* __restrict__ head, const uint32_t* __restrict__ hscan, const uint64_t* __restrict__ key,
                             uint64_t* __restrict__ dkey) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n && head[i]) dkey[hscan[i] - 1] = key[i];
}
__global__ void k_bp_cols(int64_t n, const uint64_t* __restrict__ dkey, int cbits, int64_t base, int32_t* __restrict__ cols) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r < n) cols[base + r] = (int32_t)(dkey[r] & ((1ull << cbits) - 1ull));
}
// first slot of the tile's groups [g0, g0 + ng): base + the first distinct key of the group or a later one (a binary search per group)
__global__ void k_bp_ptr(int32_t ng, int32_t g0, int64_t n, const uint64_t* __restrict__ dkey, int cbits, int64_t base, int64_t* __restrict__ gptr) {
  const int32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= ng) return;
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = lo + (hi - lo) / 2;
    if ((dkey[mid] >> cbits) < (uint64_t)g) lo = mid + 1; else hi = mid;
  }
  gptr[g0 + g] = base + lo;
}
// a group with more entries than a tile holds: its columns are marked in a K-sized row (every lane writes the same word) ...
__global__ void k_bp_mark(int64_t n, const int32_t* __restrict__ rows, const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices,
                          uint32_t* __restrict__ flag) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int32_t row = rows[i];
  for (int64_t e = indptr[row]; e < indptr[row + 1]; ++e) flag[indices[e]] = 1u;
}
// ... and the marked columns listed in order, the row cleared
__global__ void k_bp_flag_cols(int32_t K, uint32_t* __restrict__ flag, const uint32_t* __restrict__ fscan, int64_t base, int32_t* __restrict__ cols) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= K) return;
  if (flag[j]) cols[base + fscan[j] - 1] = j;
  flag[j] = 0u;
}

int grow_pattern(tsem_ctx* h, int64_t need) {
  if (need <= h->bp_cap && h->d_bp_cols) return TSEM_OK;
  const int64_t cap = std::max<int64_t>(need, std::max<int64_t>(2 * h->bp_cap, 1 << 16));
  int32_t* c = nullptr;
  TSEM_ALLOC(c, cap);
  if (h->bp_nnz && h->d_bp_cols) {
    (void)hipMemcpyAsync(c, h->d_bp_cols, 4 * (size_t)h->bp_nnz, hipMemcpyDeviceToDevice, h->stream);
    const hipError_t e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) { dfree(c); TSEM_HIP(e); }
  }
  dfree(h->d_bp_cols);
  h->d_bp_cols = c; h->bp_cap = cap;
  return TSEM_OK;
}

int build_pattern(tsem_ctx* h) {
  if (h->bp_version == h->groups_version && h->d_bp_gptr) return TSEM_OK;
  if (int rc = build_grouping(h)) return rc;
  PhaseTimer pt(h->stream);
  const int32_t G = h->n_groups;
  const int K = h->K;
  h->bp_version = ~0ull; h->bp_nnz = 0; h->bp_groups = 0;
  TSEM_ALLOC(h->d_bp_gptr, (int64_t)G + 1);
  if (int rc = grow_pattern(h, 1)) return rc;
  CsrIds ids(h);
  const int64_t total = G ? h->gc_gent[G] : 0, grouped = G ? h->gc_rptr[G] : 0;
  const int64_t budget = h->opt_group_tile > 0 ? h->opt_group_tile : ((int64_t)1 << 30);
  int64_t cap = std::min<int64_t>(std::max<int64_t>(budget / BP_BYTES_PER_ENTRY, (int64_t)K + 1), (int64_t)1 << 30);
  cap = std::max<int64_t>(1, std::min(cap, std::max<int64_t>(total, grouped)));
  const int cbits = bits_for((uint64_t)std::max(0, K - 1));
  DevTmp bufs, flag_t, fscan_t, ftmp_t;
  int64_t* off = nullptr; uint64_t *key = nullptr, *key2 = nullptr; uint32_t *head = nullptr, *hscan = nullptr;
  void* sort_tmp = nullptr;
  size_t sort_bytes = 0, flag_bytes = 0;
  if (total > 0) {
    if (int rc = ids.acquire()) return rc;
    size_t sb = 0, sc = 0;
    TSEM_HIP(rocprim::radix_sort_keys(nullptr, sb, (uint64_t*)nullptr, (uint64_t*)nullptr, (size_t)cap, 0, std::min(64, cbits + 32), h->stream));
    TSEM_HIP(rocprim::inclusive_scan(nullptr, sc, (uint32_t*)nullptr, (uint32_t*)nullptr, (size_t)cap, rocprim::plus<uint32_t>(), h->stream));
    sort_bytes = std::max(sb, sc);
    auto up = [](size_t x) { return (x + 255) / 256 * 256; };
    const size_t c1 = (size_t)cap + 1;
    const size_t sz[5] = {8 * c1, 8 * c1, 8 * c1, 4 * c1, 4 * c1};
    size_t tot = sort_bytes;
    for (size_t s : sz) tot += up(s);
    TSEM_TMP(bufs, tot);
    char* p = bufs.as<char>();
    off = (int64_t*)p; p += up(sz[0]);
    key = (uint64_t*)p; p += up(sz[1]);
    key2 = (uint64_t*)p; p += up(sz[2]);
    head = (uint32_t*)p; p += up(sz[3]);
    hscan = (uint32_t*)p; p += up(sz[4]);
    sort_tmp = p;
  }
  for (int32_t g = 0; g < G;) {
    const int64_t r0 = h->gc_rptr[g], e0 = h->gc_gent[g];
    if (h->gc_gent[g + 1] - e0 > cap || h->gc_rptr[g + 1] - r0 > cap) {   // one group beyond a tile: marks instead of a sort
      const int64_t nr = h->gc_rptr[g + 1] - r0;
      if (!flag_t.p) {
        TSEM_TMP(flag_t, 4 * (size_t)K); TSEM_TMP(fscan_t, 4 * (size_t)K);
        TSEM_HIP(rocprim::inclusive_scan(nullptr, flag_bytes, (uint32_t*)nullptr, (uint32_t*)nullptr, (size_t)K, rocprim::plus<uint32_t>(), h->stream));
        TSEM_TMP(ftmp_t, flag_bytes);
        TSEM_HIP(hipMemsetAsync(flag_t.p, 0, 4 * (size_t)K, h->stream));
      }
      k_bp_mark<<<cdiv64(nr, 256), 256, 0, h->stream>>>(nr, h->d_gc_rows + r0, h->d_indptr, h->d_indices, flag_t.as<uint32_t>());
      TSEM_HIP(hipGetLastError());
      size_t tb = flag_bytes;
      TSEM_HIP(rocprim::inclusive_scan(ftmp_t.p, tb, flag_t.as<uint32_t>(), fscan_t.as<uint32_t>(), (size_t)K, rocprim::plus<uint32_t>(), h->stream));
      uint32_t n_cols = 0;
      TSEM_HIP(hipMemcpyAsync(&n_cols, fscan_t.as<uint32_t>() + K - 1, 4, hipMemcpyDeviceToHost, h->stream));
      TSEM_HIP(hipStreamSynchronize(h->stream));
      if (int rc = grow_pattern(h, h->bp_nnz + n_cols)) return rc;
      k_bp_flag_cols<<<cdiv64(K, 256), 256, 0, h->stream>>>(K, flag_t.as<uint32_t>(), fscan_t.as<uint32_t>(), h->bp_nnz, h->d_bp_cols);
      TSEM_HIP(hipGetLastError());
      TSEM_HIP(hipMemcpyAsync(h->d_bp_gptr + g, &h->bp_nnz, 8, hipMemcpyHostToDevice, h->stream));
      TSEM_HIP(hipStreamSynchronize(h->stream));
      h->bp_nnz += n_cols;
      ++g;
      continue;
    }
    int32_t g1 = g + 1;
    while (g1 < G && h->gc_gent[g1 + 1] - e0 <= cap && h->gc_rptr[g1 + 1] - r0 <= cap) ++g1;
    const int64_t n = h->gc_rptr[g1] - r0, ne = h->gc_gent[g1] - e0;
    uint32_t n_runs = 0;
    if (ne > 0) {
      const int kbits = cbits + bits_for((uint64_t)(g1 - g - 1));
      k_gc_tile_rows<<<cdiv64(n + 1, 256), 256, 0, h->stream>>>(n, r0, h->d_gc_rows, h->d_gc_eoff, nullptr, off, nullptr);
      TSEM_HIP(hipGetLastError());
      k_gc_entry_keys<<<cdiv64(n, 256), 256, 0, h->stream>>>(n, r0, h->d_gc_rows, h->d_gc_key, off, h->d_indptr, h->d_indices, g, cbits, key);
      TSEM_HIP(hipGetLastError());
      size_t tb = sort_bytes;
      TSEM_HIP(rocprim::radix_sort_keys(sort_tmp, tb, key, key2, (size_t)ne, 0, kbits, h->stream));
      k_run_heads<<<cdiv64(ne, 256), 256, 0, h->stream>>>(ne, key2, head);
      TSEM_HIP(hipGetLastError());
      tb = sort_bytes;
      TSEM_HIP(rocprim::inclusive_scan(sort_tmp, tb, head, hscan, (size_t)ne, rocprim::plus<uint32_t>(), h->stream));
      TSEM_HIP(hipMemcpyAsync(&n_runs, hscan + ne - 1, 4, hipMemcpyDeviceToHost, h->stream));
      TSEM_HIP(hipStreamSynchronize(h->stream));
      k_bp_compact<<<cdiv64(ne, 256), 256, 0, h->stream>>>(ne, head, hscan, key2, key);   // (the unsorted keys are no longer needed)
      TSEM_HIP(hipGetLastError());
      if (int rc = grow_pattern(h, h->bp_nnz + n_runs)) return rc;
      k_bp_cols<<<cdiv64(n_runs, 256), 256, 0, h->stream>>>(n_runs, key, cbits, h->bp_nnz, h->d_bp_cols);
      TSEM_HIP(hipGetLastError());
    }
    k_bp_ptr<<<cdiv64(g1 - g, 256), 256, 0, h->stream>>>(g1 - g, g, (int64_t)n_runs, key, cbits, h->bp_nnz, h->d_bp_gptr);
    TSEM_HIP(hipGetLastError());
    h->bp_nnz += n_runs;
    g = g1;
  }
  TSEM_HIP(hipMemcpyAsync(h->d_bp_gptr + G, &h->bp_nnz, 8, hipMemcpyHostToDevice, h->stream));
  TSEM_HIP(hipStreamSynchronize(h->stream));
  h->bp_groups = G;
  h->bp_version = h->groups_version;
  pt.lap("bootstrap_groups: pattern");
  return TSEM_OK;
}

}  // namespace

extern "C" {

int tsem_build_grouping(tsem_ctx* h) { return build_grouping(h); }   // (the per-cell fits start from the same grouping)
int tsem_build_group_pattern(tsem_ctx* h) { return build_pattern(h); }

// scTelescope.output_report's per-barcode counts (model.py:611-625) as a sparse matrix: see the top of this file.
int tsem_group_counts(tsem_ctx* h, int method, double thresh, int which, const int32_t* picks, int64_t* nnz) {
  if (!h || !h->d_indptr || !nnz) return TSEM_ERR_ARG;
  if (method < TSEM_RA_EXCLUDE || method > TSEM_RA_ALL) TSEM_FAIL(TSEM_ERR_ARG, "bad reassign method");
  if (int rc = ensure_device(h)) return rc;
  if (!h->d_group && h->N) TSEM_FAIL(TSEM_ERR_ARG, "tsem_group_counts: no group map (tsem_set_groups)");
  if (tsem_comm_on(h)) TSEM_FAIL(TSEM_ERR_ARG, "tsem_group_counts: row-sharded group counts are not supported (one GPU per run)");
  *nnz = 0;
  h->gc_nnz = 0; h->gc_groups = 0;
  const int32_t G = h->n_groups;
  const int K = h->K;
  if (int rc = build_grouping(h)) return rc;
  CsrIds ids(h);                                           // (acquired by the first tile's row pass: no tile, no rebuild)
  const int64_t budget = h->opt_group_tile > 0 ? h->opt_group_tile : ((int64_t)1 << 30);
  // entries (and rows) per tile: at least one row of the widest possible length, at most 2^31 (32-bit run positions)
  int64_t cap = std::min<int64_t>(std::max<int64_t>(budget / GC_BYTES_PER_ENTRY, (int64_t)K + 1), (int64_t)1 << 30);
  const int64_t total = G ? h->gc_gent[G] : 0;
  cap = std::max<int64_t>(1, std::min(cap, std::max<int64_t>(total, h->gc_rptr.empty() ? 1 : h->gc_rptr[G])));
  DevTmp dpk, bufs, carry_t;
  int32_t* d_picks = nullptr;
  if (method == TSEM_RA_CHOOSE && picks && h->N) {
    TSEM_TMP(dpk, 4 * h->N);
    TSEM_HIP(hipMemcpyAsync(dpk.p, picks, 4 * (size_t)h->N, hipMemcpyHostToDevice, h->stream));
    d_picks = dpk.as<int32_t>();
  }
  TileBufs B{};
  if (total > 0) {
    const int cbits = bits_for((uint64_t)std::max(0, K - 1));
    if (int rc = sorted_runs_tmp_bytes(h, (double*)nullptr, (double*)nullptr, cap, std::min(64, cbits + 32), &B.sort_bytes)) return rc;
    const size_t a = 256;                                  // (every array 256-byte aligned)
    auto up = [&](size_t x) { return (x + a - 1) / a * a; };
    const size_t c1 = (size_t)cap + 1;
    size_t sz[12] = {8 * c1, 4 * c1, 8 * c1, 8 * c1, 8 * c1, 8 * c1, 4 * c1, 4 * c1, 4 * c1, 4 * c1, 4 * c1, 8 * c1};
    size_t tot = B.sort_bytes;
    for (size_t s : sz) tot += up(s);
    TSEM_TMP(bufs, tot);
    char* p = bufs.as<char>();
    void* ptrs[12];
    for (int i = 0; i < 12; ++i) { ptrs[i] = p; p += up(sz[i]); }
    B.off = (int64_t*)ptrs[0]; B.lpicks = (int32_t*)ptrs[1]; B.val = (double*)ptrs[2]; B.val2 = (double*)ptrs[3];
    B.key = (uint64_t*)ptrs[4]; B.key2 = (uint64_t*)ptrs[5]; B.head = (uint32_t*)ptrs[6]; B.hscan = (uint32_t*)ptrs[7];
    B.start = (uint32_t*)ptrs[8]; B.rgrp = (int32_t*)ptrs[9]; B.rcol = (int32_t*)ptrs[10]; B.rval = (double*)ptrs[11];
    B.sort_tmp = p;
  }
  // tiles: consecutive whole groups up to `cap` entries and rows; a group beyond that alone is cut into pieces of rows
  std::vector<int64_t> eoff_slice;
  for (int32_t g = 0; g < G && total > 0;) {
    const int64_t r0 = h->gc_rptr[g], e0 = h->gc_gent[g];
    if (h->gc_gent[g + 1] - e0 > cap || h->gc_rptr[g + 1] - r0 > cap) {
      const int64_t nr = h->gc_rptr[g + 1] - r0;
      eoff_slice.resize((size_t)nr + 1);
      TSEM_HIP(hipMemcpyAsync(eoff_slice.data(), h->d_gc_eoff + r0, 8 * ((size_t)nr + 1), hipMemcpyDeviceToHost, h->stream));
      TSEM_HIP(hipStreamSynchronize(h->stream));
      if (!carry_t.p) {
        TSEM_TMP(carry_t, 8 * (size_t)K);
        TSEM_HIP(hipMemsetAsync(carry_t.p, 0, 8 * (size_t)K, h->stream));
      }
      for (int64_t a = 0; a < nr;) {
        int64_t b = a + 1;                                 // (one row never exceeds cap: cap > K)
        while (b < nr && b - a < cap && eoff_slice[b + 1] - eoff_slice[a] <= cap) ++b;
        if (int rc = run_tile(h, ids, B, method, thresh, which, d_picks, r0 + a, r0 + b, eoff_slice[b] - eoff_slice[a], g, g + 1,
                              carry_t.as<double>())) return rc;
        a = b;
      }
      k_carry_runs<<<cdiv64(K, 256), 256, 0, h->stream>>>(K, g, carry_t.as<double>(), B.rgrp, B.rcol, B.rval, B.head);
      TSEM_HIP(hipGetLastError());
      if (int rc = keep_runs(h, B, K)) return rc;
      ++g;
      continue;
    }
    int32_t g1 = g + 1;
    while (g1 < G && h->gc_gent[g1 + 1] - e0 <= cap && h->gc_rptr[g1 + 1] - r0 <= cap) ++g1;
    if (int rc = run_tile(h, ids, B, method, thresh, which, d_picks, r0, h->gc_rptr[g1], h->gc_gent[g1] - e0, g, g1, nullptr)) return rc;
    g = g1;
  }
  TSEM_ALLOC(h->d_gc_gptr, (int64_t)G + 1);
  if (int rc = grow_result(h, std::max<int64_t>(h->gc_nnz, 1))) return rc;
  k_lower_bounds<int32_t><<<cdiv64((int64_t)G + 1, 256), 256, 0, h->stream>>>((int64_t)G + 1, h->gc_nnz, h->d_gc_ogrp, h->d_gc_gptr);
  TSEM_HIP(hipGetLastError());
  TSEM_HIP(hipStreamSynchronize(h->stream));
  h->gc_groups = G;
  *nnz = h->gc_nnz;
  return TSEM_OK;
}

int tsem_group_counts_shape(tsem_ctx* h, int32_t* n_groups, int64_t* nnz) {
  if (!h || !n_groups || !nnz) return TSEM_ERR_ARG;
  if (!h->d_gc_gptr) TSEM_FAIL(TSEM_ERR_ARG, "tsem_group_counts_shape: no result (tsem_group_counts)");
  *n_groups = h->gc_groups;
  *nnz = h->gc_nnz;
  return TSEM_OK;
}

int tsem_group_counts_copy(tsem_ctx* h, int64_t* group_ptr, int32_t* cols, double* vals) {
  if (!h || !group_ptr || (h->gc_nnz && (!cols || !vals))) return TSEM_ERR_ARG;
  if (!h->d_gc_gptr) TSEM_FAIL(TSEM_ERR_ARG, "tsem_group_counts_copy: no result (tsem_group_counts)");
  if (int rc = ensure_device(h)) return rc;
  TSEM_HIP(hipMemcpyAsync(group_ptr, h->d_gc_gptr, 8 * ((size_t)h->gc_groups + 1), hipMemcpyDeviceToHost, h->stream));
  if (h->gc_nnz) {
    TSEM_HIP(hipMemcpyAsync(cols, h->d_gc_ocol, 4 * (size_t)h->gc_nnz, hipMemcpyDeviceToHost, h->stream));
    TSEM_HIP(hipMemcpyAsync(vals, h->d_gc_oval, 8 * (size_t)h->gc_nnz, hipMemcpyDeviceToHost, h->stream));
  }
  TSEM_HIP(hipStreamSynchronize(h->stream));
  return TSEM_OK;
}

}  // extern "C"
