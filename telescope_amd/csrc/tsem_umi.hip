// libtelescope_em.so, UMI unit: collapse the PCR duplicates of a single-cell run on the device (tsem_umi_dedup, include/telescope_em.h).
//
// A CLASS is the set of rows with one (cell, UMI), both >= 0.  Two rows of a class are LINKED if both store an entry in one column
// (the score does not matter), a COMPONENT is a connected set of a class under the links, and its REPRESENTATIVE the row whose largest
// raw score code is largest, the smallest row index among equals.  A row in no class, and a row without entries, is a component by
// itself.  rep[i] = the representative of i's component: integer work only, one answer whatever the launch order.
//
//   classes     row keys cell << ubits | umi (a row in no class: the sentinel n_cells << ubits, behind every class), stably radix-sorted
//               with the row as value (sorted_runs, tsem_runs.h): run c of equal keys is class c, its rows ascending.  Rows of one-row
//               classes are done: rep = the row.
//   links       every stored entry of a row in a multi-row class is keyed class << cbits | column with its row as value and sorted the
//               same way: two neighbours inside a run of equal keys are an edge between their rows (the sorted arrays ARE the edge list).
//   components  label[row] = row; one kernel per round lowers, for every edge, the larger of the two labels (of both rows and of the
//               row the larger label names) to the smaller, and replaces every class row's label by its label's label.  Labels only
//               fall and always name a row of the same component, so a round that changes nothing (the host reads one word between
//               rounds) has label = the component's smallest row everywhere.  A round moves the smallest row's label along every edge
//               at least: the rows of the longest class bound the rounds, and a call that exceeds the bound ends with an error.
//   result      one 64-bit atomicMax of maxcode << 32 | ~row per row on its component's label, then a gather.
//
// Memory: 8 B per row for the two maps, 44 B per row for keys, sorted rows, run numbers, labels, maxima and the result, up to 20 B per
// row in a class for entry counts, offsets and class starts, and 32 B per stored entry of the rows in multi-row classes (keys x 2,
// rows x 2, run heads, their scan) plus the sort's storage; what does not fit is refused (TSEM_ERR_NOMEM), not tiled.
#include "tsem_runs.h"

namespace {

// counts[0] += the values out of range, counts[1] += the rows in a class — one atomic per wave
__device__ __forceinline__ void ud_count(bool pred, uint32_t* __restrict__ slot) {
  const unsigned long long b = __ballot(pred);
  if ((threadIdx.x & 63) == 0 && b) atomicAdd(slot, (uint32_t)__popcll(b));
}
__global__ void k_ud_keys(int64_t N, const int32_t* __restrict__ cell, const int32_t* __restrict__ umi, int32_t n_cells, int32_t n_umis,
                          int ubits, uint64_t* __restrict__ key, uint32_t* __restrict__ counts) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  bool bad = false, in = false;
  if (i < N) {
    const int32_t c = cell[i], u = umi[i];
    bad = c < -1 || c >= n_cells || u < -1 || u >= n_umis;
    in = !bad && c >= 0 && u >= 0;
    key[i] = in ? ((uint64_t)c << ubits) | (uint64_t)u : (uint64_t)n_cells << ubits;
  }
  ud_count(bad, counts + 0);
  ud_count(in, counts + 1);
}
__global__ void k_ud_init(int64_t N, int32_t* __restrict__ label, unsigned long long* __restrict__ best, int32_t* __restrict__ rep) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < N) { label[i] = (int32_t)i; best[i] = 0ull; rep[i] = (int32_t)i; }
}
// position i of the sorted rows [0, M) lies in a class of several rows unless its run starts at i and ends there
__device__ __forceinline__ bool ud_multi(int64_t i, int64_t N, const uint32_t* __restrict__ head) {
  return !(head[i] && (i + 1 == N || head[i + 1]));
}
// len[i] = the stored entries of sorted row i if its class has several rows, else 0 (len[M] = 0); start[c] = class c's first position
__global__ void k_ud_class_rows(int64_t M, int64_t N, const int32_t* __restrict__ srow, const uint32_t* __restrict__ head,
                                const uint32_t* __restrict__ hscan, const int64_t* __restrict__ indptr, int64_t* __restrict__ len,
                                uint32_t* __restrict__ start) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i > M) return;
  if (i == M) { len[i] = 0; return; }
  const int32_t r = srow[i];
  len[i] = ud_multi(i, N, head) ? indptr[r + 1] - indptr[r] : 0;
  if (head[i]) start[hscan[i] - 1] = (uint32_t)i;
}
__global__ void k_ud_longest(int64_t C, int64_t M, const uint32_t* __restrict__ start, uint32_t* __restrict__ longest) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  const uint32_t n = (uint32_t)((c + 1 < C ? (int64_t)start[c + 1] : M) - (int64_t)start[c]);
  if (n > 1) atomicMax(longest, n);
}
// key class << cbits | column and value row of every entry of the rows in multi-row classes (one lane per row: rows are short)
__global__ void k_ud_entry_keys(int64_t M, const int32_t* __restrict__ srow, const uint32_t* __restrict__ hscan, const int64_t* __restrict__ eoff,
                                const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices, int cbits, uint64_t* __restrict__ key,
                                int32_t* __restrict__ val) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= M) return;
  const int64_t o = eoff[i], len = eoff[i + 1] - o;
  if (len <= 0) return;
  const int32_t r = srow[i];
  const uint64_t hi = (uint64_t)(hscan[i] - 1u) << cbits;
  const int64_t s = indptr[r];
  for (int64_t k = 0; k < len; ++k) { key[o + k] = hi | (uint32_t)indices[s + k]; val[o + k] = r; }
}
// One round.  Lane t < E: the edge between sorted entries t - 1 and t of one (class, column) run; lane t < M: the pointer jump of sorted
// row t.  A lane that reads an older label reads a larger one that names a row of the same component: nothing it writes is wrong, and
// a round in which no lane wrote read the labels as the round found them.
__global__ void k_ud_round(int64_t E, int64_t M, const int32_t* __restrict__ erow, const uint32_t* __restrict__ ehead,
                           const int32_t* __restrict__ srow, int32_t* label, uint32_t* changed) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  bool ch = false;
  if (t > 0 && t < E && !ehead[t]) {
    const int32_t a = erow[t - 1], b = erow[t];
    const int32_t la = label[a], lb = label[b];
    if (la != lb) {
      const int32_t lo = min(la, lb), hi = max(la, lb);
      atomicMin(&label[hi], lo);
      atomicMin(&label[a], lo);
      atomicMin(&label[b], lo);
      ch = true;
    }
  }
  if (t < M) {
    const int32_t r = srow[t];
    const int32_t l = label[r], ll = label[l];
    if (ll != l) { atomicMin(&label[r], ll); ch = true; }
  }
  if (ch) *changed = 1u;
}
// the rows of multi-row classes: largest raw score code << 32 | ~row onto the component's label (the smallest row wins a tie)
__global__ void k_ud_best(int64_t M, int64_t N, const int32_t* __restrict__ srow, const uint32_t* __restrict__ head,
                          const int64_t* __restrict__ indptr, const uint16_t* __restrict__ raw, const int32_t* __restrict__ label,
                          unsigned long long* __restrict__ best) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= M || !ud_multi(i, N, head)) return;
  const int32_t r = srow[i];
  uint32_t mc = 0;
  for (int64_t e = indptr[r]; e < indptr[r + 1]; ++e) mc = max(mc, (uint32_t)raw[e]);
  atomicMax(&best[label[r]], ((unsigned long long)mc << 32) | (unsigned long long)(~(uint32_t)r));
}
// rep of the rows of multi-row classes; counts[2] += the components among the rows in classes, counts[3] += the rows dropped
__global__ void k_ud_gather(int64_t M, int64_t N, const int32_t* __restrict__ srow, const uint32_t* __restrict__ head,
                            const int32_t* __restrict__ label, const unsigned long long* __restrict__ best, int32_t* __restrict__ rep,
                            uint32_t* __restrict__ counts) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  bool root = false, dropped = false;
  if (i < M) {
    const int32_t r = srow[i];
    const int32_t l = label[r];
    root = l == r;
    if (ud_multi(i, N, head)) {
      const int32_t p = (int32_t)(~(uint32_t)(best[l] & 0xFFFFFFFFull));
      rep[r] = p;
      dropped = p != r;
    }
  }
  ud_count(root, counts + 2);
  ud_count(dropped, counts + 3);
}

}  // namespace

extern "C" {

// The representative of every row's UMI component: see the top of this file and include/telescope_em.h.
int tsem_umi_dedup(tsem_ctx* h, const int32_t* cell_of_row, const int32_t* umi_of_row, int32_t n_cells, int32_t n_umis,
                   int32_t* rep_of_row, int64_t* stats4) {
  if (!h) return TSEM_ERR_ARG;
  if (!h->d_indptr) TSEM_FAIL(TSEM_ERR_ARG, "tsem_umi_dedup: no matrix loaded (tsem_load_scores)");
  if (tsem_comm_on(h)) TSEM_FAIL(TSEM_ERR_ARG, "tsem_umi_dedup: a row-sharded handle is not supported (one GPU per run)");
  if (!stats4) TSEM_FAIL(TSEM_ERR_ARG, "tsem_umi_dedup: stats4 is NULL");
  if (n_cells < 0 || n_umis < 0) TSEM_FAIL(TSEM_ERR_ARG, "tsem_umi_dedup: n_cells and n_umis must be >= 0");
  const int64_t N = h->N;
  if (N > 0 && (!cell_of_row || !umi_of_row || !rep_of_row)) TSEM_FAIL(TSEM_ERR_ARG, "tsem_umi_dedup: NULL cell_of_row, umi_of_row or rep_of_row");
  if (N >= (int64_t)INT32_MAX) TSEM_FAIL(TSEM_ERR_ARG, "tsem_umi_dedup: more than 2^31-1 rows");
  stats4[0] = stats4[1] = stats4[2] = stats4[3] = 0;
  if (N == 0) return TSEM_OK;
  if (int rc = ensure_device(h)) return rc;
  PhaseTimer pt(h->stream);

  // ---- classes -------------------------------------------------------------------------------------------------------
  const int ubits = bits_for((uint64_t)std::max(0, n_umis - 1));
  const int kbits = bits_for((uint64_t)n_cells << ubits);
  DevTmp dcell, dumi, key, key2, srow, head, hscan, counts, stmp;
  TSEM_TMP(dcell, 4 * N); TSEM_TMP(dumi, 4 * N); TSEM_TMP(key, 8 * N); TSEM_TMP(key2, 8 * N); TSEM_TMP(srow, 4 * N);
  TSEM_TMP(head, 4 * N); TSEM_TMP(hscan, 4 * N); TSEM_TMP(counts, 32);
  rocprim::counting_iterator<int32_t> iota(0);
  size_t sbytes = 0;
  if (int rc = sorted_runs_tmp_bytes(h, iota, (int32_t*)nullptr, N, kbits, &sbytes)) return rc;
  TSEM_TMP(stmp, sbytes);
  TSEM_HIP(hipMemcpyAsync(dcell.p, cell_of_row, 4 * (size_t)N, hipMemcpyHostToDevice, h->stream));
  TSEM_HIP(hipMemcpyAsync(dumi.p, umi_of_row, 4 * (size_t)N, hipMemcpyHostToDevice, h->stream));
  TSEM_HIP(hipMemsetAsync(counts.p, 0, 32, h->stream));
  uint32_t* d_counts = counts.as<uint32_t>();              // [0] bad values [1] rows in classes [2] components [3] dropped [4] longest class [5] changed
  k_ud_keys<<<cdiv64(N, 256), 256, 0, h->stream>>>(N, dcell.as<int32_t>(), dumi.as<int32_t>(), n_cells, n_umis, ubits, key.as<uint64_t>(), d_counts);
  TSEM_HIP(hipGetLastError());
  uint32_t hc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  TSEM_HIP(hipMemcpyAsync(hc, d_counts, 32, hipMemcpyDeviceToHost, h->stream));
  TSEM_HIP(hipStreamSynchronize(h->stream));
  if (hc[0]) TSEM_FAIL(TSEM_ERR_ARG, "tsem_umi_dedup: " + std::to_string(hc[0]) + " rows with cell_of_row outside [-1, n_cells) or umi_of_row outside [-1, n_umis)");
  const int64_t M = hc[1];                                 // rows in classes: the first M of the sorted rows
  DevTmp label, best, drep;
  TSEM_TMP(label, 4 * N); TSEM_TMP(best, 8 * N); TSEM_TMP(drep, 4 * N);
  k_ud_init<<<cdiv64(N, 256), 256, 0, h->stream>>>(N, label.as<int32_t>(), best.as<unsigned long long>(), drep.as<int32_t>());
  TSEM_HIP(hipGetLastError());
  int64_t C = 0, E = 0, ws_bytes = 0;
  int rounds = 0;
  uint32_t longest = 0;
  if (M > 0) {
    uint32_t n_runs = 0;
    if (int rc = sorted_runs(h, stmp.p, sbytes, key.as<uint64_t>(), key2.as<uint64_t>(), iota, srow.as<int32_t>(), N, kbits,
                             head.as<uint32_t>(), hscan.as<uint32_t>(), &n_runs)) return rc;
    TSEM_HIP(hipStreamSynchronize(h->stream));
    C = (int64_t)n_runs - (M < N ? 1 : 0);                 // (the rows in no class are one more run, the last)
    DevTmp len, eoff, start, sctmp;
    TSEM_TMP(len, 8 * (M + 1)); TSEM_TMP(eoff, 8 * (M + 1)); TSEM_TMP(start, 4 * C);
    size_t scb = 0;
    TSEM_HIP(rocprim::exclusive_scan(nullptr, scb, (int64_t*)nullptr, (int64_t*)nullptr, (int64_t)0, (size_t)M + 1, rocprim::plus<int64_t>(), h->stream));
    TSEM_TMP(sctmp, scb);
    k_ud_class_rows<<<cdiv64(M + 1, 256), 256, 0, h->stream>>>(M, N, srow.as<int32_t>(), head.as<uint32_t>(), hscan.as<uint32_t>(), h->d_indptr,
                                                              len.as<int64_t>(), start.as<uint32_t>());
    TSEM_HIP(hipGetLastError());
    k_ud_longest<<<cdiv64(C, 256), 256, 0, h->stream>>>(C, M, start.as<uint32_t>(), d_counts + 4);
    TSEM_HIP(hipGetLastError());
    TSEM_HIP(rocprim::exclusive_scan(sctmp.p, scb, len.as<int64_t>(), eoff.as<int64_t>(), (int64_t)0, (size_t)M + 1, rocprim::plus<int64_t>(), h->stream));
    TSEM_HIP(hipMemcpyAsync(&E, eoff.as<int64_t>() + M, 8, hipMemcpyDeviceToHost, h->stream));
    TSEM_HIP(hipMemcpyAsync(&longest, d_counts + 4, 4, hipMemcpyDeviceToHost, h->stream));
    TSEM_HIP(hipStreamSynchronize(h->stream));
    pt.lap("umi_dedup: classes");

    // ---- links and components ----------------------------------------------------------------------------------------
    if (E > 0) {
      const int cbits = bits_for((uint64_t)std::max(0, h->K - 1));
      const int ebits = cbits + bits_for((uint64_t)(C - 1));
      size_t ebytes = 0;
      if (int rc = sorted_runs_tmp_bytes(h, (int32_t*)nullptr, (int32_t*)nullptr, E, ebits, &ebytes)) return rc;
      auto up = [](size_t x) { return (x + 255) / 256 * 256; };
      const size_t sz[6] = {8 * (size_t)E, 8 * (size_t)E, 4 * (size_t)E, 4 * (size_t)E, 4 * (size_t)E, 4 * (size_t)E};
      size_t tot = up(ebytes);
      for (size_t s : sz) tot += up(s);
      ws_bytes = (int64_t)tot;
      size_t mfree = 0, mtotal = 0;
      TSEM_HIP(hipMemGetInfo(&mfree, &mtotal));
      if (tot > mfree)
        TSEM_FAIL(TSEM_ERR_NOMEM, "tsem_umi_dedup: the workspace of " + std::to_string(E) + " stored entries in multi-row classes needs " +
                                      std::to_string(tot) + " B, " + std::to_string(mfree) + " B are free (the call is not tiled)");
      DevTmp ws;
      TSEM_TMP(ws, tot);
      char* p = ws.as<char>();
      uint64_t* ekey = (uint64_t*)p; p += up(sz[0]);
      uint64_t* ekey2 = (uint64_t*)p; p += up(sz[1]);
      int32_t* erow = (int32_t*)p; p += up(sz[2]);
      int32_t* erow2 = (int32_t*)p; p += up(sz[3]);
      uint32_t* ehead = (uint32_t*)p; p += up(sz[4]);
      uint32_t* ehscan = (uint32_t*)p; p += up(sz[5]);
      void* etmp = p;
      {
        CsrIds ids(h);                                     // (option "drop_csr_indices": rebuilt for the keys, dropped again behind them)
        if (int rc = ids.acquire()) return rc;
        k_ud_entry_keys<<<cdiv64(M, 256), 256, 0, h->stream>>>(M, srow.as<int32_t>(), hscan.as<uint32_t>(), eoff.as<int64_t>(), h->d_indptr,
                                                              h->d_indices, cbits, ekey, erow);
        TSEM_HIP(hipGetLastError());
      }
      uint32_t n_eruns = 0;
      if (int rc = sorted_runs(h, etmp, ebytes, ekey, ekey2, erow, erow2, E, ebits, ehead, ehscan, &n_eruns)) return rc;
      // the rounds: a host loop, bounded by the rows of the longest class (its last round only finds nothing left to change)
      const int64_t bound = std::max<int64_t>(1, longest);
      const int64_t lanes = std::max(E, M);
      for (;;) {
        if (rounds >= bound)
          TSEM_FAIL(TSEM_ERR_TIMEOUT, "tsem_umi_dedup: the components did not settle within " + std::to_string(bound) +
                                          " rounds, the rows of the longest class (internal error: no result)");
        TSEM_HIP(hipMemsetAsync(d_counts + 5, 0, 4, h->stream));
        k_ud_round<<<cdiv64(lanes, 256), 256, 0, h->stream>>>(E, M, erow2, ehead, srow.as<int32_t>(), label.as<int32_t>(), d_counts + 5);
        TSEM_HIP(hipGetLastError());
        uint32_t changed = 0;
        TSEM_HIP(hipMemcpyAsync(&changed, d_counts + 5, 4, hipMemcpyDeviceToHost, h->stream));
        TSEM_HIP(hipStreamSynchronize(h->stream));
        ++rounds;
        if (!changed) break;
      }
      pt.lap("umi_dedup: links and components");
    }
    // ---- representatives ---------------------------------------------------------------------------------------------
    k_ud_best<<<cdiv64(M, 256), 256, 0, h->stream>>>(M, N, srow.as<int32_t>(), head.as<uint32_t>(), h->d_indptr, h->d_raw, label.as<int32_t>(),
                                                    best.as<unsigned long long>());
    TSEM_HIP(hipGetLastError());
    k_ud_gather<<<cdiv64(M, 256), 256, 0, h->stream>>>(M, N, srow.as<int32_t>(), head.as<uint32_t>(), label.as<int32_t>(),
                                                      best.as<unsigned long long>(), drep.as<int32_t>(), d_counts);
    TSEM_HIP(hipGetLastError());
    TSEM_HIP(hipMemcpyAsync(hc, d_counts, 32, hipMemcpyDeviceToHost, h->stream));
  }
  TSEM_HIP(hipMemcpyAsync(rep_of_row, drep.p, 4 * (size_t)N, hipMemcpyDeviceToHost, h->stream));
  TSEM_HIP(hipStreamSynchronize(h->stream));
  stats4[0] = M; stats4[1] = C; stats4[2] = M ? hc[2] : 0; stats4[3] = M ? hc[3] : 0;
  pt.lap("umi_dedup: representatives");
  if (pt.on)
    fprintf(stderr, "[tsem] umi_dedup: %lld rows in %lld classes (longest %u), %lld entries in multi-row classes, %d rounds, workspace %lld B\n",
            (long long)M, (long long)C, longest, (long long)E, rounds, (long long)ws_bytes);
  return TSEM_OK;
}

}  // extern "C"
