// The sorted-runs step of the single-cell units (included by tsem_cells.hip, tsem_cellem.hip and tsem_umi.hip only): every stored entry
// is keyed (group << cbits | column); the keys are stably radix-sorted with a value each and the runs of equal keys — one (group, column) each,
// its entries in the order they had — are numbered.  Unnamed namespace: each unit launches its own copy of the kernel (tsem_internal.h).
#pragma once
#include "tsem_internal.h"
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/iterator/counting_iterator.hpp>

namespace {
int bits_for(uint64_t v) { int b = 1; while (b < 64 && (v >> b) != 0) ++b; return b; }   // bits to hold 0..v (at least 1)
__global__ void k_run_heads(int64_t n, const uint64_t* __restrict__ key, uint32_t* __restrict__ head) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) head[i] = (i == 0 || key[i] != key[i - 1]) ? 1u : 0u;
}
// rocPRIM's temporary storage for sorted_runs (below) over up to n entries
template <typename VIn, typename VOut> int sorted_runs_tmp_bytes(tsem_ctx* h, VIn val, VOut val2, int64_t n, int kbits, size_t* bytes) {
  size_t sb = 0, sc = 0;
  TSEM_HIP(rocprim::radix_sort_pairs(nullptr, sb, (uint64_t*)nullptr, (uint64_t*)nullptr, val, val2, (size_t)n, 0, kbits, h->stream));
  TSEM_HIP(rocprim::inclusive_scan(nullptr, sc, (uint32_t*)nullptr, (uint32_t*)nullptr, (size_t)n, rocprim::plus<uint32_t>(), h->stream));
  *bytes = std::max(sb, sc);
  return TSEM_OK;
}
// n > 0 entries: (key, val) -> (key2, val2) sorted by the keys' low `kbits` bits, equal keys in their old order; head[i] = 1 where a run
// starts in key2 (`head` may be the unsorted keys' buffer); hscan = the inclusive scan of the heads: entry i lies in run hscan[i] - 1.
// The number of runs is on its way to *n_runs when this returns: valid after the caller's next stream synchronisation.
template <typename VIn, typename VOut> int sorted_runs(tsem_ctx* h, void* tmp, size_t tmp_bytes, uint64_t* key, uint64_t* key2, VIn val,
                                                       VOut val2, int64_t n, int kbits, uint32_t* head, uint32_t* hscan, uint32_t* n_runs) {
  size_t tb = tmp_bytes;
  TSEM_HIP(rocprim::radix_sort_pairs(tmp, tb, key, key2, val, val2, (size_t)n, 0, kbits, h->stream));
  k_run_heads<<<cdiv64(n, 256), 256, 0, h->stream>>>(n, key2, head);
  TSEM_HIP(hipGetLastError());
  tb = tmp_bytes;
  TSEM_HIP(rocprim::inclusive_scan(tmp, tb, head, hscan, (size_t)n, rocprim::plus<uint32_t>(), h->stream));
  TSEM_HIP(hipMemcpyAsync(n_runs, hscan + n - 1, 4, hipMemcpyDeviceToHost, h->stream));
  return TSEM_OK;
}
}  // namespace
