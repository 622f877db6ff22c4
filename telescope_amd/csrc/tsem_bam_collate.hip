// libtelescope_em.so, collate unit: the records of a BAM that is not name-collated brought into the order `assign` reads
// (tsem_bam_collate / tsem_bam_collate_host, include/telescope_em.h; the definition and the bodies: tsem_bam_collate.h).
//
//   k_collate_hash     one lane per record: bam_collate_check, bam_collate_hash; the first refused record in input order by one 64-bit
//                      atomicMin of record << 8 | code
//   k_collate_insert   one lane per record: bam_collate_insert into the table of {rep, first} slots
//   k_collate_key      one lane per record: first[slot[i]] << 32 | i; the groups are counted where a record is its group's first
//   rocprim::radix_sort_keys over the bits of the high word only: the keys enter in the order of their low words and the sort is
//                      stable (as tsem_runs.h relies on), which is the order of the whole key at less than half the passes
//   k_collate_size     one lane per output record: order[k] = the low word, the record's framed length
//   rocprim::exclusive_scan of the lengths: the output offsets
//   k_collate_gather   W lanes per output record (16, or 64 when the records average 1 KiB and more): the destination is written in
//                      aligned dwords, lane j of the group dword j, j + W, ...; each is built from the two aligned source dwords that
//                      hold its bytes (funnel shift by the byte distance of the two alignments, one value per record).  The up to 3
//                      bytes in front of the first aligned destination dword and behind the last go byte by byte.  A record of any
//                      length loops.  Neighbouring lanes read and write neighbouring dwords; a group's store is 64 B (256 B) in a row.
//
// Reads of the input go through aligned dwords that may begin up to 3 bytes in front of a record and end up to 3 behind: the input's
// device buffer is padded to a multiple of 4 and 8 bytes more, so every such dword lies inside it.  Writes are bounded by the scan's
// total, which the host checks against the input's size before the gather is launched.
#include "tsem_internal.h"
#include "tsem_bam_collate.h"
#include "tsem_stage.h"

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include <vector>

__global__ __launch_bounds__(256) void k_collate_hash(int64_t n, const uint8_t* __restrict__ bytes, const int64_t* __restrict__ rec_off,
                                                      int32_t hash_bits, uint64_t* __restrict__ hash, unsigned long long* first_bad) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const bam_col_stream R{bytes, rec_off};
  const int st = bam_collate_check(R.rec(i), R.len(i));
  if (st) { hash[i] = 0; atomicMin(first_bad, ((unsigned long long)i << 8) | (unsigned long long)st); return; }
  hash[i] = bam_collate_hash(R.rec(i), hash_bits);
}

__global__ __launch_bounds__(256) void k_collate_insert(int64_t n, const uint8_t* __restrict__ bytes, const int64_t* __restrict__ rec_off,
                                                        const uint64_t* __restrict__ hash, bam_col_slot* table, uint64_t cap,
                                                        uint32_t* __restrict__ slot) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  bam_collate_insert(i, bam_col_stream{bytes, rec_off}, hash, table, cap, slot);
}

__global__ __launch_bounds__(256) void k_collate_key(int64_t n, const bam_col_slot* __restrict__ table, const uint32_t* __restrict__ slot,
                                                     uint64_t* __restrict__ key, unsigned long long* n_names) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  bool f = false;
  if (i < n) key[i] = bam_collate_key(i, table, slot, &f);
  const unsigned long long m = __ballot(f);                  // one atomic per wave
  if ((threadIdx.x & 63) == 0 && m) atomicAdd(n_names, (unsigned long long)__popcll(m));
}

__global__ __launch_bounds__(256) void k_collate_size(int64_t n, const uint64_t* __restrict__ key, const int64_t* __restrict__ rec_off,
                                                      int64_t* __restrict__ size) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  const int64_t i = (int64_t)(key[k] & 0xFFFFFFFFull);
  size[k] = rec_off[i + 1] - rec_off[i];
}

template <int W>
__global__ __launch_bounds__(256) void k_collate_gather(int64_t n, const uint8_t* __restrict__ in, const int64_t* __restrict__ rec_off,
                                                        const uint64_t* __restrict__ key, const int64_t* __restrict__ out_off,
                                                        uint8_t* __restrict__ out) {
  const int64_t k = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / W;
  const int j = (int)(threadIdx.x % W);
  if (k >= n) return;
  const int64_t i = (int64_t)(key[k] & 0xFFFFFFFFull);
  const int64_t s = rec_off[i], len = rec_off[i + 1] - s, d = out_off[k];
  const int head = (int)((4 - (d & 3)) & 3);                  // (len >= 37: head, dwords and tail never overlap)
  if (j < head) out[d + j] = in[s + j];
  const int64_t nd = (len - head) >> 2;                       // aligned destination dwords
  const int tail = (int)((len - head) & 3);
  const int64_t sa = s + head;                                // the source byte of destination dword 0
  const unsigned sh = (unsigned)(sa & 3) * 8;
  const uint32_t* src = reinterpret_cast<const uint32_t*>(in + (sa & ~(int64_t)3));
  uint32_t* dst = reinterpret_cast<uint32_t*>(out + d + head);
  for (int64_t q = j; q < nd; q += W) {
    const uint32_t lo = src[q], hi = sh ? src[q + 1] : 0u;
    dst[q] = __funnelshift_r(lo, hi, sh);
  }
  if (j < tail) out[d + head + 4 * nd + j] = in[sa + 4 * nd + j];
}

namespace {

// a buffer of this call alone (the unit keeps nothing between calls); TSEM_ERR_NOMEM is what the caller's advice hangs on
int col_tmp(DevTmp& tmp, size_t bytes, const char* what) {
  if (hipMalloc(&tmp.p, std::max<size_t>(1, bytes)) == hipSuccess) return TSEM_OK;
  tmp.p = nullptr;
  return stage_fail(TSEM_ERR_NOMEM, "tsem_bam_collate: hipMalloc(" + std::to_string(bytes) + " B) for the " + what +
                                        " failed: the step holds the whole stream twice and 44 to 60 B per record on the device");
}

// the argument checks that both entries share; *total = the bytes of the records.  The offsets are held to bam_collate_chain, not to
// stage_check_rec_off: this step accepts every chain that does not descend and stays inside the bytes, and a record too short to
// hold a name is the kernels' to report (bam_collate_check, status 1, with the record's number) — not an argument error of the call.
int col_args(const char* fn, const uint8_t* bytes, int64_t n_bytes, const int64_t* rec_off, int64_t n_rec, int32_t hash_bits, uint8_t* out,
             int64_t* order, int64_t* n_names, int64_t* status2, int64_t* total) {
  const std::string f(fn);
  if (n_bytes < 0 || n_rec < 0 || !rec_off || !n_names || !status2 || (n_bytes && (!bytes || !out)) || (n_rec && !order))
    return stage_fail(TSEM_ERR_ARG, f + ": NULL pointer or negative size");
  if (n_rec >= (int64_t)0xFFFFFFFFll) return stage_fail(TSEM_ERR_ARG, f + ": 2^32 - 1 records or more");
  if (hash_bits < 0 || hash_bits > 64) return stage_fail(TSEM_ERR_ARG, f + ": hash_bits must be 0 .. 64");
  const int64_t bad = bam_collate_chain(rec_off, n_rec, n_bytes);
  if (bad >= 0) return stage_fail(TSEM_ERR_ARG, f + ": the offsets of record " + std::to_string(bad) + " descend or leave the bytes");
  *total = rec_off[n_rec] - rec_off[0];
  *n_names = 0; status2[0] = 0; status2[1] = -1;
  return TSEM_OK;
}

}  // namespace

extern "C" {

int tsem_bam_collate_host(const uint8_t* bytes, int64_t n_bytes, const int64_t* rec_off, int64_t n_rec, int32_t hash_bits, uint8_t* out,
                          int64_t* order, int64_t* n_names, int64_t* status2) {
  int64_t total = 0;
  if (int rc = col_args("tsem_bam_collate_host", bytes, n_bytes, rec_off, n_rec, hash_bits, out, order, n_names, status2, &total)) return rc;
  if (n_rec == 0) return TSEM_OK;
  const size_t n = (size_t)n_rec;
  std::vector<uint64_t> hash(n), key(n);
  std::vector<uint32_t> slot(n);
  std::vector<bam_col_slot> table((size_t)bam_collate_table_slots(n_rec));
  const unsigned long long st = bam_collate_run(bam_col_stream{bytes, rec_off}, n_rec, hash_bits, out, order, n_names, hash.data(), slot.data(),
                                                key.data(), table.data(), [](uint64_t* k, int64_t m) { std::sort(k, k + m); });
  (void)stage_status_decode(st, status2);
  return TSEM_OK;
}

int tsem_bam_collate(int device, const uint8_t* bytes, int64_t n_bytes, const int64_t* rec_off, int64_t n_rec, int32_t hash_bits, uint8_t* out,
                     int64_t* order, int64_t* n_names, int64_t* status2, double* ms) {
  int64_t total = 0;
  if (int rc = col_args("tsem_bam_collate", bytes, n_bytes, rec_off, n_rec, hash_bits, out, order, n_names, status2, &total)) return rc;
  if (ms) for (int k = 0; k < 5; ++k) ms[k] = 0;
  if (n_rec == 0) return TSEM_OK;
  if (hipSetDevice(device) != hipSuccess) return stage_fail(TSEM_ERR_HIP, "tsem_bam_collate: hipSetDevice failed (no usable HIP device)");
  const size_t n = (size_t)n_rec;
  const uint64_t cap = bam_collate_table_slots(n_rec);
  const int bits = [&] { int b = 1; while (b < 32 && ((uint64_t)(n_rec - 1) >> b) != 0) ++b; return b; }();   // of a record index
  size_t sort_b = 0, scan_b = 0;
  STAGE_HIP(rocprim::radix_sort_keys(nullptr, sort_b, (uint64_t*)nullptr, (uint64_t*)nullptr, n, 32, 32 + bits, (hipStream_t)0));
  STAGE_HIP(rocprim::exclusive_scan(nullptr, scan_b, (int64_t*)nullptr, (int64_t*)nullptr, (int64_t)0, n, rocprim::plus<int64_t>(), (hipStream_t)0));
  // every buffer is freed when the call returns, on every path (DevTmp)
  DevTmp t_in, t_out, t_off, t_a, t_b, t_slot, t_table, t_tmp, t_word;
  const size_t in_bytes = (((size_t)n_bytes + 3) & ~(size_t)3) + 8;
  int rc = col_tmp(t_in, in_bytes, "stream");
  if (!rc) rc = col_tmp(t_out, (size_t)total + 4, "collated stream");
  if (!rc) rc = col_tmp(t_off, (n + 1) * 8, "record offsets");
  if (!rc) rc = col_tmp(t_a, n * 8, "keys");
  if (!rc) rc = col_tmp(t_b, n * 8, "hashes");
  if (!rc) rc = col_tmp(t_slot, n * 4, "slots");
  if (!rc) rc = col_tmp(t_table, (size_t)cap * sizeof(bam_col_slot), "name table");
  if (!rc) rc = col_tmp(t_tmp, std::max(sort_b, scan_b), "sort's storage");
  if (!rc) rc = col_tmp(t_word, 16, "status words");
  if (rc) return rc;
  uint8_t *d_in = t_in.as<uint8_t>(), *d_out = t_out.as<uint8_t>();
  int64_t* d_off = t_off.as<int64_t>();
  uint64_t *d_key = t_a.as<uint64_t>(), *d_hash = t_b.as<uint64_t>(), *d_key2 = d_hash;       // (the hashes are done with before the sort)
  int64_t *d_size = t_a.as<int64_t>(), *d_pos = t_table.as<int64_t>();                       // (the keys before the sizes, the table before the scan)
  uint32_t* d_slot = t_slot.as<uint32_t>();
  bam_col_slot* d_table = t_table.as<bam_col_slot>();
  unsigned long long *d_bad = t_word.as<unsigned long long>(), *d_names = d_bad + 1;
  static_assert(sizeof(bam_col_slot) == 8, "the output offsets take the table's place: 8 B per record fit into >= 2 slots per record");
  StageClock<6, 5> clock;                                       // h2d, hash / insert / key, sort and scan, gather, d2h
  STAGE_HIP(clock.create());
  const unsigned grid = (unsigned)cdiv64(n_rec, 256);
  unsigned long long h_word[2] = {~0ull, 0};

  STAGE_HIP(clock.begin());
  STAGE_HIP(hipMemsetAsync(d_in + ((size_t)n_bytes & ~(size_t)3), 0, in_bytes - ((size_t)n_bytes & ~(size_t)3), 0));   // (the padding: read by the gather, never used)
  if (n_bytes) STAGE_HIP(hipMemcpyAsync(d_in, bytes, (size_t)n_bytes, hipMemcpyHostToDevice, 0));
  STAGE_HIP(hipMemcpyAsync(d_off, rec_off, (n + 1) * 8, hipMemcpyHostToDevice, 0));
  STAGE_HIP(hipMemsetAsync(d_bad, 0xFF, 8, 0));
  STAGE_HIP(hipMemsetAsync(d_names, 0, 8, 0));
  STAGE_HIP(hipMemsetAsync(d_table, 0xFF, (size_t)cap * sizeof(bam_col_slot), 0));
  STAGE_HIP(clock.mark());
  k_collate_hash<<<grid, 256>>>(n_rec, d_in, d_off, hash_bits, d_hash, d_bad);
  STAGE_HIP(hipGetLastError());
  STAGE_HIP(hipMemcpyAsync(&h_word[0], d_bad, 8, hipMemcpyDeviceToHost, 0));
  STAGE_HIP(hipStreamSynchronize(0));
  if (stage_status_decode(h_word[0], status2)) return TSEM_OK;                               // refused: nothing behind the check runs
  k_collate_insert<<<grid, 256>>>(n_rec, d_in, d_off, d_hash, d_table, cap, d_slot);
  STAGE_HIP(hipGetLastError());
  k_collate_key<<<grid, 256>>>(n_rec, d_table, d_slot, d_key, d_names);
  STAGE_HIP(hipGetLastError());
  STAGE_HIP(clock.mark());
  size_t tb = sort_b;
  STAGE_HIP(rocprim::radix_sort_keys(t_tmp.p, tb, d_key, d_key2, n, 32, 32 + bits, (hipStream_t)0));
  k_collate_size<<<grid, 256>>>(n_rec, d_key2, d_off, d_size);
  STAGE_HIP(hipGetLastError());
  tb = scan_b;
  STAGE_HIP(rocprim::exclusive_scan(t_tmp.p, tb, d_size, d_pos, (int64_t)0, n, rocprim::plus<int64_t>(), (hipStream_t)0));
  STAGE_HIP(clock.mark());
  // the last record's offset and length bound every write of the gather: checked before it runs
  int64_t h_last[2] = {0, 0};
  STAGE_HIP(hipMemcpyAsync(&h_last[0], d_pos + (n - 1), 8, hipMemcpyDeviceToHost, 0));
  STAGE_HIP(hipMemcpyAsync(&h_last[1], d_size + (n - 1), 8, hipMemcpyDeviceToHost, 0));
  STAGE_HIP(hipStreamSynchronize(0));
  if (h_last[0] + h_last[1] != total)
    return stage_fail(TSEM_ERR_HIP, "tsem_bam_collate: the output offsets end at " + std::to_string(h_last[0] + h_last[1]) + ", the records hold " +
                                      std::to_string(total) + " bytes");
  if (total / n_rec >= 1024)
    k_collate_gather<64><<<(unsigned)cdiv64(n_rec * 64, 256), 256>>>(n_rec, d_in, d_off, d_key2, d_pos, d_out);
  else
    k_collate_gather<16><<<(unsigned)cdiv64(n_rec * 16, 256), 256>>>(n_rec, d_in, d_off, d_key2, d_pos, d_out);
  STAGE_HIP(hipGetLastError());
  STAGE_HIP(clock.mark());
  std::vector<uint64_t> h_key(n);
  if (total) STAGE_HIP(hipMemcpyAsync(out, d_out, (size_t)total, hipMemcpyDeviceToHost, 0));
  STAGE_HIP(hipMemcpyAsync(h_key.data(), d_key2, n * 8, hipMemcpyDeviceToHost, 0));
  STAGE_HIP(hipMemcpyAsync(&h_word[1], d_names, 8, hipMemcpyDeviceToHost, 0));
  STAGE_HIP(clock.mark());
  STAGE_HIP(hipStreamSynchronize(0));
  for (size_t k = 0; k < n; ++k) order[k] = (int64_t)(h_key[k] & 0xFFFFFFFFull);
  *n_names = (int64_t)h_word[1];
  if (ms) {
    int64_t calls = 0;
    STAGE_HIP(clock.finish({0, 1, 2, 3, 4}));
    clock.read(0, ms, &calls);
  }
  return TSEM_OK;
}

}  // extern "C"
