// libtelescope_em.so, BAM unit: the device loader of `assign` (tsem_bam_*, include/telescope_em.h).  The host inflates the BGZF blocks,
// cuts the byte stream into chunks that begin on a record boundary and end on a bundle boundary (a bundle = the records of one query
// name in a row) and finds the record offsets (tsem_bam_scan, tsem_bam_scan.h); one call of tsem_bam_chunk then turns a chunk into
// per-bundle lists of (locus, alnscore, alnlen) with four kernels — integer work, one answer whatever the launch order:
//
// The stages' bodies are the __host__ __device__ functions of tsem_bam_stages.h; the kernels give each lane its index.
//
//   k_bam_decode    one lane per record: the fixed fields, "the name differs from the previous record's", the aux walk (AS from any
//                   integer type, the barcode / UMI Z tags) — bam_decode_record (tsem_bam_rec.h), the same code a host program runs.
//   k_bam_pair      one lane per bundle (the lane of its first record; the others leave at once): the fragment code SU SM PU PM PX from
//                   the first record and the pairing of loader._fragments.classify.  The PM mate cache is a Python dict: a list of record
//                   indices in insertion order in the bundle's own scratch slots, a popped entry leaves a hole, an equal key replaces the
//                   value in place.  Pairs are written into the bundle's own record slots (never more pairs than records).
//   k_bam_overlap   one lane per pair slot: the reference blocks of r1 and r2 straight from the CIGARs, merged on the fly
//                   (merge_blocks(., 1) over the stable two-way merge by block start), alnlen, alnscore, and for every merged block
//                   Annotation.intersect_blocks: two binary searches bound the candidates, the overlap is summed per locus in a table of
//                   8 (a pair that hits more marks its bundle for the host), the winner is the largest sum, the first inserted among
//                   equals, kept iff overlap > alnlen * overlap_threshold in double arithmetic.
//   k_bam_fragment  one lane per bundle: the mapped pairs grouped by locus in first-appearance order, per locus the first pair reaching
//                   the largest alnscore + alnlen, the loci stably ordered by alnscore descending; the fragment class and the range of
//                   alnscore over the mapped pairs.
//
// Every walk inside a record is bounded by the record's end; one that would leave it stops and lowers the call's status word to
// (record << 8 | code), so the first such record in file order is the one reported.  What these kernels do not reproduce exactly — a
// bundle above the record cap, more than 8 loci per pair, a value outside int32, a reference id outside the header's list — marks
// the bundle for the host (class 5), which runs the Python loader's own code on that bundle's bytes.
//
// The BAMs of `--updated_sam` (tsem_bam_edit.h holds the bodies) come from three more kernels, one lane per bundle or per output slot:
//
//   k_bam_rw_plan   one lane per bundle: which record each of the bundle's output slots writes (pair order, r1 then r2).
//   k_bam_rw_size   one lane per slot: other or tmp, PRI or SEC (the first pair of its locus reaching the largest alnscore + alnlen),
//                   and the record's new length: the aux walk that skips ZF / ZT / ZB plus the bytes of the new fields.
//                   k_bam_upd_size is its sibling of the update stage: the edit comes from the record's word.
//   k_bam_rw_write  one lane per slot, behind an exclusive scan of the lengths per stream (rocprim): the record's bytes, edited.
//
// A lane per record, not a wave: the aux walk that decides which bytes stay is serial, and a wave per record of about 260 B would run
// it on one lane while 63 wait, then copy four bytes per lane.  The lane's byte copy does not coalesce (64 lanes read 64 records);
// DESIGN.md 4.12 has the measured rate and why it does not matter next to the host's deflate.
#include "tsem_internal.h"
#include <rocprim/device/device_scan.hpp>
#include "tsem_bam_edit.h"
#include "tsem_bam_scan.h"

struct tsem_bam {
  int device = 0;
  int32_t n_ref = 0;
  int64_t n_iv = 0;
  int32_t *d_ref_lo = nullptr, *d_ref_hi = nullptr, *d_locus = nullptr;
  int64_t *d_starts = nullptr, *d_maxend = nullptr, *d_ends = nullptr;
  int8_t* d_strand = nullptr;
  uint8_t* d_bytes = nullptr; size_t cap_bytes = 0;
  int64_t* d_off = nullptr; int32_t* d_cols = nullptr; size_t cap_rec = 0;
  unsigned long long* d_status = nullptr;
  unsigned long long h_status = 0;                // (the word's host copy: it must outlive a call that fails behind the copy's launch)
  hipEvent_t ev[7] = {};
  bool have_ev = false;
  double ms[6] = {0, 0, 0, 0, 0, 0};             // host-to-device, decode, pair, overlap, fragment, device-to-host
  int64_t calls = 0;
  // ---- the rewriting of --updated_sam
  int32_t max_locus = -1;                         // the largest locus id of the annotation: the name table must reach it
  uint8_t* d_names = nullptr; int64_t* d_name_off = nullptr; int32_t n_loci = -1;   // tsem_bam_names (-1: none yet)
  int64_t chunk_n = -1;                           // records of the chunk the device holds (-1: none a rewrite may use)
  int64_t sized_n = -1;                           // slots of the last *_size call (-1: nothing to fetch)
  int64_t total_other = 0, total_tmp = 0;         // ... and the lengths of its streams
  bool sized_update = false;
  int32_t* d_rw = nullptr; int64_t* d_pos = nullptr; uint32_t* d_words = nullptr; size_t cap_rw = 0;
  void* d_scan = nullptr; size_t cap_scan = 0;
  uint8_t *d_other = nullptr, *d_tmp = nullptr; size_t cap_other = 0, cap_tmp = 0;
  double rw_ms[5] = {0, 0, 0, 0, 0};              // host-to-device, plan, size and scan, write, device-to-host
  int64_t rw_calls = 0;
};

// (file scope, not the unnamed namespace: a profile lists them as k_bam_decode, k_bam_pair, k_bam_overlap, k_bam_fragment)
__global__ __launch_bounds__(256) void k_bam_decode(int64_t N, const uint8_t* __restrict__ bytes, const int64_t* __restrict__ off,
                                                    int32_t btag, int32_t utag, BamCols C, unsigned long long* status) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < N) bam_decode_stage(i, bytes, off, btag, utag, C, status);
}
__global__ __launch_bounds__(256) void k_bam_pair(int64_t N, int32_t cap, BamCols C) {
  const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s < N) bam_pair_stage(s, N, cap, C);
}
__global__ __launch_bounds__(256) void k_bam_overlap(int64_t N, const uint8_t* __restrict__ bytes, const int64_t* __restrict__ off, BamCols C,
                                                     BamAnnot A, int32_t stranded, int32_t first_f, int32_t last_f, double threshold,
                                                     unsigned long long* status) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < N) bam_overlap_stage(i, bytes, off, C, A, stranded, first_f, last_f, threshold, status);
}
__global__ __launch_bounds__(256) void k_bam_fragment(int64_t N, BamCols C) {
  const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s < N) bam_fragment_stage(s, C);
}

__global__ __launch_bounds__(256) void k_bam_rw_plan(int64_t N, BamCols C, BamRw W) {
  const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s < N) bam_rw_plan_stage(s, N, C, W);
}
__global__ __launch_bounds__(256) void k_bam_rw_size(int64_t N, const uint8_t* __restrict__ bytes, const int64_t* __restrict__ off, BamCols C,
                                                     BamNames nm, BamRw W, unsigned long long* status) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < N) bam_rw_size_stage(i, bytes, off, C, nm, W, status);
  if (i == N) { W.pos_other[N] = 0; W.pos_tmp[N] = 0; }       // (the scan's last element: the stream's length)
}
__global__ __launch_bounds__(256) void k_bam_upd_size(int64_t N, const uint8_t* __restrict__ bytes, const int64_t* __restrict__ off,
                                                      const uint32_t* __restrict__ words, BamRw W, unsigned long long* status) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < N) bam_upd_size_stage(i, bytes, off, words, W, status);
  if (i == N) { W.pos_other[N] = 0; W.pos_tmp[N] = 0; }
}
__global__ __launch_bounds__(256) void k_bam_rw_write(int64_t N, const uint8_t* __restrict__ bytes, const int64_t* __restrict__ off, BamCols C,
                                                      BamNames nm, const uint32_t* __restrict__ words, BamRw W, uint8_t* __restrict__ other,
                                                      uint8_t* __restrict__ tmp) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < N) bam_rw_write_stage(i, bytes, off, C, nm, words, W, other, tmp);
}

namespace {

int bam_fail(int rc, const std::string& msg) { g_create_err = msg; return rc; }
#define BAM_HIP(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) return bam_fail(TSEM_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(e_)); } while (0)

template <typename T>
int bam_upload(T** d, const T* h, size_t n) {
  if (hipMalloc((void**)d, std::max<size_t>(1, n) * sizeof(T)) != hipSuccess) { *d = nullptr; return bam_fail(TSEM_ERR_NOMEM, "tsem_bam_open: hipMalloc failed"); }
  if (n) BAM_HIP(hipMemcpy(*d, h, n * sizeof(T), hipMemcpyHostToDevice));
  return TSEM_OK;
}

}  // namespace

extern "C" {

int tsem_bam_scan(const uint8_t* bytes, int64_t n_bytes, int64_t* rec_off, int64_t cap, int64_t* n_rec, int64_t* consumed) {
  if (n_bytes < 0 || cap < 0 || (!bytes && n_bytes) || !rec_off || !n_rec || !consumed)
    return bam_fail(TSEM_ERR_ARG, "tsem_bam_scan: NULL pointer or negative size");
  char msg[200];
  if (tsem_bam_scan_chain(bytes, n_bytes, rec_off, cap, n_rec, consumed, msg, sizeof msg)) return bam_fail(TSEM_ERR_ARG, msg);
  return TSEM_OK;
}

int tsem_bam_close(tsem_bam* b) {
  if (!b) return TSEM_OK;
  (void)hipSetDevice(b->device);
  dfree(b->d_ref_lo); dfree(b->d_ref_hi); dfree(b->d_locus); dfree(b->d_starts); dfree(b->d_maxend); dfree(b->d_ends); dfree(b->d_strand);
  dfree(b->d_bytes); dfree(b->d_off); dfree(b->d_cols); dfree(b->d_status);
  dfree(b->d_names); dfree(b->d_name_off); dfree(b->d_rw); dfree(b->d_pos); dfree(b->d_words); dfree(b->d_scan); dfree(b->d_other); dfree(b->d_tmp);
  if (b->have_ev) for (hipEvent_t& e : b->ev) (void)hipEventDestroy(e);
  delete b;
  return TSEM_OK;
}

int tsem_bam_open(tsem_bam** out, int device, int32_t n_ref, const int32_t* ref_lo, const int32_t* ref_hi, int64_t n_iv,
                  const int64_t* starts, const int64_t* maxend, const int64_t* ends, const int32_t* locus, const int8_t* strand) {
  if (!out) return bam_fail(TSEM_ERR_ARG, "tsem_bam_open: out is NULL");
  *out = nullptr;
  if (n_ref < 0 || n_iv < 0 || n_iv >= (int64_t)INT32_MAX) return bam_fail(TSEM_ERR_ARG, "tsem_bam_open: n_ref or n_intervals out of range");
  if ((n_ref && (!ref_lo || !ref_hi)) || (n_iv && (!starts || !maxend || !ends || !locus || !strand)))
    return bam_fail(TSEM_ERR_ARG, "tsem_bam_open: NULL array");
  for (int32_t r = 0; r < n_ref; ++r)
    if (ref_lo[r] < 0 || ref_hi[r] < ref_lo[r] || (int64_t)ref_hi[r] > n_iv)
      return bam_fail(TSEM_ERR_ARG, "tsem_bam_open: reference " + std::to_string(r) + " has an interval range outside [0, n_intervals]");
  for (int32_t r = 0; r < n_ref; ++r)
    for (int32_t j = ref_lo[r]; j + 1 < ref_hi[r]; ++j)
      if (starts[j + 1] < starts[j] || maxend[j + 1] < maxend[j])
        return bam_fail(TSEM_ERR_ARG, "tsem_bam_open: starts / maxend of reference " + std::to_string(r) + " do not ascend");
  if (hipSetDevice(device) != hipSuccess) return bam_fail(TSEM_ERR_HIP, "hipSetDevice failed (no usable HIP device)");
  tsem_bam* b = new tsem_bam;
  b->device = device; b->n_ref = n_ref; b->n_iv = n_iv;
  for (int64_t j = 0; j < n_iv; ++j) b->max_locus = std::max(b->max_locus, locus[j]);
  int rc = bam_upload(&b->d_ref_lo, ref_lo, (size_t)n_ref);
  if (!rc) rc = bam_upload(&b->d_ref_hi, ref_hi, (size_t)n_ref);
  if (!rc) rc = bam_upload(&b->d_starts, starts, (size_t)n_iv);
  if (!rc) rc = bam_upload(&b->d_maxend, maxend, (size_t)n_iv);
  if (!rc) rc = bam_upload(&b->d_ends, ends, (size_t)n_iv);
  if (!rc) rc = bam_upload(&b->d_locus, locus, (size_t)n_iv);
  if (!rc) rc = bam_upload(&b->d_strand, strand, (size_t)n_iv);
  if (!rc && hipMalloc((void**)&b->d_status, 8) != hipSuccess) { b->d_status = nullptr; rc = bam_fail(TSEM_ERR_NOMEM, "tsem_bam_open: hipMalloc failed"); }
  if (!rc) {
    for (hipEvent_t& e : b->ev)
      if (hipEventCreate(&e) != hipSuccess) rc = bam_fail(TSEM_ERR_HIP, "tsem_bam_open: hipEventCreate failed");
    b->have_ev = rc == TSEM_OK;
  }
  if (rc) { tsem_bam_close(b); return rc; }
  *out = b;
  return TSEM_OK;
}

int tsem_bam_chunk(tsem_bam* b, const uint8_t* bytes, int64_t n_bytes, const int64_t* rec_off, int64_t n_rec, int32_t barcode_tag,
                   int32_t umi_tag, int32_t run_stranded, int32_t first_f, int32_t last_f, double overlap_threshold, int32_t record_cap,
                   int32_t* out, int64_t* status2) {
  if (!b) return bam_fail(TSEM_ERR_ARG, "tsem_bam_chunk: NULL handle");
  if (n_rec < 0 || n_bytes < 0 || n_rec >= (int64_t)INT32_MAX || !rec_off || !status2 || (n_rec && (!bytes || !out)))
    return bam_fail(TSEM_ERR_ARG, "tsem_bam_chunk: NULL pointer, negative size or more than 2^31 - 2 records");
  if (record_cap < 1) return bam_fail(TSEM_ERR_ARG, "tsem_bam_chunk: record_cap must be >= 1");
  // the offsets bound every read of the kernels: checked here, before the device sees them
  if (rec_off[0] < 0 || rec_off[n_rec] > n_bytes) return bam_fail(TSEM_ERR_ARG, "tsem_bam_chunk: rec_off leaves the chunk");
  for (int64_t i = 0; i < n_rec; ++i)
    if (rec_off[i + 1] - rec_off[i] < 36 || rec_off[i + 1] - rec_off[i] > (int64_t)INT32_MAX)
      return bam_fail(TSEM_ERR_ARG, "tsem_bam_chunk: record " + std::to_string(i) + " is shorter than 36 bytes or longer than 2^31 - 1 (rec_off must ascend)");
  status2[0] = 0; status2[1] = -1;
  b->chunk_n = -1; b->sized_n = -1;
  if (n_rec == 0) return TSEM_OK;
  BAM_HIP(hipSetDevice(b->device));
  const size_t nb = (size_t)rec_off[n_rec];
  if (nb > b->cap_bytes) {
    dfree(b->d_bytes); b->cap_bytes = 0;
    if (hipMalloc((void**)&b->d_bytes, nb + nb / 4) != hipSuccess) { b->d_bytes = nullptr; return bam_fail(TSEM_ERR_NOMEM, "tsem_bam_chunk: hipMalloc(" + std::to_string(nb + nb / 4) + " B) failed"); }
    b->cap_bytes = nb + nb / 4;
  }
  if ((size_t)n_rec > b->cap_rec) {
    dfree(b->d_off); dfree(b->d_cols); b->cap_rec = 0;
    const size_t cr = (size_t)n_rec + (size_t)n_rec / 4;
    if (hipMalloc((void**)&b->d_off, (cr + 1) * 8) != hipSuccess) { b->d_off = nullptr; return bam_fail(TSEM_ERR_NOMEM, "tsem_bam_chunk: hipMalloc failed"); }
    if (hipMalloc((void**)&b->d_cols, cr * 4 * TSEM_BAM_COLS) != hipSuccess) { b->d_cols = nullptr; return bam_fail(TSEM_ERR_NOMEM, "tsem_bam_chunk: hipMalloc failed"); }
    b->cap_rec = cr;
  }
  const unsigned long long none = ~0ull;
  unsigned long long& st = b->h_status;
  st = none;
  BamCols C{b->d_cols, n_rec};
  BamAnnot A{b->n_ref, b->d_ref_lo, b->d_ref_hi, b->d_locus, b->d_starts, b->d_maxend, b->d_ends, b->d_strand};
  const int grid = cdiv64(n_rec, 256);
  BAM_HIP(hipEventRecord(b->ev[0], 0));
  BAM_HIP(hipMemcpyAsync(b->d_bytes, bytes, nb, hipMemcpyHostToDevice, 0));
  BAM_HIP(hipMemcpyAsync(b->d_off, rec_off, (size_t)(n_rec + 1) * 8, hipMemcpyHostToDevice, 0));
  BAM_HIP(hipMemsetAsync(b->d_status, 0xFF, 8, 0));
  BAM_HIP(hipEventRecord(b->ev[1], 0));
  k_bam_decode<<<grid, 256>>>(n_rec, b->d_bytes, b->d_off, barcode_tag, umi_tag, C, b->d_status);
  BAM_HIP(hipGetLastError());
  BAM_HIP(hipEventRecord(b->ev[2], 0));
  k_bam_pair<<<grid, 256>>>(n_rec, record_cap, C);
  BAM_HIP(hipGetLastError());
  BAM_HIP(hipEventRecord(b->ev[3], 0));
  k_bam_overlap<<<grid, 256>>>(n_rec, b->d_bytes, b->d_off, C, A, run_stranded, first_f, last_f, overlap_threshold, b->d_status);
  BAM_HIP(hipGetLastError());
  BAM_HIP(hipEventRecord(b->ev[4], 0));
  k_bam_fragment<<<grid, 256>>>(n_rec, C);
  BAM_HIP(hipGetLastError());
  BAM_HIP(hipEventRecord(b->ev[5], 0));
  BAM_HIP(hipMemcpyAsync(out, b->d_cols, (size_t)n_rec * 4 * TSEM_BAM_COLS, hipMemcpyDeviceToHost, 0));
  BAM_HIP(hipMemcpyAsync(&st, b->d_status, 8, hipMemcpyDeviceToHost, 0));
  BAM_HIP(hipEventRecord(b->ev[6], 0));
  BAM_HIP(hipStreamSynchronize(0));
  for (int k = 0; k < 6; ++k) {
    float ms = 0.f;
    BAM_HIP(hipEventElapsedTime(&ms, b->ev[k], b->ev[k + 1]));
    b->ms[k] += ms;
  }
  ++b->calls;
  if (st != none) { status2[0] = (int64_t)(st & 0xFF); status2[1] = (int64_t)(st >> 8); }
  else b->chunk_n = n_rec;
  return TSEM_OK;
}

int tsem_bam_names(tsem_bam* b, const uint8_t* bytes, const int64_t* off, int32_t n_names) {
  if (!b) return bam_fail(TSEM_ERR_ARG, "tsem_bam_names: NULL handle");
  if (n_names < 1 || !off) return bam_fail(TSEM_ERR_ARG, "tsem_bam_names: no offsets, or fewer than one name (the last one is the no_feature_key)");
  if ((int64_t)n_names - 1 <= (int64_t)b->max_locus)
    return bam_fail(TSEM_ERR_ARG, "tsem_bam_names: " + std::to_string(n_names - 1) + " locus names, the annotation's locus ids reach " + std::to_string(b->max_locus));
  if (off[0] != 0) return bam_fail(TSEM_ERR_ARG, "tsem_bam_names: off[0] must be 0");
  for (int32_t j = 0; j < n_names; ++j)
    if (off[j + 1] < off[j]) return bam_fail(TSEM_ERR_ARG, "tsem_bam_names: the offsets of name " + std::to_string(j) + " descend");
  if (off[n_names] && !bytes) return bam_fail(TSEM_ERR_ARG, "tsem_bam_names: NULL bytes");
  BAM_HIP(hipSetDevice(b->device));
  dfree(b->d_names); dfree(b->d_name_off); b->n_loci = -1;
  int rc = bam_upload(&b->d_names, bytes, (size_t)off[n_names]);
  if (!rc) rc = bam_upload(&b->d_name_off, off, (size_t)n_names + 1);
  if (rc) return rc;
  b->n_loci = n_names - 1;
  return TSEM_OK;
}

namespace {

// the slot arrays of n slots, and the scan's scratch
int bam_rw_reserve(tsem_bam* b, int64_t n) {
  if ((size_t)n > b->cap_rw) {
    dfree(b->d_rw); dfree(b->d_pos); dfree(b->d_words); b->cap_rw = 0;
    const size_t cr = (size_t)n + (size_t)n / 4;
    if (hipMalloc((void**)&b->d_rw, cr * 12) != hipSuccess) { b->d_rw = nullptr; return bam_fail(TSEM_ERR_NOMEM, "tsem_bam rewrite: hipMalloc failed"); }
    if (hipMalloc((void**)&b->d_pos, (cr + 1) * 16) != hipSuccess) { b->d_pos = nullptr; return bam_fail(TSEM_ERR_NOMEM, "tsem_bam rewrite: hipMalloc failed"); }
    if (hipMalloc((void**)&b->d_words, cr * 4) != hipSuccess) { b->d_words = nullptr; return bam_fail(TSEM_ERR_NOMEM, "tsem_bam rewrite: hipMalloc failed"); }
    b->cap_rw = cr;
  }
  size_t tb = 0;
  BAM_HIP(rocprim::exclusive_scan(nullptr, tb, (int64_t*)nullptr, (int64_t*)nullptr, (int64_t)0, (size_t)n + 1, rocprim::plus<int64_t>(), 0));
  if (tb > b->cap_scan) {
    dfree(b->d_scan); b->cap_scan = 0;
    if (hipMalloc(&b->d_scan, tb) != hipSuccess) { b->d_scan = nullptr; return bam_fail(TSEM_ERR_NOMEM, "tsem_bam rewrite: hipMalloc failed"); }
    b->cap_scan = tb;
  }
  return TSEM_OK;
}
BamRw bam_rw_of(tsem_bam* b, int64_t n) {
  return BamRw{b->d_rw, b->d_rw + b->cap_rw, b->d_rw + 2 * b->cap_rw, b->d_pos, b->d_pos + n + 1};
}
// behind the size kernel: both scans, the positions and the status word to the host
int bam_rw_scan_fetch(tsem_bam* b, int64_t n, int64_t* pos_other, int64_t* pos_tmp, int64_t* status2) {
  BamRw W = bam_rw_of(b, n);
  size_t tb = b->cap_scan;
  BAM_HIP(rocprim::exclusive_scan(b->d_scan, tb, W.pos_other, W.pos_other, (int64_t)0, (size_t)n + 1, rocprim::plus<int64_t>(), 0));
  tb = b->cap_scan;
  BAM_HIP(rocprim::exclusive_scan(b->d_scan, tb, W.pos_tmp, W.pos_tmp, (int64_t)0, (size_t)n + 1, rocprim::plus<int64_t>(), 0));
  BAM_HIP(hipEventRecord(b->ev[3], 0));
  if (pos_other) BAM_HIP(hipMemcpyAsync(pos_other, W.pos_other, (size_t)(n + 1) * 8, hipMemcpyDeviceToHost, 0));
  BAM_HIP(hipMemcpyAsync(pos_tmp, W.pos_tmp, (size_t)(n + 1) * 8, hipMemcpyDeviceToHost, 0));
  BAM_HIP(hipMemcpyAsync(&b->h_status, b->d_status, 8, hipMemcpyDeviceToHost, 0));
  BAM_HIP(hipEventRecord(b->ev[4], 0));
  BAM_HIP(hipStreamSynchronize(0));
  static const int slot[4] = {0, 1, 2, 4};                    // ev[k] .. ev[k + 1]: h2d, plan, size and scan, d2h
  for (int k = 0; k < 4; ++k) {
    float ms = 0.f;
    BAM_HIP(hipEventElapsedTime(&ms, b->ev[k], b->ev[k + 1]));
    b->rw_ms[slot[k]] += ms;
  }
  ++b->rw_calls;
  if (b->h_status != ~0ull) { status2[0] = (int64_t)(b->h_status & 0xFF); status2[1] = (int64_t)(b->h_status >> 8); return TSEM_OK; }
  b->sized_n = n; b->total_tmp = pos_tmp[n]; b->total_other = pos_other ? pos_other[n] : 0;
  return TSEM_OK;
}

}  // namespace

int tsem_bam_rewrite_size(tsem_bam* b, int64_t* pos_other, int64_t* pos_tmp, int64_t* status2) {
  if (!b || !pos_other || !pos_tmp || !status2) return bam_fail(TSEM_ERR_ARG, "tsem_bam_rewrite_size: NULL pointer");
  status2[0] = 0; status2[1] = -1;
  b->sized_n = -1;
  if (b->chunk_n < 1) return bam_fail(TSEM_ERR_ARG, "tsem_bam_rewrite_size: no chunk on the device (tsem_bam_chunk with status 0 comes first)");
  if (b->n_loci < 0) return bam_fail(TSEM_ERR_ARG, "tsem_bam_rewrite_size: no names (tsem_bam_names comes first)");
  const int64_t n = b->chunk_n;
  BAM_HIP(hipSetDevice(b->device));
  if (int rc = bam_rw_reserve(b, n)) return rc;
  BamCols C{b->d_cols, n};
  BamRw W = bam_rw_of(b, n);
  BamNames nm{b->d_names, b->d_name_off, b->n_loci};
  b->sized_update = false;
  BAM_HIP(hipEventRecord(b->ev[0], 0));
  BAM_HIP(hipMemsetAsync(b->d_status, 0xFF, 8, 0));
  BAM_HIP(hipEventRecord(b->ev[1], 0));
  k_bam_rw_plan<<<cdiv64(n, 256), 256>>>(n, C, W);
  BAM_HIP(hipGetLastError());
  BAM_HIP(hipEventRecord(b->ev[2], 0));
  k_bam_rw_size<<<cdiv64(n + 1, 256), 256>>>(n, b->d_bytes, b->d_off, C, nm, W, b->d_status);
  BAM_HIP(hipGetLastError());
  return bam_rw_scan_fetch(b, n, pos_other, pos_tmp, status2);
}

int tsem_bam_update_size(tsem_bam* b, const uint8_t* bytes, int64_t n_bytes, const int64_t* rec_off, int64_t n_rec, const uint32_t* words,
                         int64_t* pos, int64_t* status2) {
  if (!b) return bam_fail(TSEM_ERR_ARG, "tsem_bam_update_size: NULL handle");
  if (n_rec < 0 || n_bytes < 0 || n_rec >= (int64_t)INT32_MAX || !rec_off || !status2 || !pos || (n_rec && (!bytes || !words)))
    return bam_fail(TSEM_ERR_ARG, "tsem_bam_update_size: NULL pointer, negative size or more than 2^31 - 2 records");
  if (rec_off[0] < 0 || rec_off[n_rec] > n_bytes) return bam_fail(TSEM_ERR_ARG, "tsem_bam_update_size: rec_off leaves the chunk");
  for (int64_t i = 0; i < n_rec; ++i)
    if (rec_off[i + 1] - rec_off[i] < 36 || rec_off[i + 1] - rec_off[i] > (int64_t)INT32_MAX)
      return bam_fail(TSEM_ERR_ARG, "tsem_bam_update_size: record " + std::to_string(i) + " is shorter than 36 bytes or longer than 2^31 - 1 (rec_off must ascend)");
  status2[0] = 0; status2[1] = -1;
  b->chunk_n = -1; b->sized_n = -1;
  pos[0] = 0;
  if (n_rec == 0) return TSEM_OK;
  BAM_HIP(hipSetDevice(b->device));
  const size_t nb = (size_t)rec_off[n_rec];
  if (nb > b->cap_bytes) {
    dfree(b->d_bytes); b->cap_bytes = 0;
    if (hipMalloc((void**)&b->d_bytes, nb + nb / 4) != hipSuccess) { b->d_bytes = nullptr; return bam_fail(TSEM_ERR_NOMEM, "tsem_bam_update_size: hipMalloc(" + std::to_string(nb + nb / 4) + " B) failed"); }
    b->cap_bytes = nb + nb / 4;
  }
  if ((size_t)n_rec > b->cap_rec) {                            // (d_cols is not used here, but one capacity covers both arrays)
    dfree(b->d_off); dfree(b->d_cols); b->cap_rec = 0;
    const size_t cr = (size_t)n_rec + (size_t)n_rec / 4;
    if (hipMalloc((void**)&b->d_off, (cr + 1) * 8) != hipSuccess) { b->d_off = nullptr; return bam_fail(TSEM_ERR_NOMEM, "tsem_bam_update_size: hipMalloc failed"); }
    if (hipMalloc((void**)&b->d_cols, cr * 4 * TSEM_BAM_COLS) != hipSuccess) { b->d_cols = nullptr; return bam_fail(TSEM_ERR_NOMEM, "tsem_bam_update_size: hipMalloc failed"); }
    b->cap_rec = cr;
  }
  if (int rc = bam_rw_reserve(b, n_rec)) return rc;
  BamRw W = bam_rw_of(b, n_rec);
  b->sized_update = true;
  BAM_HIP(hipEventRecord(b->ev[0], 0));
  BAM_HIP(hipMemcpyAsync(b->d_bytes, bytes, nb, hipMemcpyHostToDevice, 0));
  BAM_HIP(hipMemcpyAsync(b->d_off, rec_off, (size_t)(n_rec + 1) * 8, hipMemcpyHostToDevice, 0));
  BAM_HIP(hipMemcpyAsync(b->d_words, words, (size_t)n_rec * 4, hipMemcpyHostToDevice, 0));
  BAM_HIP(hipMemsetAsync(b->d_status, 0xFF, 8, 0));
  BAM_HIP(hipEventRecord(b->ev[1], 0));
  BAM_HIP(hipEventRecord(b->ev[2], 0));
  k_bam_upd_size<<<cdiv64(n_rec + 1, 256), 256>>>(n_rec, b->d_bytes, b->d_off, b->d_words, W, b->d_status);
  BAM_HIP(hipGetLastError());
  return bam_rw_scan_fetch(b, n_rec, nullptr, pos, status2);
}

int tsem_bam_rewrite_fetch(tsem_bam* b, uint8_t* other, int64_t n_other, uint8_t* tmp, int64_t n_tmp) {
  if (!b) return bam_fail(TSEM_ERR_ARG, "tsem_bam_rewrite_fetch: NULL handle");
  if (b->sized_n < 1) return bam_fail(TSEM_ERR_ARG, "tsem_bam_rewrite_fetch: nothing sized (tsem_bam_rewrite_size or tsem_bam_update_size with status 0 comes first)");
  if (n_other != b->total_other || n_tmp != b->total_tmp || (n_other && !other) || (n_tmp && !tmp))
    return bam_fail(TSEM_ERR_ARG, "tsem_bam_rewrite_fetch: the buffers must hold exactly " + std::to_string(b->total_other) + " and " +
                                  std::to_string(b->total_tmp) + " bytes");
  const int64_t n = b->sized_n;
  b->sized_n = -1;
  BAM_HIP(hipSetDevice(b->device));
  if ((size_t)n_other > b->cap_other) {
    dfree(b->d_other); b->cap_other = 0;
    if (hipMalloc((void**)&b->d_other, (size_t)n_other + (size_t)n_other / 4) != hipSuccess) { b->d_other = nullptr; return bam_fail(TSEM_ERR_NOMEM, "tsem_bam_rewrite_fetch: hipMalloc failed"); }
    b->cap_other = (size_t)n_other + (size_t)n_other / 4;
  }
  if ((size_t)n_tmp > b->cap_tmp) {
    dfree(b->d_tmp); b->cap_tmp = 0;
    if (hipMalloc((void**)&b->d_tmp, (size_t)n_tmp + (size_t)n_tmp / 4) != hipSuccess) { b->d_tmp = nullptr; return bam_fail(TSEM_ERR_NOMEM, "tsem_bam_rewrite_fetch: hipMalloc failed"); }
    b->cap_tmp = (size_t)n_tmp + (size_t)n_tmp / 4;
  }
  BamCols C{b->d_cols, n};
  BamNames nm{b->d_names, b->d_name_off, b->n_loci};
  BAM_HIP(hipEventRecord(b->ev[0], 0));
  k_bam_rw_write<<<cdiv64(n, 256), 256>>>(n, b->d_bytes, b->d_off, C, nm, b->d_words, bam_rw_of(b, n), b->d_other, b->d_tmp);
  BAM_HIP(hipGetLastError());
  BAM_HIP(hipEventRecord(b->ev[1], 0));
  if (n_other) BAM_HIP(hipMemcpyAsync(other, b->d_other, (size_t)n_other, hipMemcpyDeviceToHost, 0));
  if (n_tmp) BAM_HIP(hipMemcpyAsync(tmp, b->d_tmp, (size_t)n_tmp, hipMemcpyDeviceToHost, 0));
  BAM_HIP(hipEventRecord(b->ev[2], 0));
  BAM_HIP(hipStreamSynchronize(0));
  float ms = 0.f;
  BAM_HIP(hipEventElapsedTime(&ms, b->ev[0], b->ev[1])); b->rw_ms[3] += ms;
  BAM_HIP(hipEventElapsedTime(&ms, b->ev[1], b->ev[2])); b->rw_ms[4] += ms;
  return TSEM_OK;
}

int tsem_bam_rewrite_slots(tsem_bam* b, int32_t* kind, int32_t* pair, int64_t n) {
  if (!b || !kind || !pair) return bam_fail(TSEM_ERR_ARG, "tsem_bam_rewrite_slots: NULL pointer");
  if (b->sized_n < 1 || n != b->sized_n) return bam_fail(TSEM_ERR_ARG, "tsem_bam_rewrite_slots: n is not the slot count of the last size call");
  BAM_HIP(hipSetDevice(b->device));
  const BamRw W = bam_rw_of(b, n);
  BAM_HIP(hipMemcpy(kind, W.kind, (size_t)n * 4, hipMemcpyDeviceToHost));
  BAM_HIP(hipMemcpy(pair, W.pair, (size_t)n * 4, hipMemcpyDeviceToHost));
  return TSEM_OK;
}

int tsem_bam_rewrite_times(tsem_bam* b, int reset, double* ms5, int64_t* calls) {
  if (!b || !ms5 || !calls) return bam_fail(TSEM_ERR_ARG, "tsem_bam_rewrite_times: NULL pointer");
  for (int k = 0; k < 5; ++k) ms5[k] = b->rw_ms[k];
  *calls = b->rw_calls;
  if (reset) { for (double& m : b->rw_ms) m = 0; b->rw_calls = 0; }
  return TSEM_OK;
}

int tsem_bam_times(tsem_bam* b, int reset, double* ms6, int64_t* calls) {
  if (!b || !ms6 || !calls) return bam_fail(TSEM_ERR_ARG, "tsem_bam_times: NULL pointer");
  for (int k = 0; k < 6; ++k) ms6[k] = b->ms[k];
  *calls = b->calls;
  if (reset) { for (double& m : b->ms) m = 0; b->calls = 0; }
  return TSEM_OK;
}

}  // extern "C"
