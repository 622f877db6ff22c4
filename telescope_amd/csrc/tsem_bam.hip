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
#include "tsem_stage.h"

enum { CK_H2D, CK_DECODE, CK_PAIR, CK_OVERLAP, CK_FRAGMENT, CK_D2H, CK_N };      // the stages of tsem_bam_times
enum { RW_H2D, RW_PLAN, RW_SIZE, RW_WRITE, RW_D2H, RW_N };                      // ... of tsem_bam_rewrite_times (size: with both scans)

struct tsem_bam {
  int device = 0;
  int32_t n_ref = 0;
  int64_t n_iv = 0;
  DevBuf<int32_t> ref_lo, ref_hi, locus;          // the annotation (tsem_bam_open)
  DevBuf<int64_t> starts, maxend, ends;
  DevBuf<int8_t> strand;
  DevBuf<uint8_t> bytes;                          // the chunk: its records, their offsets [n + 1], the result matrix
  DevBuf<int64_t> off;
  DevBuf<int32_t> cols;
  StatusWord status;
  StageClock<CK_N + 1, CK_N> clock;
  // ---- the rewriting of --updated_sam
  int32_t max_locus = -1;                         // the largest locus id of the annotation: the name table must reach it
  DevBuf<uint8_t> names; DevBuf<int64_t> name_off; int32_t n_loci = -1;   // tsem_bam_names (-1: none yet)
  int64_t chunk_n = -1;                           // records of the chunk the device holds (-1: none a rewrite may use)
  int64_t sized_n = -1;                           // slots of the last *_size call (-1: nothing to fetch)
  int64_t total_other = 0, total_tmp = 0;         // ... and the lengths of its streams
  bool sized_update = false;
  DevBuf<int32_t> rw;                             // of n slots: rec, pair, kind [n] each (bam_rw_of)
  DevBuf<int64_t> pos;                            //   ... and both streams' lengths, then offsets [n + 1] each
  DevBuf<uint32_t> words;
  DevBuf<uint8_t> scan, other, tmp;               // rocprim's scratch; the streams of the fetch
  StageClock<5, RW_N> rw_clock;                   // (one timing over the sizing call and its fetch; the sizing calls are counted)
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

// an array that stays as it is until the handle closes (the annotation) or is replaced (the names)
template <typename T>
int bam_upload(const char* fn, DevBuf<T>& d, const T* h, size_t n, const char* what) {
  if (int rc = d.alloc(n, what, fn)) return rc;
  if (n) STAGE_HIP(hipMemcpy(d.p, h, n * sizeof(T), hipMemcpyHostToDevice));
  return TSEM_OK;
}

}  // namespace

extern "C" {

int tsem_bam_scan(const uint8_t* bytes, int64_t n_bytes, int64_t* rec_off, int64_t cap, int64_t* n_rec, int64_t* consumed) {
  if (n_bytes < 0 || cap < 0 || (!bytes && n_bytes) || !rec_off || !n_rec || !consumed)
    return stage_fail(TSEM_ERR_ARG, "tsem_bam_scan: NULL pointer or negative size");
  char msg[200];
  if (tsem_bam_scan_chain(bytes, n_bytes, rec_off, cap, n_rec, consumed, msg, sizeof msg)) return stage_fail(TSEM_ERR_ARG, msg);
  return TSEM_OK;
}

int tsem_bam_close(tsem_bam* b) {
  if (!b) return TSEM_OK;
  (void)hipSetDevice(b->device);
  delete b;                                       // (every buffer and event is a member that releases itself)
  return TSEM_OK;
}

int tsem_bam_open(tsem_bam** out, int device, int32_t n_ref, const int32_t* ref_lo, const int32_t* ref_hi, int64_t n_iv,
                  const int64_t* starts, const int64_t* maxend, const int64_t* ends, const int32_t* locus, const int8_t* strand) {
  if (!out) return stage_fail(TSEM_ERR_ARG, "tsem_bam_open: out is NULL");
  *out = nullptr;
  if (n_ref < 0 || n_iv < 0 || n_iv >= (int64_t)INT32_MAX) return stage_fail(TSEM_ERR_ARG, "tsem_bam_open: n_ref or n_intervals out of range");
  if ((n_ref && (!ref_lo || !ref_hi)) || (n_iv && (!starts || !maxend || !ends || !locus || !strand)))
    return stage_fail(TSEM_ERR_ARG, "tsem_bam_open: NULL array");
  for (int32_t r = 0; r < n_ref; ++r)
    if (ref_lo[r] < 0 || ref_hi[r] < ref_lo[r] || (int64_t)ref_hi[r] > n_iv)
      return stage_fail(TSEM_ERR_ARG, "tsem_bam_open: reference " + std::to_string(r) + " has an interval range outside [0, n_intervals]");
  for (int32_t r = 0; r < n_ref; ++r)
    for (int32_t j = ref_lo[r]; j + 1 < ref_hi[r]; ++j)
      if (starts[j + 1] < starts[j] || maxend[j + 1] < maxend[j])
        return stage_fail(TSEM_ERR_ARG, "tsem_bam_open: starts / maxend of reference " + std::to_string(r) + " do not ascend");
  if (hipSetDevice(device) != hipSuccess) return stage_fail(TSEM_ERR_HIP, "hipSetDevice failed (no usable HIP device)");
  tsem_bam* b = new tsem_bam;
  b->device = device; b->n_ref = n_ref; b->n_iv = n_iv;
  for (int64_t j = 0; j < n_iv; ++j) b->max_locus = std::max(b->max_locus, locus[j]);
  const char* fn = "tsem_bam_open";
  int rc = bam_upload(fn, b->ref_lo, ref_lo, (size_t)n_ref, "annotation");
  if (!rc) rc = bam_upload(fn, b->ref_hi, ref_hi, (size_t)n_ref, "annotation");
  if (!rc) rc = bam_upload(fn, b->starts, starts, (size_t)n_iv, "annotation");
  if (!rc) rc = bam_upload(fn, b->maxend, maxend, (size_t)n_iv, "annotation");
  if (!rc) rc = bam_upload(fn, b->ends, ends, (size_t)n_iv, "annotation");
  if (!rc) rc = bam_upload(fn, b->locus, locus, (size_t)n_iv, "annotation");
  if (!rc) rc = bam_upload(fn, b->strand, strand, (size_t)n_iv, "annotation");
  if (!rc) rc = b->status.create(fn);
  if (!rc && (b->clock.create() != hipSuccess || b->rw_clock.create() != hipSuccess)) rc = stage_fail(TSEM_ERR_HIP, "tsem_bam_open: hipEventCreate failed");
  if (rc) { tsem_bam_close(b); return rc; }
  *out = b;
  return TSEM_OK;
}

int tsem_bam_chunk(tsem_bam* b, const uint8_t* bytes, int64_t n_bytes, const int64_t* rec_off, int64_t n_rec, int32_t barcode_tag,
                   int32_t umi_tag, int32_t run_stranded, int32_t first_f, int32_t last_f, double overlap_threshold, int32_t record_cap,
                   int32_t* out, int64_t* status2) {
  if (!b) return stage_fail(TSEM_ERR_ARG, "tsem_bam_chunk: NULL handle");
  if (n_rec < 0 || n_bytes < 0 || n_rec >= (int64_t)INT32_MAX || !rec_off || !status2 || (n_rec && (!bytes || !out)))
    return stage_fail(TSEM_ERR_ARG, "tsem_bam_chunk: NULL pointer, negative size or more than 2^31 - 2 records");
  if (record_cap < 1) return stage_fail(TSEM_ERR_ARG, "tsem_bam_chunk: record_cap must be >= 1");
  if (int rc = stage_check_rec_off("tsem_bam_chunk", rec_off, n_rec, n_bytes)) return rc;
  status2[0] = 0; status2[1] = -1;
  b->chunk_n = -1; b->sized_n = -1;
  if (n_rec == 0) return TSEM_OK;
  STAGE_HIP(hipSetDevice(b->device));
  if (int rc = b->cols.reserve((size_t)n_rec * TSEM_BAM_COLS, "result matrix", "tsem_bam_chunk")) return rc;
  if (int rc = stage_upload_chunk("tsem_bam_chunk", b->bytes, b->off, bytes, rec_off, n_rec, b->clock)) return rc;
  BamCols C{b->cols.p, n_rec};
  BamAnnot A{b->n_ref, b->ref_lo.p, b->ref_hi.p, b->locus.p, b->starts.p, b->maxend.p, b->ends.p, b->strand.p};
  const int grid = cdiv64(n_rec, 256);
  STAGE_HIP(b->status.arm());
  STAGE_HIP(b->clock.mark());
  k_bam_decode<<<grid, 256>>>(n_rec, b->bytes.p, b->off.p, barcode_tag, umi_tag, C, b->status.d.p);
  STAGE_HIP(hipGetLastError());
  STAGE_HIP(b->clock.mark());
  k_bam_pair<<<grid, 256>>>(n_rec, record_cap, C);
  STAGE_HIP(hipGetLastError());
  STAGE_HIP(b->clock.mark());
  k_bam_overlap<<<grid, 256>>>(n_rec, b->bytes.p, b->off.p, C, A, run_stranded, first_f, last_f, overlap_threshold, b->status.d.p);
  STAGE_HIP(hipGetLastError());
  STAGE_HIP(b->clock.mark());
  k_bam_fragment<<<grid, 256>>>(n_rec, C);
  STAGE_HIP(hipGetLastError());
  STAGE_HIP(b->clock.mark());
  STAGE_HIP(hipMemcpyAsync(out, b->cols.p, (size_t)n_rec * 4 * TSEM_BAM_COLS, hipMemcpyDeviceToHost, 0));
  STAGE_HIP(b->status.fetch());
  STAGE_HIP(b->clock.mark());
  STAGE_HIP(hipStreamSynchronize(0));
  STAGE_HIP(b->clock.finish({CK_H2D, CK_DECODE, CK_PAIR, CK_OVERLAP, CK_FRAGMENT, CK_D2H}));
  if (!b->status.decode(status2)) b->chunk_n = n_rec;
  return TSEM_OK;
}

int tsem_bam_names(tsem_bam* b, const uint8_t* bytes, const int64_t* off, int32_t n_names) {
  if (!b) return stage_fail(TSEM_ERR_ARG, "tsem_bam_names: NULL handle");
  if (n_names < 1 || !off) return stage_fail(TSEM_ERR_ARG, "tsem_bam_names: no offsets, or fewer than one name (the last one is the no_feature_key)");
  if ((int64_t)n_names - 1 <= (int64_t)b->max_locus)
    return stage_fail(TSEM_ERR_ARG, "tsem_bam_names: " + std::to_string(n_names - 1) + " locus names, the annotation's locus ids reach " + std::to_string(b->max_locus));
  if (off[0] != 0) return stage_fail(TSEM_ERR_ARG, "tsem_bam_names: off[0] must be 0");
  for (int32_t j = 0; j < n_names; ++j)
    if (off[j + 1] < off[j]) return stage_fail(TSEM_ERR_ARG, "tsem_bam_names: the offsets of name " + std::to_string(j) + " descend");
  if (off[n_names] && !bytes) return stage_fail(TSEM_ERR_ARG, "tsem_bam_names: NULL bytes");
  STAGE_HIP(hipSetDevice(b->device));
  b->n_loci = -1;
  int rc = bam_upload("tsem_bam_names", b->names, bytes, (size_t)off[n_names], "locus names");
  if (!rc) rc = bam_upload("tsem_bam_names", b->name_off, off, (size_t)n_names + 1, "locus names");
  if (rc) return rc;
  b->n_loci = n_names - 1;
  return TSEM_OK;
}

namespace {

// the slot arrays of n slots, and the scan's scratch
int bam_rw_reserve(tsem_bam* b, int64_t n) {
  const char* fn = "tsem_bam rewrite";
  if (int rc = b->rw.reserve(3 * (size_t)n, "slots", fn)) return rc;
  if (int rc = b->pos.reserve(2 * ((size_t)n + 1), "slot offsets", fn)) return rc;
  if (int rc = b->words.reserve((size_t)n, "slot words", fn)) return rc;
  size_t tb = 0;
  STAGE_HIP(rocprim::exclusive_scan(nullptr, tb, (int64_t*)nullptr, (int64_t*)nullptr, (int64_t)0, (size_t)n + 1, rocprim::plus<int64_t>(), 0));
  return b->scan.reserve(tb, "scan's storage", fn);
}
// (the arrays of a sizing call and of its fetch lie at the same places: both pass the same n, and only a sizing call reserves)
BamRw bam_rw_of(tsem_bam* b, int64_t n) { return BamRw{b->rw.p, b->rw.p + n, b->rw.p + 2 * n, b->pos.p, b->pos.p + n + 1}; }
// behind the size kernel: both scans, the positions and the status word to the host
int bam_rw_scan_fetch(tsem_bam* b, int64_t n, int64_t* pos_other, int64_t* pos_tmp, int64_t* status2) {
  BamRw W = bam_rw_of(b, n);
  size_t tb = b->scan.cap;
  STAGE_HIP(rocprim::exclusive_scan(b->scan.p, tb, W.pos_other, W.pos_other, (int64_t)0, (size_t)n + 1, rocprim::plus<int64_t>(), 0));
  tb = b->scan.cap;
  STAGE_HIP(rocprim::exclusive_scan(b->scan.p, tb, W.pos_tmp, W.pos_tmp, (int64_t)0, (size_t)n + 1, rocprim::plus<int64_t>(), 0));
  STAGE_HIP(b->rw_clock.mark());
  if (pos_other) STAGE_HIP(hipMemcpyAsync(pos_other, W.pos_other, (size_t)(n + 1) * 8, hipMemcpyDeviceToHost, 0));
  STAGE_HIP(hipMemcpyAsync(pos_tmp, W.pos_tmp, (size_t)(n + 1) * 8, hipMemcpyDeviceToHost, 0));
  STAGE_HIP(b->status.fetch());
  STAGE_HIP(b->rw_clock.mark());
  STAGE_HIP(hipStreamSynchronize(0));
  STAGE_HIP(b->rw_clock.finish({RW_H2D, RW_PLAN, RW_SIZE, RW_D2H}));
  if (b->status.decode(status2)) return TSEM_OK;
  b->sized_n = n; b->total_tmp = pos_tmp[n]; b->total_other = pos_other ? pos_other[n] : 0;
  return TSEM_OK;
}

}  // namespace

int tsem_bam_rewrite_size(tsem_bam* b, int64_t* pos_other, int64_t* pos_tmp, int64_t* status2) {
  if (!b || !pos_other || !pos_tmp || !status2) return stage_fail(TSEM_ERR_ARG, "tsem_bam_rewrite_size: NULL pointer");
  status2[0] = 0; status2[1] = -1;
  b->sized_n = -1;
  if (b->chunk_n < 1) return stage_fail(TSEM_ERR_ARG, "tsem_bam_rewrite_size: no chunk on the device (tsem_bam_chunk with status 0 comes first)");
  if (b->n_loci < 0) return stage_fail(TSEM_ERR_ARG, "tsem_bam_rewrite_size: no names (tsem_bam_names comes first)");
  const int64_t n = b->chunk_n;
  STAGE_HIP(hipSetDevice(b->device));
  if (int rc = bam_rw_reserve(b, n)) return rc;
  BamCols C{b->cols.p, n};
  BamRw W = bam_rw_of(b, n);
  BamNames nm{b->names.p, b->name_off.p, b->n_loci};
  b->sized_update = false;
  STAGE_HIP(b->rw_clock.begin());
  STAGE_HIP(b->status.arm());
  STAGE_HIP(b->rw_clock.mark());
  k_bam_rw_plan<<<cdiv64(n, 256), 256>>>(n, C, W);
  STAGE_HIP(hipGetLastError());
  STAGE_HIP(b->rw_clock.mark());
  k_bam_rw_size<<<cdiv64(n + 1, 256), 256>>>(n, b->bytes.p, b->off.p, C, nm, W, b->status.d.p);
  STAGE_HIP(hipGetLastError());
  return bam_rw_scan_fetch(b, n, pos_other, pos_tmp, status2);
}

int tsem_bam_update_size(tsem_bam* b, const uint8_t* bytes, int64_t n_bytes, const int64_t* rec_off, int64_t n_rec, const uint32_t* words,
                         int64_t* pos, int64_t* status2) {
  if (!b) return stage_fail(TSEM_ERR_ARG, "tsem_bam_update_size: NULL handle");
  if (n_rec < 0 || n_bytes < 0 || n_rec >= (int64_t)INT32_MAX || !rec_off || !status2 || !pos || (n_rec && (!bytes || !words)))
    return stage_fail(TSEM_ERR_ARG, "tsem_bam_update_size: NULL pointer, negative size or more than 2^31 - 2 records");
  if (int rc = stage_check_rec_off("tsem_bam_update_size", rec_off, n_rec, n_bytes)) return rc;
  status2[0] = 0; status2[1] = -1;
  b->chunk_n = -1; b->sized_n = -1;                            // (the chunk's bytes and offsets are overwritten below; its matrix is not used here)
  pos[0] = 0;
  if (n_rec == 0) return TSEM_OK;
  STAGE_HIP(hipSetDevice(b->device));
  if (int rc = bam_rw_reserve(b, n_rec)) return rc;
  if (int rc = stage_upload_chunk("tsem_bam_update_size", b->bytes, b->off, bytes, rec_off, n_rec, b->rw_clock)) return rc;
  BamRw W = bam_rw_of(b, n_rec);
  b->sized_update = true;
  STAGE_HIP(hipMemcpyAsync(b->words.p, words, (size_t)n_rec * 4, hipMemcpyHostToDevice, 0));
  STAGE_HIP(b->status.arm());
  STAGE_HIP(b->rw_clock.mark());
  STAGE_HIP(b->rw_clock.mark());                                 // (no plan stage: its slot gets the time between two events)
  k_bam_upd_size<<<cdiv64(n_rec + 1, 256), 256>>>(n_rec, b->bytes.p, b->off.p, b->words.p, W, b->status.d.p);
  STAGE_HIP(hipGetLastError());
  return bam_rw_scan_fetch(b, n_rec, nullptr, pos, status2);
}

int tsem_bam_rewrite_fetch(tsem_bam* b, uint8_t* other, int64_t n_other, uint8_t* tmp, int64_t n_tmp) {
  if (!b) return stage_fail(TSEM_ERR_ARG, "tsem_bam_rewrite_fetch: NULL handle");
  if (b->sized_n < 1) return stage_fail(TSEM_ERR_ARG, "tsem_bam_rewrite_fetch: nothing sized (tsem_bam_rewrite_size or tsem_bam_update_size with status 0 comes first)");
  if (n_other != b->total_other || n_tmp != b->total_tmp || (n_other && !other) || (n_tmp && !tmp))
    return stage_fail(TSEM_ERR_ARG, "tsem_bam_rewrite_fetch: the buffers must hold exactly " + std::to_string(b->total_other) + " and " +
                                  std::to_string(b->total_tmp) + " bytes");
  const int64_t n = b->sized_n;
  b->sized_n = -1;
  STAGE_HIP(hipSetDevice(b->device));
  if (int rc = b->other.reserve((size_t)n_other, "other stream", "tsem_bam_rewrite_fetch")) return rc;
  if (int rc = b->tmp.reserve((size_t)n_tmp, "tmp stream", "tsem_bam_rewrite_fetch")) return rc;
  BamCols C{b->cols.p, n};
  BamNames nm{b->names.p, b->name_off.p, b->n_loci};
  STAGE_HIP(b->rw_clock.begin());
  k_bam_rw_write<<<cdiv64(n, 256), 256>>>(n, b->bytes.p, b->off.p, C, nm, b->words.p, bam_rw_of(b, n), b->other.p, b->tmp.p);
  STAGE_HIP(hipGetLastError());
  STAGE_HIP(b->rw_clock.mark());
  if (n_other) STAGE_HIP(hipMemcpyAsync(other, b->other.p, (size_t)n_other, hipMemcpyDeviceToHost, 0));
  if (n_tmp) STAGE_HIP(hipMemcpyAsync(tmp, b->tmp.p, (size_t)n_tmp, hipMemcpyDeviceToHost, 0));
  STAGE_HIP(b->rw_clock.mark());
  STAGE_HIP(hipStreamSynchronize(0));
  STAGE_HIP(b->rw_clock.finish({RW_WRITE, RW_D2H}, false));      // (the sizing call was counted)
  return TSEM_OK;
}

int tsem_bam_rewrite_slots(tsem_bam* b, int32_t* kind, int32_t* pair, int64_t n) {
  if (!b || !kind || !pair) return stage_fail(TSEM_ERR_ARG, "tsem_bam_rewrite_slots: NULL pointer");
  if (b->sized_n < 1 || n != b->sized_n) return stage_fail(TSEM_ERR_ARG, "tsem_bam_rewrite_slots: n is not the slot count of the last size call");
  STAGE_HIP(hipSetDevice(b->device));
  const BamRw W = bam_rw_of(b, n);
  STAGE_HIP(hipMemcpy(kind, W.kind, (size_t)n * 4, hipMemcpyDeviceToHost));
  STAGE_HIP(hipMemcpy(pair, W.pair, (size_t)n * 4, hipMemcpyDeviceToHost));
  return TSEM_OK;
}

int tsem_bam_rewrite_times(tsem_bam* b, int reset, double* ms5, int64_t* calls) {
  if (!b || !ms5 || !calls) return stage_fail(TSEM_ERR_ARG, "tsem_bam_rewrite_times: NULL pointer");
  b->rw_clock.read(reset, ms5, calls);
  return TSEM_OK;
}

int tsem_bam_times(tsem_bam* b, int reset, double* ms6, int64_t* calls) {
  if (!b || !ms6 || !calls) return stage_fail(TSEM_ERR_ARG, "tsem_bam_times: NULL pointer");
  b->clock.read(reset, ms6, calls);
  return TSEM_OK;
}

}  // extern "C"
