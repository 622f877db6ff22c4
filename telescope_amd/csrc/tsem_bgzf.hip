// libtelescope_em.so, BGZF unit: the blocks of a BAM file inflated on the device (tsem_bgzf_*, include/telescope_em.h).  The host walks
// the chain of block headers of a piece of the file (tsem_bgzf_scan, tsem_bgzf_scan.h); one call of tsem_bgzf_inflate then uploads the
// compressed bytes and the block table and inflates every block into its own range of one output buffer, at the prefix sums of the
// ISIZEs — the blocks need nothing from each other.
//
//   k_bgzf_inflate  one wave per block (a workgroup is one wave): bgzf_inflate_block (tsem_bgzf_inflate.h), the same code a host
//                   program runs with one lane.  Symbol decoding is a serial chain, so every lane follows it with the same values and
//                   the wave never diverges; the Huffman tables are built in LDS, the lanes share the table fill, the bytes of stored
//                   blocks and of matches, and the CRC-32, which they take in 64 slices joined by multiplication by x^(8 len).  A block
//                   whose ISIZE exceeds 65,536 is not touched (status 255: the host inflates it).  Per block one status word; per call
//                   the first failing block in file order, by one 64-bit atomicMin of block << 8 | code.
//
// Every read is bounded by the block's payload, every write by its ISIZE, every back-reference by the start of its own output; the
// payload ranges and the total of the ISIZEs are checked on the host before the device sees them.
#include "tsem_internal.h"
#include "tsem_bgzf_inflate.h"
#include "tsem_bgzf_scan.h"

#include <vector>

struct bgzf_dev_block {          // what the kernel reads per block (32 bytes)
  int64_t pay_off, out_off;
  int32_t pay_len; uint32_t isize, crc; int32_t pad;
};

struct tsem_bgzf {
  int device = 0;
  uint8_t *d_in = nullptr, *d_out = nullptr; size_t cap_in = 0, cap_out = 0;
  bgzf_dev_block* d_blk = nullptr; int32_t* d_status = nullptr; size_t cap_blk = 0;
  unsigned long long* d_first = nullptr;
  unsigned long long h_first = 0;                 // (the word's host copy: it must outlive a call that fails behind the copy's launch)
  std::vector<bgzf_dev_block> h_blk;
  hipEvent_t ev[4] = {};
  bool have_ev = false;
  double ms[3] = {0, 0, 0};                       // host-to-device, k_bgzf_inflate, device-to-host
  int64_t calls = 0;
};

// (file scope, not the unnamed namespace: a profile lists it as k_bgzf_inflate)
__global__ __launch_bounds__(64) void k_bgzf_inflate(int32_t n_blocks, const uint8_t* __restrict__ in, const bgzf_dev_block* __restrict__ blk,
                                                     uint8_t* out, int32_t* __restrict__ status, unsigned long long* first) {
  __shared__ tsem_bgzf_tables T;
  const int32_t b = (int32_t)blockIdx.x;
  if (b >= n_blocks) return;
  const bgzf_dev_block B = blk[b];
  int st = BGZF_ST_HOST;
  if (B.isize <= (uint32_t)BGZF_MAX_ISIZE)
    st = bgzf_inflate_block(in + B.pay_off, B.pay_len, out + B.out_off, (int32_t)B.isize, B.crc, &T, (int)threadIdx.x, 64);
  if (threadIdx.x == 0) {
    status[b] = st;
    if (st != BGZF_ST_OK && st != BGZF_ST_HOST) atomicMin(first, ((unsigned long long)b << 8) | (unsigned long long)st);
  }
}

namespace {

int bgzf_fail(int rc, const std::string& msg) { g_create_err = msg; return rc; }
#define BGZF_HIP(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) return bgzf_fail(TSEM_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(e_)); } while (0)

template <typename T>
int bgzf_grow(T** d, size_t* cap, size_t need, const char* what) {
  if (need <= *cap) return TSEM_OK;
  dfree(*d); *cap = 0;
  const size_t n = need + need / 4;
  if (hipMalloc((void**)d, n * sizeof(T)) != hipSuccess) {
    *d = nullptr;
    return bgzf_fail(TSEM_ERR_NOMEM, std::string("tsem_bgzf_inflate: hipMalloc(") + std::to_string(n * sizeof(T)) + " B) for the " + what + " failed");
  }
  *cap = n;
  return TSEM_OK;
}

}  // namespace

extern "C" {

int tsem_bgzf_scan(const uint8_t* bytes, int64_t n_bytes, int64_t* blocks, int64_t cap, int64_t* n_blocks, int64_t* consumed, int32_t* not_bgzf) {
  if (n_bytes < 0 || cap < 0 || (!bytes && n_bytes) || (!blocks && cap) || !n_blocks || !consumed || !not_bgzf)
    return bgzf_fail(TSEM_ERR_ARG, "tsem_bgzf_scan: NULL pointer or negative size");
  char msg[200];
  if (tsem_bgzf_scan_chain(bytes, n_bytes, blocks, cap, n_blocks, consumed, not_bgzf, msg, sizeof msg)) return bgzf_fail(TSEM_ERR_ARG, msg);
  return TSEM_OK;
}

int tsem_bgzf_close(tsem_bgzf* z) {
  if (!z) return TSEM_OK;
  (void)hipSetDevice(z->device);
  dfree(z->d_in); dfree(z->d_out); dfree(z->d_blk); dfree(z->d_status); dfree(z->d_first);
  if (z->have_ev) for (hipEvent_t& e : z->ev) (void)hipEventDestroy(e);
  delete z;
  return TSEM_OK;
}

int tsem_bgzf_open(tsem_bgzf** out, int device) {
  if (!out) return bgzf_fail(TSEM_ERR_ARG, "tsem_bgzf_open: out is NULL");
  *out = nullptr;
  if (hipSetDevice(device) != hipSuccess) return bgzf_fail(TSEM_ERR_HIP, "hipSetDevice failed (no usable HIP device)");
  tsem_bgzf* z = new tsem_bgzf;
  z->device = device;
  int rc = TSEM_OK;
  if (hipMalloc((void**)&z->d_first, 8) != hipSuccess) { z->d_first = nullptr; rc = bgzf_fail(TSEM_ERR_NOMEM, "tsem_bgzf_open: hipMalloc failed"); }
  if (!rc) {
    for (hipEvent_t& e : z->ev)
      if (hipEventCreate(&e) != hipSuccess) rc = bgzf_fail(TSEM_ERR_HIP, "tsem_bgzf_open: hipEventCreate failed");
    z->have_ev = rc == TSEM_OK;
  }
  if (rc) { tsem_bgzf_close(z); return rc; }
  *out = z;
  return TSEM_OK;
}

int tsem_bgzf_inflate(tsem_bgzf* z, const uint8_t* bytes, int64_t n_bytes, const int64_t* blocks, int64_t n_blocks, uint8_t* out,
                      int64_t out_cap, int32_t* status, int64_t* first2, int64_t* out_bytes) {
  if (n_bytes < 0 || n_blocks < 0 || out_cap < 0 || n_blocks >= (int64_t)INT32_MAX || !first2 || !out_bytes ||
      (n_blocks && (!bytes || !blocks || !status)) || (out_cap && !out))
    return bgzf_fail(TSEM_ERR_ARG, "tsem_bgzf_inflate: NULL pointer, negative size or more than 2^31 - 2 blocks");
  // the table bounds every access of the kernel: checked here, before the device sees it (and before the handle is looked at)
  std::vector<bgzf_dev_block> tab((size_t)n_blocks);
  int64_t total = 0, in_end = 0;
  for (int64_t k = 0; k < n_blocks; ++k) {
    const int64_t po = blocks[5 * k + 1], pl = blocks[5 * k + 2], isize = blocks[5 * k + 3], crc = blocks[5 * k + 4];
    if (po < 0 || pl < 0 || pl > 65536 || po > n_bytes - pl)
      return bgzf_fail(TSEM_ERR_ARG, "tsem_bgzf_inflate: the payload of block " + std::to_string(k) + " lies outside the bytes (or is longer than 65,536)");
    if (isize < 0 || isize > (int64_t)UINT32_MAX || crc < 0 || crc > (int64_t)UINT32_MAX)
      return bgzf_fail(TSEM_ERR_ARG, "tsem_bgzf_inflate: ISIZE or CRC-32 of block " + std::to_string(k) + " is no 32-bit value");
    tab[(size_t)k] = bgzf_dev_block{po, total, (int32_t)pl, (uint32_t)isize, (uint32_t)crc, 0};
    if (isize <= BGZF_MAX_ISIZE) total += isize;            // (a larger claim is the host's: no output range here)
    in_end = std::max(in_end, po + pl);
  }
  if (total > out_cap)
    return bgzf_fail(TSEM_ERR_ARG, "tsem_bgzf_inflate: the blocks inflate to " + std::to_string(total) + " bytes, out holds " + std::to_string(out_cap));
  if (!z) return bgzf_fail(TSEM_ERR_ARG, "tsem_bgzf_inflate: NULL handle");
  z->h_blk.swap(tab);                                        // (kept by the handle: the copy below is asynchronous)
  first2[0] = 0; first2[1] = -1;
  *out_bytes = total;
  if (n_blocks == 0) return TSEM_OK;
  BGZF_HIP(hipSetDevice(z->device));
  int rc = bgzf_grow(&z->d_in, &z->cap_in, (size_t)std::max<int64_t>(1, in_end), "compressed bytes");
  if (!rc) rc = bgzf_grow(&z->d_out, &z->cap_out, (size_t)std::max<int64_t>(1, total), "inflated bytes");
  if (!rc && (size_t)n_blocks > z->cap_blk) {
    size_t c1 = z->cap_blk, c2 = z->cap_blk;
    rc = bgzf_grow(&z->d_blk, &c1, (size_t)n_blocks, "block table");
    if (!rc) rc = bgzf_grow(&z->d_status, &c2, (size_t)n_blocks, "status words");
    z->cap_blk = rc ? 0 : std::min(c1, c2);
  }
  if (rc) return rc;
  const unsigned long long none = ~0ull;
  unsigned long long& st = z->h_first;
  st = none;
  BGZF_HIP(hipEventRecord(z->ev[0], 0));
  if (in_end) BGZF_HIP(hipMemcpyAsync(z->d_in, bytes, (size_t)in_end, hipMemcpyHostToDevice, 0));
  BGZF_HIP(hipMemcpyAsync(z->d_blk, z->h_blk.data(), (size_t)n_blocks * sizeof(bgzf_dev_block), hipMemcpyHostToDevice, 0));
  BGZF_HIP(hipMemsetAsync(z->d_first, 0xFF, 8, 0));
  BGZF_HIP(hipEventRecord(z->ev[1], 0));
  k_bgzf_inflate<<<(unsigned)n_blocks, 64>>>((int32_t)n_blocks, z->d_in, z->d_blk, z->d_out, z->d_status, z->d_first);
  BGZF_HIP(hipGetLastError());
  BGZF_HIP(hipEventRecord(z->ev[2], 0));
  if (total) BGZF_HIP(hipMemcpyAsync(out, z->d_out, (size_t)total, hipMemcpyDeviceToHost, 0));
  BGZF_HIP(hipMemcpyAsync(status, z->d_status, (size_t)n_blocks * 4, hipMemcpyDeviceToHost, 0));
  BGZF_HIP(hipMemcpyAsync(&st, z->d_first, 8, hipMemcpyDeviceToHost, 0));
  BGZF_HIP(hipEventRecord(z->ev[3], 0));
  BGZF_HIP(hipStreamSynchronize(0));
  for (int k = 0; k < 3; ++k) {
    float ms = 0.f;
    BGZF_HIP(hipEventElapsedTime(&ms, z->ev[k], z->ev[k + 1]));
    z->ms[k] += ms;
  }
  ++z->calls;
  if (st != none) { first2[0] = (int64_t)(st & 0xFF); first2[1] = (int64_t)(st >> 8); }
  return TSEM_OK;
}

int tsem_bgzf_times(tsem_bgzf* z, int reset, double* ms3, int64_t* calls) {
  if (!z || !ms3 || !calls) return bgzf_fail(TSEM_ERR_ARG, "tsem_bgzf_times: NULL pointer");
  for (int k = 0; k < 3; ++k) ms3[k] = z->ms[k];
  *calls = z->calls;
  if (reset) { for (double& m : z->ms) m = 0; z->calls = 0; }
  return TSEM_OK;
}

}  // extern "C"
