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
//
// The other direction, tsem_bgzf_deflate (`--deflate device`): a host stream is uploaded once, cut every 0xff00 bytes, and comes back
// as the finished BGZF file image of those blocks.
//
//   k_bgzf_deflate  one wave per block (a workgroup is one wave): bgzf_deflate_block (tsem_bgzf_deflate.h) into the block's own slot of
//                   0xff00 + 5 bytes; its tokens in a scratch range of the handle (4 B per input byte).  Per block the stream's length,
//                   the CRC-32 of its input and a status word (0; 1: the body refused, which no input can make it do).
//   k_bgzf_offsets  one workgroup: the prefix sum of length + 26 over the blocks.
//   k_bgzf_pack     one workgroup per block: the 18 header bytes, the stream, CRC-32 and ISIZE at the block's prefix sum.
//
// tsem_bgzf_deflate_host is the same body with one lane on the CPU and gives the same bytes (the body's phases do not depend on
// the number of lanes).
#include "tsem_internal.h"
#include "tsem_bgzf_inflate.h"
#include "tsem_bgzf_deflate.h"
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
  hipEvent_t ev[5] = {};                          // (the inflate uses the first four)
  bool have_ev = false;
  double ms[3] = {0, 0, 0};                       // host-to-device, k_bgzf_inflate, device-to-host
  int64_t calls = 0;
  // tsem_bgzf_deflate: the stream, the slots, the tokens, the file image; per block length / CRC-32 / status and the offsets
  uint8_t *e_in = nullptr, *e_slot = nullptr, *e_img = nullptr; uint32_t* e_tok = nullptr;
  size_t ecap_in = 0, ecap_slot = 0, ecap_img = 0, ecap_tok = 0;
  int32_t* e_len = nullptr; uint32_t* e_crc = nullptr; int32_t* e_status = nullptr; int64_t* e_off = nullptr;
  size_t ecap_len = 0, ecap_crc = 0, ecap_status = 0, ecap_off = 0;
  int64_t h_total = 0; int32_t h_bad = 0;
  double ems[4] = {0, 0, 0, 0};                   // host-to-device, k_bgzf_deflate, offsets and pack, device-to-host
  int64_t ecalls = 0;
};

enum { BGZF_DEF_SLOT = BGZF_DEF_BLOCK + 5, BGZF_DEF_TOKS = BGZF_DEF_BLOCK + 1, BGZF_FRAME = 26 };   // (header 18 + trailer 8)

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

__global__ __launch_bounds__(64) void k_bgzf_deflate(int32_t n_blocks, const uint8_t* __restrict__ in, int64_t n_bytes, uint8_t* slots,
                                                     uint32_t* toks, int32_t* __restrict__ out_len, uint32_t* __restrict__ out_crc,
                                                     int32_t* __restrict__ status, int32_t* bad) {
  __shared__ tsem_bgzf_deflate_tables T;
  const int64_t b = (int64_t)blockIdx.x;
  if (b >= n_blocks) return;
  const int64_t at = b * BGZF_DEF_BLOCK;
  const int32_t len = (int32_t)(n_bytes - at < BGZF_DEF_BLOCK ? n_bytes - at : BGZF_DEF_BLOCK);
  uint32_t crc = 0;
  int32_t form = 0;
  const int32_t n = bgzf_deflate_block(in + at, len, slots + b * BGZF_DEF_SLOT, len + 5, &crc, &form, &T, toks + b * BGZF_DEF_TOKS,
                                       (int)threadIdx.x, 64);
  if (threadIdx.x == 0) {
    const bool ok = n >= 2 && n <= len + 5;
    out_len[b] = ok ? n : 0; out_crc[b] = crc; status[b] = ok ? 0 : 1;
    if (!ok) atomicAdd(bad, 1);
  }
}

// off[k] = the bytes of the blocks in front of block k in the file image, off[n_blocks] = all of them
__global__ __launch_bounds__(256) void k_bgzf_offsets(int32_t n_blocks, const int32_t* __restrict__ len, int64_t* __restrict__ off) {
  __shared__ int64_t part[256];
  const int t = (int)threadIdx.x;
  const int32_t per = (n_blocks + 255) / 256, lo = t * per < n_blocks ? t * per : n_blocks, hi = lo + per < n_blocks ? lo + per : n_blocks;
  int64_t s = 0;
  for (int32_t k = lo; k < hi; ++k) s += (int64_t)len[k] + BGZF_FRAME;
  part[t] = s;
  __syncthreads();
  int64_t base = 0;
  for (int k = 0; k < t; ++k) base += part[k];
  for (int32_t k = lo; k < hi; ++k) { off[k] = base; base += (int64_t)len[k] + BGZF_FRAME; }
  if (t == 255) off[n_blocks] = base;
}

__global__ __launch_bounds__(256) void k_bgzf_pack(int32_t n_blocks, int64_t n_bytes, const uint8_t* __restrict__ slots, const int32_t* __restrict__ len,
                                                   const uint32_t* __restrict__ crc, const int64_t* __restrict__ off, uint8_t* __restrict__ img) {
  const int64_t b = (int64_t)blockIdx.x;
  if (b >= n_blocks) return;
  const int32_t n = len[b];
  const int64_t rest = n_bytes - b * BGZF_DEF_BLOCK;
  const uint32_t isize = (uint32_t)(rest < BGZF_DEF_BLOCK ? rest : BGZF_DEF_BLOCK), c = crc[b], bsize = (uint32_t)n + BGZF_FRAME - 1;
  uint8_t* o = img + off[b];
  const uint8_t* p = slots + b * BGZF_DEF_SLOT;
  const int t = (int)threadIdx.x;
  if (t < 18) {                                             // 1f 8b 08 04, MTIME 0, XFL 0, OS ff, XLEN 6, 'B' 'C' 2 0, BSIZE - 1
    const uint64_t lo = 0x1full | 0x8bull << 8 | 8ull << 16 | 4ull << 24, hi = 0xffull << 8 | 6ull << 16 | 0x42ull << 32 | 0x43ull << 40 | 2ull << 48;
    o[t] = (uint8_t)(t < 8 ? lo >> (8 * t) : t < 16 ? hi >> (8 * (t - 8)) : bsize >> (8 * (t - 16)));
  } else if (t < 26) {
    o[18 + n + (t - 18)] = (uint8_t)(t < 22 ? c >> (8 * (t - 18)) : isize >> (8 * (t - 22)));
  }
  for (int32_t i = t; i < n; i += 256) o[18 + i] = p[i];
}

namespace {

int bgzf_fail(int rc, const std::string& msg) { g_create_err = msg; return rc; }
#define BGZF_HIP(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) return bgzf_fail(TSEM_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(e_)); } while (0)

template <typename T>
int bgzf_grow(T** d, size_t* cap, size_t need, const char* what, const char* fn = "tsem_bgzf_inflate") {
  if (need <= *cap) return TSEM_OK;
  dfree(*d); *cap = 0;
  const size_t n = need + need / 4;
  if (hipMalloc((void**)d, n * sizeof(T)) != hipSuccess) {
    *d = nullptr;
    return bgzf_fail(TSEM_ERR_NOMEM, std::string(fn) + ": hipMalloc(" + std::to_string(n * sizeof(T)) + " B) for the " + what + " failed");
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
  dfree(z->e_in); dfree(z->e_slot); dfree(z->e_img); dfree(z->e_tok); dfree(z->e_len); dfree(z->e_crc); dfree(z->e_status); dfree(z->e_off);
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

// the argument checks and the block count that both deflate entries share; need = the worst case of out
static int bgzf_deflate_args(const char* fn, const uint8_t* bytes, int64_t n_bytes, uint8_t* out, int64_t out_cap, int64_t* out_bytes,
                             int64_t* n_blocks, int64_t* nb) {
  if (n_bytes < 0 || out_cap < 0 || !out_bytes || !n_blocks || (n_bytes && !bytes))
    return bgzf_fail(TSEM_ERR_ARG, std::string(fn) + ": NULL pointer or negative size");
  *nb = (n_bytes + BGZF_DEF_BLOCK - 1) / BGZF_DEF_BLOCK;
  if (*nb >= (int64_t)INT32_MAX) return bgzf_fail(TSEM_ERR_ARG, std::string(fn) + ": more than 2^31 - 2 blocks");
  const int64_t need = n_bytes + (5 + BGZF_FRAME) * *nb;
  if (out_cap < need || (need && !out))
    return bgzf_fail(TSEM_ERR_ARG, std::string(fn) + ": out holds " + std::to_string(out_cap) + " bytes, the worst case of " +
                                       std::to_string(*nb) + " blocks is " + std::to_string(need) + " (n_bytes + 31 per block)");
  return TSEM_OK;
}

int tsem_bgzf_deflate_host(const uint8_t* bytes, int64_t n_bytes, uint8_t* out, int64_t out_cap, int64_t* out_bytes, int64_t* n_blocks) {
  int64_t nb = 0;
  if (int rc = bgzf_deflate_args("tsem_bgzf_deflate_host", bytes, n_bytes, out, out_cap, out_bytes, n_blocks, &nb)) return rc;
  std::vector<uint32_t> tok(BGZF_DEF_TOKS);
  std::vector<tsem_bgzf_deflate_tables> T(1);
  int64_t o = 0;
  for (int64_t b = 0; b < nb; ++b) {
    const int64_t at = b * BGZF_DEF_BLOCK;
    const int32_t len = (int32_t)std::min<int64_t>(n_bytes - at, BGZF_DEF_BLOCK);
    uint32_t crc = 0;
    int32_t form = 0;
    const int32_t n = bgzf_deflate_block(bytes + at, len, out + o + 18, len + 5, &crc, &form, T.data(), tok.data(), 0, 1);
    if (n < 2 || n > len + 5) return bgzf_fail(TSEM_ERR_ARG, "tsem_bgzf_deflate_host: block " + std::to_string(b) + " was not deflated (" + std::to_string(n) + ")");
    const uint32_t bsize = (uint32_t)n + BGZF_FRAME - 1, isize = (uint32_t)len;
    const uint8_t head[18] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, (uint8_t)(bsize & 255u), (uint8_t)(bsize >> 8)};
    memcpy(out + o, head, 18);
    for (int i = 0; i < 4; ++i) { out[o + 18 + n + i] = (uint8_t)(crc >> (8 * i)); out[o + 22 + n + i] = (uint8_t)(isize >> (8 * i)); }
    o += n + BGZF_FRAME;
  }
  *out_bytes = o; *n_blocks = nb;
  return TSEM_OK;
}

int tsem_bgzf_deflate(tsem_bgzf* z, const uint8_t* bytes, int64_t n_bytes, uint8_t* out, int64_t out_cap, int64_t* out_bytes, int64_t* n_blocks) {
  int64_t nb = 0;
  if (int rc = bgzf_deflate_args("tsem_bgzf_deflate", bytes, n_bytes, out, out_cap, out_bytes, n_blocks, &nb)) return rc;
  if (!z) return bgzf_fail(TSEM_ERR_ARG, "tsem_bgzf_deflate: NULL handle");
  *out_bytes = 0; *n_blocks = nb;
  if (nb == 0) return TSEM_OK;
  BGZF_HIP(hipSetDevice(z->device));
  const size_t n = (size_t)nb;
  int rc = bgzf_grow(&z->e_in, &z->ecap_in, (size_t)n_bytes, "stream", "tsem_bgzf_deflate");
  if (!rc) rc = bgzf_grow(&z->e_slot, &z->ecap_slot, n * BGZF_DEF_SLOT, "deflate slots", "tsem_bgzf_deflate");
  if (!rc) rc = bgzf_grow(&z->e_tok, &z->ecap_tok, n * BGZF_DEF_TOKS, "tokens", "tsem_bgzf_deflate");
  if (!rc) rc = bgzf_grow(&z->e_img, &z->ecap_img, (size_t)n_bytes + n * (5 + BGZF_FRAME), "file image", "tsem_bgzf_deflate");
  if (!rc) rc = bgzf_grow(&z->e_len, &z->ecap_len, n, "stream lengths", "tsem_bgzf_deflate");
  if (!rc) rc = bgzf_grow(&z->e_crc, &z->ecap_crc, n, "CRC-32 words", "tsem_bgzf_deflate");
  if (!rc) rc = bgzf_grow(&z->e_status, &z->ecap_status, n + 1, "status words", "tsem_bgzf_deflate");
  if (!rc) rc = bgzf_grow(&z->e_off, &z->ecap_off, n + 1, "block offsets", "tsem_bgzf_deflate");
  if (rc) return rc;
  int32_t* d_bad = z->e_status + n;                           // (the word behind the blocks' status words: how many were refused)
  BGZF_HIP(hipEventRecord(z->ev[0], 0));
  BGZF_HIP(hipMemcpyAsync(z->e_in, bytes, (size_t)n_bytes, hipMemcpyHostToDevice, 0));
  BGZF_HIP(hipMemsetAsync(d_bad, 0, 4, 0));
  BGZF_HIP(hipEventRecord(z->ev[1], 0));
  k_bgzf_deflate<<<(unsigned)nb, 64>>>((int32_t)nb, z->e_in, n_bytes, z->e_slot, z->e_tok, z->e_len, z->e_crc, z->e_status, d_bad);
  BGZF_HIP(hipGetLastError());
  BGZF_HIP(hipEventRecord(z->ev[2], 0));
  k_bgzf_offsets<<<1, 256>>>((int32_t)nb, z->e_len, z->e_off);
  BGZF_HIP(hipGetLastError());
  k_bgzf_pack<<<(unsigned)nb, 256>>>((int32_t)nb, n_bytes, z->e_slot, z->e_len, z->e_crc, z->e_off, z->e_img);
  BGZF_HIP(hipGetLastError());
  BGZF_HIP(hipEventRecord(z->ev[3], 0));
  // the image's size (8 bytes) decides how much of it travels; the image itself is the one download
  BGZF_HIP(hipMemcpyAsync(&z->h_total, z->e_off + n, 8, hipMemcpyDeviceToHost, 0));
  BGZF_HIP(hipMemcpyAsync(&z->h_bad, d_bad, 4, hipMemcpyDeviceToHost, 0));
  BGZF_HIP(hipStreamSynchronize(0));
  if (z->h_bad) return bgzf_fail(TSEM_ERR_HIP, "tsem_bgzf_deflate: k_bgzf_deflate refused " + std::to_string(z->h_bad) + " blocks");
  if (z->h_total < nb * BGZF_FRAME || z->h_total > n_bytes + nb * (5 + BGZF_FRAME))
    return bgzf_fail(TSEM_ERR_HIP, "tsem_bgzf_deflate: the image's size " + std::to_string(z->h_total) + " is out of range");
  BGZF_HIP(hipMemcpyAsync(out, z->e_img, (size_t)z->h_total, hipMemcpyDeviceToHost, 0));
  BGZF_HIP(hipEventRecord(z->ev[4], 0));
  BGZF_HIP(hipStreamSynchronize(0));
  for (int k = 0; k < 4; ++k) {
    float ms = 0.f;
    BGZF_HIP(hipEventElapsedTime(&ms, z->ev[k], z->ev[k + 1]));
    z->ems[k] += ms;
  }
  ++z->ecalls;
  *out_bytes = z->h_total;
  return TSEM_OK;
}

int tsem_bgzf_deflate_times(tsem_bgzf* z, int reset, double* ms4, int64_t* calls) {
  if (!z || !ms4 || !calls) return bgzf_fail(TSEM_ERR_ARG, "tsem_bgzf_deflate_times: NULL pointer");
  for (int k = 0; k < 4; ++k) ms4[k] = z->ems[k];
  *calls = z->ecalls;
  if (reset) { for (double& m : z->ems) m = 0; z->ecalls = 0; }
  return TSEM_OK;
}

}  // extern "C"
