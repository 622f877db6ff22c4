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
#include "tsem_stage.h"

#include <vector>

struct bgzf_dev_block {          // what the kernel reads per block (32 bytes)
  int64_t pay_off, out_off;
  int32_t pay_len; uint32_t isize, crc; int32_t pad;
};

struct tsem_bgzf {
  int device = 0;
  // tsem_bgzf_inflate: the compressed bytes, the inflated bytes, the block table, per block a status word; the first failing block
  DevBuf<uint8_t> in, out;
  DevBuf<bgzf_dev_block> blk;
  DevBuf<int32_t> status;
  StatusWord first;
  std::vector<bgzf_dev_block> h_blk;
  StageClock<4, 3> clock;                         // host-to-device, k_bgzf_inflate, device-to-host
  // tsem_bgzf_deflate: the stream, the slots, the tokens, the file image; per block length / CRC-32 / status and the offsets
  DevBuf<uint8_t> e_in, e_slot, e_img;
  DevBuf<uint32_t> e_tok, e_crc;
  DevBuf<int32_t> e_len, e_status;
  DevBuf<int64_t> e_off;
  int64_t h_total = 0; int32_t h_bad = 0;
  StageClock<5, 4> e_clock;                       // host-to-device, k_bgzf_deflate, offsets and pack, device-to-host
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

extern "C" {

int tsem_bgzf_scan(const uint8_t* bytes, int64_t n_bytes, int64_t* blocks, int64_t cap, int64_t* n_blocks, int64_t* consumed, int32_t* not_bgzf) {
  if (n_bytes < 0 || cap < 0 || (!bytes && n_bytes) || (!blocks && cap) || !n_blocks || !consumed || !not_bgzf)
    return stage_fail(TSEM_ERR_ARG, "tsem_bgzf_scan: NULL pointer or negative size");
  char msg[200];
  if (tsem_bgzf_scan_chain(bytes, n_bytes, blocks, cap, n_blocks, consumed, not_bgzf, msg, sizeof msg)) return stage_fail(TSEM_ERR_ARG, msg);
  return TSEM_OK;
}

int tsem_bgzf_close(tsem_bgzf* z) {
  if (!z) return TSEM_OK;
  (void)hipSetDevice(z->device);
  delete z;                                       // (every buffer and event is a member that releases itself)
  return TSEM_OK;
}

int tsem_bgzf_open(tsem_bgzf** out, int device) {
  if (!out) return stage_fail(TSEM_ERR_ARG, "tsem_bgzf_open: out is NULL");
  *out = nullptr;
  if (hipSetDevice(device) != hipSuccess) return stage_fail(TSEM_ERR_HIP, "hipSetDevice failed (no usable HIP device)");
  tsem_bgzf* z = new tsem_bgzf;
  z->device = device;
  int rc = z->first.create("tsem_bgzf_open");
  if (!rc && (z->clock.create() != hipSuccess || z->e_clock.create() != hipSuccess)) rc = stage_fail(TSEM_ERR_HIP, "tsem_bgzf_open: hipEventCreate failed");
  if (rc) { tsem_bgzf_close(z); return rc; }
  *out = z;
  return TSEM_OK;
}

int tsem_bgzf_inflate(tsem_bgzf* z, const uint8_t* bytes, int64_t n_bytes, const int64_t* blocks, int64_t n_blocks, uint8_t* out,
                      int64_t out_cap, int32_t* status, int64_t* first2, int64_t* out_bytes) {
  if (n_bytes < 0 || n_blocks < 0 || out_cap < 0 || n_blocks >= (int64_t)INT32_MAX || !first2 || !out_bytes ||
      (n_blocks && (!bytes || !blocks || !status)) || (out_cap && !out))
    return stage_fail(TSEM_ERR_ARG, "tsem_bgzf_inflate: NULL pointer, negative size or more than 2^31 - 2 blocks");
  // the table bounds every access of the kernel: checked here, before the device sees it (and before the handle is looked at)
  std::vector<bgzf_dev_block> tab((size_t)n_blocks);
  int64_t total = 0, in_end = 0;
  for (int64_t k = 0; k < n_blocks; ++k) {
    const int64_t po = blocks[5 * k + 1], pl = blocks[5 * k + 2], isize = blocks[5 * k + 3], crc = blocks[5 * k + 4];
    if (po < 0 || pl < 0 || pl > 65536 || po > n_bytes - pl)
      return stage_fail(TSEM_ERR_ARG, "tsem_bgzf_inflate: the payload of block " + std::to_string(k) + " lies outside the bytes (or is longer than 65,536)");
    if (isize < 0 || isize > (int64_t)UINT32_MAX || crc < 0 || crc > (int64_t)UINT32_MAX)
      return stage_fail(TSEM_ERR_ARG, "tsem_bgzf_inflate: ISIZE or CRC-32 of block " + std::to_string(k) + " is no 32-bit value");
    tab[(size_t)k] = bgzf_dev_block{po, total, (int32_t)pl, (uint32_t)isize, (uint32_t)crc, 0};
    if (isize <= BGZF_MAX_ISIZE) total += isize;            // (a larger claim is the host's: no output range here)
    in_end = std::max(in_end, po + pl);
  }
  if (total > out_cap)
    return stage_fail(TSEM_ERR_ARG, "tsem_bgzf_inflate: the blocks inflate to " + std::to_string(total) + " bytes, out holds " + std::to_string(out_cap));
  if (!z) return stage_fail(TSEM_ERR_ARG, "tsem_bgzf_inflate: NULL handle");
  z->h_blk.swap(tab);                                        // (kept by the handle: the copy below is asynchronous)
  first2[0] = 0; first2[1] = -1;
  *out_bytes = total;
  if (n_blocks == 0) return TSEM_OK;
  STAGE_HIP(hipSetDevice(z->device));
  const char* fn = "tsem_bgzf_inflate";
  int rc = z->in.reserve((size_t)std::max<int64_t>(1, in_end), "compressed bytes", fn);
  if (!rc) rc = z->out.reserve((size_t)std::max<int64_t>(1, total), "inflated bytes", fn);
  if (!rc) rc = z->blk.reserve((size_t)n_blocks, "block table", fn);
  if (!rc) rc = z->status.reserve((size_t)n_blocks, "status words", fn);
  if (rc) return rc;
  STAGE_HIP(z->clock.begin());
  if (in_end) STAGE_HIP(hipMemcpyAsync(z->in.p, bytes, (size_t)in_end, hipMemcpyHostToDevice, 0));
  STAGE_HIP(hipMemcpyAsync(z->blk.p, z->h_blk.data(), (size_t)n_blocks * sizeof(bgzf_dev_block), hipMemcpyHostToDevice, 0));
  STAGE_HIP(z->first.arm());
  STAGE_HIP(z->clock.mark());
  k_bgzf_inflate<<<(unsigned)n_blocks, 64>>>((int32_t)n_blocks, z->in.p, z->blk.p, z->out.p, z->status.p, z->first.d.p);
  STAGE_HIP(hipGetLastError());
  STAGE_HIP(z->clock.mark());
  if (total) STAGE_HIP(hipMemcpyAsync(out, z->out.p, (size_t)total, hipMemcpyDeviceToHost, 0));
  STAGE_HIP(hipMemcpyAsync(status, z->status.p, (size_t)n_blocks * 4, hipMemcpyDeviceToHost, 0));
  STAGE_HIP(z->first.fetch());
  STAGE_HIP(z->clock.mark());
  STAGE_HIP(hipStreamSynchronize(0));
  STAGE_HIP(z->clock.finish({0, 1, 2}));
  (void)z->first.decode(first2);
  return TSEM_OK;
}

int tsem_bgzf_times(tsem_bgzf* z, int reset, double* ms3, int64_t* calls) {
  if (!z || !ms3 || !calls) return stage_fail(TSEM_ERR_ARG, "tsem_bgzf_times: NULL pointer");
  z->clock.read(reset, ms3, calls);
  return TSEM_OK;
}

// the argument checks and the block count that both deflate entries share; need = the worst case of out
static int bgzf_deflate_args(const char* fn, const uint8_t* bytes, int64_t n_bytes, uint8_t* out, int64_t out_cap, int64_t* out_bytes,
                             int64_t* n_blocks, int64_t* nb) {
  if (n_bytes < 0 || out_cap < 0 || !out_bytes || !n_blocks || (n_bytes && !bytes))
    return stage_fail(TSEM_ERR_ARG, std::string(fn) + ": NULL pointer or negative size");
  *nb = (n_bytes + BGZF_DEF_BLOCK - 1) / BGZF_DEF_BLOCK;
  if (*nb >= (int64_t)INT32_MAX) return stage_fail(TSEM_ERR_ARG, std::string(fn) + ": more than 2^31 - 2 blocks");
  const int64_t need = n_bytes + (5 + BGZF_FRAME) * *nb;
  if (out_cap < need || (need && !out))
    return stage_fail(TSEM_ERR_ARG, std::string(fn) + ": out holds " + std::to_string(out_cap) + " bytes, the worst case of " +
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
    if (n < 2 || n > len + 5) return stage_fail(TSEM_ERR_ARG, "tsem_bgzf_deflate_host: block " + std::to_string(b) + " was not deflated (" + std::to_string(n) + ")");
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
  if (!z) return stage_fail(TSEM_ERR_ARG, "tsem_bgzf_deflate: NULL handle");
  *out_bytes = 0; *n_blocks = nb;
  if (nb == 0) return TSEM_OK;
  STAGE_HIP(hipSetDevice(z->device));
  const size_t n = (size_t)nb;
  const char* fn = "tsem_bgzf_deflate";
  int rc = z->e_in.reserve((size_t)n_bytes, "stream", fn);
  if (!rc) rc = z->e_slot.reserve(n * BGZF_DEF_SLOT, "deflate slots", fn);
  if (!rc) rc = z->e_tok.reserve(n * BGZF_DEF_TOKS, "tokens", fn);
  if (!rc) rc = z->e_img.reserve((size_t)n_bytes + n * (5 + BGZF_FRAME), "file image", fn);
  if (!rc) rc = z->e_len.reserve(n, "stream lengths", fn);
  if (!rc) rc = z->e_crc.reserve(n, "CRC-32 words", fn);
  if (!rc) rc = z->e_status.reserve(n + 1, "status words", fn);
  if (!rc) rc = z->e_off.reserve(n + 1, "block offsets", fn);
  if (rc) return rc;
  int32_t* d_bad = z->e_status.p + n;                         // (the word behind the blocks' status words: how many were refused)
  STAGE_HIP(z->e_clock.begin());
  STAGE_HIP(hipMemcpyAsync(z->e_in.p, bytes, (size_t)n_bytes, hipMemcpyHostToDevice, 0));
  STAGE_HIP(hipMemsetAsync(d_bad, 0, 4, 0));
  STAGE_HIP(z->e_clock.mark());
  k_bgzf_deflate<<<(unsigned)nb, 64>>>((int32_t)nb, z->e_in.p, n_bytes, z->e_slot.p, z->e_tok.p, z->e_len.p, z->e_crc.p, z->e_status.p, d_bad);
  STAGE_HIP(hipGetLastError());
  STAGE_HIP(z->e_clock.mark());
  k_bgzf_offsets<<<1, 256>>>((int32_t)nb, z->e_len.p, z->e_off.p);
  STAGE_HIP(hipGetLastError());
  k_bgzf_pack<<<(unsigned)nb, 256>>>((int32_t)nb, n_bytes, z->e_slot.p, z->e_len.p, z->e_crc.p, z->e_off.p, z->e_img.p);
  STAGE_HIP(hipGetLastError());
  STAGE_HIP(z->e_clock.mark());
  // the image's size (8 bytes) decides how much of it travels; the image itself is the one download
  STAGE_HIP(hipMemcpyAsync(&z->h_total, z->e_off.p + n, 8, hipMemcpyDeviceToHost, 0));
  STAGE_HIP(hipMemcpyAsync(&z->h_bad, d_bad, 4, hipMemcpyDeviceToHost, 0));
  STAGE_HIP(hipStreamSynchronize(0));
  if (z->h_bad) return stage_fail(TSEM_ERR_HIP, "tsem_bgzf_deflate: k_bgzf_deflate refused " + std::to_string(z->h_bad) + " blocks");
  if (z->h_total < nb * BGZF_FRAME || z->h_total > n_bytes + nb * (5 + BGZF_FRAME))
    return stage_fail(TSEM_ERR_HIP, "tsem_bgzf_deflate: the image's size " + std::to_string(z->h_total) + " is out of range");
  STAGE_HIP(hipMemcpyAsync(out, z->e_img.p, (size_t)z->h_total, hipMemcpyDeviceToHost, 0));
  STAGE_HIP(z->e_clock.mark());
  STAGE_HIP(hipStreamSynchronize(0));
  STAGE_HIP(z->e_clock.finish({0, 1, 2, 3}));
  *out_bytes = z->h_total;
  return TSEM_OK;
}

int tsem_bgzf_deflate_times(tsem_bgzf* z, int reset, double* ms4, int64_t* calls) {
  if (!z || !ms4 || !calls) return stage_fail(TSEM_ERR_ARG, "tsem_bgzf_deflate_times: NULL pointer");
  z->e_clock.read(reset, ms4, calls);
  return TSEM_OK;
}

}  // extern "C"
