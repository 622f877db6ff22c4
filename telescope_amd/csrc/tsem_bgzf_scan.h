// BGZF block chain of a piece of a compressed file (tsem_bgzf_scan, include/telescope_em.h): host only, plain C++ — no HIP header, so
// that a stand-alone program can include it (tests/c_host/bgzf_inflate_check.cc).
//
// A piece begins on a block boundary.  A block is a gzip member: 1f 8b 08 04, MTIME, XFL, OS (12 bytes with XLEN), XLEN bytes of extra
// subfields (SI1 SI2 SLEN data) of which one is 'B' 'C' with SLEN 2 and holds BSIZE = the whole block's size - 1, the raw DEFLATE
// payload, CRC-32 and ISIZE (4 bytes each).  Row k of `blk` is { block offset, payload offset, payload length, ISIZE, CRC-32 }.  The
// walk stops in front of the first block that the piece does not hold completely, or at `cap` blocks: *consumed = the offset behind
// the last whole block.  *not_bgzf = 1 when the piece's first bytes are a header, or anything else, that is no BGZF header (nothing is
// consumed then): a plain gzip file, for one.  Behind the first block such bytes cannot be stepped over: -1 and a text in `msg`.
#pragma once
#include <cstdint>
#include <cstdio>

static inline uint32_t tsem_bgzf_le16(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }
static inline uint32_t tsem_bgzf_le32(const uint8_t* p) {
  return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}

static inline int tsem_bgzf_scan_chain(const uint8_t* bytes, int64_t n_bytes, int64_t* blk /* cap x 5 */, int64_t cap, int64_t* n_blocks,
                                       int64_t* consumed, int32_t* not_bgzf, char* msg, size_t msg_len) {
  int64_t p = 0, n = 0;
  *not_bgzf = 0;
  while (n < cap && p + 12 <= n_bytes) {
    const uint8_t* h = bytes + p;
    const char* what = nullptr;
    int64_t bsize = -1;
    const int64_t xlen = (int64_t)tsem_bgzf_le16(h + 10);
    if (!(h[0] == 0x1f && h[1] == 0x8b && h[2] == 8 && h[3] == 4)) what = "does not begin with 1f 8b 08 04";
    else {
      if (p + 12 + xlen > n_bytes) break;                   // (the extra field is not whole yet)
      int64_t q = 12;
      while (q + 4 <= 12 + xlen) {
        const int64_t slen = (int64_t)tsem_bgzf_le16(h + q + 2);
        if (q + 4 + slen > 12 + xlen) break;
        if (h[q] == 'B' && h[q + 1] == 'C' && slen == 2) { bsize = (int64_t)tsem_bgzf_le16(h + q + 4) + 1; break; }
        q += 4 + slen;
      }
      if (bsize < 0) what = "has no BC subfield in its extra field";
      else if (bsize < xlen + 20) what = "has a BSIZE smaller than its header and trailer";
    }
    if (what) {
      if (n == 0) { *not_bgzf = 1; break; }
      if (msg && msg_len) snprintf(msg, msg_len, "tsem_bgzf_scan: block %lld at byte %lld %s", (long long)n, (long long)p, what);
      return -1;
    }
    if (p + bsize > n_bytes) break;
    int64_t* row = blk + 5 * n++;
    row[0] = p; row[1] = p + 12 + xlen; row[2] = bsize - xlen - 20;
    row[3] = (int64_t)tsem_bgzf_le32(h + bsize - 4); row[4] = (int64_t)tsem_bgzf_le32(h + bsize - 8);
    p += bsize;
  }
  *n_blocks = n;
  *consumed = p;
  return 0;
}
