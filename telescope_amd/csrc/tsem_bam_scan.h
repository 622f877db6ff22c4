// BAM record chain of a chunk of inflated bytes (tsem_bam_scan, include/telescope_em.h): host only, plain C++ — no HIP header, so that
// a stand-alone program can include it (tests/c_host/bam_decode_check.cc).
//
// A chunk begins on a record boundary.  Every record is `int32 block_size` followed by block_size bytes; rec_off[i] is the offset of
// record i's block_size field.  The walk stops in front of the first record that the chunk does not hold completely (its size field
// included), or at `cap` records: rec_off[n] = *consumed = the offset behind the last complete record, what lies behind it belongs to
// the next chunk.  A block_size below 32 (the fixed fields) cannot be stepped over: -1 and a text in `msg`.
#pragma once
#include <cstdint>
#include <cstdio>

static inline int32_t tsem_bam_scan_le32(const uint8_t* p) {
  return (int32_t)((uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24));
}

static inline int tsem_bam_scan_chain(const uint8_t* bytes, int64_t n_bytes, int64_t* rec_off /* cap + 1 */, int64_t cap, int64_t* n_rec,
                                      int64_t* consumed, char* msg, size_t msg_len) {
  int64_t p = 0, n = 0;
  while (n < cap && p + 4 <= n_bytes) {
    const int32_t bs = tsem_bam_scan_le32(bytes + p);
    if (bs < 32) {
      if (msg && msg_len) snprintf(msg, msg_len, "tsem_bam_scan: record %lld at byte %lld has block_size %d, below the 32 bytes of the fixed fields",
                                   (long long)n, (long long)p, (int)bs);
      return -1;
    }
    if (p + 4 + (int64_t)bs > n_bytes) break;
    rec_off[n++] = p;
    p += 4 + (int64_t)bs;
  }
  rec_off[n] = p;
  *n_rec = n;
  *consumed = p;
  return 0;
}
