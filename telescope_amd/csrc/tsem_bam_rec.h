// One BAM record's fields, decoded from the bytes of a chunk: the body of k_bam_decode (tsem_bam.hip) as a __host__ __device__ inline
// function, so that a stand-alone host program runs the very same code (tests/c_host/bam_decode_check.cc).  No HIP header is needed.
//
// Every read is bounded by the record's end (`end`, the offset behind its last byte): bam_rd* are only called behind a check against
// it, and a walk that would leave the record stops with a status code.  Multi-byte fields are assembled from bytes — nothing in a
// BAM record is aligned.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define TSEM_BAM_HD __host__ __device__ inline
#else
#define TSEM_BAM_HD inline
#endif

// rows of the int32 result matrix [TSEM_BAM_COLS][n_rec] of tsem_bam_chunk: 0-15 per record (tsem_bam_rec, in this order), the rest
// per pair slot / map slot / bundle (include/telescope_em.h)
enum {
  BAM_C_REF = 0, BAM_C_POS, BAM_C_NREF, BAM_C_NPOS, BAM_C_ATLEN, BAM_C_FLAG, BAM_C_LRN, BAM_C_NCIG, BAM_C_LSEQ, BAM_C_AS, BAM_C_BITS,
  BAM_C_BCOFF, BAM_C_BCLEN, BAM_C_UMIOFF, BAM_C_UMILEN, BAM_C_STATUS,
  BAM_C_PAIR1, BAM_C_PAIR2, BAM_C_BUNDLE, BAM_C_PFEAT, BAM_C_PAS, BAM_C_PLEN, BAM_C_MFEAT, BAM_C_MAS, BAM_C_MLEN,
  BAM_C_BCODE, BAM_C_BNPAIRS, BAM_C_BNMAPS, BAM_C_BCLASS, BAM_C_BMIN, BAM_C_BMAX, BAM_C_BNMAPPED, BAM_C_BFLAG, BAM_C_SCRATCH,
  TSEM_BAM_COLS_
};
static_assert(TSEM_BAM_COLS_ == 34, "include/telescope_em.h: TSEM_BAM_COLS");

enum { BAM_BIT_AS = 1, BAM_BIT_NEWNAME = 2, BAM_BIT_HOST = 4 };
// status of a record (0 = fine); 10 is set by k_bam_overlap
enum { BAM_ST_SIZE = 1, BAM_ST_NAME = 2, BAM_ST_CIGAR = 3, BAM_ST_SEQ = 4, BAM_ST_AUX_HEAD = 5, BAM_ST_AUX_VALUE = 6, BAM_ST_AUX_NUL = 7,
       BAM_ST_AUX_ARRAY = 8, BAM_ST_AUX_TYPE = 9, BAM_ST_NO_AS = 10 };

struct tsem_bam_rec {
  int32_t ref_id, pos, nref, npos;
  int32_t atlen;       // |tlen| as a uint32 bit pattern (|INT32_MIN| = 2^31 keeps its own value: the mate keys only test equality)
  int32_t flag, l_rn, n_cig, l_seq;
  int32_t as;          // AS (valid with BAM_BIT_AS)
  int32_t bits;        // BAM_BIT_*
  int32_t bc_off, bc_len, umi_off, umi_len;   // the barcode / UMI Z tag's value: offset from the record's size field and length, -1 = no such tag
  int32_t status;      // BAM_ST_*
};

TSEM_BAM_HD uint32_t bam_rd16(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }
TSEM_BAM_HD uint32_t bam_rd32(const uint8_t* p) {
  return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}
// bytes of a fixed-size aux value, 0 for every other type letter
TSEM_BAM_HD int bam_aux_size(uint8_t t) {
  switch (t) {
    case 'c': case 'C': return 1;
    case 's': case 'S': return 2;
    case 'i': case 'I': case 'f': return 4;
    default: return 0;
  }
}

// Record at [off, end) of `bytes` (off = its size field; end - off >= 36 is the caller's promise, as tsem_bam_scan gives it);
// [prev_off, prev_end) = the record in front of it, prev_off < 0 for the first of a chunk.  btag / utag: the two letters of the
// barcode / UMI tag as first | second << 8, or -1.
TSEM_BAM_HD void bam_decode_record(const uint8_t* bytes, int64_t off, int64_t end, int64_t prev_off, int64_t prev_end, int32_t btag,
                                   int32_t utag, tsem_bam_rec* r) {
  const uint8_t* b = bytes + off + 4;                          // the record's body
  const int64_t bs = end - off - 4;                            // ... and its length, >= 32
  r->ref_id = (int32_t)bam_rd32(b + 0);
  r->pos = (int32_t)bam_rd32(b + 4);
  r->l_rn = b[8];
  r->n_cig = (int32_t)bam_rd16(b + 12);
  r->flag = (int32_t)bam_rd16(b + 14);
  r->l_seq = (int32_t)bam_rd32(b + 16);
  r->nref = (int32_t)bam_rd32(b + 20);
  r->npos = (int32_t)bam_rd32(b + 24);
  const int32_t tlen = (int32_t)bam_rd32(b + 28);
  r->atlen = (int32_t)(tlen < 0 ? 0u - (uint32_t)tlen : (uint32_t)tlen);
  r->as = 0; r->bits = 0; r->bc_off = r->bc_len = r->umi_off = r->umi_len = -1; r->status = 0;
  if ((int64_t)(int32_t)bam_rd32(bytes + off) != bs) { r->status = BAM_ST_SIZE; r->bits = BAM_BIT_NEWNAME; return; }
  if (r->l_rn < 1 || 32 + (int64_t)r->l_rn > bs) { r->status = BAM_ST_NAME; r->bits = BAM_BIT_NEWNAME; return; }
  // "the name differs from the previous record's": the length and the l_rn - 1 bytes in front of the terminator
  bool differs = true;
  if (prev_off >= 0 && prev_end - prev_off >= 36) {
    const uint8_t* pb = bytes + prev_off + 4;
    const int32_t pl = pb[8];
    if (pl == r->l_rn && prev_off + 4 + 32 + (int64_t)pl <= prev_end) {
      differs = false;
      for (int32_t k = 0; k + 1 < pl; ++k)
        if (pb[32 + k] != b[32 + k]) { differs = true; break; }
    }
  }
  if (differs) r->bits |= BAM_BIT_NEWNAME;
  int64_t p = 32 + (int64_t)r->l_rn;
  if (p + 4 * (int64_t)r->n_cig > bs) { r->status = BAM_ST_CIGAR; return; }
  p += 4 * (int64_t)r->n_cig;
  if (r->l_seq < 0) { r->bits |= BAM_BIT_HOST; return; }       // (the host loader steps backwards here: its answer, not ours)
  p += ((int64_t)r->l_seq + 1) / 2 + (int64_t)r->l_seq;
  if (p > bs) { r->status = BAM_ST_SEQ; return; }
  while (p < bs) {
    if (p + 3 > bs) { r->status = BAM_ST_AUX_HEAD; return; }
    const int32_t tag = (int32_t)bam_rd16(b + p);
    const uint8_t typ = b[p + 2];
    p += 3;
    const int sz = bam_aux_size(typ);
    if (sz) {
      if (p + sz > bs) { r->status = BAM_ST_AUX_VALUE; return; }
      if (tag == ('A' | ('S' << 8))) {
        r->bits |= BAM_BIT_AS;
        switch (typ) {
          case 'c': r->as = (int8_t)b[p]; break;
          case 'C': r->as = b[p]; break;
          case 's': r->as = (int16_t)bam_rd16(b + p); break;
          case 'S': r->as = (int32_t)bam_rd16(b + p); break;
          case 'i': r->as = (int32_t)bam_rd32(b + p); break;
          case 'I': r->as = (int32_t)bam_rd32(b + p); if (r->as < 0) r->bits |= BAM_BIT_HOST; break;   // above 2^31 - 1
          default: r->bits |= BAM_BIT_HOST; break;                                                    // a float AS
        }
      }
      p += sz;
    } else if (typ == 'A') {
      if (p + 1 > bs) { r->status = BAM_ST_AUX_VALUE; return; }
      p += 1;
    } else if (typ == 'Z' || typ == 'H') {
      int64_t q = p;
      while (q < bs && b[q] != 0) ++q;
      if (q >= bs) { r->status = BAM_ST_AUX_NUL; return; }
      if (typ == 'Z' && tag == btag) { r->bc_off = (int32_t)(4 + p); r->bc_len = (int32_t)(q - p); }
      if (typ == 'Z' && tag == utag) { r->umi_off = (int32_t)(4 + p); r->umi_len = (int32_t)(q - p); }
      p = q + 1;
    } else if (typ == 'B') {
      if (p + 5 > bs) { r->status = BAM_ST_AUX_ARRAY; return; }
      const int esz = bam_aux_size(b[p]);
      const int32_t cnt = (int32_t)bam_rd32(b + p + 1);
      if (!esz || cnt < 0 || p + 5 + (int64_t)cnt * esz > bs) { r->status = BAM_ST_AUX_ARRAY; return; }
      p += 5 + (int64_t)cnt * esz;
    } else {
      r->status = BAM_ST_AUX_TYPE; return;
    }
  }
}
