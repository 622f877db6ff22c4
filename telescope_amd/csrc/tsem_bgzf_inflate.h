// One raw DEFLATE stream (RFC 1951) inflated: the body of k_bgzf_inflate (tsem_bgzf.hip) as __host__ __device__ inline functions, so
// that a stand-alone host program runs the very same code (tests/c_host/bgzf_inflate_check.cc).  No HIP header is needed.
//
// The functions are written for `nl` lanes that run them side by side with the same arguments but their own `lane` in [0, nl): the
// device passes a wave (nl = 64), a host program nl = 1.  Everything that decides the control flow — the bit buffer, the symbols, the
// positions — is computed by every lane from the same bytes, so the lanes never part ways; what is spread over them is the storing:
// the Huffman look-up tables, the bytes of a stored block, the bytes of a match (distance < length included: byte i of a match comes
// from out[at - distance + i % distance], which lies in front of the match), the CRC-32 slices.  Tables that one pass walks in order
// (counts, canonical symbol order, the code lengths) are stored by lane 0.  TSEM_BGZF_SYNC() stands between a store by one lane and a
// load of it by another; with one lane it is nothing.
//
// Bounds: every read of the input lies in [in, in + in_len), every write of the output in [out, out + out_cap), every back-reference
// in [out, write position).  A stream that breaks a bound or the format ends the call with a status code; nothing outside the two
// ranges is touched.
//
// Decoding: a primary table indexed by the next BGZF_LL_BITS (literal/length) or BGZF_D_BITS (distance) bits of the stream gives
// symbol << 4 | code length for the codes that short; 0 there means a longer code, or none, and the canonical walk of the counts per
// length (one bit at a time) settles it.  The code-length code is walked only.
//
// Which code sets are accepted is zlib's rule (inftrees.c): over-subscribed never; incomplete only for a literal/length or distance set
// whose longest code has one bit (in practice: a single distance code), or a distance set without any code; an unused code of such
// a set in the stream is an invalid symbol.  HLIT above 286 or HDIST above 30 count as invalid symbols (status 5); a repeat (16) with
// nothing in front of it, and a repeat that runs past HLIT + HDIST lengths, count as a broken code description (status 3).
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define TSEM_BGZF_HD __host__ __device__ inline
#else
#define TSEM_BGZF_HD inline
#endif
#if defined(__HIP_DEVICE_COMPILE__)
#define TSEM_BGZF_SYNC() __syncthreads()
#else
#define TSEM_BGZF_SYNC() ((void)0)
#endif

// status of a block (0 = fine); 9 and 10 come from the trailer's checks, 255 is set without inflating (include/telescope_em.h)
enum { BGZF_ST_OK = 0, BGZF_ST_BTYPE = 1, BGZF_ST_STORED_LEN = 2, BGZF_ST_CODE = 3, BGZF_ST_NO_EOB = 4, BGZF_ST_SYMBOL = 5,
       BGZF_ST_DISTANCE = 6, BGZF_ST_OUT_LONG = 7, BGZF_ST_INPUT = 8, BGZF_ST_OUT_SHORT = 9, BGZF_ST_CRC = 10, BGZF_ST_HOST = 255 };
enum { BGZF_LL_BITS = 10, BGZF_D_BITS = 8, BGZF_MAX_ISIZE = 65536, BGZF_MAX_LANES = 64 };

// the working storage of one stream: LDS on the device, anywhere on the host (4,968 bytes)
struct tsem_bgzf_tables {
  uint16_t lut_ll[1 << BGZF_LL_BITS], lut_d[1 << BGZF_D_BITS];
  uint16_t sym_ll[288], sym_d[32], sym_cl[20];              // symbols in canonical order
  uint16_t cnt_ll[16], cnt_d[16], cnt_cl[16], offs[16];     // codes per length; offs: scratch of the ordering
  uint8_t lens[320];                                        // code lengths as the block's header gives them
  uint32_t crc_tab[256], crc_part[BGZF_MAX_LANES];
};

struct bgzf_bits {
  const uint8_t* in; int32_t n, pos;
  uint64_t hold; int32_t bits;                              // the next `bits` bits of the stream, the first one lowest
};

// at least 32 bits in the buffer, or all that the input still has
TSEM_BGZF_HD void bgzf_refill(bgzf_bits& b) {
  if (b.bits >= 32) return;
  if (b.pos + 4 <= b.n) {
    const uint8_t* p = b.in + b.pos;
    const uint32_t w = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
    b.hold |= (uint64_t)w << b.bits;
    b.pos += 4; b.bits += 32;
    return;
  }
  while (b.pos < b.n) { b.hold |= (uint64_t)b.in[b.pos++] << b.bits; b.bits += 8; }     // (at most three bytes)
}
// k <= 16 bits off the buffer; false: the input does not have them
TSEM_BGZF_HD bool bgzf_take(bgzf_bits& b, int k, uint32_t* v) {
  if (b.bits < k) return false;
  *v = (uint32_t)b.hold & ((1u << k) - 1u);
  b.hold >>= k; b.bits -= k;
  return true;
}

// One symbol: >= 0, -1 the bits are no code of the set, -2 the input ends inside the code.  lut may be NULL (walk only).
TSEM_BGZF_HD int bgzf_decode(bgzf_bits& b, const uint16_t* lut, int lut_bits, const uint16_t* cnt, const uint16_t* sym) {
  if (lut) {
    const uint32_t e = lut[(uint32_t)b.hold & ((1u << lut_bits) - 1u)];
    if (e) {
      const int l = (int)(e & 15u);
      if (l > b.bits) return -2;
      b.hold >>= l; b.bits -= l;
      return (int)(e >> 4);
    }
  }
  int code = 0, first = 0, index = 0;
  uint64_t h = b.hold;
  for (int len = 1; len <= 15; ++len) {
    if (len > b.bits) return -2;
    code |= (int)(h & 1u); h >>= 1;
    const int count = cnt[len];
    if (code - count < first) { b.hold = h; b.bits -= len; return sym[index + (code - first)]; }
    index += count; first += count; first <<= 1; code <<= 1;
  }
  return -1;
}

// lens[0, n) -> cnt[0..15] and the symbols in canonical order (by length, then by value).  -1 over-subscribed, 0 complete, 1 incomplete;
// *max_len = the longest code's length (0: no code at all).
TSEM_BGZF_HD int bgzf_canon(const uint8_t* lens, int n, uint16_t* cnt, uint16_t* sym, uint16_t* offs, int lane, int* max_len) {
  TSEM_BGZF_SYNC();                                         // the lengths are stored; the tables of the block before are not read any more
  if (lane == 0) {
    for (int l = 0; l < 16; ++l) cnt[l] = 0;
    for (int s = 0; s < n; ++s) cnt[lens[s] & 15]++;
  }
  TSEM_BGZF_SYNC();
  int left = 1, mx = 0;
  for (int l = 1; l <= 15; ++l) {
    left <<= 1; left -= (int)cnt[l];
    if (left < 0) return -1;
    if (cnt[l]) mx = l;
  }
  if (lane == 0) {
    offs[1] = 0;
    for (int l = 1; l < 15; ++l) offs[l + 1] = (uint16_t)(offs[l] + cnt[l]);
    for (int s = 0; s < n; ++s)
      if (lens[s]) sym[offs[lens[s] & 15]++] = (uint16_t)s;
  }
  TSEM_BGZF_SYNC();
  *max_len = mx;
  return left > 0 ? 1 : 0;
}

TSEM_BGZF_HD uint32_t bgzf_rev16(uint32_t x) {
  x = ((x & 0xAAAAu) >> 1) | ((x & 0x5555u) << 1);
  x = ((x & 0xCCCCu) >> 2) | ((x & 0x3333u) << 2);
  x = ((x & 0xF0F0u) >> 4) | ((x & 0x0F0Fu) << 4);
  return ((x & 0xFF00u) >> 8) | ((x & 0x00FFu) << 8);
}

// the primary table of a set that bgzf_canon accepted (so no two codes claim one slot); the lanes share the symbols
TSEM_BGZF_HD void bgzf_fill_lut(uint16_t* lut, int lut_bits, const uint16_t* cnt, const uint16_t* sym, int lane, int nl) {
  const int size = 1 << lut_bits;
  for (int i = lane; i < size; i += nl) lut[i] = 0;
  TSEM_BGZF_SYNC();
  int code = 0, index = 0;                                  // the first code of this length (its first bit highest), its symbol's place
  for (int len = 1; len <= lut_bits; ++len) {
    const int c = cnt[len];
    for (int k = lane; k < c; k += nl) {
      const uint32_t r = bgzf_rev16((uint32_t)(code + k)) >> (16 - len);
      const uint16_t e = (uint16_t)((sym[index + k] << 4) | len);
      for (int j = (int)r; j < size; j += 1 << len) lut[j] = e;
    }
    code = (code + c) << 1; index += c;
  }
  TSEM_BGZF_SYNC();
}

// position i of the code-length code's lengths in the header: 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15 (five bits each)
TSEM_BGZF_HD int bgzf_cl_order(int i) {
  const uint64_t a = 16ull | 17ull << 5 | 18ull << 10 | 0ull << 15 | 8ull << 20 | 7ull << 25 | 9ull << 30 | 6ull << 35 | 10ull << 40 |
                     5ull << 45 | 11ull << 50 | 4ull << 55;
  const uint64_t c = 12ull | 3ull << 5 | 13ull << 10 | 2ull << 15 | 14ull << 20 | 1ull << 25 | 15ull << 30;
  return (int)((i < 12 ? a >> (5 * i) : c >> (5 * (i - 12))) & 31u);
}

// The stream in[0, in_len) into out[0, out_cap): BGZF_ST_*; *out_len = the bytes written when the final block ended (status 0 only).
TSEM_BGZF_HD int bgzf_inflate_stream(const uint8_t* in, int32_t in_len, uint8_t* out, int32_t out_cap, tsem_bgzf_tables* T, int lane,
                                     int nl, int32_t* out_len) {
  bgzf_bits b{in, in_len, 0, 0, 0};
  int32_t op = 0;
  uint32_t v = 0, last = 0;
  do {
    bgzf_refill(b);
    if (!bgzf_take(b, 3, &v)) return BGZF_ST_INPUT;
    last = v & 1u;
    const uint32_t type = v >> 1;
    if (type == 3) return BGZF_ST_BTYPE;
    if (type == 0) {                                        // stored: back to the byte boundary, LEN, NLEN, the bytes
      b.pos -= b.bits >> 3;                                 // (whole bytes that were buffered go back)
      b.hold = 0; b.bits = 0;
      if (b.pos + 4 > in_len) return BGZF_ST_INPUT;
      const uint32_t len = (uint32_t)in[b.pos] | ((uint32_t)in[b.pos + 1] << 8);
      const uint32_t nlen = (uint32_t)in[b.pos + 2] | ((uint32_t)in[b.pos + 3] << 8);
      b.pos += 4;
      if (len != (~nlen & 0xFFFFu)) return BGZF_ST_STORED_LEN;
      if (b.pos + (int32_t)len > in_len) return BGZF_ST_INPUT;
      if (op + (int32_t)len > out_cap) return BGZF_ST_OUT_LONG;
      for (int32_t i = lane; i < (int32_t)len; i += nl) out[op + i] = in[b.pos + i];
      b.pos += (int32_t)len; op += (int32_t)len;
      continue;
    }
    int nlen = 288, ndist = 32, mx = 0, r;
    if (type == 1) {                                        // fixed: the lengths of RFC 1951 3.2.6, all 32 distance codes
      TSEM_BGZF_SYNC();
      for (int s = lane; s < 320; s += nl) T->lens[s] = (uint8_t)(s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : s < 288 ? 8 : 5);
    } else {
      if (!bgzf_take(b, 14, &v)) return BGZF_ST_INPUT;
      nlen = (int)(v & 31u) + 257; ndist = (int)((v >> 5) & 31u) + 1;
      const int ncode = (int)(v >> 10) + 4;
      if (nlen > 286 || ndist > 30) return BGZF_ST_SYMBOL;
      TSEM_BGZF_SYNC();
      for (int i = 0; i < 19; ++i) {
        v = 0;
        if (i < ncode) {
          bgzf_refill(b);
          if (!bgzf_take(b, 3, &v)) return BGZF_ST_INPUT;
        }
        if (lane == 0) T->lens[bgzf_cl_order(i)] = (uint8_t)v;
      }
      r = bgzf_canon(T->lens, 19, T->cnt_cl, T->sym_cl, T->offs, lane, &mx);
      if (r != 0) return BGZF_ST_CODE;
      const int total = nlen + ndist;
      int i = 0, prev = 0, eob = 0;
      while (i < total) {
        bgzf_refill(b);
        const int s = bgzf_decode(b, nullptr, 0, T->cnt_cl, T->sym_cl);
        if (s < 0) return s == -2 ? BGZF_ST_INPUT : BGZF_ST_CODE;
        int rep = 1, val = s;
        if (s == 16) {
          if (i == 0) return BGZF_ST_CODE;
          if (!bgzf_take(b, 2, &v)) return BGZF_ST_INPUT;
          rep = 3 + (int)v; val = prev;
        } else if (s == 17) {
          if (!bgzf_take(b, 3, &v)) return BGZF_ST_INPUT;
          rep = 3 + (int)v; val = 0;
        } else if (s == 18) {
          if (!bgzf_take(b, 7, &v)) return BGZF_ST_INPUT;
          rep = 11 + (int)v; val = 0;
        }
        if (i + rep > total) return BGZF_ST_CODE;
        if (lane == 0)
          for (int k = 0; k < rep; ++k) T->lens[i + k] = (uint8_t)val;       // (a repeat may run from the literal/length lengths into the distance lengths)
        if (i <= 256 && 256 < i + rep) eob = val;
        i += rep; prev = val;
      }
      if (!eob) return BGZF_ST_NO_EOB;
    }
    r = bgzf_canon(T->lens, nlen, T->cnt_ll, T->sym_ll, T->offs, lane, &mx);
    if (r < 0 || (r > 0 && mx > 1)) return BGZF_ST_CODE;
    r = bgzf_canon(T->lens + nlen, ndist, T->cnt_d, T->sym_d, T->offs, lane, &mx);
    if (r < 0 || (r > 0 && mx > 1)) return BGZF_ST_CODE;
    bgzf_fill_lut(T->lut_ll, BGZF_LL_BITS, T->cnt_ll, T->sym_ll, lane, nl);
    bgzf_fill_lut(T->lut_d, BGZF_D_BITS, T->cnt_d, T->sym_d, lane, nl);
    for (;;) {
      bgzf_refill(b);
      int s = bgzf_decode(b, T->lut_ll, BGZF_LL_BITS, T->cnt_ll, T->sym_ll);
      if (s < 0) return s == -2 ? BGZF_ST_INPUT : BGZF_ST_SYMBOL;
      if (s < 256) {
        if (op >= out_cap) return BGZF_ST_OUT_LONG;
        if (lane == 0) out[op] = (uint8_t)s;
        ++op;
        continue;
      }
      if (s == 256) break;
      if (s >= 286) return BGZF_ST_SYMBOL;
      s -= 257;                                             // length 3 .. 258: base and extra bits from the symbol's number
      int eb = s < 8 || s == 28 ? 0 : (s - 4) >> 2;
      int32_t len = s < 8 ? 3 + s : s == 28 ? 258 : 3 + ((4 + (s & 3)) << eb);
      if (!bgzf_take(b, eb, &v)) return BGZF_ST_INPUT;
      len += (int32_t)v;
      bgzf_refill(b);
      const int d = bgzf_decode(b, T->lut_d, BGZF_D_BITS, T->cnt_d, T->sym_d);
      if (d < 0) return d == -2 ? BGZF_ST_INPUT : BGZF_ST_SYMBOL;
      if (d >= 30) return BGZF_ST_SYMBOL;
      eb = d < 4 ? 0 : (d - 2) >> 1;                        // distance 1 .. 32768 likewise
      int32_t dist = d < 4 ? 1 + d : 1 + ((2 + (d & 1)) << eb);
      if (!bgzf_take(b, eb, &v)) return BGZF_ST_INPUT;
      dist += (int32_t)v;
      if (dist > op) return BGZF_ST_DISTANCE;
      if (op + len > out_cap) return BGZF_ST_OUT_LONG;
      TSEM_BGZF_SYNC();                                     // what the match copies was stored by other lanes
      const uint8_t* from = out + (op - dist);
      if (dist >= len) {
        for (int32_t i = lane; i < len; i += nl) out[op + i] = from[i];
      } else {
        for (int32_t i = lane; i < len; i += nl) out[op + i] = from[i % dist];
      }
      op += len;
    }
  } while (!last);
  *out_len = op;
  return BGZF_ST_OK;
}

// ---- CRC-32 (the gzip polynomial, reflected): a slice per lane, joined by multiplication by x^(8 * length) modulo the polynomial
TSEM_BGZF_HD void bgzf_crc_table(uint32_t* tab, int lane, int nl) {
  for (int i = lane; i < 256; i += nl) {
    uint32_t c = (uint32_t)i;
    for (int k = 0; k < 8; ++k) c = (c & 1u) ? 0xEDB88320u ^ (c >> 1) : c >> 1;
    tab[i] = c;
  }
}
TSEM_BGZF_HD uint32_t bgzf_crc_bytes(const uint32_t* tab, const uint8_t* p, int32_t n) {
  uint32_t c = 0xFFFFFFFFu;
  for (int32_t i = 0; i < n; ++i) c = tab[(c ^ p[i]) & 255u] ^ (c >> 8);
  return ~c;
}
// a * b modulo the polynomial; bit 31 is x^0
TSEM_BGZF_HD uint32_t bgzf_multmodp(uint32_t a, uint32_t b) {
  uint32_t p = 0;
  for (uint32_t m = 0x80000000u; m; m >>= 1) {
    if (a & m) p ^= b;
    b = (b & 1u) ? (b >> 1) ^ 0xEDB88320u : b >> 1;
  }
  return p;
}
// x^(8 n) modulo the polynomial
TSEM_BGZF_HD uint32_t bgzf_x8n(uint32_t n) {
  uint32_t r = 0x80000000u, sq = 0x00800000u;              // 1, x^8
  for (; n; n >>= 1) {
    if (n & 1u) r = bgzf_multmodp(sq, r);
    sq = bgzf_multmodp(sq, sq);
  }
  return r;
}
// slice `lane` of p[0, n): bytes [lane * S, (lane + 1) * S) with S = ceil(n / nl)
TSEM_BGZF_HD void bgzf_crc_slice(tsem_bgzf_tables* T, const uint8_t* p, int32_t n, int lane, int nl) {
  const int32_t S = (n + nl - 1) / nl;
  const int32_t lo = lane * S < n ? lane * S : n, hi = lo + S < n ? lo + S : n;
  T->crc_part[lane] = bgzf_crc_bytes(T->crc_tab, p + lo, hi - lo);
}
// crc(A B) = crc(A) * x^(8 |B|) + crc(B), slice after slice
TSEM_BGZF_HD uint32_t bgzf_crc_join(const tsem_bgzf_tables* T, int32_t n, int nl) {
  const int32_t S = (n + nl - 1) / nl;
  const uint32_t xs = bgzf_x8n((uint32_t)S);
  uint32_t acc = 0;
  for (int l = 0; l < nl; ++l) {
    const int32_t lo = l * S < n ? l * S : n, hi = lo + S < n ? lo + S : n;
    if (hi == lo) break;
    acc = bgzf_multmodp(hi - lo == S ? xs : bgzf_x8n((uint32_t)(hi - lo)), acc) ^ T->crc_part[l];
  }
  return acc;
}

// One BGZF block: the payload in[0, in_len) into out[0, isize), then the trailer's two checks.  nl <= BGZF_MAX_LANES, isize <=
// BGZF_MAX_ISIZE (the caller leaves a larger claim to the host: BGZF_ST_HOST).
TSEM_BGZF_HD int bgzf_inflate_block(const uint8_t* in, int32_t in_len, uint8_t* out, int32_t isize, uint32_t crc, tsem_bgzf_tables* T,
                                    int lane, int nl) {
  int32_t n = 0;
  const int st = bgzf_inflate_stream(in, in_len, out, isize, T, lane, nl, &n);
  if (st) return st;
  if (n != isize) return BGZF_ST_OUT_SHORT;
  bgzf_crc_table(T->crc_tab, lane, nl);
  TSEM_BGZF_SYNC();                                         // the table, and the output's last bytes
  bgzf_crc_slice(T, out, n, lane, nl);
  TSEM_BGZF_SYNC();
  return bgzf_crc_join(T, n, nl) == crc ? BGZF_ST_OK : BGZF_ST_CRC;
}
