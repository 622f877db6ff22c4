// One raw DEFLATE stream (RFC 1951) written: the body of k_bgzf_deflate (tsem_bgzf.hip) as __host__ __device__ inline functions, the
// counterpart of tsem_bgzf_inflate.h.  A stand-alone host program runs the very same code (tests/c_host/bgzf_deflate_check.cc), and
// tsem_bgzf_deflate_host is this body with one lane.
//
// The body is a sequence of PHASES with TSEM_BGZF_SYNC() between them.  Within a phase the `nl` lanes (lane in [0, nl)) share work
// that is indexed by position, token, symbol or chunk, and they meet only through operations whose result does not depend on their
// order: a maximum (the hash heads), integer additions (the histograms), stores to places that one index owns.  What decides the
// control flow is read from the shared tables by every lane alike, so the lanes never part ways.  THE BYTES THEREFORE DO NOT DEPEND ON
// nl: one lane on the host gives what a wave of 64 gives, in every run.
//
//   1  matches    The input goes by in tiles of BGZF_DEF_TILE positions (the tile is a constant of the format of the work, not nl).
//                 1a  every position of the tile: its hash of three bytes, the candidate in head[hash] — the latest position with that
//                     hash in an EARLIER tile — and the candidate one byte back (runs; the head table cannot see into its own tile);
//                     the longer match of the two, 3..258 bytes, never past in + len, a candidate more than 32,768 back dropped, a
//                     match of 3 bytes more than 4,096 back too (it costs more bits than three literals).
//                 1b  every position: head[hash] = max(head[hash], position + 1).
//                 1c  the greedy parse, a serial chain that every lane follows: at `cur` take the match if there is one, else the
//                     literal; lane 0 stores the token.  A tile that a match covers whole is hashed only.
//   2  histogram  of the tokens' literal/length and distance symbols (end-of-block counted once).
//   3  codes      bgzf_build_lengths for both sets (limit 15), then for the code-length code (limit 7): rank of every used symbol by
//                 (count, symbol) in parallel, then lane 0: the in-place minimum-redundancy construction of Moffat and Katajainen on
//                 the sorted counts, the count of codes per length, lengths above the limit folded into it and the Kraft sum brought
//                 back to exactly 1 by moving one code down a level at a time, the lengths dealt out longest first to the rarest.
//                 The lengths of a dynamic block are SPELLED OUT, one code-length symbol 0..15 each, without the run symbols 16/17/18.
//   4  choice     the bits of the stored, the fixed and the dynamic form from the histograms; the smallest, a tie to the simpler one.
//                 Stored is len + 5 bytes, so no stream is longer than that.
//   5  emit       chunks of BGZF_DEF_CHUNK tokens (chunk 0 is the block header): the bits per chunk, their prefix sum, then every chunk
//                 writes its own whole bytes; a byte that a chunk shares with a neighbour goes to a list and is stored by one lane,
//                 OR-ed together, afterwards.
//   6  CRC-32     bgzf_crc_slice / bgzf_crc_join of tsem_bgzf_inflate.h over the input.
//
// Bounds: reads lie in [in, in + len), writes in [out, out + len + 5) and tok[0, len + 1).
#pragma once
#include <cstdint>
#include <cstring>

#include "tsem_bgzf_inflate.h"

#if defined(__HIP_DEVICE_COMPILE__)
#define TSEM_BGZF_ATOMIC_MAX(p, v) atomicMax((p), (v))
#define TSEM_BGZF_ATOMIC_ADD(p, v) atomicAdd((p), (v))
#else
#define TSEM_BGZF_ATOMIC_MAX(p, v) do { if (*(p) < (v)) *(p) = (v); } while (0)
#define TSEM_BGZF_ATOMIC_ADD(p, v) do { *(p) += (v); } while (0)
#endif

enum { BGZF_DEF_BLOCK = 0xff00, BGZF_DEF_HASH_BITS = 13, BGZF_DEF_TILE = 64, BGZF_DEF_CHUNK = 128,
       BGZF_DEF_MAX_CHUNKS = (BGZF_DEF_BLOCK + 1 + BGZF_DEF_CHUNK - 1) / BGZF_DEF_CHUNK + 1,       // token chunks and the header: 512
       BGZF_DEF_WINDOW = 32768, BGZF_DEF_TOO_FAR = 4096, BGZF_DEF_NONE = 0xFFFF };
enum { BGZF_DEF_STORED = 0, BGZF_DEF_FIXED = 1, BGZF_DEF_DYNAMIC = 2 };

// working storage of the code-length builder
struct bgzf_code_work {
  uint32_t a[288];                                          // the used symbols' counts in ascending order; then their depths
  uint16_t sym[288];                                        // the symbol at each place of that order
  uint16_t cnt[34];                                         // codes per length (depths above 32 counted at 33)
};

// the working storage of one block: LDS on the device, anywhere on the host (about 38 KiB).  The head table is dead when the
// matches are found; what the later phases need lies over it.
struct tsem_bgzf_deflate_tables {
  union {
    uint32_t head[1 << BGZF_DEF_HASH_BITS];                 // position + 1 of the latest occurrence of a hash; 0: none
    struct {
      tsem_bgzf_tables crc;
      uint32_t chunk_bits[BGZF_DEF_MAX_CHUNKS + 1];         // bits per chunk, then the bit at which each begins
      uint16_t part_idx[2 * BGZF_DEF_MAX_CHUNKS];           // shared bytes: where, BGZF_DEF_NONE for none
      uint8_t part_val[2 * BGZF_DEF_MAX_CHUNKS];            // ... and the chunk's bits of them
    } late;
  } u;
  uint16_t mlen[BGZF_DEF_TILE], mdist[BGZF_DEF_TILE], mhash[BGZF_DEF_TILE];      // per position of the tile: length (0: none), distance - 1, hash
  uint8_t mlit[BGZF_DEF_TILE];
  uint32_t hist_ll[288], hist_d[32], hist_cl[16];
  uint8_t len_ll[288], len_d[32], len_cl[16];
  uint16_t code_ll[288], code_d[32], code_cl[16];           // the codes, their first bit lowest
  bgzf_code_work work;
};

TSEM_BGZF_HD int bgzf_len_extra(int sym /* 257 .. 285 */) { const int s = sym - 257; return s < 8 || s == 28 ? 0 : (s - 4) >> 2; }
TSEM_BGZF_HD int bgzf_dist_extra(int sym /* 0 .. 29 */) { return sym < 4 ? 0 : (sym - 2) >> 1; }
// length - 3 in [0, 255] -> symbol and the number of extra bits (their value: the low bits of l)
TSEM_BGZF_HD int bgzf_len_symbol(int l, int* eb) {
  if (l < 8) { *eb = 0; return 257 + l; }
  if (l == 255) { *eb = 0; return 285; }
  const int n = 31 - __builtin_clz((unsigned)l);
  *eb = n - 2;
  return 257 + 4 * (n - 2) + 4 + ((l >> (n - 2)) & 3);
}
// distance - 1 in [0, 32767] likewise
TSEM_BGZF_HD int bgzf_dist_symbol(int d, int* eb) {
  if (d < 4) { *eb = 0; return d; }
  const int n = 31 - __builtin_clz((unsigned)d);
  *eb = n - 1;
  return 2 * n + ((d >> (n - 1)) & 1);
}

// the bytes that a[0, maxl) and b[0, maxl) share at their start; a < b, b + maxl within the input
TSEM_BGZF_HD int bgzf_match_len(const uint8_t* a, const uint8_t* b, int maxl) {
  int k = 0;
  while (k + 8 <= maxl) {
    uint64_t x, y;
    memcpy(&x, a + k, 8); memcpy(&y, b + k, 8);
    const uint64_t d = x ^ y;
    if (d) return k + (__builtin_ctzll(d) >> 3);
    k += 8;
  }
  while (k < maxl && a[k] == b[k]) ++k;
  return k;
}

// hist[0, n) -> lens[0, n): a prefix code of at most `limit` bits per symbol over the symbols with a count; one used symbol gets one
// bit, two or more a complete code (Kraft sum 1).  n <= 288, 2^limit >= n.
TSEM_BGZF_HD void bgzf_build_lengths(const uint32_t* hist, int n, int limit, uint8_t* lens, bgzf_code_work* W, int lane, int nl) {
  TSEM_BGZF_SYNC();                                         // the counts are stored; W is free
  for (int s = lane; s < n; s += nl) {
    const uint32_t f = hist[s];
    lens[s] = 0;
    if (!f) continue;
    int r = 0;
    for (int t = 0; t < n; ++t) { const uint32_t g = hist[t]; r += (g && (g < f || (g == f && t < s))) ? 1 : 0; }
    W->a[r] = f; W->sym[r] = (uint16_t)s;
  }
  int used = 0;
  for (int t = 0; t < n; ++t) used += hist[t] ? 1 : 0;
  TSEM_BGZF_SYNC();
  if (used == 0) return;
  if (lane == 0) {
    if (used == 1) {
      lens[W->sym[0]] = 1;
    } else {
      uint32_t* A = W->a;
      // minimum-redundancy depths in place (Moffat & Katajainen 1995): parents, then depths of internal nodes, then of the leaves
      A[0] += A[1];
      int root = 0, leaf = 2;
      for (int next = 1; next < used - 1; ++next) {
        if (leaf >= used || A[root] < A[leaf]) { A[next] = A[root]; A[root++] = (uint32_t)next; } else A[next] = A[leaf++];
        if (leaf >= used || (root < next && A[root] < A[leaf])) { A[next] += A[root]; A[root++] = (uint32_t)next; } else A[next] += A[leaf++];
      }
      A[used - 2] = 0;
      for (int next = used - 3; next >= 0; --next) A[next] = A[A[next]] + 1;
      int avbl = 1, usd = 0, dpth = 0, next = used - 1;
      root = used - 2;
      while (avbl > 0) {
        while (root >= 0 && (int)A[root] == dpth) { ++usd; --root; }
        while (avbl > usd) { A[next--] = (uint32_t)dpth; --avbl; }
        avbl = 2 * usd; ++dpth; usd = 0;
      }
      // codes per length, the depths above the limit folded into it; then one code of the limit's length leaves and one shorter
      // code moves a level down to make room for two, until the Kraft sum is 1 again
      uint16_t* cnt = W->cnt;
      for (int l = 0; l <= limit; ++l) cnt[l] = 0;
      for (int i = 0; i < used; ++i) cnt[(int)A[i] < limit ? (int)A[i] : limit]++;
      uint32_t total = 0;
      for (int l = 1; l <= limit; ++l) total += (uint32_t)cnt[l] << (limit - l);
      while (total > (1u << limit)) {
        cnt[limit]--;
        for (int l = limit - 1; l >= 1; --l)
          if (cnt[l]) { cnt[l]--; cnt[l + 1] += 2; break; }
        --total;
      }
      int i = 0;                                            // the rarest symbol first: the longest codes
      for (int l = limit; l >= 1; --l)
        for (int k = 0; k < (int)cnt[l]; ++k) lens[W->sym[i++]] = (uint8_t)l;
    }
  }
  TSEM_BGZF_SYNC();
}

// lens[0, n) -> the canonical codes of RFC 1951 3.2.2, their first bit lowest (as the stream takes them).  One lane.
TSEM_BGZF_HD void bgzf_assign_codes(const uint8_t* lens, int n, uint16_t* code, uint16_t* cnt /* 34 */) {
  for (int l = 0; l < 17; ++l) cnt[l] = 0;
  for (int s = 0; s < n; ++s) cnt[lens[s]]++;
  cnt[0] = 0;
  uint32_t c = 0, prev = 0;
  for (int l = 1; l <= 15; ++l) { c = (c + prev) << 1; prev = cnt[l]; cnt[l] = (uint16_t)c; }   // cnt[l]: now the next code of length l
  for (int s = 0; s < n; ++s) {
    const int l = lens[s];
    code[s] = l ? (uint16_t)(bgzf_rev16((uint32_t)cnt[l]++) >> (16 - l)) : 0;
  }
}

// a writer of the bits [start, ...) of the stream on behalf of chunk k: whole bytes go to out, the byte it begins in (unless it
// begins on a boundary) and the byte it ends in go to the chunk's two places of the shared-byte list
struct bgzf_bitw {
  uint8_t* out; int32_t pos; uint64_t acc; int nb; bool head;
  uint16_t* pidx; uint8_t* pval;
};
TSEM_BGZF_HD void bgzf_bitw_open(bgzf_bitw& w, uint8_t* out, uint32_t start, tsem_bgzf_deflate_tables* T, int k) {
  w.out = out; w.pos = (int32_t)(start >> 3); w.acc = 0; w.nb = (int)(start & 7u); w.head = w.nb != 0;
  w.pidx = T->u.late.part_idx + 2 * k; w.pval = T->u.late.part_val + 2 * k;
  w.pidx[0] = w.pidx[1] = BGZF_DEF_NONE;
}
TSEM_BGZF_HD void bgzf_bitw_put(bgzf_bitw& w, uint32_t v, int n) { w.acc |= (uint64_t)v << w.nb; w.nb += n; }   // (at most 56 bits between flushes)
TSEM_BGZF_HD void bgzf_bitw_flush(bgzf_bitw& w) {
  while (w.nb >= 8) {
    const uint8_t b = (uint8_t)(w.acc & 255u);
    if (w.head) { w.pidx[0] = (uint16_t)w.pos; w.pval[0] = b; w.head = false; } else w.out[w.pos] = b;
    ++w.pos; w.acc >>= 8; w.nb -= 8;
  }
}
TSEM_BGZF_HD void bgzf_bitw_close(bgzf_bitw& w) {
  bgzf_bitw_flush(w);
  if (w.nb == 0) return;
  const int at = w.head ? 0 : 1;                            // (a chunk that never left its first byte has that one only)
  w.pidx[at] = (uint16_t)w.pos; w.pval[at] = (uint8_t)(w.acc & 255u);
}

// the bits of token t under the codes of T
TSEM_BGZF_HD int bgzf_token_bits(const tsem_bgzf_deflate_tables* T, uint32_t t) {
  if (!(t >> 31)) return T->len_ll[t];
  int e1, e2;
  const int ls = bgzf_len_symbol((int)((t >> 16) & 255u), &e1), ds = bgzf_dist_symbol((int)(t & 0x7FFFu), &e2);
  return T->len_ll[ls] + e1 + T->len_d[ds] + e2;
}

// The stream of in[0, len), 0 <= len <= 0xff00, into out[0, cap), cap >= len + 5: its length (>= 2), or -1 for arguments out of range
// (-2: the emit's bit count is not the one that step 4 counted — a defect of this code that no input is known to reach; nothing is written).
// *crc = CRC-32 of the input; *form = BGZF_DEF_STORED / _FIXED / _DYNAMIC.  tok: len + 1 words of scratch that this block owns.
TSEM_BGZF_HD int32_t bgzf_deflate_block(const uint8_t* in, int32_t len, uint8_t* out, int32_t cap, uint32_t* crc, int32_t* form,
                                        tsem_bgzf_deflate_tables* T, uint32_t* tok, int lane, int nl) {
  if (len < 0 || len > BGZF_DEF_BLOCK || cap < len + 5) return -1;
  // ---- 1: matches
  for (int i = lane; i < (1 << BGZF_DEF_HASH_BITS); i += nl) T->u.head[i] = 0;
  for (int s = lane; s < 288; s += nl) { T->hist_ll[s] = 0; T->len_ll[s] = 0; }
  for (int s = lane; s < 32; s += nl) { T->hist_d[s] = 0; T->len_d[s] = 0; }
  for (int s = lane; s < 16; s += nl) T->hist_cl[s] = 0;
  TSEM_BGZF_SYNC();
  int32_t cur = 0, ntok = 0;
  for (int32_t t0 = 0; t0 < len; t0 += BGZF_DEF_TILE) {
    const bool covered = cur >= t0 + BGZF_DEF_TILE;         // a match runs over the whole tile: its positions are hashed only
    for (int j = lane; j < BGZF_DEF_TILE; j += nl) {
      const int32_t p = t0 + j;
      int ml = 0, md = 0;
      uint32_t h = BGZF_DEF_NONE;
      if (p < len) {
        const int maxl = len - p < 258 ? len - p : 258;
        if (maxl >= 3) {
          h = (((uint32_t)in[p] | ((uint32_t)in[p + 1] << 8) | ((uint32_t)in[p + 2] << 16)) * 0x9E3779B1u) >> (32 - BGZF_DEF_HASH_BITS);
          if (!covered) {
            const uint32_t c = T->u.head[h];
            if (c) {
              const int32_t dist = p - (int32_t)(c - 1);
              if (dist <= BGZF_DEF_WINDOW) {
                const int l = bgzf_match_len(in + (c - 1), in + p, maxl);
                if (l > 3 || (l == 3 && dist <= BGZF_DEF_TOO_FAR)) { ml = l; md = dist; }
              }
            }
            if (p >= 1) {
              const int l = bgzf_match_len(in + p - 1, in + p, maxl);
              if (l >= 3 && l >= ml) { ml = l; md = 1; }
            }
          }
        }
        T->mlit[j] = in[p];
      }
      T->mlen[j] = (uint16_t)ml; T->mdist[j] = (uint16_t)(ml ? md - 1 : 0); T->mhash[j] = (uint16_t)h;
    }
    TSEM_BGZF_SYNC();
    for (int j = lane; j < BGZF_DEF_TILE; j += nl) {
      const uint32_t h = T->mhash[j];
      if (h != BGZF_DEF_NONE) TSEM_BGZF_ATOMIC_MAX(&T->u.head[h], (uint32_t)(t0 + j + 1));
    }
    const int32_t t1 = t0 + BGZF_DEF_TILE < len ? t0 + BGZF_DEF_TILE : len;
    while (cur < t1) {
      const int j = cur - t0;
      const uint32_t ml = T->mlen[j];
      const uint32_t t = ml ? 0x80000000u | ((ml - 3u) << 16) | T->mdist[j] : (uint32_t)T->mlit[j];
      if (lane == 0) tok[ntok] = t;
      ++ntok;
      cur += ml ? (int32_t)ml : 1;
    }
    TSEM_BGZF_SYNC();
  }
  if (lane == 0) tok[ntok] = 256u;                          // end-of-block
  ++ntok;
  TSEM_BGZF_SYNC();
  // ---- 2: histogram
  for (int32_t i = lane; i < ntok; i += nl) {
    const uint32_t t = tok[i];
    if (!(t >> 31)) { TSEM_BGZF_ATOMIC_ADD(&T->hist_ll[t], 1u); continue; }
    int e;
    TSEM_BGZF_ATOMIC_ADD(&T->hist_ll[bgzf_len_symbol((int)((t >> 16) & 255u), &e)], 1u);
    TSEM_BGZF_ATOMIC_ADD(&T->hist_d[bgzf_dist_symbol((int)(t & 0x7FFFu), &e)], 1u);
  }
  // ---- 3: codes of a dynamic block
  bgzf_build_lengths(T->hist_ll, 286, 15, T->len_ll, &T->work, lane, nl);
  bgzf_build_lengths(T->hist_d, 30, 15, T->len_d, &T->work, lane, nl);
  int hlit = 257, hdist = 1;
  for (int s = 257; s < 286; ++s) if (T->len_ll[s]) hlit = s + 1;
  for (int s = 1; s < 30; ++s) if (T->len_d[s]) hdist = s + 1;
  for (int i = lane; i < hlit + hdist; i += nl) TSEM_BGZF_ATOMIC_ADD(&T->hist_cl[i < hlit ? T->len_ll[i] : T->len_d[i - hlit]], 1u);
  TSEM_BGZF_SYNC();
  if (lane == 0) {                                          // the code-length code must be complete: a second symbol where one is used
    int used = 0;
    for (int s = 0; s < 16; ++s) used += T->hist_cl[s] ? 1 : 0;
    if (used < 2) T->hist_cl[T->hist_cl[0] ? 1 : 0] += 1;
  }
  bgzf_build_lengths(T->hist_cl, 16, 7, T->len_cl, &T->work, lane, nl);
  int hclen = 4;
  for (int i = 4; i < 19; ++i) { const int s = bgzf_cl_order(i); if (s < 16 && T->len_cl[s]) hclen = i + 1; }
  // ---- 4: the three forms' bits
  uint32_t dyn_head = 3 + 14 + 3 * (uint32_t)hclen;         // (from the lengths, not hist_cl: a symbol added above is never written)
  for (int i = 0; i < hlit + hdist; ++i) dyn_head += T->len_cl[i < hlit ? T->len_ll[i] : T->len_d[i - hlit]];
  uint32_t fixed_bits = 3, dyn_bits = dyn_head;
  for (int s = 0; s < 286; ++s) {
    const uint32_t f = T->hist_ll[s], e = s > 256 ? (uint32_t)bgzf_len_extra(s) : 0u;
    fixed_bits += f * ((s < 144 ? 8u : s < 256 ? 9u : s < 280 ? 7u : 8u) + e);
    dyn_bits += f * (T->len_ll[s] + e);
  }
  for (int s = 0; s < 30; ++s) {
    const uint32_t f = T->hist_d[s], e = (uint32_t)bgzf_dist_extra(s);
    fixed_bits += f * (5u + e);
    dyn_bits += f * (T->len_d[s] + e);
  }
  const uint32_t stored_bits = 8u * (uint32_t)(len + 5);
  const int choice = stored_bits <= fixed_bits && stored_bits <= dyn_bits ? BGZF_DEF_STORED : fixed_bits <= dyn_bits ? BGZF_DEF_FIXED : BGZF_DEF_DYNAMIC;
  *form = choice;
  int32_t out_len;
  TSEM_BGZF_SYNC();                                         // every lane has read the dynamic lengths; the head table is dead
  if (choice == BGZF_DEF_STORED) {
    if (lane == 0) {
      out[0] = 1;
      out[1] = (uint8_t)(len & 255); out[2] = (uint8_t)(len >> 8);
      out[3] = (uint8_t)(~len & 255); out[4] = (uint8_t)((~len >> 8) & 255);
    }
    for (int32_t i = lane; i < len; i += nl) out[5 + i] = in[i];
    out_len = len + 5;
  } else {
    // ---- 5: emit
    if (choice == BGZF_DEF_FIXED) {
      for (int s = lane; s < 288; s += nl) T->len_ll[s] = (uint8_t)(s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8);
      for (int s = lane; s < 32; s += nl) T->len_d[s] = 5;
      TSEM_BGZF_SYNC();
    }
    if (lane == 0) {
      bgzf_assign_codes(T->len_ll, 288, T->code_ll, T->work.cnt);
      bgzf_assign_codes(T->len_d, 32, T->code_d, T->work.cnt);
      if (choice == BGZF_DEF_DYNAMIC) bgzf_assign_codes(T->len_cl, 16, T->code_cl, T->work.cnt);
    }
    const int nchunk = (ntok + BGZF_DEF_CHUNK - 1) / BGZF_DEF_CHUNK;   // token chunks; chunk k of the list is token chunk k - 1
    TSEM_BGZF_SYNC();
    for (int k = lane; k < nchunk; k += nl) {
      const int32_t i0 = k * BGZF_DEF_CHUNK, i1 = i0 + BGZF_DEF_CHUNK < ntok ? i0 + BGZF_DEF_CHUNK : ntok;
      uint32_t bits = 0;
      for (int32_t i = i0; i < i1; ++i) bits += (uint32_t)bgzf_token_bits(T, tok[i]);
      T->u.late.chunk_bits[k + 1] = bits;
    }
    TSEM_BGZF_SYNC();
    if (lane == 0) {
      uint32_t at = choice == BGZF_DEF_FIXED ? 3u : dyn_head;      // the header's bits
      T->u.late.chunk_bits[0] = 0;
      for (int k = 1; k <= nchunk; ++k) { const uint32_t b = T->u.late.chunk_bits[k]; T->u.late.chunk_bits[k] = at; at += b; }
      T->u.late.chunk_bits[nchunk + 1] = at;
    }
    TSEM_BGZF_SYNC();
    // what is about to be written is what step 4 counted (so it fits): anything else is a defect of this code, and nothing is written
    if (T->u.late.chunk_bits[nchunk + 1] != (choice == BGZF_DEF_FIXED ? fixed_bits : dyn_bits)) return -2;
    if (lane == 0) {                                        // the block header: chunk 0
      bgzf_bitw w;
      bgzf_bitw_open(w, out, 0, T, 0);
      bgzf_bitw_put(w, 1u | ((uint32_t)choice << 1), 3);
      if (choice == BGZF_DEF_DYNAMIC) {
        bgzf_bitw_put(w, (uint32_t)(hlit - 257) | ((uint32_t)(hdist - 1) << 5) | ((uint32_t)(hclen - 4) << 10), 14);
        bgzf_bitw_flush(w);
        for (int i = 0; i < hclen; ++i) {
          const int s = bgzf_cl_order(i);
          bgzf_bitw_put(w, s < 16 ? T->len_cl[s] : 0u, 3);
          bgzf_bitw_flush(w);
        }
        for (int i = 0; i < hlit + hdist; ++i) {
          const int v = i < hlit ? T->len_ll[i] : T->len_d[i - hlit];
          bgzf_bitw_put(w, T->code_cl[v], T->len_cl[v]);
          bgzf_bitw_flush(w);
        }
      }
      bgzf_bitw_close(w);
    }
    for (int k = lane; k < nchunk; k += nl) {
      const int32_t i0 = k * BGZF_DEF_CHUNK, i1 = i0 + BGZF_DEF_CHUNK < ntok ? i0 + BGZF_DEF_CHUNK : ntok;
      bgzf_bitw w;
      bgzf_bitw_open(w, out, T->u.late.chunk_bits[k + 1], T, k + 1);
      for (int32_t i = i0; i < i1; ++i) {
        const uint32_t t = tok[i];
        if (!(t >> 31)) {
          bgzf_bitw_put(w, T->code_ll[t], T->len_ll[t]);
        } else {
          int e1, e2;
          const uint32_t l = (t >> 16) & 255u, d = t & 0x7FFFu;
          const int ls = bgzf_len_symbol((int)l, &e1), ds = bgzf_dist_symbol((int)d, &e2);
          bgzf_bitw_put(w, T->code_ll[ls], T->len_ll[ls]);
          bgzf_bitw_put(w, ls == 285 ? 0u : l & ((1u << e1) - 1u), e1);
          bgzf_bitw_put(w, T->code_d[ds], T->len_d[ds]);
          bgzf_bitw_put(w, d & ((1u << e2) - 1u), e2);
        }
        bgzf_bitw_flush(w);
      }
      bgzf_bitw_close(w);
    }
    TSEM_BGZF_SYNC();
    // the shared bytes: the first chunk that has one stores it, with the bits of the chunks after it that have it too
    const int nent = 2 * (nchunk + 1);
    for (int e = lane; e < nent; e += nl) {
      const uint32_t at = T->u.late.part_idx[e];
      if (at == BGZF_DEF_NONE) continue;
      int q = e - 1;
      while (q >= 0 && T->u.late.part_idx[q] == BGZF_DEF_NONE) --q;
      if (q >= 0 && T->u.late.part_idx[q] == at) continue;
      uint32_t v = T->u.late.part_val[e];
      for (q = e + 1; q < nent; ++q) {
        const uint32_t a2 = T->u.late.part_idx[q];
        if (a2 == BGZF_DEF_NONE) continue;
        if (a2 != at) break;
        v |= T->u.late.part_val[q];
      }
      out[at] = (uint8_t)v;
    }
    out_len = (int32_t)(((choice == BGZF_DEF_FIXED ? fixed_bits : dyn_bits) + 7u) >> 3);
  }
  // ---- 6: CRC-32 of the input
  TSEM_BGZF_SYNC();
  bgzf_crc_table(T->u.late.crc.crc_tab, lane, nl);
  TSEM_BGZF_SYNC();
  bgzf_crc_slice(&T->u.late.crc, in, len, lane, nl);
  TSEM_BGZF_SYNC();
  *crc = bgzf_crc_join(&T->u.late.crc, len, nl);
  return out_len;
}
