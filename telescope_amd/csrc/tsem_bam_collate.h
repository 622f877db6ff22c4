// The collate step of `assign --collate` as __host__ __device__ inline functions (the style of tsem_bam_edit.h): the kernels of
// tsem_bam_collate.hip call them with their lane's record, tsem_bam_collate_host and a stand-alone host program run the same code in
// plain loops (tests/c_host/bam_collate_check.cc).  No HIP header is needed.
//
// THE DEFINITION.  The input is a stream of n FRAMED records (int32 block_size and the bytes behind it; record i is
// bytes[rec_off[i], rec_off[i + 1]), as tsem_bam_scan leaves rec_off).  A record's NAME is the l_read_name bytes at offset 36 of the
// framed record (32 of the part behind the block_size), the trailing NUL included, compared as bytes.  A GROUP is the set of records
// with equal names.  The collated stream holds the same framed records: the groups in the order of their first records, the records
// of a group in their input order.  order[k] = the input index of output record k.
//
// THE STEPS.
//   bam_collate_check    a record whose framed length is below 37 (32 fixed bytes and one of the name), whose l_read_name is 0 or whose
//                        name runs past its end is refused with a code: nothing behind the check reads outside a record
//   bam_collate_hash     64 bits of the name (FNV-1a, then a finishing mix), masked to `hash_bits` bits (0: all 64).  Few bits make
//                        distinct names share hash values and probe chains (tests): the exact comparison keeps them apart
//   bam_collate_insert   open addressing, linear probing, in a table of a power of two >= 2 n slots.  A slot is {rep, first}: the
//                        record that claimed it (compare-and-swap from BAM_COL_EMPTY) and the smallest index of the records that joined
//                        it (minimum).  A probe that meets a claimed slot compares the hashes, then the names, with the
//                        representative's: equal joins, unequal goes on to the next slot.  Which record becomes the representative
//                        is a race between the lanes, so a group's slot and the chains differ from run to run; first[slot[i]],
//                        the only thing that leaves the step, does not
//   bam_collate_key      first[slot[i]] << 32 | i: sorted, the low words are `order`
// On the host the two atomic operations are plain reads and writes (one thread).
#pragma once
#include <cstring>

#include "tsem_bam_rec.h"

enum { BAM_COL_ST_SHORT = 1, BAM_COL_ST_NONAME = 2, BAM_COL_ST_NAME = 3 };
static constexpr uint32_t BAM_COL_EMPTY = 0xFFFFFFFFu;
static constexpr int64_t BAM_COL_NAME_AT = 36, BAM_COL_MIN_REC = 37;

struct bam_col_slot { uint32_t rep, first; };

// Where the records lie: the stream of the entry points.  (The stand-alone program has its own, one heap block per record.)
struct bam_col_stream {
  const uint8_t* bytes; const int64_t* rec_off;
  TSEM_BAM_HD const uint8_t* rec(int64_t i) const { return bytes + rec_off[i]; }
  TSEM_BAM_HD int64_t len(int64_t i) const { return rec_off[i + 1] - rec_off[i]; }
};

// 0, or why the framed record rec[0, len) cannot be collated
TSEM_BAM_HD int bam_collate_check(const uint8_t* rec, int64_t len) {
  if (len < BAM_COL_MIN_REC) return BAM_COL_ST_SHORT;
  const int64_t l = rec[12];
  if (l == 0) return BAM_COL_ST_NONAME;
  if (BAM_COL_NAME_AT + l > len) return BAM_COL_ST_NAME;
  return 0;
}

TSEM_BAM_HD uint64_t bam_collate_mask(int32_t hash_bits) { return hash_bits <= 0 || hash_bits >= 64 ? ~0ull : (1ull << hash_bits) - 1; }

// of a record that passed bam_collate_check
TSEM_BAM_HD uint64_t bam_collate_hash(const uint8_t* rec, int32_t hash_bits) {
  const int l = rec[12];
  const uint8_t* p = rec + BAM_COL_NAME_AT;
  uint64_t h = 0xcbf29ce484222325ull;
  for (int k = 0; k < l; ++k) h = (h ^ p[k]) * 0x100000001b3ull;
  h ^= h >> 33; h *= 0xff51afd7ed558ccdull; h ^= h >> 33; h *= 0xc4ceb9fe1a85ec53ull; h ^= h >> 33;
  return h & bam_collate_mask(hash_bits);
}

// of two records that passed bam_collate_check
TSEM_BAM_HD bool bam_collate_same(const uint8_t* a, const uint8_t* b) {
  const int l = a[12];
  if (l != b[12]) return false;
  for (int k = 0; k < l; ++k)
    if (a[BAM_COL_NAME_AT + k] != b[BAM_COL_NAME_AT + k]) return false;
  return true;
}

// the slot's representative: `i` if it claimed the empty slot, else who holds it
TSEM_BAM_HD uint32_t bam_col_claim(bam_col_slot* s, uint32_t i) {
#if defined(__HIP_DEVICE_COMPILE__)
  uint32_t r = __hip_atomic_load(&s->rep, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (r == BAM_COL_EMPTY) {
    r = atomicCAS(&s->rep, BAM_COL_EMPTY, i);
    if (r == BAM_COL_EMPTY) r = i;
  }
  return r;
#else
  if (s->rep == BAM_COL_EMPTY) s->rep = i;
  return s->rep;
#endif
}
TSEM_BAM_HD void bam_col_join(bam_col_slot* s, uint32_t i) {
#if defined(__HIP_DEVICE_COMPILE__)
  atomicMin(&s->first, i);
#else
  if (i < s->first) s->first = i;
#endif
}

// record i into the table of `cap` slots (a power of two >= 2 n, every slot {EMPTY, EMPTY} before the first insert): slot[i] = the
// slot of its group.  Fewer groups than slots: the probe always ends.
template <typename Recs>
TSEM_BAM_HD void bam_collate_insert(int64_t i, const Recs& R, const uint64_t* hash, bam_col_slot* table, uint64_t cap, uint32_t* slot) {
  const uint64_t h = hash[i], mask = cap - 1;
  uint64_t s = h & mask;
  for (;;) {
    const uint32_t r = bam_col_claim(table + s, (uint32_t)i);
    if (r == (uint32_t)i || (hash[r] == h && bam_collate_same(R.rec(i), R.rec(r)))) break;
    s = (s + 1) & mask;
  }
  bam_col_join(table + s, (uint32_t)i);
  slot[i] = (uint32_t)s;
}

// (the group's first record) << 32 | i; *is_first: record i is that record
TSEM_BAM_HD uint64_t bam_collate_key(int64_t i, const bam_col_slot* table, const uint32_t* slot, bool* is_first) {
  const uint32_t f = table[slot[i]].first;
  *is_first = f == (uint32_t)i;
  return ((uint64_t)f << 32) | (uint64_t)i;
}

static inline uint64_t bam_collate_table_slots(int64_t n) { uint64_t c = 2; while (c < 2 * (uint64_t)n) c <<= 1; return c; }

// What both entry points check of rec_off before anything reads through it: n + 1 offsets inside [0, n_bytes], not descending.
// -> -1, or the first record whose offsets are wrong.
static inline int64_t bam_collate_chain(const int64_t* rec_off, int64_t n, int64_t n_bytes) {
  if (rec_off[0] < 0 || rec_off[0] > n_bytes) return 0;
  for (int64_t i = 0; i < n; ++i)
    if (rec_off[i + 1] < rec_off[i] || rec_off[i + 1] > n_bytes) return i;
  return -1;
}

// The whole step on one thread: out holds the sum of the records' lengths; hash [n], slot [n], key [n] and table
// [bam_collate_table_slots(n)] are the caller's scratch, sort_keys(key, n) sorts ascending.  -> ~0, or (record << 8 | code) of the first
// record in input order that bam_collate_check refuses (out, order and n_names are then untouched).
template <typename Recs, typename Sort>
static inline unsigned long long bam_collate_run(const Recs& R, int64_t n, int32_t hash_bits, uint8_t* out, int64_t* order, int64_t* n_names,
                                                 uint64_t* hash, uint32_t* slot, uint64_t* key, bam_col_slot* table, Sort sort_keys) {
  for (int64_t i = 0; i < n; ++i) {
    const int st = bam_collate_check(R.rec(i), R.len(i));
    if (st) return ((unsigned long long)i << 8) | (unsigned long long)st;
    hash[i] = bam_collate_hash(R.rec(i), hash_bits);
  }
  const uint64_t cap = bam_collate_table_slots(n);
  for (uint64_t s = 0; s < cap; ++s) table[s] = bam_col_slot{BAM_COL_EMPTY, BAM_COL_EMPTY};
  for (int64_t i = 0; i < n; ++i) bam_collate_insert(i, R, hash, table, cap, slot);
  int64_t names = 0;
  for (int64_t i = 0; i < n; ++i) {
    bool f;
    key[i] = bam_collate_key(i, table, slot, &f);
    names += f;
  }
  sort_keys(key, n);
  int64_t o = 0;
  for (int64_t k = 0; k < n; ++k) {
    const int64_t i = (int64_t)(key[k] & 0xFFFFFFFFull), len = R.len(i);
    order[k] = i;
    memcpy(out + o, R.rec(i), (size_t)len);
    o += len;
  }
  *n_names = names;
  return ~0ull;
}
