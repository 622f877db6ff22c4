// The record rewriting of `--updated_sam` as __host__ __device__ inline functions (the style of tsem_bam_rec.h): the kernels of
// tsem_bam.hip call them with their lane's index, a stand-alone host program runs the same code in plain loops under a sanitizer
// (tests/c_host/bam_edit_check.cc).
//
// THE EDIT BODY.  A record here is FRAMED: its int32 block_size and the block_size bytes behind it, `len` bytes in all.  An edit
// (tsem_bam_edit) changes the flag (AND, then OR), sets the MAPQ or keeps it, removes every aux field whose two-letter name is listed,
// whatever its type (bam_out.set_tag: "the old tag goes"), and leaves room for `append_len` bytes of new aux fields behind the kept
// ones; the block_size is rewritten.  Two passes:
//   bam_edit_size   walks the record and returns the new framed length, or -(BAM_ST_* code) for a record it cannot walk;
//   bam_edit_write  writes out[0, new_len - append_len) and returns that offset, where the caller puts its append_len bytes.
// Every read is checked against `len` first; bam_edit_write writes each byte of [0, new_len - append_len) once and nothing else.
// Offsets are 64-bit.
//
// THE UPDATE STAGE (Telescope.update_sam, bam_out.update_pair): one uint32 per record, kind << 30 | the tsem_entry_tags word
// (bits 0-7 MAPQ, 8-15 XP, 16 assigned, 17 z >= 0.2): bam_update_edit / bam_update_append.
//
// THE LOAD STAGE (loader.load_alignment's two BAMs): after the four stages of tsem_bam_stages.h, per bundle the output order
// (bam_rw_plan_stage), per output slot the destination, PRI / SEC and the new length (bam_rw_size_stage), and behind an exclusive scan
// per destination the bytes (bam_rw_write_stage).
#pragma once
#include "tsem_bam_stages.h"

struct tsem_bam_edit {
  uint32_t flag_and, flag_or;                     // flag = (flag & flag_and) | flag_or
  int32_t mapq;                                   // 0 .. 255, or -1: keep
  int32_t n_strip;                                // 0 .. 3
  uint16_t strip[4];                              // names as first | second << 8
};

static constexpr int BAM_EDIT_MAPQ = 13, BAM_EDIT_FLAG = 18;   // offsets in a framed record

TSEM_BAM_HD uint16_t bam_name16(char a, char b) { return (uint16_t)((uint8_t)a | ((uint8_t)b << 8)); }

// the offset of the first aux field of the framed record rec[0, len), or -(code)
TSEM_BAM_HD int64_t bam_edit_aux_start(const uint8_t* rec, int64_t len) {
  if (len < 36 || (int64_t)(int32_t)bam_rd32(rec) != len - 4) return -BAM_ST_SIZE;
  const int64_t l_rn = rec[12];
  if (l_rn < 1 || 36 + l_rn > len) return -BAM_ST_NAME;
  int64_t p = 36 + l_rn + 4 * (int64_t)bam_rd16(rec + 16);
  if (p > len) return -BAM_ST_CIGAR;
  const int64_t l_seq = (int32_t)bam_rd32(rec + 20);
  if (l_seq < 0) return -BAM_ST_SEQ;
  p += (l_seq + 1) / 2 + l_seq;
  return p > len ? -BAM_ST_SEQ : p;
}

// the offset behind the aux field that begins at p < len, or -(code)
TSEM_BAM_HD int64_t bam_edit_field_end(const uint8_t* rec, int64_t len, int64_t p) {
  if (p + 3 > len) return -BAM_ST_AUX_HEAD;
  const uint8_t typ = rec[p + 2];
  p += 3;
  const int sz = bam_aux_size(typ);
  if (sz) return p + sz > len ? -BAM_ST_AUX_VALUE : p + sz;
  if (typ == 'A') return p + 1 > len ? -BAM_ST_AUX_VALUE : p + 1;
  if (typ == 'Z' || typ == 'H') {
    while (p < len && rec[p] != 0) ++p;
    return p >= len ? -BAM_ST_AUX_NUL : p + 1;
  }
  if (typ == 'B') {
    if (p + 5 > len) return -BAM_ST_AUX_ARRAY;
    const int esz = bam_aux_size(rec[p]);
    const int64_t cnt = (int32_t)bam_rd32(rec + p + 1);
    if (!esz || cnt < 0 || p + 5 + cnt * esz > len) return -BAM_ST_AUX_ARRAY;
    return p + 5 + cnt * esz;
  }
  return -BAM_ST_AUX_TYPE;
}

TSEM_BAM_HD bool bam_edit_strips(const tsem_bam_edit& e, uint32_t name) {
  bool hit = false;
  for (int k = 0; k < 4; ++k) hit |= k < e.n_strip && e.strip[k] == name;
  return hit;
}

TSEM_BAM_HD int64_t bam_edit_size(const uint8_t* rec, int64_t len, const tsem_bam_edit& e, int64_t append_len) {
  int64_t p = bam_edit_aux_start(rec, len);
  if (p < 0) return p;
  int64_t kept = p;
  while (p < len) {
    const int64_t q = bam_edit_field_end(rec, len, p);
    if (q < 0) return q;
    if (!bam_edit_strips(e, bam_rd16(rec + p))) kept += q - p;
    p = q;
  }
  if (kept + append_len - 4 > (int64_t)INT32_MAX) return -BAM_ST_SIZE;        // (no block_size can say it)
  return kept + append_len;
}

// `new_len` = what bam_edit_size returned for the same record, edit and append_len (>= 0)
TSEM_BAM_HD int64_t bam_edit_write(const uint8_t* rec, int64_t len, const tsem_bam_edit& e, int64_t new_len, uint8_t* out) {
  const int64_t a = bam_edit_aux_start(rec, len);
  const uint32_t bs = (uint32_t)(new_len - 4);
  const uint32_t flag = (bam_rd16(rec + BAM_EDIT_FLAG) & e.flag_and) | e.flag_or;
  for (int64_t k = 0; k < a; ++k) {
    uint8_t v = rec[k];
    if (k < 4) v = (uint8_t)(bs >> (8 * k));
    else if (k == BAM_EDIT_MAPQ && e.mapq >= 0) v = (uint8_t)e.mapq;
    else if (k == BAM_EDIT_FLAG) v = (uint8_t)flag;
    else if (k == BAM_EDIT_FLAG + 1) v = (uint8_t)(flag >> 8);
    out[k] = v;
  }
  int64_t p = a, o = a;
  while (p < len) {
    const int64_t q = bam_edit_field_end(rec, len, p);
    if (q < 0) break;                                          // (bam_edit_size refused such a record)
    if (!bam_edit_strips(e, bam_rd16(rec + p)))
      for (int64_t k = p; k < q; ++k) out[o++] = rec[k];
    p = q;
  }
  return o;
}

TSEM_BAM_HD int64_t bam_put(uint8_t* out, int64_t o, const char* s, int n) {
  for (int k = 0; k < n; ++k) out[o + k] = (uint8_t)s[k];
  return o + n;
}

// ------------------------------------------------------------------------------------------------------------- update stage
static constexpr uint32_t BAM_UPD_KEEP = 0, BAM_UPD_SEC = 1, BAM_UPD_PRI = 2;   // word >> 30

// the YC colour of a PRI word (bam_out.YC_ASSIGNED / YC_HIGH / YC_LOW) and its length
TSEM_BAM_HD const char* bam_update_colour(uint32_t w, int* n) {
  if (w >> 16 & 1) { *n = 8; return "217,95,2"; }
  if (w >> 17 & 1) { *n = 9; return "230,171,2"; }
  *n = 11; return "209,236,228";
}

// -> the edit of a record with word w and the length of what bam_update_append writes; false: an unknown kind
TSEM_BAM_HD bool bam_update_edit(uint32_t w, tsem_bam_edit* e, int64_t* append_len) {
  const uint32_t kind = w >> 30;
  e->flag_and = 0xFFFF; e->flag_or = 0; e->mapq = -1; e->n_strip = 0;
  e->strip[0] = e->strip[1] = e->strip[2] = e->strip[3] = 0;
  *append_len = 0;
  if (kind == BAM_UPD_KEEP) return true;
  if (kind == BAM_UPD_SEC) {
    e->flag_or = 0x100; e->mapq = 0; e->n_strip = 1; e->strip[0] = bam_name16('Y', 'C');
    *append_len = 3 + 11 + 1;
    return true;
  }
  if (kind != BAM_UPD_PRI) return false;
  e->mapq = (int32_t)(w & 0xFF);
  if (w >> 16 & 1) e->flag_and = 0xFFFF & ~0x100u; else e->flag_or = 0x100;
  e->n_strip = 2; e->strip[0] = bam_name16('X', 'P'); e->strip[1] = bam_name16('Y', 'C');
  int n;
  (void)bam_update_colour(w, &n);
  *append_len = 4 + 3 + n + 1;
  return true;
}

TSEM_BAM_HD void bam_update_append(uint32_t w, uint8_t* out) {
  const uint32_t kind = w >> 30;
  if (kind == BAM_UPD_SEC) { (void)bam_put(out, 0, "YCZ248,248,248\0", 15); return; }
  if (kind != BAM_UPD_PRI) return;
  int n;
  const char* c = bam_update_colour(w, &n);
  int64_t o = bam_put(out, 0, "XPC", 3);
  out[o++] = (uint8_t)(w >> 8);
  o = bam_put(out, o, "YCZ", 3);
  o = bam_put(out, o, c, n);
  out[o] = 0;
}

// --------------------------------------------------------------------------------------------------------------- load stage
// the names the load stage writes: name j = bytes[off[j], off[j + 1]), j = a locus id, j = n_loci: the no_feature_key
struct BamNames {
  const uint8_t* bytes; const int64_t* off; int32_t n_loci;
  TSEM_BAM_HD int64_t idx(int32_t f) const { return f >= 0 ? f : n_loci; }
  TSEM_BAM_HD int64_t len(int32_t f) const { return off[idx(f) + 1] - off[idx(f)]; }
  TSEM_BAM_HD int64_t put(int32_t f, uint8_t* out, int64_t o) const {
    for (int64_t k = off[idx(f)]; k < off[idx(f) + 1]; ++k) out[o++] = bytes[k];
    return o;
  }
};
// per output slot (the slots of a bundle are its records' indices: a bundle never writes more records than it holds)
static constexpr int32_t BAM_RW_NONE = 0, BAM_RW_OTHER = 1, BAM_RW_TMP_COPY = 2, BAM_RW_TMP_PRI = 3, BAM_RW_TMP_SEC = 4, BAM_RW_UPDATE = 5;
struct BamRw {
  int32_t *rec, *pair, *kind;                     // the record a slot writes (-1: none), its pair slot, BAM_RW_*
  int64_t *pos_other, *pos_tmp;                   // [N + 1]: the slot's length in either stream, after the scan its offset
};

// the output order of the bundle that starts at record s: loader._fragments' pairs, r1 then r2; class 0 writes its first pair only
TSEM_BAM_HD void bam_rw_plan_stage(int64_t s, int64_t N, BamCols C, BamRw W) {
  if (!(C[BAM_C_BITS][s] & BAM_BIT_NEWNAME)) return;
  const int32_t* bits = C[BAM_C_BITS];
  int64_t e = s + 1;
  while (e < N && !(bits[e] & BAM_BIT_NEWNAME)) ++e;
  for (int64_t i = s; i < e; ++i) { W.rec[i] = -1; W.pair[i] = -1; }
  const int32_t cls = C[BAM_C_BCLASS][s];
  if (cls < 0 || cls >= BAM_CLS_HOST) return;
  int64_t np = C[BAM_C_BNPAIRS][s];
  if (cls == 0 && np > 1) np = 1;
  if (np > e - s) np = e - s;
  const int32_t *p1 = C[BAM_C_PAIR1], *p2 = C[BAM_C_PAIR2];
  int64_t j = s;
  for (int64_t k = s; k < s + np; ++k) {
    const int32_t r1 = p1[k], r2 = p2[k];
    if (r1 >= s && r1 < e && j < e) { W.rec[j] = r1; W.pair[j] = (int32_t)k; ++j; }
    if (r2 >= s && r2 < e && j < e) { W.rec[j] = r2; W.pair[j] = (int32_t)k; ++j; }
  }
}

TSEM_BAM_HD void bam_load_edit(tsem_bam_edit* e) {
  e->flag_and = 0xFFFF; e->flag_or = 0; e->mapq = -1; e->n_strip = 3;
  e->strip[0] = bam_name16('Z', 'F'); e->strip[1] = bam_name16('Z', 'T'); e->strip[2] = bam_name16('Z', 'B'); e->strip[3] = 0;
}
// ZF:Z:<name> ZT:Z:PRI|SEC ZB:Z:<the mappings whose alnscore is the first one's, comma-joined>: the length, or the bytes at out
TSEM_BAM_HD int64_t bam_load_append(const BamNames& nm, int32_t feat, bool pri, const int32_t* mfeat, const int32_t* mas, int32_t g,
                                    uint8_t* out) {
  int64_t o = 0;
  if (out) { o = bam_put(out, o, "ZFZ", 3); o = nm.put(feat, out, o); out[o++] = 0; o = bam_put(out, o, pri ? "ZTZPRI\0" : "ZTZSEC\0", 7); o = bam_put(out, o, "ZBZ", 3); }
  else o = 3 + nm.len(feat) + 1 + 7 + 3;
  bool first = true;
  for (int32_t m = 0; m < g; ++m) {
    if (mas[m] != mas[0]) continue;
    if (!first) { if (out) out[o] = ','; ++o; }
    first = false;
    if (out) o = nm.put(mfeat[m], out, o); else o += nm.len(mfeat[m]);
  }
  if (out) out[o] = 0;
  return o + 1;
}

// slot i: where its record goes, PRI or SEC, and its new length into pos_other[i] / pos_tmp[i]
TSEM_BAM_HD void bam_rw_size_stage(int64_t i, const uint8_t* bytes, const int64_t* off, BamCols C, const BamNames& nm, BamRw W,
                                   unsigned long long* status) {
  W.pos_other[i] = 0; W.pos_tmp[i] = 0; W.kind[i] = BAM_RW_NONE;
  const int32_t r = W.rec[i];
  if (r < 0) return;
  const int32_t s = C[BAM_C_BUNDLE][r], k = W.pair[i];
  const int32_t cls = C[BAM_C_BCLASS][s];
  const int64_t len = off[r + 1] - off[r];
  if (cls <= 2) { W.kind[i] = BAM_RW_OTHER; W.pos_other[i] = len; return; }
  const int32_t f = C[BAM_C_PFEAT][k];
  if (f == BAM_PF_UNMAPPED || f == BAM_PF_SKIPPED) { W.kind[i] = BAM_RW_TMP_COPY; W.pos_tmp[i] = len; return; }
  // PRI: the first pair of its feature, in pair order, that reaches the feature's largest alnscore + alnlen
  const int32_t *pf = C[BAM_C_PFEAT], *pa = C[BAM_C_PAS], *pl = C[BAM_C_PLEN];
  const int64_t sum = (int64_t)pa[k] + pl[k];
  bool pri = true;
  const int32_t np = C[BAM_C_BNPAIRS][s];
  for (int32_t j = s; j < s + np; ++j) {
    if (j == k || pf[j] != f) continue;
    const int64_t sj = (int64_t)pa[j] + pl[j];
    if (j < k ? sj >= sum : sj > sum) pri = false;
  }
  tsem_bam_edit e;
  bam_load_edit(&e);
  const int64_t app = bam_load_append(nm, f, pri, C[BAM_C_MFEAT] + s, C[BAM_C_MAS] + s, C[BAM_C_BNMAPS][s], nullptr);
  const int64_t n = bam_edit_size(bytes + off[r], len, e, app);
  if (n < 0) { bam_report(status, r, (int)-n); return; }
  W.kind[i] = pri ? BAM_RW_TMP_PRI : BAM_RW_TMP_SEC;
  W.pos_tmp[i] = n;
}

// slot i of the update stage: record i with its word
TSEM_BAM_HD void bam_upd_size_stage(int64_t i, const uint8_t* bytes, const int64_t* off, const uint32_t* words, BamRw W,
                                    unsigned long long* status) {
  W.pos_other[i] = 0; W.pos_tmp[i] = 0; W.kind[i] = BAM_RW_NONE; W.rec[i] = (int32_t)i; W.pair[i] = -1;
  tsem_bam_edit e;
  int64_t app;
  if (!bam_update_edit(words[i], &e, &app)) { bam_report(status, i, BAM_ST_AUX_TYPE); return; }
  const int64_t n = bam_edit_size(bytes + off[i], off[i + 1] - off[i], e, app);
  if (n < 0) { bam_report(status, i, (int)-n); return; }
  W.kind[i] = BAM_RW_UPDATE;
  W.pos_tmp[i] = n;
}

// slot i writes [pos[i], pos[i + 1]) of its stream (pos: the exclusive scan of the lengths)
TSEM_BAM_HD void bam_rw_write_stage(int64_t i, const uint8_t* bytes, const int64_t* off, BamCols C, const BamNames& nm, const uint32_t* words,
                                    BamRw W, uint8_t* other, uint8_t* tmp) {
  const int32_t kind = W.kind[i];
  if (kind == BAM_RW_NONE) return;
  const int32_t r = W.rec[i];
  const uint8_t* rec = bytes + off[r];
  const int64_t len = off[r + 1] - off[r];
  if (kind == BAM_RW_OTHER || kind == BAM_RW_TMP_COPY) {
    uint8_t* out = kind == BAM_RW_OTHER ? other + W.pos_other[i] : tmp + W.pos_tmp[i];
    for (int64_t k = 0; k < len; ++k) out[k] = rec[k];
    return;
  }
  uint8_t* out = tmp + W.pos_tmp[i];
  const int64_t n = W.pos_tmp[i + 1] - W.pos_tmp[i];
  tsem_bam_edit e;
  if (kind == BAM_RW_UPDATE) {
    int64_t app;
    (void)bam_update_edit(words[i], &e, &app);
    const int64_t o = bam_edit_write(rec, len, e, n, out);
    bam_update_append(words[i], out + o);
    return;
  }
  const int32_t s = C[BAM_C_BUNDLE][r];
  bam_load_edit(&e);
  const int64_t o = bam_edit_write(rec, len, e, n, out);
  (void)bam_load_append(nm, C[BAM_C_PFEAT][W.pair[i]], kind == BAM_RW_TMP_PRI, C[BAM_C_MFEAT] + s, C[BAM_C_MAS] + s, C[BAM_C_BNMAPS][s],
                        out + o);
}
