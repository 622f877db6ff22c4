// The four stages of tsem_bam_chunk as __host__ __device__ inline functions of one record / pair slot / bundle: the kernels of
// tsem_bam.hip call them with their lane's index, and a stand-alone host program runs the same code in plain loops
// (tests/c_host/bam_decode_check.cc).  What every stage reads and writes: the top of tsem_bam.hip and include/telescope_em.h.
#pragma once
#include "tsem_bam_rec.h"

static constexpr int BAM_CODE_SU = 0, BAM_CODE_SM = 1, BAM_CODE_PU = 2, BAM_CODE_PM = 3, BAM_CODE_PX = 4;
static constexpr int BAM_CLS_HOST = 5;
static constexpr int BAM_BF_HOST = 1;
static constexpr int BAM_PF_NONE = -1, BAM_PF_UNMAPPED = -2, BAM_PF_SKIPPED = -3;
static constexpr int BAM_LOCI = 8;

struct BamCols {                                  // the result matrix, row c at base + c * N
  int32_t* base; int64_t N;
  TSEM_BAM_HD int32_t* operator[](int c) const { return base + (int64_t)c * N; }
};
struct BamAnnot {
  int32_t n_ref; const int32_t *ref_lo, *ref_hi, *locus; const int64_t *starts, *maxend, *ends; const int8_t* strand;
};

TSEM_BAM_HD int64_t bam_min64(int64_t a, int64_t b) { return a < b ? a : b; }
TSEM_BAM_HD int64_t bam_max64(int64_t a, int64_t b) { return a > b ? a : b; }
// the call's status word falls to (record << 8 | code): the first bad record in file order is the one reported
TSEM_BAM_HD void bam_report(unsigned long long* status, int64_t rec, int code) {
  const unsigned long long w = ((unsigned long long)rec << 8) | (unsigned long long)code;
#if defined(__HIP_DEVICE_COMPILE__)
  atomicMin(status, w);
#else
  if (w < *status) *status = w;
#endif
}
TSEM_BAM_HD void bam_mark_host(int32_t* flag) {
#if defined(__HIP_DEVICE_COMPILE__)
  atomicOr(flag, BAM_BF_HOST);
#else
  *flag |= BAM_BF_HOST;
#endif
}

// record i: its fields into rows 0-15, and the slots the later stages fill only in part
TSEM_BAM_HD void bam_decode_stage(int64_t i, const uint8_t* bytes, const int64_t* off, int32_t btag, int32_t utag, BamCols C,
                                  unsigned long long* status) {
  tsem_bam_rec r;
  bam_decode_record(bytes, off[i], off[i + 1], i ? off[i - 1] : -1, off[i], btag, utag, &r);
  C[BAM_C_REF][i] = r.ref_id; C[BAM_C_POS][i] = r.pos; C[BAM_C_NREF][i] = r.nref; C[BAM_C_NPOS][i] = r.npos; C[BAM_C_ATLEN][i] = r.atlen;
  C[BAM_C_FLAG][i] = r.flag; C[BAM_C_LRN][i] = r.l_rn; C[BAM_C_NCIG][i] = r.n_cig; C[BAM_C_LSEQ][i] = r.l_seq; C[BAM_C_AS][i] = r.as;
  C[BAM_C_BITS][i] = r.bits; C[BAM_C_BCOFF][i] = r.bc_off; C[BAM_C_BCLEN][i] = r.bc_len; C[BAM_C_UMIOFF][i] = r.umi_off;
  C[BAM_C_UMILEN][i] = r.umi_len; C[BAM_C_STATUS][i] = r.status;
  // the slots the later kernels fill only in part
  C[BAM_C_PAIR1][i] = -1; C[BAM_C_PAIR2][i] = -1; C[BAM_C_BUNDLE][i] = -1; C[BAM_C_PFEAT][i] = BAM_PF_SKIPPED; C[BAM_C_PAS][i] = 0;
  C[BAM_C_PLEN][i] = 0; C[BAM_C_MFEAT][i] = BAM_PF_SKIPPED; C[BAM_C_MAS][i] = 0; C[BAM_C_MLEN][i] = 0; C[BAM_C_BCODE][i] = -1;
  C[BAM_C_BNPAIRS][i] = 0; C[BAM_C_BNMAPS][i] = 0; C[BAM_C_BCLASS][i] = -1; C[BAM_C_BMIN][i] = 0; C[BAM_C_BMAX][i] = 0;
  C[BAM_C_BNMAPPED][i] = 0; C[BAM_C_BFLAG][i] = 0; C[BAM_C_SCRATCH][i] = -1;
  if (r.status) bam_report(status, i, r.status);
}

// classify (loader._fragments) of the bundle that starts at record s
TSEM_BAM_HD void bam_pair_stage(int64_t s, int64_t N, int32_t cap, BamCols C) {
  if (!(C[BAM_C_BITS][s] & BAM_BIT_NEWNAME)) return;
  const int32_t* bits = C[BAM_C_BITS]; const int32_t* flag = C[BAM_C_FLAG];
  int32_t *p1 = C[BAM_C_PAIR1], *p2 = C[BAM_C_PAIR2], *bundle = C[BAM_C_BUNDLE], *cache = C[BAM_C_SCRATCH];
  int64_t e = s + 1;
  while (e < N && !(bits[e] & BAM_BIT_NEWNAME)) ++e;
  const int64_t n = e - s;
  bool host = n > (int64_t)cap, bad = false;
  for (int64_t i = s; i < e; ++i) {
    bundle[i] = (int32_t)s;
    host |= (bits[i] & BAM_BIT_HOST) != 0;
    bad |= C[BAM_C_STATUS][i] != 0;
  }
  const int32_t f0 = flag[s];
  int code;
  if (!(f0 & 0x1)) code = (f0 & 0x4) ? BAM_CODE_SU : BAM_CODE_SM;
  else if (f0 & 0x2) code = BAM_CODE_PM;
  else if (n == 2 && (flag[s] & 0x4) && (flag[s + 1] & 0x4)) code = BAM_CODE_PU;
  else code = BAM_CODE_PX;
  C[BAM_C_BCODE][s] = code;
  if (host || bad) { if (host) C[BAM_C_BFLAG][s] = BAM_BF_HOST; return; }   // (a bad record ends the call with its error)
  int64_t np = 0;
  if (code == BAM_CODE_PU) {
    p1[s] = (int32_t)s; p2[s] = (int32_t)(s + 1); np = 1;
  } else if (code != BAM_CODE_PM) {
    for (int64_t i = s; i < e; ++i) { p1[i] = (int32_t)i; p2[i] = -1; }
    np = n;
  } else {
    const int32_t *ref = C[BAM_C_REF], *pos = C[BAM_C_POS], *nref = C[BAM_C_NREF], *npos = C[BAM_C_NPOS], *atl = C[BAM_C_ATLEN];
    int64_t nc = 0;                                            // the cache list's length, holes (-1) included
    for (int64_t a = s; a < e; ++a) {
      const int32_t r1a = flag[a] & 0x40;
      int64_t hit = -1, same = -1;                             // a cached record whose key is a's mate key | a's own key
      for (int64_t k = 0; k < nc; ++k) {
        const int32_t c = cache[s + k];
        if (c < 0) continue;
        const int32_t r1c = flag[c] & 0x40;
        if (atl[c] != atl[a]) continue;
        if (r1c != r1a && ref[c] == nref[a] && pos[c] == npos[a] && nref[c] == ref[a] && npos[c] == pos[a]) { hit = k; break; }
        if (r1c == r1a && ref[c] == ref[a] && pos[c] == pos[a] && nref[c] == nref[a] && npos[c] == npos[a]) same = k;
      }
      if (hit >= 0) {                                          // cache.pop(mate key)
        const int32_t m = cache[s + hit];
        cache[s + hit] = -1;
        p1[s + np] = r1a ? (int32_t)a : m; p2[s + np] = r1a ? m : (int32_t)a; ++np;
      } else if (same >= 0) {
        cache[s + same] = (int32_t)a;                          // an equal key: the value goes, the position stays
      } else {
        cache[s + nc++] = (int32_t)a;
      }
    }
    for (int64_t k = 0; k < nc; ++k) {                          // the leftovers, in order of first insertion
      const int32_t c = cache[s + k];
      if (c >= 0) { p1[s + np] = c; p2[s + np] = -1; ++np; }
    }
  }
  C[BAM_C_BNPAIRS][s] = (int32_t)np;
}

// the reference blocks of one read, one at a time: M, =, X emit and advance, D and N advance
struct BamBlocks {
  const uint8_t* cig; int32_t n, k; int64_t pos, b, e; bool valid;
  TSEM_BAM_HD void open(const uint8_t* c, int32_t n_cig, int64_t p) { cig = c; n = n_cig; k = 0; pos = p; next(); }
  TSEM_BAM_HD void close() { n = k = 0; valid = false; }
  TSEM_BAM_HD void next() {
    valid = false;
    while (k < n) {
      const uint32_t c = bam_rd32(cig + 4 * (int64_t)k); ++k;
      const int64_t ln = c >> 4; const uint32_t op = c & 0xF;
      if (op == 0 || op == 7 || op == 8) { b = pos; e = pos + ln; pos += ln; valid = true; return; }
      if (op == 2 || op == 3) pos += ln;
    }
  }
};

struct BamTable { int32_t loc[BAM_LOCI]; int64_t sum[BAM_LOCI]; int32_t n; bool overflow; };

// Annotation.intersect_blocks for one merged block [bs, be) of a pair on intervals [lo0, hi0)
TSEM_BAM_HD void bam_intersect(const BamAnnot& A, int32_t lo0, int32_t hi0, int64_t bs, int64_t be, bool stranded,
                                              int8_t fstrand, BamTable& T) {
  const int64_t qb = bs, qe = be + 1;
  int32_t a = lo0, b = hi0;
  while (a < b) { const int32_t m = a + (b - a) / 2; if (A.starts[m] < qe) a = m + 1; else b = m; }   // searchsorted(starts, qe, 'left')
  const int32_t hi = a;
  if (hi == lo0) return;
  a = lo0; b = hi0;
  while (a < b) { const int32_t m = a + (b - a) / 2; if (A.maxend[m] <= qb) a = m + 1; else b = m; }   // searchsorted(maxend, qb, 'right')
  for (int32_t j = a; j < hi; ++j) {
    const int64_t ib = A.starts[j], ie = A.ends[j];
    if (!(ib < qe && qb < ie) || (stranded && A.strand[j] != fstrand)) continue;
    const int64_t ov = bam_max64(0, bam_min64(ie, qe) - bam_max64(ib, qb));
    const int32_t loc = A.locus[j];
    bool found = false;
#pragma unroll
    for (int k = 0; k < BAM_LOCI; ++k)
      if (k < T.n && T.loc[k] == loc) { T.sum[k] += ov; found = true; }
    if (found) continue;
    if (T.n == BAM_LOCI) { T.overflow = true; return; }
#pragma unroll
    for (int k = 0; k < BAM_LOCI; ++k)
      if (k == T.n) { T.loc[k] = loc; T.sum[k] = ov; }
    ++T.n;
  }
}

// the pair at slot i: alnlen, alnscore and its locus
TSEM_BAM_HD void bam_overlap_stage(int64_t i, const uint8_t* bytes, const int64_t* off, BamCols C, const BamAnnot& A, int32_t stranded,
                                   int32_t first_f, int32_t last_f, double threshold, unsigned long long* status) {
  const int32_t r1 = C[BAM_C_PAIR1][i], r2 = C[BAM_C_PAIR2][i];
  if (r1 < 0) return;
  const int32_t s = C[BAM_C_BUNDLE][i];
  const int32_t f1 = C[BAM_C_FLAG][r1];
  if (f1 & 0x4) { C[BAM_C_PFEAT][i] = BAM_PF_UNMAPPED; return; }
  if (C[BAM_C_STATUS][r1] || (r2 >= 0 && C[BAM_C_STATUS][r2])) return;
  if (!(C[BAM_C_BITS][r1] & BAM_BIT_AS)) { bam_report(status, r1, BAM_ST_NO_AS); return; }
  if (r2 >= 0 && !(C[BAM_C_BITS][r2] & BAM_BIT_AS)) { bam_report(status, r2, BAM_ST_NO_AS); return; }
  const int32_t ref = C[BAM_C_REF][r1];
  if (ref < 0 || ref >= A.n_ref) { bam_mark_host(&C[BAM_C_BFLAG][s]); return; }
  const int64_t as = (int64_t)C[BAM_C_AS][r1] + (r2 >= 0 ? (int64_t)C[BAM_C_AS][r2] : 0);
  const bool paired = r2 >= 0;
  const bool plus = (f1 & 0x10) ? (paired ? last_f != 0 : first_f == 0) : (paired ? last_f == 0 : first_f != 0);
  const int8_t fstrand = plus ? 0 : 1;
  const int32_t lo0 = A.ref_lo[ref], hi0 = A.ref_hi[ref];
  // (the CIGAR lies inside the record: k_bam_decode checked 32 + l_rn + 4 n_cig <= block_size for every record of status 0)
  BamBlocks x, y;
  x.open(bytes + off[r1] + 36 + C[BAM_C_LRN][r1], C[BAM_C_NCIG][r1], (int64_t)C[BAM_C_POS][r1]);
  if (paired) y.open(bytes + off[r2] + 36 + C[BAM_C_LRN][r2], C[BAM_C_NCIG][r2], (int64_t)C[BAM_C_POS][r2]);
  else y.close();
  BamTable T; T.n = 0; T.overflow = false;
#pragma unroll
  for (int k = 0; k < BAM_LOCI; ++k) { T.loc[k] = -1; T.sum[k] = 0; }
  int64_t alnlen = 0, cb = 0, ce = 0;
  bool have = false;
  while (x.valid || y.valid) {                                 // the stable merge by block start: r1's block first among equal starts
    const bool take_x = x.valid && (!y.valid || x.b <= y.b);
    const int64_t b = take_x ? x.b : y.b, e = take_x ? x.e : y.e;
    if (take_x) x.next(); else y.next();
    if (!have) { cb = b; ce = e; have = true; }
    else if (b - ce > 1) {                                     // merge_blocks(., 1): a gap of two or more starts a new block
      alnlen += ce - cb;
      bam_intersect(A, lo0, hi0, cb, ce, stranded != 0, fstrand, T);
      cb = b; ce = e;
    } else ce = bam_max64(ce, e);
  }
  if (have) { alnlen += ce - cb; bam_intersect(A, lo0, hi0, cb, ce, stranded != 0, fstrand, T); }
  if (T.overflow || alnlen > (int64_t)INT32_MAX || as > (int64_t)INT32_MAX || as < (int64_t)INT32_MIN) {
    bam_mark_host(&C[BAM_C_BFLAG][s]);
    return;
  }
  int32_t best = BAM_PF_NONE; int64_t bsum = 0;                // Counter.most_common()[0]: the largest sum, the first inserted among equals
#pragma unroll
  for (int k = 0; k < BAM_LOCI; ++k)
    if (k < T.n && (best == BAM_PF_NONE || T.sum[k] > bsum)) { best = T.loc[k]; bsum = T.sum[k]; }
  if (best != BAM_PF_NONE && !((double)bsum > (double)alnlen * threshold)) best = BAM_PF_NONE;
  C[BAM_C_PFEAT][i] = best; C[BAM_C_PAS][i] = (int32_t)as; C[BAM_C_PLEN][i] = (int32_t)alnlen;
}

// the map list, the class and the score range of the bundle that starts at record s
TSEM_BAM_HD void bam_fragment_stage(int64_t s, BamCols C) {
  if (!(C[BAM_C_BITS][s] & BAM_BIT_NEWNAME)) return;
  if (C[BAM_C_BFLAG][s] & BAM_BF_HOST) { C[BAM_C_BCLASS][s] = BAM_CLS_HOST; return; }
  const int code = C[BAM_C_BCODE][s];
  if (code == BAM_CODE_SU || code == BAM_CODE_PU) { C[BAM_C_BCLASS][s] = 0; return; }
  const int32_t np = C[BAM_C_BNPAIRS][s];
  const int32_t *pf = C[BAM_C_PFEAT] + s, *pa = C[BAM_C_PAS] + s, *pl = C[BAM_C_PLEN] + s;
  int32_t *mf = C[BAM_C_MFEAT] + s, *ma = C[BAM_C_MAS] + s, *ml = C[BAM_C_MLEN] + s;
  int32_t g = 0, nmapped = 0, mn = INT32_MAX, mx = INT32_MIN;
  bool any = false;
  for (int32_t k = 0; k < np; ++k) {
    const int32_t f = pf[k];
    if (f == BAM_PF_UNMAPPED || f == BAM_PF_SKIPPED) continue;
    ++nmapped;
    mn = pa[k] < mn ? pa[k] : mn; mx = pa[k] > mx ? pa[k] : mx;
    any |= f >= 0;
    int32_t j = 0;
    while (j < g && mf[j] != f) ++j;
    if (j == g) { mf[g] = f; ma[g] = pa[k]; ml[g] = pl[k]; ++g; }          // first appearance of the locus
    else if ((int64_t)pa[k] + pl[k] > (int64_t)ma[j] + ml[j]) { ma[j] = pa[k]; ml[j] = pl[k]; }   // (the first pair keeps a tie)
  }
  C[BAM_C_BNMAPPED][s] = nmapped; C[BAM_C_BMIN][s] = mn; C[BAM_C_BMAX][s] = mx;
  if (!any) { C[BAM_C_BCLASS][s] = nmapped > 1 ? 2 : 1; return; }
  C[BAM_C_BCLASS][s] = nmapped > 1 ? 4 : 3;
  for (int32_t j = 1; j < g; ++j) {                            // stable, alnscore descending
    const int32_t f = mf[j], a = ma[j], l = ml[j];
    int32_t t = j - 1;
    while (t >= 0 && ma[t] < a) { mf[t + 1] = mf[t]; ma[t + 1] = ma[t]; ml[t + 1] = ml[t]; --t; }
    mf[t + 1] = f; ma[t + 1] = a; ml[t + 1] = l;
  }
  C[BAM_C_BNMAPS][s] = g;
}

