// Stand-alone host run of the record rewriting of `--updated_sam` (telescope_amd/csrc/tsem_bam_edit.h): the same functions the kernels
// of tsem_bam.hip call, on one record at a time, so that a host sanitizer sees every read and every write they make.
//
//   bam_edit_check CASES OUT
//
// CASES: a sequence of cases, little endian.  Each begins with int32 mode, int64 len and the len bytes of one FRAMED record, then
//   mode 0 (the edit body)    uint32 flag_and, flag_or; int32 mapq, n_strip; uint16 strip[4]; int64 append_len; the bytes to append
//   mode 1 (update stage)     uint32 word
//   mode 2 (load stage)       int32 n_names; int64 off[n_names + 1]; the names' bytes; int32 feat, pri, g; int32 mfeat[g]; int32 mas[g]
// OUT: per case int64 new_len, or -(status code), and the new_len bytes of the rewritten record.
// Every record lies in a heap block of exactly its size and every output in one of exactly the sized length: a byte read or written
// outside either is a sanitizer report.
//
//   bam_edit_check --load RECORDS ANNOT NAMES STRANDED FIRST_F LAST_F THRESHOLD CAP OTHER TMP
//
// The whole load stage of one chunk on the host: RECORDS and ANNOT as for bam_decode_check; NAMES: int32 n_names, int64
// off[n_names + 1], the names' bytes (the no_feature_key last).  OTHER / TMP get the two framed streams, each written into a heap block
// of exactly the scan's total.  Prints "status <code>" and, with status 0, per bundle "B first class pos_other pos_tmp".
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "tsem_bam_edit.h"
#include "tsem_bam_scan.h"

struct Reader {
  const std::vector<uint8_t>& v; size_t p = 0; bool ok = true;
  explicit Reader(const std::vector<uint8_t>& x) : v(x) {}
  void get(void* dst, size_t n) {
    if (p + n > v.size()) { ok = false; memset(dst, 0, n); return; }
    if (n) memcpy(dst, v.data() + p, n);
    p += n;
  }
  template <typename T> T one() { T x; get(&x, sizeof x); return x; }
  uint8_t* block(size_t n) {                                   // an exact heap block of the next n bytes
    uint8_t* b = (uint8_t*)malloc(n ? n : 1);
    get(b, n);
    return b;
  }
};

static bool read_file(const char* path, std::vector<uint8_t>& v) {
  FILE* f = fopen(path, "rb");
  if (!f) return false;
  fseek(f, 0, SEEK_END);
  const long n = ftell(f);
  fseek(f, 0, SEEK_SET);
  v.resize((size_t)n);
  const bool ok = n == 0 || fread(v.data(), 1, (size_t)n, f) == (size_t)n;
  fclose(f);
  return ok;
}

// the whole load stage of one chunk in plain loops: the four stages of tsem_bam_stages.h, then plan, size, the two scans and write
static int load_stage(char** a) {
  std::vector<uint8_t> bytes, ab, nb;
  if (!read_file(a[0], bytes) || !read_file(a[1], ab) || ab.size() < 16 || !read_file(a[2], nb) || nb.size() < 4) { fprintf(stderr, "cannot read the inputs\n"); return 2; }
  const int64_t cap = (int64_t)bytes.size() / 36 + 1;
  std::vector<int64_t> off((size_t)cap + 1);
  int64_t n = 0, used = 0;
  char msg[200];
  if (tsem_bam_scan_chain(bytes.data(), (int64_t)bytes.size(), off.data(), cap, &n, &used, msg, sizeof msg) || used != (int64_t)bytes.size() || !n) {
    fprintf(stderr, "the records do not form a chain\n"); return 2;
  }
  int64_t n_ref, n_iv;
  memcpy(&n_ref, ab.data(), 8); memcpy(&n_iv, ab.data() + 8, 8);
  if (n_ref < 0 || n_iv < 0 || ab.size() != (size_t)(16 + 8 * n_ref + 29 * n_iv)) { fprintf(stderr, "%s: wrong size\n", a[1]); return 2; }
  std::vector<int32_t> ref_lo((size_t)n_ref), ref_hi((size_t)n_ref), locus((size_t)n_iv);
  std::vector<int64_t> starts((size_t)n_iv), maxend((size_t)n_iv), ends((size_t)n_iv);
  std::vector<int8_t> strand((size_t)n_iv);
  const uint8_t* p = ab.data() + 16;
  memcpy(ref_lo.data(), p, 4 * (size_t)n_ref); p += 4 * n_ref;
  memcpy(ref_hi.data(), p, 4 * (size_t)n_ref); p += 4 * n_ref;
  memcpy(starts.data(), p, 8 * (size_t)n_iv); p += 8 * n_iv;
  memcpy(maxend.data(), p, 8 * (size_t)n_iv); p += 8 * n_iv;
  memcpy(ends.data(), p, 8 * (size_t)n_iv); p += 8 * n_iv;
  memcpy(locus.data(), p, 4 * (size_t)n_iv); p += 4 * n_iv;
  memcpy(strand.data(), p, (size_t)n_iv);
  BamAnnot A{(int32_t)n_ref, ref_lo.data(), ref_hi.data(), locus.data(), starts.data(), maxend.data(), ends.data(), strand.data()};
  int32_t n_names;
  memcpy(&n_names, nb.data(), 4);
  if (n_names < 1 || nb.size() < 4 + 8 * ((size_t)n_names + 1)) { fprintf(stderr, "%s: wrong size\n", a[2]); return 2; }
  std::vector<int64_t> noff((size_t)n_names + 1);
  memcpy(noff.data(), nb.data() + 4, noff.size() * 8);
  std::vector<uint8_t> names(nb.begin() + 4 + (long)noff.size() * 8, nb.end());
  if ((int64_t)names.size() != noff[n_names]) { fprintf(stderr, "%s: wrong size\n", a[2]); return 2; }
  for (int32_t l : locus) if (l < 0 || l >= n_names - 1) { fprintf(stderr, "a locus id outside the names\n"); return 2; }
  BamNames nm{names.data(), noff.data(), n_names - 1};
  const int32_t stranded = atoi(a[3]), first_f = atoi(a[4]), last_f = atoi(a[5]), rcap = atoi(a[7]);
  const double threshold = atof(a[6]);
  std::vector<int32_t> cols((size_t)n * TSEM_BAM_COLS_), rw((size_t)n * 3);
  std::vector<int64_t> pos(2 * ((size_t)n + 1), 0);
  BamCols C{cols.data(), n};
  BamRw W{rw.data(), rw.data() + n, rw.data() + 2 * n, pos.data(), pos.data() + n + 1};
  unsigned long long status = ~0ull;
  for (int64_t i = 0; i < n; ++i) bam_decode_stage(i, bytes.data(), off.data(), -1, -1, C, &status);
  for (int64_t s = 0; s < n; ++s) bam_pair_stage(s, n, rcap, C);
  for (int64_t i = 0; i < n; ++i) bam_overlap_stage(i, bytes.data(), off.data(), C, A, stranded, first_f, last_f, threshold, &status);
  for (int64_t s = 0; s < n; ++s) bam_fragment_stage(s, C);
  if (status != ~0ull) { printf("status %llu\n", status & 0xFF); return 0; }
  for (int64_t s = 0; s < n; ++s) bam_rw_plan_stage(s, n, C, W);
  for (int64_t i = 0; i < n; ++i) bam_rw_size_stage(i, bytes.data(), off.data(), C, nm, W, &status);
  if (status != ~0ull) { printf("status %llu\n", status & 0xFF); return 0; }
  int64_t so = 0, st = 0;
  for (int64_t i = 0; i <= n; ++i) {                            // the exclusive scans
    const int64_t lo = W.pos_other[i], lt = W.pos_tmp[i];
    W.pos_other[i] = so; W.pos_tmp[i] = st;
    so += lo; st += lt;
  }
  uint8_t* other = (uint8_t*)malloc(so ? (size_t)so : 1);     // exactly the scans' totals
  uint8_t* tmp = (uint8_t*)malloc(st ? (size_t)st : 1);
  for (int64_t i = 0; i < n; ++i) bam_rw_write_stage(i, bytes.data(), off.data(), C, nm, nullptr, W, other, tmp);
  FILE* fo = fopen(a[8], "wb");
  FILE* ft = fopen(a[9], "wb");
  if (!fo || !ft) { fprintf(stderr, "cannot write the outputs\n"); return 2; }
  fwrite(other, 1, (size_t)so, fo); fwrite(tmp, 1, (size_t)st, ft);
  fclose(fo); fclose(ft);
  free(other); free(tmp);
  printf("status 0\n");
  for (int64_t s = 0; s < n; ++s)                              // per bundle: first record, class, where its bytes begin in either stream
    if (C[BAM_C_BITS][s] & BAM_BIT_NEWNAME) printf("B %" PRId64 " %d %" PRId64 " %" PRId64 "\n", s, (int)C[BAM_C_BCLASS][s], W.pos_other[s], W.pos_tmp[s]);
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 12 && !strcmp(argv[1], "--load")) return load_stage(argv + 2);
  if (argc != 3) { fprintf(stderr, "usage: bam_edit_check CASES OUT | --load RECORDS ANNOT NAMES STRANDED FIRST_F LAST_F THRESHOLD CAP OTHER TMP\n"); return 2; }
  std::vector<uint8_t> in;
  if (!read_file(argv[1], in)) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
  FILE* out = fopen(argv[2], "wb");
  if (!out) { fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
  Reader r(in);
  int64_t cases = 0;
  while (r.p < in.size()) {
    const int32_t mode = r.one<int32_t>();
    const int64_t len = r.one<int64_t>();
    if (!r.ok || len < 0 || mode < 0 || mode > 2) { fprintf(stderr, "case %" PRId64 ": bad head\n", cases); return 2; }
    uint8_t* rec = r.block((size_t)len);
    tsem_bam_edit e;
    int64_t app = 0, n = 0;
    uint8_t *append = nullptr, *names = nullptr;
    std::vector<int64_t> off;
    std::vector<int32_t> mfeat, mas;
    int32_t feat = 0, pri = 0, g = 0;
    uint32_t word = 0;
    BamNames nm{nullptr, nullptr, 0};
    if (mode == 0) {
      e.flag_and = r.one<uint32_t>(); e.flag_or = r.one<uint32_t>(); e.mapq = r.one<int32_t>(); e.n_strip = r.one<int32_t>();
      r.get(e.strip, 8);
      app = r.one<int64_t>();
      if (!r.ok || app < 0) { fprintf(stderr, "case %" PRId64 ": bad edit\n", cases); return 2; }
      append = r.block((size_t)app);
    } else if (mode == 1) {
      word = r.one<uint32_t>();
      if (!bam_update_edit(word, &e, &app)) { fprintf(stderr, "case %" PRId64 ": bad word\n", cases); return 2; }
    } else {
      const int32_t n_names = r.one<int32_t>();
      if (!r.ok || n_names < 1) { fprintf(stderr, "case %" PRId64 ": bad names\n", cases); return 2; }
      off.resize((size_t)n_names + 1);
      r.get(off.data(), off.size() * 8);
      names = r.block((size_t)off[n_names]);
      feat = r.one<int32_t>(); pri = r.one<int32_t>(); g = r.one<int32_t>();
      if (!r.ok || g < 0) { fprintf(stderr, "case %" PRId64 ": bad maps\n", cases); return 2; }
      mfeat.resize((size_t)g); mas.resize((size_t)g);
      r.get(mfeat.data(), (size_t)g * 4); r.get(mas.data(), (size_t)g * 4);
      nm = BamNames{names, off.data(), n_names - 1};
      bam_load_edit(&e);
      app = bam_load_append(nm, feat, pri != 0, mfeat.data(), mas.data(), g, nullptr);
    }
    if (!r.ok) { fprintf(stderr, "case %" PRId64 ": truncated\n", cases); return 2; }
    n = bam_edit_size(rec, len, e, app);                       // the sizing pass
    fwrite(&n, 8, 1, out);
    if (n >= 0) {
      uint8_t* o = (uint8_t*)malloc((size_t)n ? (size_t)n : 1);
      memset(o, 0xEE, (size_t)n);
      const int64_t at = bam_edit_write(rec, len, e, n, o);    // the writing pass
      if (at + app != n) { fprintf(stderr, "case %" PRId64 ": the writing pass ends at %" PRId64 " + %" PRId64 ", sized %" PRId64 "\n", cases, at, app, n); return 3; }
      if (mode == 0) { if (app) memcpy(o + at, append, (size_t)app); }
      else if (mode == 1) bam_update_append(word, o + at);
      else if (bam_load_append(nm, feat, pri != 0, mfeat.data(), mas.data(), g, o + at) != app) { fprintf(stderr, "case %" PRId64 ": append length\n", cases); return 3; }
      fwrite(o, 1, (size_t)n, out);
      free(o);
    }
    free(rec); free(append); free(names);
    ++cases;
  }
  fclose(out);
  printf("cases %" PRId64 "\n", cases);
  return 0;
}
