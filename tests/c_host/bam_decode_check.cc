// Stand-alone host run of the device loader's record code (telescope_amd/csrc/tsem_bam_scan.h, tsem_bam_rec.h, tsem_bam_stages.h): the
// same functions the kernels of tsem_bam.hip call, in plain loops, so that a host sanitizer sees every read they make.
//
//   bam_decode_check RECORDS [BTAG UTAG [ANNOT STRANDED FIRST_F LAST_F THRESHOLD CAP OUT]]
//
// RECORDS: inflated BAM bytes from the first record on (possibly truncated or damaged).  BTAG / UTAG: two letters, or "--".
// Prints "scan <records> <consumed>" (or "scan error: ..." and stops), then one line per record: "R index" and the 16 fields of
// tsem_bam_rec.  With ANNOT (int64 n_ref, n_iv; int32 ref_lo[n_ref], ref_hi[n_ref]; int64 starts[n_iv], maxend[n_iv], ends[n_iv];
// int32 locus[n_iv]; int8 strand[n_iv]) the pair, overlap and fragment stages run as well and the int32 matrix
// [TSEM_BAM_COLS][records] goes to OUT, followed by the two int64 of the status word (code, record).
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "tsem_bam_scan.h"
#include "tsem_bam_stages.h"

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
static int32_t tag16(const char* t) { return (strlen(t) == 2 && strcmp(t, "--")) ? ((uint8_t)t[0] | ((uint8_t)t[1] << 8)) : -1; }

int main(int argc, char** argv) {
  if (argc != 2 && argc != 4 && argc != 11) { fprintf(stderr, "usage: see the top of bam_decode_check.cc\n"); return 2; }
  std::vector<uint8_t> bytes;
  if (!read_file(argv[1], bytes)) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
  const int32_t btag = argc >= 4 ? tag16(argv[2]) : -1, utag = argc >= 4 ? tag16(argv[3]) : -1;
  // the exact size, no slack: a read behind the last byte is a read behind the allocation
  std::vector<uint8_t> exact(bytes.begin(), bytes.end());
  const int64_t cap = (int64_t)exact.size() / 36 + 1;
  std::vector<int64_t> off((size_t)cap + 1);
  int64_t n = 0, used = 0;
  char msg[200];
  if (tsem_bam_scan_chain(exact.data(), (int64_t)exact.size(), off.data(), cap, &n, &used, msg, sizeof msg)) {
    printf("scan error: %s\n", msg);
    return 0;
  }
  printf("scan %" PRId64 " %" PRId64 "\n", n, used);
  if (n == 0) return 0;
  std::vector<int32_t> out((size_t)n * TSEM_BAM_COLS_);
  BamCols C{out.data(), n};
  unsigned long long status = ~0ull;
  for (int64_t i = 0; i < n; ++i) bam_decode_stage(i, exact.data(), off.data(), btag, utag, C, &status);
  for (int64_t i = 0; i < n; ++i) {
    printf("R %" PRId64, i);
    for (int c = 0; c < 16; ++c) printf(" %d", (int)C[c][i]);
    printf("\n");
  }
  if (argc == 11) {
    std::vector<uint8_t> ab;
    if (!read_file(argv[4], ab) || ab.size() < 16) { fprintf(stderr, "cannot read %s\n", argv[4]); return 2; }
    int64_t n_ref, n_iv;
    memcpy(&n_ref, ab.data(), 8); memcpy(&n_iv, ab.data() + 8, 8);
    if (n_ref < 0 || n_iv < 0 || ab.size() != (size_t)(16 + 8 * n_ref + 29 * n_iv)) { fprintf(stderr, "%s: wrong size\n", argv[4]); return 2; }
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
    for (int64_t r = 0; r < n_ref; ++r)
      if (ref_lo[r] < 0 || ref_hi[r] < ref_lo[r] || ref_hi[r] > n_iv) { fprintf(stderr, "%s: bad range\n", argv[4]); return 2; }
    BamAnnot A{(int32_t)n_ref, ref_lo.data(), ref_hi.data(), locus.data(), starts.data(), maxend.data(), ends.data(), strand.data()};
    const int32_t stranded = atoi(argv[5]), first_f = atoi(argv[6]), last_f = atoi(argv[7]), rcap = atoi(argv[9]);
    const double threshold = atof(argv[8]);
    for (int64_t s = 0; s < n; ++s) bam_pair_stage(s, n, rcap, C);
    for (int64_t i = 0; i < n; ++i) bam_overlap_stage(i, exact.data(), off.data(), C, A, stranded, first_f, last_f, threshold, &status);
    for (int64_t s = 0; s < n; ++s) bam_fragment_stage(s, C);
    FILE* f = fopen(argv[10], "wb");
    if (!f) { fprintf(stderr, "cannot write %s\n", argv[10]); return 2; }
    const int64_t st[2] = {status == ~0ull ? 0 : (int64_t)(status & 0xFF), status == ~0ull ? -1 : (int64_t)(status >> 8)};
    fwrite(out.data(), 4, out.size(), f);
    fwrite(st, 8, 2, f);
    fclose(f);
  }
  printf("status %lld\n", status == ~0ull ? 0ll : (long long)(status & 0xFF));
  return 0;
}
