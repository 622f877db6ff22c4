// Stand-alone host run of the collate step of `--collate` (telescope_amd/csrc/tsem_bam_collate.h): the same functions the kernels of
// tsem_bam_collate.hip and tsem_bam_collate_host call, in plain loops, so that a host sanitizer sees every read and every write they
// make.
//
//   bam_collate_check RECORDS OUT HASH_BITS
//
// RECORDS: int64 n, then per record int64 len and the len bytes of one FRAMED record, little endian.
// OUT: int64 order[n], then the collated stream.  Prints "names <groups>", or "refused <code> <record>" and writes nothing.
// Every record lies in a heap block of exactly its size, the collated stream in one of exactly the sum of the sizes and every scratch
// array in one of exactly its length: a byte read or written outside any of them is a sanitizer report.
#include <algorithm>
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "tsem_bam_collate.h"

struct Blocks {                                                  // one heap block per record
  std::vector<uint8_t*> p; std::vector<int64_t> n;
  const uint8_t* rec(int64_t i) const { return p[(size_t)i]; }
  int64_t len(int64_t i) const { return n[(size_t)i]; }
};

template <typename T> static T* exact(size_t n) { return (T*)malloc(n ? n * sizeof(T) : 1); }

int main(int argc, char** argv) {
  if (argc != 4) { fprintf(stderr, "usage: bam_collate_check RECORDS OUT HASH_BITS\n"); return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
  const int32_t hash_bits = atoi(argv[3]);
  int64_t n = 0, total = 0;
  if (fread(&n, 8, 1, f) != 1 || n < 0) { fprintf(stderr, "bad head\n"); return 2; }
  Blocks R;
  for (int64_t i = 0; i < n; ++i) {
    int64_t len = 0;
    if (fread(&len, 8, 1, f) != 1 || len < 0) { fprintf(stderr, "record %" PRId64 ": bad length\n", i); return 2; }
    uint8_t* b = exact<uint8_t>((size_t)len);
    if (len && fread(b, 1, (size_t)len, f) != (size_t)len) { fprintf(stderr, "record %" PRId64 ": truncated\n", i); return 2; }
    R.p.push_back(b); R.n.push_back(len);
    total += len;
  }
  fclose(f);
  const uint64_t cap = bam_collate_table_slots(n);
  uint64_t *hash = exact<uint64_t>((size_t)n), *key = exact<uint64_t>((size_t)n);
  uint32_t* slot = exact<uint32_t>((size_t)n);
  int64_t* order = exact<int64_t>((size_t)n);
  bam_col_slot* table = exact<bam_col_slot>((size_t)cap);
  uint8_t* out = exact<uint8_t>((size_t)total);
  int64_t names = 0;
  const unsigned long long st = bam_collate_run(R, n, hash_bits, out, order, &names, hash, slot, key, table,
                                                [](uint64_t* k, int64_t m) { std::sort(k, k + m); });
  if (st != ~0ull) {
    printf("refused %llu %llu\n", st & 0xFF, st >> 8);
  } else {
    FILE* o = fopen(argv[2], "wb");
    if (!o) { fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
    if (n) fwrite(order, 8, (size_t)n, o);
    if (total) fwrite(out, 1, (size_t)total, o);
    fclose(o);
    printf("names %" PRId64 "\n", names);
  }
  for (uint8_t* b : R.p) free(b);
  free(hash); free(key); free(slot); free(order); free(table); free(out);
  return 0;
}
