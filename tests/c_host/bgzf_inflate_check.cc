// The inflate body of k_bgzf_inflate (telescope_amd/csrc/tsem_bgzf_inflate.h) and the header walk (tsem_bgzf_scan.h) as an ordinary
// host program: built with the address and undefined-behaviour sanitizers by tests/_bgzf_reference.py and run over every case of the
// suite, the corrupt ones included.
//
//   bgzf_inflate_check IN OUT
//
// IN is a BGZF byte string.  Every whole block is inflated with one lane, from a heap copy of exactly its payload into a heap buffer of
// exactly ISIZE bytes, so that a read or write one byte outside either range is a sanitizer report.  The CRC-32 of every good block
// is then taken a second time the way a wave does it: 64 slices, joined.  stdout: "scan <blocks> <consumed> <not_bgzf>", then per
// block "<k> <status> <isize>"; OUT receives the blocks' output ranges one after the other (ISIZE bytes each, none for status 255).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "tsem_bgzf_inflate.h"
#include "tsem_bgzf_scan.h"

int main(int argc, char** argv) {
  if (argc != 3) { fprintf(stderr, "usage: %s IN OUT\n", argv[0]); return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  std::vector<uint8_t> in;
  uint8_t tmp[65536];
  for (size_t k; (k = fread(tmp, 1, sizeof tmp, f)) > 0;) in.insert(in.end(), tmp, tmp + k);
  fclose(f);
  const int64_t cap = (int64_t)in.size() / 26 + 1;
  std::vector<int64_t> blk((size_t)cap * 5);
  int64_t n = 0, used = 0;
  int32_t not_bgzf = 0;
  char msg[200] = "";
  if (tsem_bgzf_scan_chain(in.data(), (int64_t)in.size(), blk.data(), cap, &n, &used, &not_bgzf, msg, sizeof msg)) {
    printf("scan error: %s\n", msg);
    return 0;
  }
  printf("scan %lld %lld %d\n", (long long)n, (long long)used, (int)not_bgzf);
  FILE* o = fopen(argv[2], "wb");
  if (!o) { perror(argv[2]); return 2; }
  tsem_bgzf_tables* T = new tsem_bgzf_tables;
  int bad = 0;
  for (int64_t k = 0; k < n; ++k) {
    const int64_t* r = &blk[(size_t)k * 5];
    int st = BGZF_ST_HOST;
    if (r[3] <= BGZF_MAX_ISIZE) {
      uint8_t* pay = (uint8_t*)malloc((size_t)r[2] ? (size_t)r[2] : 1);
      uint8_t* out = (uint8_t*)calloc((size_t)r[3] ? (size_t)r[3] : 1, 1);
      memcpy(pay, in.data() + r[1], (size_t)r[2]);
      st = bgzf_inflate_block(pay, (int32_t)r[2], out, (int32_t)r[3], (uint32_t)r[4], T, 0, 1);
      if (st == BGZF_ST_OK) {                               // the wave's CRC: 64 slices and the join
        for (int lane = 0; lane < 64; ++lane) bgzf_crc_slice(T, out, (int32_t)r[3], lane, 64);
        if (bgzf_crc_join(T, (int32_t)r[3], 64) != (uint32_t)r[4]) { fprintf(stderr, "block %lld: the joined CRC-32 differs\n", (long long)k); bad = 1; }
      }
      fwrite(out, 1, (size_t)r[3], o);
      free(pay); free(out);
    }
    printf("%lld %d %lld\n", (long long)k, st, (long long)r[3]);
  }
  delete T;
  fclose(o);
  return bad;
}
