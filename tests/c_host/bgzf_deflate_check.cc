// The deflate body of k_bgzf_deflate (telescope_amd/csrc/tsem_bgzf_deflate.h) as an ordinary host program: built with the address and
// undefined-behaviour sanitizers by tests/_bgzf_deflate_reference.py.
//
//   bgzf_deflate_check blocks IN OUT    IN is a raw byte stream, cut every 0xff00 bytes (an empty IN is one empty block).  Every block
//                                       is taken from a heap copy of exactly its bytes into a heap buffer of exactly len + 5, so that
//                                       an access one byte outside either is a sanitizer report.  The body runs once with one lane and
//                                       once with 64 lanes, and the two must agree byte for byte, in length, form and CRC-32; the
//                                       stream is then inflated with bgzf_inflate_block (status 0, the input back).  stdout per block:
//                                       "<k> <len> <stream length> <form>"; OUT receives the BGZF blocks (header, stream, trailer).
//   bgzf_deflate_check blocks1 IN OUT   the same with the one-lane run only (cheap: for a stream of hundreds of blocks)
//   bgzf_deflate_check lengths         histograms straight into bgzf_build_lengths, with 1 and with 64 lanes: the limit, the Kraft
//                                       sum, no used symbol without a code and no code for an unused one.
//
// The 64 lanes are 64 threads of which exactly one runs at a time: a lane runs to the next TSEM_BGZF_SYNC(), then the next lane does,
// and after lane 63 lane 0 goes on — the phases of the device, lane after lane.
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <thread>
#include <vector>

#include "tsem_bgzf_inflate.h"

namespace {
int g_lanes = 1, g_turn = 0;
std::mutex g_mu;
std::condition_variable g_cv[64];
thread_local int t_lane = 0;

void lane_wait(std::unique_lock<std::mutex>& l) { g_cv[t_lane].wait(l, [] { return g_turn == t_lane; }); }
void lane_pass(int to) { g_turn = to; g_cv[to].notify_one(); }
void lane_barrier() {
  if (g_lanes == 1) return;
  std::unique_lock<std::mutex> l(g_mu);
  lane_pass((t_lane + 1) % g_lanes);
  lane_wait(l);
}
// f(lane, lanes) on `lanes` lanes, one at a time, phase by phase
template <typename F>
void run_lanes(int lanes, F f) {
  g_lanes = lanes; g_turn = 0;
  if (lanes == 1) { t_lane = 0; f(0, 1); return; }
  std::vector<std::thread> th;
  for (int k = 0; k < lanes; ++k)
    th.emplace_back([k, lanes, &f] {
      t_lane = k;
      { std::unique_lock<std::mutex> l(g_mu); lane_wait(l); }
      f(k, lanes);
      std::unique_lock<std::mutex> l(g_mu);
      if (k + 1 < lanes) lane_pass(k + 1);
    });
  for (std::thread& t : th) t.join();
  g_lanes = 1;
}
}  // namespace

#undef TSEM_BGZF_SYNC
#define TSEM_BGZF_SYNC() lane_barrier()
#include "tsem_bgzf_deflate.h"

static int check_lengths(const char* name, const std::vector<uint32_t>& hist, int limit) {
  const int n = (int)hist.size();
  std::vector<uint8_t> got[2];
  for (int r = 0; r < 2; ++r) {
    got[r].assign((size_t)n, 0xEE);
    bgzf_code_work* W = new bgzf_code_work;
    uint8_t* lens = got[r].data();
    run_lanes(r ? 64 : 1, [&](int lane, int nl) { bgzf_build_lengths(hist.data(), n, limit, lens, W, lane, nl); });
    delete W;
  }
  int used = 0, mx = 0, bad = 0;
  unsigned long long kraft = 0;
  for (int s = 0; s < n; ++s) {
    const int l = got[0][(size_t)s];
    if (hist[(size_t)s]) { ++used; if (l == 0) { fprintf(stderr, "%s: symbol %d is used and has no code\n", name, s); bad = 1; } }
    else if (l != 0) { fprintf(stderr, "%s: symbol %d is not used and has a code\n", name, s); bad = 1; }
    if (l > mx) mx = l;
    if (l > 0 && l <= limit) kraft += 1ull << (limit - l);
  }
  if (mx > limit) { fprintf(stderr, "%s: a code of %d bits, the limit is %d\n", name, mx, limit); bad = 1; }
  if (used >= 2 && kraft != 1ull << limit) { fprintf(stderr, "%s: Kraft sum %llu / %llu\n", name, kraft, 1ull << limit); bad = 1; }
  if (used == 1 && (mx != 1 || kraft != 1ull << (limit - 1))) { fprintf(stderr, "%s: one symbol must get one bit\n", name); bad = 1; }
  if (got[0] != got[1]) { fprintf(stderr, "%s: 64 lanes give other lengths than one\n", name); bad = 1; }
  printf("%s n %d limit %d used %d max %d %s\n", name, n, limit, used, mx, bad ? "FAILED" : "ok");
  return bad;
}

static int lengths_mode() {
  int bad = 0;
  static const int sets[3][2] = {{286, 15}, {30, 15}, {19, 7}};
  for (const int* p : {sets[0], sets[1], sets[2]}) {
    const int n = p[0], limit = p[1];
    char name[64];
    std::vector<uint32_t> h((size_t)n, 0);
    uint32_t a = 1, b = 1;                                  // Fibonacci counts up to 2^23, then level: 286 of them stay below 2^32 in sum
    for (int s = 0; s < n; ++s) { h[(size_t)s] = a; if (b < 0x800000u) { const uint32_t c = a + b; a = b; b = c; } }
    snprintf(name, sizeof name, "fibonacci_%d", n); bad |= check_lengths(name, h, limit);
    for (int s = 0; s < n; ++s) h[(size_t)s] = 1u << ((s * 7) % 24);                                         // powers of two, not in order (sum below 2^32)
    snprintf(name, sizeof name, "powers_%d", n); bad |= check_lengths(name, h, limit);
    h.assign((size_t)n, 7);
    snprintf(name, sizeof name, "all_equal_%d", n); bad |= check_lengths(name, h, limit);
    h.assign((size_t)n, 0); h[(size_t)(n / 2)] = 5;
    snprintf(name, sizeof name, "one_symbol_%d", n); bad |= check_lengths(name, h, limit);
    h[(size_t)(n - 1)] = 1000000;
    snprintf(name, sizeof name, "two_symbols_%d", n); bad |= check_lengths(name, h, limit);
    h[0] = 1;
    snprintf(name, sizeof name, "three_symbols_%d", n); bad |= check_lengths(name, h, limit);
    h.assign((size_t)n, 0);
    snprintf(name, sizeof name, "no_symbol_%d", n); bad |= check_lengths(name, h, limit);
  }
  return bad;
}

struct Result { std::vector<uint8_t> out; int32_t len = 0, form = -1; uint32_t crc = 0; };

static Result deflate_with(const uint8_t* src, int32_t len, int lanes) {
  Result r;
  uint8_t* in = (uint8_t*)malloc(len ? (size_t)len : 1);
  uint8_t* out = (uint8_t*)calloc((size_t)len + 5, 1);
  uint32_t* tok = (uint32_t*)malloc(((size_t)len + 1) * 4);
  if (len) memcpy(in, src, (size_t)len);
  tsem_bgzf_deflate_tables* T = new tsem_bgzf_deflate_tables;
  run_lanes(lanes, [&](int lane, int nl) {
    uint32_t crc = 0;
    int32_t form = -1;
    const int32_t n = bgzf_deflate_block(in, len, out, len + 5, &crc, &form, T, tok, lane, nl);
    if (lane == 0) { r.len = n; r.crc = crc; r.form = form; }
  });
  if (r.len > 0) r.out.assign(out, out + r.len);
  delete T;
  free(in); free(out); free(tok);
  return r;
}

int main(int argc, char** argv) {
  if (argc == 2 && !strcmp(argv[1], "lengths")) return lengths_mode();
  const bool wave_too = argc == 4 && !strcmp(argv[1], "blocks");
  if (argc != 4 || (!wave_too && strcmp(argv[1], "blocks1"))) { fprintf(stderr, "usage: %s blocks IN OUT | blocks1 IN OUT | lengths\n", argv[0]); return 2; }
  FILE* f = fopen(argv[2], "rb");
  if (!f) { perror(argv[2]); return 2; }
  std::vector<uint8_t> in;
  uint8_t tmp[65536];
  for (size_t k; (k = fread(tmp, 1, sizeof tmp, f)) > 0;) in.insert(in.end(), tmp, tmp + k);
  fclose(f);
  FILE* o = fopen(argv[3], "wb");
  if (!o) { perror(argv[3]); return 2; }
  const int64_t nb = in.empty() ? 1 : ((int64_t)in.size() + BGZF_DEF_BLOCK - 1) / BGZF_DEF_BLOCK;
  tsem_bgzf_tables* TI = new tsem_bgzf_tables;
  int bad = 0;
  for (int64_t k = 0; k < nb; ++k) {
    const int64_t at = k * BGZF_DEF_BLOCK;
    const int32_t len = (int32_t)((int64_t)in.size() - at < BGZF_DEF_BLOCK ? (int64_t)in.size() - at : BGZF_DEF_BLOCK);
    const Result one = deflate_with(in.data() + at, len, 1), wave = wave_too ? deflate_with(in.data() + at, len, 64) : one;
    if (one.len < 2 || one.len > len + 5) { fprintf(stderr, "block %lld: the body returns %d for %d bytes\n", (long long)k, one.len, len); bad = 1; continue; }
    if (one.len != wave.len || one.form != wave.form || one.crc != wave.crc || one.out != wave.out) {
      fprintf(stderr, "block %lld: 64 lanes give another stream than one lane (%d / %d bytes)\n", (long long)k, wave.len, one.len);
      bad = 1;
    }
    uint8_t* pay = (uint8_t*)malloc((size_t)one.len);
    uint8_t* back = (uint8_t*)calloc(len ? (size_t)len : 1, 1);
    memcpy(pay, one.out.data(), (size_t)one.len);
    g_lanes = 1;
    const int st = bgzf_inflate_block(pay, one.len, back, len, one.crc, TI, 0, 1);
    if (st != BGZF_ST_OK || (len && memcmp(back, in.data() + at, (size_t)len))) {
      fprintf(stderr, "block %lld: bgzf_inflate_block gives status %d%s\n", (long long)k, st, st ? "" : " and other bytes");
      bad = 1;
    }
    free(pay); free(back);
    const uint32_t bsize = (uint32_t)one.len + 25;
    const uint8_t head[18] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, (uint8_t)(bsize & 255), (uint8_t)(bsize >> 8)};
    uint8_t tail[8];
    for (int i = 0; i < 4; ++i) { tail[i] = (uint8_t)(one.crc >> (8 * i)); tail[4 + i] = (uint8_t)((uint32_t)len >> (8 * i)); }
    fwrite(head, 1, 18, o); fwrite(one.out.data(), 1, (size_t)one.len, o); fwrite(tail, 1, 8, o);
    printf("%lld %d %d %d\n", (long long)k, len, one.len, one.form);
  }
  delete TI;
  fclose(o);
  return bad;
}
