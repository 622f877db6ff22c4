// The host side of a device loader stage, shared by tsem_bam.hip, tsem_bgzf.hip and tsem_bam_collate.hip: how such a call fails, keeps
// its device buffers, times its stages, reports a record and uploads a chunk.  Host code only (nothing __device__ or __global__), and
// not for the headers of host / device bodies, which the programs under tests/c_host compile without HIP.  Everything runs on the null
// stream of the device that is current; the caller has set it.
#pragma once
#include "tsem_internal.h"

#include <initializer_list>
#include <string>

// ---- failure: the text goes where tsem_last_error(NULL) reads it, the code back to the caller
static inline int stage_fail(int rc, const std::string& msg) { g_create_err = msg; return rc; }
#define STAGE_HIP(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) return stage_fail(TSEM_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(e_)); } while (0)

// ---- a device buffer that only grows and is kept: pointer and capacity (in elements) change together, so the capacity never
// overstates the memory behind the pointer; freed with its owner (a handle is deleted behind its hipSetDevice)
template <typename T>
struct DevBuf {
  T* p = nullptr;
  size_t cap = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { dfree(p); }
  // exactly n elements (one where n is 0), what was there is freed first; a failure leaves the buffer empty
  int alloc(size_t n, const char* what, const char* fn) {
    dfree(p); cap = 0;
    const size_t bytes = std::max<size_t>(1, n) * sizeof(T);
    if (hipMalloc((void**)&p, bytes) != hipSuccess) {
      p = nullptr;
      return stage_fail(TSEM_ERR_NOMEM, std::string(fn) + ": hipMalloc(" + std::to_string(bytes) + " B) for the " + what + " failed");
    }
    cap = n;
    return TSEM_OK;
  }
  // room for `need` elements: a quarter more than asked, so that chunks of slowly growing size do not reallocate every time
  int reserve(size_t need, const char* what, const char* fn) { return need <= cap ? TSEM_OK : alloc(need + need / 4, what, fn); }
};

// ---- HIP-event time per stage, summed over calls.  A call records NEV events at most: begin(), then mark() behind every stage;
// finish() behind the call's synchronise adds the time between event k and event k + 1 to ms[slot[k]].
template <int NEV, int NMS>
struct StageClock {
  hipEvent_t ev[NEV] = {};
  int made = 0, at = 0;
  double ms[NMS] = {};
  int64_t calls = 0;
  StageClock() = default;
  StageClock(const StageClock&) = delete;
  StageClock& operator=(const StageClock&) = delete;
  ~StageClock() { for (int k = 0; k < made; ++k) (void)hipEventDestroy(ev[k]); }
  hipError_t create() {
    for (; made < NEV; ++made)
      if (hipError_t e = hipEventCreate(&ev[made])) return e;
    return hipSuccess;
  }
  hipError_t mark() { return at < made ? hipEventRecord(ev[at++], 0) : hipErrorInvalidValue; }
  hipError_t begin() { at = 0; return mark(); }                // (a call that failed half way leaves its events behind: start over)
  // slot: one per pair of neighbouring events of this call; count: the call is one of those that `calls` counts
  hipError_t finish(std::initializer_list<int> slot, bool count = true) {
    if ((int)slot.size() + 1 != at) return hipErrorInvalidValue;
    int k = 0;
    for (int s : slot) {
      float m = 0.f;
      if (s < 0 || s >= NMS) return hipErrorInvalidValue;
      if (hipError_t e = hipEventElapsedTime(&m, ev[k], ev[k + 1])) return e;
      ms[s] += m;
      ++k;
    }
    calls += count;
    return hipSuccess;
  }
  void read(int reset, double* out, int64_t* n) {
    for (int k = 0; k < NMS; ++k) out[k] = ms[k];
    *n = calls;
    if (reset) { for (double& m : ms) m = 0; calls = 0; }
  }
};

// ---- the word in which a call's kernels report the first record (or block) in input order that they refuse: all ones, lowered by
// atomicMin(record << 8 | code).  status2 = {code, record}; the caller has set it to {0, -1}.
static inline bool stage_status_decode(unsigned long long word, int64_t* status2) {
  if (word == ~0ull) return false;
  status2[0] = (int64_t)(word & 0xFF); status2[1] = (int64_t)(word >> 8);
  return true;
}
struct StatusWord {
  DevBuf<unsigned long long> d;
  unsigned long long h = ~0ull;                   // (the word's host copy: it must outlive a call that fails behind the copy's launch)
  int create(const char* fn) { return d.alloc(1, "status word", fn); }
  hipError_t arm() { h = ~0ull; return hipMemsetAsync(d.p, 0xFF, 8, 0); }
  hipError_t fetch() { return hipMemcpyAsync(&h, d.p, 8, hipMemcpyDeviceToHost, 0); }
  bool decode(int64_t* status2) const { return stage_status_decode(h, status2); }   // behind the synchronise: was a record reported?
};

// ---- a chunk of BAM records.  The offsets bound every read of the kernels: checked on the host, before the device sees them.
static inline int stage_check_rec_off(const char* fn, const int64_t* rec_off, int64_t n_rec, int64_t n_bytes) {
  const std::string f(fn);
  if (rec_off[0] < 0 || rec_off[n_rec] > n_bytes) return stage_fail(TSEM_ERR_ARG, f + ": rec_off leaves the chunk");
  for (int64_t i = 0; i < n_rec; ++i)
    if (rec_off[i + 1] - rec_off[i] < 36 || rec_off[i + 1] - rec_off[i] > (int64_t)INT32_MAX)
      return stage_fail(TSEM_ERR_ARG, f + ": record " + std::to_string(i) + " is shorter than 36 bytes or longer than 2^31 - 1 (rec_off must ascend)");
  return TSEM_OK;
}
// ... and onto the device: both buffers grown, then the clock begun and both copies enqueued (the call's first stage)
template <typename Clock>
static inline int stage_upload_chunk(const char* fn, DevBuf<uint8_t>& d_bytes, DevBuf<int64_t>& d_off, const uint8_t* bytes,
                                     const int64_t* rec_off, int64_t n_rec, Clock& clock) {
  const size_t nb = (size_t)rec_off[n_rec];
  if (int rc = d_bytes.reserve(nb, "chunk's bytes", fn)) return rc;
  if (int rc = d_off.reserve((size_t)n_rec + 1, "record offsets", fn)) return rc;
  STAGE_HIP(clock.begin());
  STAGE_HIP(hipMemcpyAsync(d_bytes.p, bytes, nb, hipMemcpyHostToDevice, 0));
  STAGE_HIP(hipMemcpyAsync(d_off.p, rec_off, (size_t)(n_rec + 1) * 8, hipMemcpyHostToDevice, 0));
  return TSEM_OK;
}
