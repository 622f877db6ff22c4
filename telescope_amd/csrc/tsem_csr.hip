// libtelescope_em.so: csr_matrix_plus primitives on a caller's fp64 CSR (sparse_plus.py:26-129: norm, scale, binmax), stateless;
// numpy's legacy MT19937 bounded draw for choose_random (sparse_plus.py:140-154).
#include "tsem_internal.h"

// ---- csr_matrix_plus primitives on fp64 CSR --------------------------------
// np.maximum, not fmax: scipy's max() keeps a NaN once it has seen one (the row of scale(1) / binmax(1), the matrix of scale())
__host__ __device__ __forceinline__ double max_nan(double a, double b) { return (a > b || a != a) ? a : b; }
template <int W>
__device__ __forceinline__ double sg_max_nan(double v) {
#pragma unroll
  for (int o = W / 2; o > 0; o >>= 1) v = max_nan(v, __shfl_xor(v, o, W));
  return v;
}
__global__ __launch_bounds__(256) void k_norm_rows(int64_t N, const int64_t* __restrict__ indptr,
                                                   const double* __restrict__ data, double* __restrict__ out) {
  const int sub = threadIdx.x / RP_SUB, lane = threadIdx.x % RP_SUB, subs = blockDim.x / RP_SUB;
  for (int64_t row = (int64_t)blockIdx.x * subs + sub; row < N; row += (int64_t)gridDim.x * subs) {
    int64_t s = indptr[row], e = indptr[row + 1];
    double y = 0.0;
    for (int64_t k = s + lane; k < e; k += RP_SUB) y += data[k];
    y = sg_sum<RP_SUB>(y);
    double r = recip0(y);
    for (int64_t k = s + lane; k < e; k += RP_SUB) out[k] = data[k] * r;
  }
}
__global__ __launch_bounds__(256) void k_binmax_rows(int64_t N, int32_t K, const int64_t* __restrict__ indptr,
                                                     const double* __restrict__ data, int8_t* __restrict__ out) {
  const int sub = threadIdx.x / RP_SUB, lane = threadIdx.x % RP_SUB, subs = blockDim.x / RP_SUB;
  for (int64_t row = (int64_t)blockIdx.x * subs + sub; row < N; row += (int64_t)gridDim.x * subs) {
    int64_t s = indptr[row], e = indptr[row + 1];
    bool any = false;
    double m = 0.0;
    for (int64_t k = s + lane; k < e; k += RP_SUB) { m = any ? max_nan(m, data[k]) : data[k]; any = true; }
    // combine: lanes without entries must not contribute
    double mm = any ? m : -INFINITY;
    mm = sg_max_nan<RP_SUB>(mm);
    if ((e - s) < K) mm = max_nan(mm, 0.0);  // implicit zeros take part in max(1)
    for (int64_t k = s + lane; k < e; k += RP_SUB) out[k] = (data[k] == mm) ? 1 : 0;   // a NaN maximum marks nothing
  }
}

// whole-matrix reductions for csr_matrix_plus.norm() / scale() (sparse_plus.py:46-48, 93-95)
__global__ __launch_bounds__(256) void k_reduce_all(const double* __restrict__ v, int64_t n, int want_max,
                                                    double* __restrict__ part) {
  __shared__ double scratch[16];
  double acc = want_max ? -INFINITY : 0.0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    acc = want_max ? max_nan(acc, v[i]) : acc + v[i];
  if (want_max) {
    acc = sg_max_nan<64>(acc);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) scratch[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) { double m = scratch[0]; for (int i = 1; i < (int)(blockDim.x >> 6); ++i) m = max_nan(m, scratch[i]); part[blockIdx.x] = m; }
  } else {
    double t = block_sum(acc, scratch);
    if (threadIdx.x == 0) part[blockIdx.x] = t;
  }
}
__global__ void k_scale_all(const double* __restrict__ v, int64_t n, double f, double* __restrict__ out) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = v[i] * f;
}
__global__ __launch_bounds__(256) void k_scale_rows(int64_t N, int32_t K, const int64_t* __restrict__ indptr,
                                                    const double* __restrict__ data, double* __restrict__ out) {
  const int sub = threadIdx.x / RP_SUB, lane = threadIdx.x % RP_SUB, subs = blockDim.x / RP_SUB;
  for (int64_t row = (int64_t)blockIdx.x * subs + sub; row < N; row += (int64_t)gridDim.x * subs) {
    int64_t s = indptr[row], e = indptr[row + 1];
    double m = -INFINITY;
    for (int64_t k = s + lane; k < e; k += RP_SUB) m = max_nan(m, data[k]);
    m = sg_max_nan<RP_SUB>(m);
    if ((e - s) < K) m = max_nan(m, 0.0);              // implicit zeros take part in max(1)
    double r = recip0(m);                              // (a NaN maximum makes the whole row NaN)
    for (int64_t k = s + lane; k < e; k += RP_SUB) out[k] = data[k] * r;
  }
}

extern "C" {

// ---------------------------------------------------------------------------
// numpy's LEGACY random stream for `choose` (sparse_plus.py:140-154)
// ---------------------------------------------------------------------------
// choose_random draws one np.random.choice per row with several best hits, on numpy's global legacy RandomState — the
// stream `telescope assign` seeds (telescope_assign.py:429-431).  One draw below a bound c is, in numpy's C
// (legacy-distributions / _bounded_integers, masked rejection): mask = the smallest 2^b - 1 >= c - 1, then 32-bit
// Mersenne-Twister outputs until (output & mask) <= c - 1.  np.random.randint(0, counts) on an array does exactly that
// per element (46 ms for the 5.6e6 tied rows of the 50M-row benchmark: it was the largest item of the whole report);
// this is the same loop in C on the caller's MT19937 state (np.random.get_state() -> here -> np.random.set_state()),
// bit for bit the same picks and the same state afterwards (tests/test_host_logic.py).  Host code: the stream is
// sequential by definition.
int tsem_legacy_randint(uint32_t* key624, int32_t* pos, const int32_t* counts, int64_t n, int32_t* out) {
  if (!key624 || !pos || (!counts && n) || (!out && n) || n < 0 || *pos < 0 || *pos > 624) return TSEM_ERR_ARG;
  constexpr int NN = 624, MM = 397;
  constexpr uint32_t UPPER = 0x80000000u, LOWER = 0x7fffffffu, MATRIX_A = 0x9908b0dfu;
  uint32_t* mt = key624;
  int p = *pos;
  // the 624 outputs of the current state, tempered in one vectorisable sweep (the draw loop then only masks and compares:
  // 2.0 -> ~1 ns per draw; the state array itself stays untempered, as numpy keeps it)
  uint32_t buf[NN];
  auto temper_all = [&]() {
    for (int kk = 0; kk < NN; ++kk) {
      uint32_t y = mt[kk];
      y ^= y >> 11; y ^= (y << 7) & 0x9d2c5680u; y ^= (y << 15) & 0xefc60000u; y ^= y >> 18;
      buf[kk] = y;
    }
  };
  auto refill = [&]() {
    int kk = 0;
    for (; kk < NN - MM; ++kk) { const uint32_t y = (mt[kk] & UPPER) | (mt[kk + 1] & LOWER); mt[kk] = mt[kk + MM] ^ (y >> 1) ^ ((y & 1u) ? MATRIX_A : 0u); }
    for (; kk < NN - 1; ++kk) { const uint32_t y = (mt[kk] & UPPER) | (mt[kk + 1] & LOWER); mt[kk] = mt[kk + (MM - NN)] ^ (y >> 1) ^ ((y & 1u) ? MATRIX_A : 0u); }
    const uint32_t y = (mt[NN - 1] & UPPER) | (mt[0] & LOWER);
    mt[NN - 1] = mt[MM - 1] ^ (y >> 1) ^ ((y & 1u) ? MATRIX_A : 0u);
    p = 0;
    temper_all();
  };
  if (p < NN) temper_all();
  for (int64_t i = 0; i < n; ++i) {
    const int32_t c = counts[i];
    if (c <= 0) return TSEM_ERR_ARG;                       // (numpy raises "low >= high")
    const uint32_t rng = (uint32_t)c - 1u;
    if (rng == 0) { out[i] = 0; continue; }                // no random number is consumed
    const uint32_t mask = 0xFFFFFFFFu >> __builtin_clz(rng);   // the smallest 2^b - 1 >= rng
    uint32_t v;
    do {
      if (p == NN) refill();
      v = buf[p++] & mask;
    } while (v > rng);
    out[i] = (int32_t)v;
  }
  *pos = p;
  return TSEM_OK;
}

// ---------------------------------------------------------------------------
// csr_matrix_plus primitives (stateless)
// ---------------------------------------------------------------------------
// The row pointers size the device buffers (indptr[n_rows]) and bound every row's reads and writes, so they are checked on the
// host before the device is touched: a malformed CSR is TSEM_ERR_ARG with or without a GPU, and never reaches a kernel.
static int csr_check_args(const char* fn, int64_t n_rows, int32_t n_cols, const int64_t* indptr, const void* data,
                          const void* out) {
  const char* why = nullptr;
  if (n_rows < 0 || n_cols < 0) why = "negative n_rows / n_cols";
  else if (!indptr) why = "indptr is NULL";
  else if (indptr[0] != 0) why = "indptr[0] is not 0";
  else {
    for (int64_t i = 0; i < n_rows && !why; ++i)
      if (indptr[i + 1] < indptr[i]) why = "indptr is not monotone";
    if (!why && indptr[n_rows] > 0 && (!data || !out)) why = "data / out is NULL with stored entries";
  }
  if (!why) return TSEM_OK;
  g_create_err = std::string(fn) + ": " + why;
  return TSEM_ERR_ARG;
}
// one HIP call of a primitive: the first failure is kept (rc, text) and the steps after it are skipped by their `rc == TSEM_OK &&`
static void csr_hip(hipError_t e, const char* what, int& rc) {
  if (e != hipSuccess && rc == TSEM_OK) { g_create_err = std::string(what) + ": " + hipGetErrorString(e); rc = TSEM_ERR_HIP; }
}
static inline int csr_row_grid(int64_t n_rows) {
  const int64_t subs = 256 / RP_SUB;                      // rows per block
  return (int)std::min<int64_t>(8192, std::max<int64_t>(1, (n_rows + subs - 1) / subs));
}

static int csr_prim(const char* fn, int device, int64_t n_rows, int32_t n_cols, const int64_t* indptr, const double* data,
                    double* out_d, int8_t* out_b) {
  int rc = csr_check_args(fn, n_rows, n_cols, indptr, data, out_d ? (const void*)out_d : (const void*)out_b);
  if (rc != TSEM_OK) return rc;
  if (hipSetDevice(device) != hipSuccess) { g_create_err = "hipSetDevice failed (no usable HIP device)"; return TSEM_ERR_HIP; }
  const int64_t nnz = indptr[n_rows];
  int64_t* d_ip = nullptr; double *d_in = nullptr, *d_od = nullptr; int8_t* d_ob = nullptr;
  TSEM_SCOPED(d_ip); TSEM_SCOPED(d_in); TSEM_SCOPED(d_od); TSEM_SCOPED(d_ob);
  bool ok = hipMalloc((void**)&d_ip, sizeof(int64_t) * (n_rows + 1)) == hipSuccess &&
            hipMalloc((void**)&d_in, sizeof(double) * std::max<int64_t>(1, nnz)) == hipSuccess;
  if (ok && out_d) ok = hipMalloc((void**)&d_od, sizeof(double) * std::max<int64_t>(1, nnz)) == hipSuccess;
  if (ok && out_b) ok = hipMalloc((void**)&d_ob, std::max<int64_t>(1, nnz)) == hipSuccess;
  if (!ok) { g_create_err = "hipMalloc failed"; return TSEM_ERR_NOMEM; }
  csr_hip(hipMemcpy(d_ip, indptr, sizeof(int64_t) * (n_rows + 1), hipMemcpyHostToDevice), "hipMemcpy(indptr)", rc);
  if (rc == TSEM_OK && nnz) csr_hip(hipMemcpy(d_in, data, sizeof(double) * nnz, hipMemcpyHostToDevice), "hipMemcpy(data)", rc);
  if (rc == TSEM_OK && n_rows) {
    const int grid = csr_row_grid(n_rows);
    if (out_d) k_norm_rows<<<grid, 256>>>(n_rows, d_ip, d_in, d_od);
    if (out_b) k_binmax_rows<<<grid, 256>>>(n_rows, n_cols, d_ip, d_in, d_ob);
    csr_hip(hipGetLastError(), "kernel launch", rc);
  }
  if (rc == TSEM_OK) csr_hip(hipDeviceSynchronize(), "hipDeviceSynchronize", rc);
  if (rc == TSEM_OK && nnz && out_d) csr_hip(hipMemcpy(out_d, d_od, sizeof(double) * nnz, hipMemcpyDeviceToHost), "hipMemcpy(out)", rc);
  if (rc == TSEM_OK && nnz && out_b) csr_hip(hipMemcpy(out_b, d_ob, nnz, hipMemcpyDeviceToHost), "hipMemcpy(out)", rc);
  return rc;
}

// mode 0: out = data * (1 / sum(data))   norm()   sparse_plus.py:47-48
// mode 1: out = data * (1 / max(data))   scale()  sparse_plus.py:94-95   (max over the matrix incl. implicit zeros)
// mode 2: out = data * recip0(row max)   scale(1) sparse_plus.py:96-97
int tsem_csr_scale(int device, int mode, int64_t n_rows, int32_t n_cols, const int64_t* indptr, const double* data,
                   double* out) {
  if (mode < 0 || mode > 2) { g_create_err = "tsem_csr_scale: mode is not 0, 1 or 2"; return TSEM_ERR_ARG; }
  int rc = csr_check_args("tsem_csr_scale", n_rows, n_cols, indptr, data, out);
  if (rc != TSEM_OK) return rc;
  if (hipSetDevice(device) != hipSuccess) { g_create_err = "hipSetDevice failed (no usable HIP device)"; return TSEM_ERR_HIP; }
  const int64_t nnz = indptr[n_rows];
  int64_t* d_ip = nullptr; double *d_in = nullptr, *d_out = nullptr, *d_part = nullptr;
  TSEM_SCOPED(d_ip); TSEM_SCOPED(d_in); TSEM_SCOPED(d_out); TSEM_SCOPED(d_part);
  const int G = 512;
  bool ok = hipMalloc((void**)&d_ip, sizeof(int64_t) * (n_rows + 1)) == hipSuccess &&
            hipMalloc((void**)&d_in, sizeof(double) * std::max<int64_t>(1, nnz)) == hipSuccess &&
            hipMalloc((void**)&d_out, sizeof(double) * std::max<int64_t>(1, nnz)) == hipSuccess &&
            hipMalloc((void**)&d_part, sizeof(double) * G) == hipSuccess;
  if (!ok) { g_create_err = "hipMalloc failed"; return TSEM_ERR_NOMEM; }
  csr_hip(hipMemcpy(d_ip, indptr, sizeof(int64_t) * (n_rows + 1), hipMemcpyHostToDevice), "hipMemcpy(indptr)", rc);
  if (rc == TSEM_OK && nnz) csr_hip(hipMemcpy(d_in, data, sizeof(double) * nnz, hipMemcpyHostToDevice), "hipMemcpy(data)", rc);
  if (rc == TSEM_OK && mode == 2 && n_rows) {
    k_scale_rows<<<csr_row_grid(n_rows), 256>>>(n_rows, n_cols, d_ip, d_in, d_out);
    csr_hip(hipGetLastError(), "kernel launch", rc);
  } else if (rc == TSEM_OK && mode != 2 && nnz) {
    k_reduce_all<<<G, 256>>>(d_in, nnz, mode == 1, d_part);
    csr_hip(hipGetLastError(), "kernel launch", rc);
    std::vector<double> part(G);
    if (rc == TSEM_OK) csr_hip(hipMemcpy(part.data(), d_part, sizeof(double) * G, hipMemcpyDeviceToHost), "hipMemcpy(partials)", rc);
    if (rc == TSEM_OK) {
      double r = mode == 1 ? -INFINITY : 0.0;
      for (int i = 0; i < G; ++i) r = mode == 1 ? max_nan(r, part[i]) : r + part[i];
      if (mode == 1 && nnz < n_rows * (int64_t)n_cols) r = max_nan(r, 0.0);
      k_scale_all<<<cdiv64(nnz, 256), 256>>>(d_in, nnz, 1.0 / r, d_out);
      csr_hip(hipGetLastError(), "kernel launch", rc);
    }
  }
  if (rc == TSEM_OK) csr_hip(hipDeviceSynchronize(), "hipDeviceSynchronize", rc);
  if (rc == TSEM_OK && nnz) csr_hip(hipMemcpy(out, d_out, sizeof(double) * nnz, hipMemcpyDeviceToHost), "hipMemcpy(out)", rc);
  return rc;
}

int tsem_csr_norm_rows(int device, int64_t n_rows, const int64_t* indptr, const double* data, double* out) {
  return csr_prim("tsem_csr_norm_rows", device, n_rows, 0, indptr, data, out, nullptr);
}
int tsem_csr_binmax_rows(int device, int64_t n_rows, int32_t n_cols, const int64_t* indptr, const double* data,
                         int8_t* out) {
  return csr_prim("tsem_csr_binmax_rows", device, n_rows, n_cols, indptr, data, nullptr, out);
}

}  // extern "C"
