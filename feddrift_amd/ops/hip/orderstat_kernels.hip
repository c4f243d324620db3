// Order-statistic aggregation (robust_agg = trimmed_mean | median) for
// gfx950: the coordinate-wise trimmed mean of every model's participant
// rows, read where they lie in the replica bank.
//
// orderstat_kernel   grid (coordinate tile, model). A block owns OS_TP
//                    consecutive coordinates of one model; lanes run along
//                    the coordinate, the OS_SR thread rows take every
//                    OS_SR-th participant. Per coordinate it finds the keys
//                    of sorted positions k and n-k-1 by bitwise bisection
//                    on the 32-bit ordered key (32 counting passes, both
//                    thresholds in one pass, slice counts combined through
//                    LDS), then one pass sums what lies strictly between
//                    and adds the tie copies of the two thresholds.
//
//                    A model of at most OS_LDS_ROWS participants has its
//                    [n x OS_TP] key tile staged in LDS once; a larger one
//                    streams every pass from global memory.
// orderstat_small_kernel   models of at most OS_SMALL_ROWS participants:
//                    one thread per coordinate, ranks by counting in
//                    registers. The other kernel leaves these models alone.
//
// No atomics; the summation order is a function of n and the block shape.
//
// The specification is comm/robust.py (ordered_key, order_stat_mean).
#include <hip/hip_runtime.h>
#include <torch/extension.h>
#include <c10/hip/HIPStream.h>

constexpr int OS_THREADS = 256;
constexpr int OS_TP = 16;                        // coordinates per block
constexpr int OS_SR = OS_THREADS / OS_TP;        // participant slices
constexpr int OS_LDS_ROWS = 768;                 // 48 KiB of keys
constexpr int OS_SMALL_ROWS = 16;                // rows the rank kernel takes

typedef unsigned int u32;

struct OrderStatArgs {
  const float* bank;         // [R, P]
  const int* mod_off;        // [K+1] participant ranges, grouped by model
  const long long* rows;     // [U] bank row of every participant
  const int* trim;           // [K] k: dropped at either end
  float* out;                // [K, out_stride], columns [0, P) written
  long long P, out_stride;
};

// total order -NaN < -Inf < ... < -0 < +0 < ... < +Inf < +NaN
static __device__ __forceinline__ u32 os_key(u32 u) {
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

static __device__ __forceinline__ float os_value(u32 q) {
  return __uint_as_float((q & 0x80000000u) ? (q & 0x7fffffffu) : ~q);
}

extern "C" __global__ __launch_bounds__(OS_THREADS)
void orderstat_kernel(OrderStatArgs a) {
  __shared__ u32 tile[OS_LDS_ROWS * OS_TP];
  __shared__ int cnt[2][2][OS_SR][OS_TP];
  __shared__ float part[OS_SR][OS_TP];
  const int tx = threadIdx.x & (OS_TP - 1);
  const int ty = threadIdx.x / OS_TP;
  const int m = blockIdx.y;
  const int u0 = a.mod_off[m];
  const int n = a.mod_off[m + 1] - u0;
  if (n <= OS_SMALL_ROWS) return;   // empty: the row keeps its bits;
                                    // small: orderstat_small_kernel's
  const int k = a.trim[m];
  const long long p = (long long)blockIdx.x * OS_TP + tx;
  const bool live = p < a.P;
  const bool staged = n <= OS_LDS_ROWS;
  const long long* rows = a.rows + u0;

  auto load_key = [&](int r) -> u32 {
    return live ? os_key(__float_as_uint(a.bank[rows[r] * a.P + p])) : 0u;
  };
  if (staged) {
    for (int r = ty; r < n; r += OS_SR) tile[r * OS_TP + tx] = load_key(r);
    __syncthreads();
  }
  auto key_at = [&](int r) -> u32 {
    return staged ? tile[r * OS_TP + tx] : load_key(r);
  };

  // sorted[j] is the largest v with count(key < v) <= j: one bit per pass
  const int j_lo = k, j_hi = n - k - 1;
  u32 lo = 0u, hi = 0u;
  for (int b = 31; b >= 0; --b) {
    const u32 t_lo = lo | (1u << b), t_hi = hi | (1u << b);
    int c_lo = 0, c_hi = 0;
    for (int r = ty; r < n; r += OS_SR) {
      const u32 q = key_at(r);
      c_lo += q < t_lo;
      c_hi += q < t_hi;
    }
    // the buffers alternate, so one barrier per pass is enough
    int (*c)[OS_SR][OS_TP] = cnt[b & 1];
    c[0][ty][tx] = c_lo;
    c[1][ty][tx] = c_hi;
    __syncthreads();
    int s_lo = 0, s_hi = 0;
#pragma unroll
    for (int j = 0; j < OS_SR; ++j) {
      s_lo += c[0][j][tx];
      s_hi += c[1][j][tx];
    }
    if (s_lo <= j_lo) lo = t_lo;
    if (s_hi <= j_hi) hi = t_hi;
  }

  // what lies strictly between the thresholds, and how many rows sit at or
  // beyond either of them (the last pass used cnt[0]; cnt[1] is free)
  float acc = 0.f;
  int c_le = 0, c_ge = 0;
  for (int r = ty; r < n; r += OS_SR) {
    const u32 q = key_at(r);
    c_le += q <= lo;
    c_ge += q >= hi;
    if (q > lo && q < hi) acc = __fadd_rn(acc, os_value(q));
  }
  cnt[1][0][ty][tx] = c_le;
  cnt[1][1][ty][tx] = c_ge;
  part[ty][tx] = acc;
  __syncthreads();
  if (ty != 0 || !live) return;
  const int s = n - 2 * k;
  const float v_lo = os_value(lo), v_hi = os_value(hi);
  float res;
  if (s == 2) {
    res = __fmul_rn(__fadd_rn(v_lo, v_hi), 0.5f);
  } else if (lo == hi) {
    res = v_lo;              // s == 1, or every survivor is this value
  } else {
    int n_le = 0, n_ge = 0;
    float sum = 0.f;
    for (int j = 0; j < OS_SR; ++j) {            // slice order
      n_le += cnt[1][0][j][tx];
      n_ge += cnt[1][1][j][tx];
      sum = __fadd_rn(sum, part[j][tx]);
    }
    sum = __fadd_rn(sum, __fmul_rn((float)(n_le - k), v_lo));
    sum = __fadd_rn(sum, __fmul_rn((float)(n_ge - k), v_hi));
    res = __fdiv_rn(sum, (float)s);
  }
  a.out[(long long)m * a.out_stride + p] = res;
}

// A model of at most OS_SMALL_ROWS participants (a CNN fleet: few rows, a
// long vector): one thread per coordinate, the keys in registers, every
// key's rank by counting (ties broken by row order), no LDS and no barrier.
// The survivors are the ranks k .. n-k-1, summed in row order.
extern "C" __global__ __launch_bounds__(OS_THREADS)
void orderstat_small_kernel(OrderStatArgs a) {
  const int m = blockIdx.y;
  const int u0 = a.mod_off[m];
  const int n = a.mod_off[m + 1] - u0;
  if (n <= 0 || n > OS_SMALL_ROWS) return;
  const long long p = (long long)blockIdx.x * OS_THREADS + threadIdx.x;
  if (p >= a.P) return;
  const int k = a.trim[m];
  const long long* rows = a.rows + u0;
  u32 q[OS_SMALL_ROWS];
#pragma unroll
  for (int i = 0; i < OS_SMALL_ROWS; ++i)
    q[i] = i < n ? os_key(__float_as_uint(a.bank[rows[i] * a.P + p])) : 0u;
  const int r_lo = k, r_hi = n - k - 1, s = n - 2 * k;
  float sum = 0.f;
  u32 q_lo = 0u, q_hi = 0u;
#pragma unroll
  for (int i = 0; i < OS_SMALL_ROWS; ++i) {
    if (i < n) {                                 // uniform over the block
      int rank = 0;
#pragma unroll
      for (int j = 0; j < OS_SMALL_ROWS; ++j)
        if (j < n) rank += (q[j] < q[i]) || (j < i && q[j] == q[i]);
      if (rank == r_lo) q_lo = q[i];
      if (rank == r_hi) q_hi = q[i];
      if (rank >= r_lo && rank <= r_hi) sum = __fadd_rn(sum, os_value(q[i]));
    }
  }
  float res;
  if (s == 1) res = os_value(q_lo);
  else if (s == 2) res = __fmul_rn(__fadd_rn(os_value(q_lo), os_value(q_hi)),
                                   0.5f);
  else res = __fdiv_rn(sum, (float)s);
  a.out[(long long)m * a.out_stride + p] = res;
}

// ---------------------------------------------------------------------------
// host wrapper
// ---------------------------------------------------------------------------

static void os_check(const torch::Tensor& t, c10::ScalarType dt,
                     const char* name) {
  TORCH_CHECK(t.is_cuda() && t.dtype() == dt && t.is_contiguous(), name,
              " must be a contiguous CUDA tensor of the expected dtype");
}

// out[m, :P] <- trimmed mean (trim[m] rows dropped at either end of every
// coordinate) of bank[rows[mod_off[m] : mod_off[m+1]]], for every model
// with a participant. The caller has checked rows against the bank and
// 0 <= 2 trim[m] < n[m] on the host (ops/orderstat_hip.py), and says which
// of the two kernels have a model to work on.
static void order_stat_impl(torch::Tensor bank, torch::Tensor mod_off,
                            torch::Tensor rows, torch::Tensor trim,
                            torch::Tensor out, bool any_small,
                            bool any_large) {
  os_check(bank, torch::kFloat32, "bank");
  os_check(mod_off, torch::kInt32, "mod_off");
  os_check(rows, torch::kInt64, "rows");
  os_check(trim, torch::kInt32, "trim");
  TORCH_CHECK(out.is_cuda() && out.dtype() == torch::kFloat32 &&
              out.dim() == 2 && out.stride(1) == 1,
              "order_stat: out must be a CUDA float32 matrix with unit "
              "column stride");
  TORCH_CHECK(bank.dim() == 2, "order_stat: bank must be [R, P]");
  const int64_t P = bank.size(1), K = out.size(0);
  TORCH_CHECK(out.size(1) == P && out.stride(0) >= P,
              "order_stat: out must be [K, P]");
  TORCH_CHECK(mod_off.size(0) == K + 1 && trim.size(0) == K,
              "order_stat: model arrays differ in size");
  TORCH_CHECK(K >= 1 && K <= 65535, "order_stat: K out of the grid range");
  if (rows.size(0) == 0 || P == 0) return;
  const int64_t tiles = (P + OS_TP - 1) / OS_TP;
  TORCH_CHECK(tiles <= 2147483647, "order_stat: P out of the grid range");

  OrderStatArgs a;
  a.bank = bank.data_ptr<float>();
  a.mod_off = mod_off.data_ptr<int>();
  a.rows = (const long long*)rows.data_ptr<int64_t>();
  a.trim = trim.data_ptr<int>();
  a.out = out.data_ptr<float>();
  a.P = P;
  a.out_stride = out.stride(0);
  auto stream = c10::hip::getCurrentHIPStream();
  if (any_small) {
    const int64_t chunks = (P + OS_THREADS - 1) / OS_THREADS;
    hipLaunchKernelGGL(orderstat_small_kernel,
                       dim3((unsigned)chunks, (unsigned)K), dim3(OS_THREADS),
                       0, stream, a);
    TORCH_CHECK(hipGetLastError() == hipSuccess,
                "orderstat_small_kernel launch");
  }
  if (any_large) {
    hipLaunchKernelGGL(orderstat_kernel, dim3((unsigned)tiles, (unsigned)K),
                       dim3(OS_THREADS), 0, stream, a);
    TORCH_CHECK(hipGetLastError() == hipSuccess, "orderstat_kernel launch");
  }
}

void register_orderstat(pybind11::module_& mod) {
  mod.def("order_stat", &order_stat_impl,
          "coordinate-wise trimmed mean / median of participant rows");
  mod.def("orderstat_tp", []() { return (int64_t)OS_TP; },
          "coordinates one block covers");
  mod.def("orderstat_lds_rows", []() { return (int64_t)OS_LDS_ROWS; },
          "participants of a model up to which its key tile stays in LDS");
  mod.def("orderstat_small_rows", []() { return (int64_t)OS_SMALL_ROWS; },
          "participants of a model up to which the rank kernel takes it");
}
