// Multi-Krum aggregation (robust_agg = multi_krum) for gfx950: every
// model's participant rows, read where they lie in the replica bank, are
// judged by their squared L2 distances to each other.
//
// A model's [n, n] double distance matrix is never held whole above a row
// bound: the op works in passes, pass t holding the rows
// [t * slab, (t + 1) * slab) of every model as a [slab, n] block of the
// scratch buffer (distances -> scores -> discard).
//
// krum_dist_kernel    grid (column tile, row tile of the slab, model x
//                     coordinate chunk). A block owns KR_TILE x KR_TILE row
//                     pairs and one chunk of KR_CHUNK coordinates; both row
//                     tiles are staged in LDS KR_PC coordinates at a time,
//                     each thread holds 2 x 2 pairs and adds (x_i - x_j)^2
//                     in double, coordinate by coordinate. A pair's sum
//                     depends on the coordinate decomposition alone and
//                     (a - b)^2 == (b - a)^2 bit for bit, so D[i, j] and
//                     D[j, i] are one value wherever, and in whichever pass,
//                     they are computed.
// krum_reduce_kernel  more than one chunk (a CNN's vector): adds a pair's
//                     chunk partials in chunk order.
// krum_score_kernel   one block per row of the slab: the q + 1 smallest of
//                     the row's n entries, the diagonal's 0 among them, by
//                     bitwise bisection on the doubles' bit patterns (they
//                     are >= +0, so the patterns order as the values), then
//                     one pass that sums what lies below the threshold and
//                     adds the threshold's tie copies.
// krum_select_kernel  ranks a model's participants by (score, id, position)
//                     and writes the first s positions in rank order.
// krum_mean_kernel    one thread per coordinate walks the selected rows in
//                     selection order; s = 1 stores the row's bits.
//
// No atomics: two launches on one input agree bit for bit, and so do any
// two slab sizes. The specification is comm/robust.py (krum_sqdist,
// krum_scores, krum_select, multi_krum_aggregate).
#include <hip/hip_runtime.h>
#include <torch/extension.h>
#include <c10/hip/HIPStream.h>

constexpr int KR_THREADS = 256;
constexpr int KR_TILE = 32;                    // rows of either tile
constexpr int KR_PC = 64;                      // coordinates staged at once
constexpr int KR_CHUNK = 4096;                 // coordinates per block
constexpr int KR_SCORE_LDS = 4096;             // row entries kept in LDS
constexpr int KR_SCRATCH_ROWS = 8192;          // default slab: 512 MiB at
                                               // n = 8192
constexpr long long KR_SCRATCH_ELEMS = 1ll << 27;   // doubles: 1 GiB

typedef unsigned long long u64;

struct KrumArgs {
  const float* bank;         // [R, P]
  const int* mod_off;        // [K+1] participant ranges, grouped by model
  const long long* rows;     // [U] bank row of every participant
  const long long* ids;      // [U] tie-break key of every participant
  const int* qsel;           // [K] q: 0-based sorted position that bounds
                             //     the q + 1 smallest entries of a row
  const int* nsel;           // [K] s: rows kept
  const long long* d_off;    // [K] a model's first scratch element
  double* scratch;           // per model [nsplit, min(slab, n), n]
  double* scores;            // [U]
  int* sel;                  // [U] a model's s kept positions, in order
  float* out;                // [K, out_stride], columns [0, P) written
  long long P, out_stride;
  int slab, nsplit;
};

static __device__ __forceinline__ double kr_canon(double v) {
  return v <= 1.79769313486231570e308 ? v : __longlong_as_double(
      0x7ff0000000000000ll);                   // NaN or Inf: +Inf
}

extern "C" __global__ __launch_bounds__(KR_THREADS)
void krum_dist_kernel(KrumArgs a, int r0) {
  __shared__ float xi[KR_TILE][KR_PC + 1];
  __shared__ float xj[KR_TILE][KR_PC + 1];
  const int m = blockIdx.z / a.nsplit;
  const int c = blockIdx.z - m * a.nsplit;
  const int u0 = a.mod_off[m];
  const int n = a.mod_off[m + 1] - u0;
  const int slab = n < a.slab ? n : a.slab;
  const int li0 = blockIdx.y * KR_TILE;        // row within the slab
  const int j0 = blockIdx.x * KR_TILE;
  if (li0 >= slab || r0 + li0 >= n || j0 >= n) return;
  const int tid = threadIdx.x;
  const int tx = tid & 15, ty = tid >> 4;
  const long long* rows = a.rows + u0;
  const long long p_begin = (long long)c * KR_CHUNK;
  const long long p_end = p_begin + KR_CHUNK < a.P ? p_begin + KR_CHUNK
                                                   : a.P;
  double acc00 = 0.0, acc01 = 0.0, acc10 = 0.0, acc11 = 0.0;
  for (long long p0 = p_begin; p0 < p_end; p0 += KR_PC) {
    for (int e = tid; e < KR_TILE * KR_PC; e += KR_THREADS) {
      const int r = e / KR_PC, col = e - r * KR_PC;
      const long long p = p0 + col;
      const int gi = r0 + li0 + r, gj = j0 + r;
      const bool in_p = p < p_end;
      xi[r][col] = (in_p && li0 + r < slab && gi < n)
          ? a.bank[rows[gi] * a.P + p] : 0.f;
      xj[r][col] = (in_p && gj < n) ? a.bank[rows[gj] * a.P + p] : 0.f;
    }
    __syncthreads();
    // padded coordinates are 0 in both tiles and add +0
#pragma unroll 8
    for (int k = 0; k < KR_PC; ++k) {
      const double a0 = xi[ty][k], a1 = xi[ty + 16][k];
      const double b0 = xj[tx][k], b1 = xj[tx + 16][k];
      const double d00 = a0 - b0, d01 = a0 - b1;
      const double d10 = a1 - b0, d11 = a1 - b1;
      acc00 += d00 * d00;
      acc01 += d01 * d01;
      acc10 += d10 * d10;
      acc11 += d11 * d11;
    }
    __syncthreads();
  }
  double* dst = a.scratch + a.d_off[m] + (long long)c * slab * n;
  auto put = [&](int li, int gj, double v) {
    const int gi = r0 + li;
    if (li < slab && gi < n && gj < n)
      dst[(long long)li * n + gj] = gi == gj ? 0.0 : kr_canon(v);
  };
  put(li0 + ty, j0 + tx, acc00);
  put(li0 + ty, j0 + tx + 16, acc01);
  put(li0 + ty + 16, j0 + tx, acc10);
  put(li0 + ty + 16, j0 + tx + 16, acc11);
}

// D <- the chunk partials added in chunk order, into chunk 0's place.
extern "C" __global__ __launch_bounds__(KR_THREADS)
void krum_reduce_kernel(KrumArgs a, int r0) {
  const int m = blockIdx.y;
  const int n = a.mod_off[m + 1] - a.mod_off[m];
  const int slab = n < a.slab ? n : a.slab;
  const long long e = (long long)blockIdx.x * KR_THREADS + threadIdx.x;
  if (n <= 0 || e >= (long long)slab * n) return;
  if (r0 + e / n >= n) return;
  double* base = a.scratch + a.d_off[m] + e;
  const long long stride = (long long)slab * n;
  double v = base[0];
  for (int c = 1; c < a.nsplit; ++c) v += base[c * stride];
  base[0] = kr_canon(v);
}

extern "C" __global__ __launch_bounds__(KR_THREADS)
void krum_score_kernel(KrumArgs a, int r0) {
  __shared__ u64 keys[KR_SCORE_LDS];
  __shared__ int cnt[2][KR_THREADS / 64];
  __shared__ int cnt_less[KR_THREADS / 64];
  __shared__ double part[KR_THREADS / 64];
  const int m = blockIdx.y;
  const int u0 = a.mod_off[m];
  const int n = a.mod_off[m + 1] - u0;
  const int slab = n < a.slab ? n : a.slab;
  const int li = blockIdx.x, i = r0 + li;
  if (li >= slab || i >= n) return;            // uniform over the block
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const u64* row = (const u64*)(a.scratch + a.d_off[m] + (long long)li * n);
  const int staged = n < KR_SCORE_LDS ? n : KR_SCORE_LDS;
  for (int e = tid; e < staged; e += KR_THREADS) keys[e] = row[e];
  __syncthreads();
  auto key_at = [&](int e) -> u64 {
    return e < KR_SCORE_LDS ? keys[e] : row[e];
  };
  // sorted[target] is the largest v with count(key < v) <= target; every
  // key is a double >= +0, so bit 63 is clear
  const int target = a.qsel[m];
  u64 thr = 0ull;
  for (int b = 62; b >= 0; --b) {
    const u64 t = thr | (1ull << b);
    int cl = 0;
    for (int e = tid; e < n; e += KR_THREADS) cl += key_at(e) < t;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) cl += __shfl_xor(cl, off);
    // the buffers alternate, so one barrier per pass is enough
    if (lane == 0) cnt[b & 1][wave] = cl;
    __syncthreads();
    int tot = 0;
#pragma unroll
    for (int w = 0; w < KR_THREADS / 64; ++w) tot += cnt[b & 1][w];
    if (tot <= target) thr = t;
  }
  // what lies strictly below the threshold, then the threshold's copies
  double acc = 0.0;
  int cl = 0;
  for (int e = tid; e < n; e += KR_THREADS) {
    const u64 k = key_at(e);
    if (k < thr) {
      acc += __longlong_as_double((long long)k);
      ++cl;
    }
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    acc += __shfl_xor(acc, off);
    cl += __shfl_xor(cl, off);
  }
  if (lane == 0) {
    part[wave] = acc;
    cnt_less[wave] = cl;
  }
  __syncthreads();
  if (tid != 0) return;
  double sum = 0.0;
  int less = 0;
  for (int w = 0; w < KR_THREADS / 64; ++w) {  // wave order
    sum += part[w];
    less += cnt_less[w];
  }
  sum += (double)(target + 1 - less) * __longlong_as_double((long long)thr);
  a.scores[u0 + i] = sum;
}

extern "C" __global__ __launch_bounds__(KR_THREADS)
void krum_select_kernel(KrumArgs a) {
  const int m = blockIdx.y;
  const int u0 = a.mod_off[m];
  const int n = a.mod_off[m + 1] - u0;
  const int i = blockIdx.x * KR_THREADS + threadIdx.x;
  if (i >= n) return;
  const double si = a.scores[u0 + i];
  const long long idi = a.ids[u0 + i];
  int rank = 0;
  for (int j = 0; j < n; ++j) {
    const double sj = a.scores[u0 + j];
    const long long idj = a.ids[u0 + j];
    rank += sj < si ||
        (sj == si && (idj < idi || (idj == idi && j < i)));
  }
  if (rank < a.nsel[m]) a.sel[u0 + rank] = u0 + i;
}

extern "C" __global__ __launch_bounds__(KR_THREADS)
void krum_mean_kernel(KrumArgs a) {
  const int m = blockIdx.y;
  const int u0 = a.mod_off[m];
  const int n = a.mod_off[m + 1] - u0;
  const long long p = (long long)blockIdx.x * KR_THREADS + threadIdx.x;
  if (n <= 0 || p >= a.P) return;              // empty: the row keeps its bits
  const int s = a.nsel[m];
  const int* sel = a.sel + u0;
  float acc = a.bank[a.rows[sel[0]] * a.P + p];
  if (s > 1) {
    for (int i = 1; i < s; ++i)
      acc = __fadd_rn(acc, a.bank[a.rows[sel[i]] * a.P + p]);
    acc = __fdiv_rn(acc, (float)s);
  }
  a.out[(long long)m * a.out_stride + p] = acc;
}

// ---------------------------------------------------------------------------
// host wrapper
// ---------------------------------------------------------------------------

static void kr_check(const torch::Tensor& t, c10::ScalarType dt,
                     const char* name) {
  TORCH_CHECK(t.is_cuda() && t.dtype() == dt && t.is_contiguous(), name,
              " must be a contiguous CUDA tensor of the expected dtype");
}

// out[m, :P] <- Multi-Krum over bank[rows[mod_off[m] : mod_off[m+1]]] for
// every model with a participant; scores and sel keep the per-participant
// scores and the kept positions. The caller (ops/krum_hip.py) has checked
// rows against the bank and 0 <= qsel[m] < n[m], 1 <= nsel[m] <= n[m] on
// the host, and laid out the scratch: n_max is the largest participant
// count, slab the rows of a model held at once, d_off[m] the first element
// of model m's [nsplit, min(slab, n), n] block and `need` their total.
static void krum_impl(torch::Tensor bank, torch::Tensor mod_off,
                      torch::Tensor rows, torch::Tensor ids,
                      torch::Tensor qsel, torch::Tensor nsel,
                      torch::Tensor d_off, torch::Tensor scratch,
                      torch::Tensor scores, torch::Tensor sel,
                      torch::Tensor out, int64_t n_max, int64_t slab,
                      int64_t need) {
  kr_check(bank, torch::kFloat32, "bank");
  kr_check(mod_off, torch::kInt32, "mod_off");
  kr_check(rows, torch::kInt64, "rows");
  kr_check(ids, torch::kInt64, "ids");
  kr_check(qsel, torch::kInt32, "qsel");
  kr_check(nsel, torch::kInt32, "nsel");
  kr_check(d_off, torch::kInt64, "d_off");
  kr_check(scratch, torch::kFloat64, "scratch");
  kr_check(scores, torch::kFloat64, "scores");
  kr_check(sel, torch::kInt32, "sel");
  TORCH_CHECK(out.is_cuda() && out.dtype() == torch::kFloat32 &&
              out.dim() == 2 && out.stride(1) == 1,
              "krum: out must be a CUDA float32 matrix with unit column "
              "stride");
  TORCH_CHECK(bank.dim() == 2, "krum: bank must be [R, P]");
  const int64_t P = bank.size(1), K = out.size(0), U = rows.size(0);
  TORCH_CHECK(out.size(1) == P && out.stride(0) >= P,
              "krum: out must be [K, P]");
  TORCH_CHECK(mod_off.size(0) == K + 1 && qsel.size(0) == K &&
              nsel.size(0) == K && d_off.size(0) == K,
              "krum: model arrays differ in size");
  TORCH_CHECK(ids.size(0) == U && scores.size(0) == U && sel.size(0) == U,
              "krum: participant arrays differ in size");
  if (U == 0 || P == 0) return;
  const int64_t nsplit = (P + KR_CHUNK - 1) / KR_CHUNK;
  TORCH_CHECK(n_max >= 1 && n_max <= U && slab >= 1 && slab <= n_max,
              "krum: slab out of range");
  TORCH_CHECK(need <= scratch.numel() && need <= KR_SCRATCH_ELEMS,
              "krum: scratch too small for the layout");
  TORCH_CHECK(K >= 1 && K * nsplit <= 65535,
              "krum: K x chunks out of the grid range");
  TORCH_CHECK(slab <= 65535 && (P + KR_THREADS - 1) / KR_THREADS <= 2147483647,
              "krum: slab or P out of the grid range");

  KrumArgs a;
  a.bank = bank.data_ptr<float>();
  a.mod_off = mod_off.data_ptr<int>();
  a.rows = (const long long*)rows.data_ptr<int64_t>();
  a.ids = (const long long*)ids.data_ptr<int64_t>();
  a.qsel = qsel.data_ptr<int>();
  a.nsel = nsel.data_ptr<int>();
  a.d_off = (const long long*)d_off.data_ptr<int64_t>();
  a.scratch = scratch.data_ptr<double>();
  a.scores = scores.data_ptr<double>();
  a.sel = sel.data_ptr<int>();
  a.out = out.data_ptr<float>();
  a.P = P;
  a.out_stride = out.stride(0);
  a.slab = (int)slab;
  a.nsplit = (int)nsplit;
  auto stream = c10::hip::getCurrentHIPStream();
  const unsigned jt = (unsigned)((n_max + KR_TILE - 1) / KR_TILE);
  const unsigned it = (unsigned)((slab + KR_TILE - 1) / KR_TILE);
  const unsigned red = (unsigned)((slab * n_max + KR_THREADS - 1) /
                                  KR_THREADS);
  for (int64_t r0 = 0; r0 < n_max; r0 += slab) {
    hipLaunchKernelGGL(krum_dist_kernel,
                       dim3(jt, it, (unsigned)(K * nsplit)),
                       dim3(KR_THREADS), 0, stream, a, (int)r0);
    TORCH_CHECK(hipGetLastError() == hipSuccess, "krum_dist_kernel launch");
    if (nsplit > 1) {
      hipLaunchKernelGGL(krum_reduce_kernel, dim3(red, (unsigned)K),
                         dim3(KR_THREADS), 0, stream, a, (int)r0);
      TORCH_CHECK(hipGetLastError() == hipSuccess,
                  "krum_reduce_kernel launch");
    }
    hipLaunchKernelGGL(krum_score_kernel, dim3((unsigned)slab, (unsigned)K),
                       dim3(KR_THREADS), 0, stream, a, (int)r0);
    TORCH_CHECK(hipGetLastError() == hipSuccess, "krum_score_kernel launch");
  }
  hipLaunchKernelGGL(krum_select_kernel,
                     dim3((unsigned)((n_max + KR_THREADS - 1) / KR_THREADS),
                          (unsigned)K),
                     dim3(KR_THREADS), 0, stream, a);
  TORCH_CHECK(hipGetLastError() == hipSuccess, "krum_select_kernel launch");
  hipLaunchKernelGGL(krum_mean_kernel,
                     dim3((unsigned)((P + KR_THREADS - 1) / KR_THREADS),
                          (unsigned)K),
                     dim3(KR_THREADS), 0, stream, a);
  TORCH_CHECK(hipGetLastError() == hipSuccess, "krum_mean_kernel launch");
}

void register_krum(pybind11::module_& mod) {
  mod.def("krum", &krum_impl,
          "Multi-Krum: pairwise distances, scores, selection, mean");
  mod.def("krum_tile", []() { return (int64_t)KR_TILE; },
          "rows of either tile of the distance kernel");
  mod.def("krum_chunk", []() { return (int64_t)KR_CHUNK; },
          "coordinates one block of the distance kernel covers");
  mod.def("krum_score_lds", []() { return (int64_t)KR_SCORE_LDS; },
          "entries of a distance row the score kernel keeps in LDS");
  mod.def("krum_scratch_rows", []() { return (int64_t)KR_SCRATCH_ROWS; },
          "default bound on the distance rows of a model held at once");
  mod.def("krum_scratch_elems", []() { return (int64_t)KR_SCRATCH_ELEMS; },
          "doubles the scratch may hold (1 GiB)");
}
