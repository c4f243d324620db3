// Ring-arithmetic secure aggregation (secure_agg=2) for gfx950.
//
// secagg_mask_kernel    this rank's contribution [K, P+1] in Z_{2^56}:
//                       sum over owned uploads of quantised(n*theta, n) plus
//                       the signed Philox4x32-10 pair masks.
// secagg_reduce_kernel  sums the upload-slice slabs of the mask kernel.
// secagg_dequant_kernel all-reduced ring sums -> the float [K, P+1] partial.
//
// The numpy specification is comm/secure_agg.py; every value here must match
// it bit for bit. All mask arithmetic is unsigned 64-bit and wraps; integer
// sums are order-independent, so the slab split cannot change a result.
#include <hip/hip_runtime.h>
#include <torch/extension.h>
#include <c10/hip/HIPStream.h>

constexpr int SA_THREADS = 256;
constexpr int SA_ELEMS = 4;                       // consecutive per thread
constexpr int SA_SPAN = SA_THREADS * SA_ELEMS;    // elements per block
constexpr int SA_RING_BITS = 56;
constexpr unsigned long long SA_RING_MASK = (1ull << SA_RING_BITS) - 1ull;

typedef unsigned long long u64;
typedef unsigned int u32;
// replica rows are only dword-aligned at odd P
typedef float f4u __attribute__((ext_vector_type(4), aligned(4)));

static __device__ __forceinline__ u64 mix64(u64 z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// Philox4x32-10, counter (j, 0, 0, 0): two ring elements per call.
static __device__ __forceinline__ void philox_pair(u32 j, u64 key, u64& r0, u64& r1) {
  u32 c0 = j, c1 = 0u, c2 = 0u, c3 = 0u;
  u32 k0 = (u32)key, k1 = (u32)(key >> 32);
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const u32 hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const u32 hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  r0 = ((u64)c0 | ((u64)c1 << 32)) & SA_RING_MASK;
  r1 = ((u64)c2 | ((u64)c3 << 32)) & SA_RING_MASK;
}

struct SecaggMaskArgs {
  const float* replicas;     // [R, P]
  const int* mod_off;        // [K+1] upload ranges, grouped by model
  const long long* up_row;   // [U] replica row
  const int* up_w;           // [U] global worker id
  const float* up_n;         // [U] aggregation weight
  const int* up_es;          // [U] first edge
  const int* up_ec;          // [U] edge count
  const int* edge_other;     // [E] neighbour worker ids
  u64* out;                  // [S, K, L] slabs (S == 1: the contribution)
  int* flag;                 // range guard, sticky
  u64 base;                  // job key prefix
  u64 agg_ctr;
  double scale;              // 2^F
  double limit;              // 2^(M-1) / n_workers
  long long P;
  int K, S;                  // models, upload slices per model
  int TQ, tq_shift;          // element quads per block row (power of two)
  int rank, world, skip_intra;
};

// quantise one upload element; violation -> 0 and *bad
static __device__ __forceinline__ u64 quant(float v, double scale, double limit,
                                     bool& bad) {
  const double s = (double)v * scale;
  const bool ok = fabs(s) < limit;          // false for NaN
  bad |= !ok;
  return ok ? (u64)(long long)rint(s) : 0ull;
}

// grid (element chunk, model x slice group). Every thread owns 4
// consecutive elements, so two Philox calls serve one edge, and keeps its
// accumulators in registers until the single store. A block is TQ element
// quads wide and 256/TQ upload slices tall: at CNN size (TQ = 256) a block
// is one slice over 1024 elements and its upload loop is uniform; at MLP
// size (a row is a few quads) the lanes that a row cannot fill take further
// slices instead of idling.
extern "C" __global__ __launch_bounds__(SA_THREADS)
void secagg_mask_kernel(SecaggMaskArgs a) {
  const long long L = a.P + 1;
  const int tx = threadIdx.x & (a.TQ - 1);
  const int ty = threadIdx.x >> a.tq_shift;
  const int TY = SA_THREADS >> a.tq_shift;
  const int SB = (a.S + TY - 1) / TY;          // blocks per model
  const long long e0 = ((long long)blockIdx.x * a.TQ + tx) * SA_ELEMS;
  const int m = blockIdx.y / SB;
  const int slice = (blockIdx.y - m * SB) * TY + ty;
  if (slice >= a.S || e0 >= L) return;
  const int u_lo = a.mod_off[m], u_hi = a.mod_off[m + 1];
  const int per = (u_hi - u_lo + a.S - 1) / a.S;
  const int u0 = u_lo + slice * per;
  const int u1 = min(u0 + per, u_hi);
  const u64 hm = mix64(mix64(a.base ^ a.agg_ctr) ^ (u64)m);
  const u32 j0 = (u32)(e0 >> 1);

  u64 acc[SA_ELEMS] = {0ull, 0ull, 0ull, 0ull};
  bool bad = false;
  for (int u = u0; u < u1; ++u) {
    const float n = a.up_n[u];
    const int w = a.up_w[u];
    const float* th = a.replicas + a.up_row[u] * a.P;
    float v[SA_ELEMS];
    if (e0 + SA_ELEMS <= a.P) {
      const f4u t = *(const f4u*)(th + e0);
#pragma unroll
      for (int i = 0; i < SA_ELEMS; ++i) v[i] = __fmul_rn(n, t[i]);
    } else {
#pragma unroll
      for (int i = 0; i < SA_ELEMS; ++i) {
        const long long e = e0 + i;
        v[i] = e < a.P ? __fmul_rn(n, th[e]) : (e == a.P ? n : 0.f);
      }
    }
#pragma unroll
    for (int i = 0; i < SA_ELEMS; ++i)
      acc[i] += quant(v[i], a.scale, a.limit, bad);
    const int es = a.up_es[u], ec = a.up_ec[u];
    for (int k = es; k < es + ec; ++k) {
      const int o = a.edge_other[k];
      if (o == w) continue;
      if (a.skip_intra && (o % a.world) == a.rank) continue;
      const bool add = w < o;
      const u64 key = mix64(mix64(hm ^ (u64)(add ? w : o)) ^
                            (u64)(add ? o : w));
      u64 r[SA_ELEMS];
      philox_pair(j0, key, r[0], r[1]);
      philox_pair(j0 + 1u, key, r[2], r[3]);
#pragma unroll
      for (int i = 0; i < SA_ELEMS; ++i)
        acc[i] = add ? acc[i] + r[i] : acc[i] - r[i];
    }
  }
  if (bad) atomicOr(a.flag, 1);
  u64* dst = a.out + ((long long)slice * a.K + m) * L;
#pragma unroll
  for (int i = 0; i < SA_ELEMS; ++i)
    if (e0 + i < L) dst[e0 + i] = acc[i] & SA_RING_MASK;
}

extern "C" __global__ __launch_bounds__(SA_THREADS)
void secagg_reduce_kernel(const u64* slabs, u64* out, long long n, int S) {
  const long long i = (long long)blockIdx.x * SA_THREADS + threadIdx.x;
  if (i >= n) return;
  u64 s = 0ull;
  for (int k = 0; k < S; ++k) s += slabs[(long long)k * n + i];
  out[i] = s & SA_RING_MASK;
}

extern "C" __global__ __launch_bounds__(SA_THREADS)
void secagg_dequant_kernel(const long long* ring, float* out, long long n,
                           double inv_scale) {
  const long long i = (long long)blockIdx.x * SA_THREADS + threadIdx.x;
  if (i >= n) return;
  const u64 r = (u64)ring[i] & SA_RING_MASK;
  // sign-extend from SA_RING_BITS
  const long long s =
      (long long)(r << (64 - SA_RING_BITS)) >> (64 - SA_RING_BITS);
  out[i] = (float)((double)s * inv_scale);
}

static void check_i32(const torch::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.dtype() == torch::kInt32 && t.is_contiguous(),
              name, " must be contiguous int32 CUDA");
}

// Contribution of this rank, [K, P+1] int64 in [0, 2^56). `slices` is the
// number of upload slices per model (>= 1); with more than one the slabs
// are summed by the reduce kernel.
static torch::Tensor secagg_mask_impl(
    torch::Tensor replicas, torch::Tensor mod_off, torch::Tensor up_row,
    torch::Tensor up_w, torch::Tensor up_n, torch::Tensor up_es,
    torch::Tensor up_ec, torch::Tensor edge_other, torch::Tensor flag,
    int64_t base, int64_t agg_ctr, int64_t frac_bits, int64_t n_workers,
    int64_t rank, int64_t world, bool skip_intra, int64_t slices) {
  TORCH_CHECK(replicas.is_cuda() && replicas.dtype() == torch::kFloat32 &&
              replicas.dim() == 2 && replicas.is_contiguous(),
              "replicas must be contiguous 2-d f32 CUDA");
  check_i32(mod_off, "mod_off"); check_i32(up_w, "up_w");
  check_i32(up_es, "up_es"); check_i32(up_ec, "up_ec");
  check_i32(edge_other, "edge_other"); check_i32(flag, "flag");
  TORCH_CHECK(up_row.is_cuda() && up_row.dtype() == torch::kInt64 &&
              up_row.is_contiguous(), "up_row must be contiguous int64 CUDA");
  TORCH_CHECK(up_n.is_cuda() && up_n.dtype() == torch::kFloat32 &&
              up_n.is_contiguous(), "up_n must be contiguous f32 CUDA");
  const int64_t K = mod_off.size(0) - 1;
  const int64_t U = up_row.size(0);
  const int64_t P = replicas.size(1);
  const int64_t L = P + 1;
  const int64_t quads = (L + SA_ELEMS - 1) / SA_ELEMS;
  int tq_shift = 0;
  while ((1 << tq_shift) < SA_THREADS && (1 << tq_shift) < quads) ++tq_shift;
  const int TQ = 1 << tq_shift, TY = SA_THREADS / TQ;
  TORCH_CHECK(slices >= 1, "secagg_mask: slices must be >= 1");
  const int64_t SB = (slices + TY - 1) / TY;
  TORCH_CHECK(K >= 1 && K * SB <= 65535,
              "secagg_mask: K * slice groups outside the grid's y range");
  TORCH_CHECK(up_w.size(0) == U && up_n.size(0) == U && up_es.size(0) == U &&
              up_ec.size(0) == U, "secagg_mask: upload arrays differ in size");
  TORCH_CHECK(frac_bits >= 0 && frac_bits < SA_RING_BITS - 1 && n_workers >= 1 &&
              world >= 1 && rank >= 0 && rank < world,
              "secagg_mask: bad frac_bits / n_workers / rank / world");
  TORCH_CHECK(L < (1ll << 32), "secagg_mask: P+1 exceeds the Philox counter");
  auto opt = torch::TensorOptions().dtype(torch::kInt64)
                 .device(replicas.device());
  auto out = torch::empty({K, L}, opt);
  auto slabs = slices > 1 ? torch::empty({slices, K, L}, opt) : out;
  auto stream = c10::hip::getCurrentHIPStream();

  SecaggMaskArgs a;
  a.replicas = replicas.data_ptr<float>();
  a.mod_off = mod_off.data_ptr<int>();
  a.up_row = (const long long*)up_row.data_ptr<int64_t>();
  a.up_w = up_w.data_ptr<int>();
  a.up_n = up_n.data_ptr<float>();
  a.up_es = up_es.data_ptr<int>();
  a.up_ec = up_ec.data_ptr<int>();
  a.edge_other = edge_other.data_ptr<int>();
  a.out = (u64*)slabs.data_ptr<int64_t>();
  a.flag = flag.data_ptr<int>();
  a.base = (u64)base;
  a.agg_ctr = (u64)agg_ctr;
  a.scale = ldexp(1.0, (int)frac_bits);
  a.limit = ldexp(1.0, SA_RING_BITS - 1) / (double)n_workers;
  a.P = P;
  a.K = (int)K; a.S = (int)slices;
  a.TQ = TQ; a.tq_shift = tq_shift;
  a.rank = (int)rank; a.world = (int)world; a.skip_intra = skip_intra ? 1 : 0;

  const unsigned gx = (unsigned)((quads + TQ - 1) / TQ);
  hipLaunchKernelGGL(secagg_mask_kernel, dim3(gx, (unsigned)(K * SB)),
                     dim3(SA_THREADS), 0, stream, a);
  TORCH_CHECK(hipGetLastError() == hipSuccess, "secagg_mask_kernel launch");
  if (slices > 1) {
    const long long n = K * L;
    hipLaunchKernelGGL(secagg_reduce_kernel,
                       dim3((unsigned)((n + SA_THREADS - 1) / SA_THREADS)),
                       dim3(SA_THREADS), 0, stream,
                       (const u64*)slabs.data_ptr<int64_t>(),
                       (u64*)out.data_ptr<int64_t>(), n, (int)slices);
    TORCH_CHECK(hipGetLastError() == hipSuccess,
                "secagg_reduce_kernel launch");
  }
  return out;
}

static void secagg_dequant_impl(torch::Tensor ring, torch::Tensor out,
                         int64_t frac_bits) {
  TORCH_CHECK(ring.is_cuda() && ring.dtype() == torch::kInt64 &&
              ring.is_contiguous(), "ring must be contiguous int64 CUDA");
  TORCH_CHECK(out.is_cuda() && out.dtype() == torch::kFloat32 &&
              out.is_contiguous() && out.numel() == ring.numel(),
              "out must be contiguous f32 CUDA of ring's size");
  const long long n = ring.numel();
  if (n == 0) return;
  hipLaunchKernelGGL(secagg_dequant_kernel,
                     dim3((unsigned)((n + SA_THREADS - 1) / SA_THREADS)),
                     dim3(SA_THREADS), 0, c10::hip::getCurrentHIPStream(),
                     (const long long*)ring.data_ptr<int64_t>(),
                     out.data_ptr<float>(), n, ldexp(1.0, -(int)frac_bits));
  TORCH_CHECK(hipGetLastError() == hipSuccess, "secagg_dequant_kernel launch");
}

void register_secagg(pybind11::module_& mod) {
  mod.def("secagg_mask", &secagg_mask_impl,
          "ring-arithmetic masked contribution of this rank");
  mod.def("secagg_dequant", &secagg_dequant_impl,
          "ring sums -> float partial");
  mod.def("secagg_span", []() { return (int64_t)SA_SPAN; },
          "elements one block of the mask kernel covers");
}
