// Defended aggregation (robust_fused=1) for gfx950: update-norm clipping,
// Gaussian noise and the FedOpt server step on the device.
//
// robust_norm_kernel    per-pair partial sums of |replica - global[model]|^2
// robust_scale_kernel   per-pair clip factor + per-model (clipped, seen) counts
// robust_accum_kernel   clipped rows written back, weighted sums per model
// robust_reduce_kernel  fixed-order sum of the accumulate kernel's pair slices
// robust_totals_kernel  parks the [K] weight totals before the apply launch
// robust_apply_kernel   average + optional noise + server-optimizer step,
//                       draining `partial` on its way out
//
// The specification is comm/robust.py (clip_and_accumulate, gaussian_noise,
// server_step); this file follows it in fp32.
#include <hip/hip_runtime.h>
#include <torch/extension.h>
#include <c10/hip/HIPStream.h>

constexpr int RB_THREADS = 256;
constexpr int RB_ELEMS = 4;                       // consecutive per thread
constexpr int RB_SPAN = RB_THREADS * RB_ELEMS;    // elements per block row
constexpr int RB_NORM_ITERS = 4;                  // quads per thread, norm pass
constexpr int RB_WAVE = 64;

typedef unsigned long long u64;
typedef unsigned int u32;
// rows of [R, P] and [K, P+1] tensors are only dword-aligned at odd P
typedef float f4u __attribute__((ext_vector_type(4), aligned(4)));

// ---------------------------------------------------------------------------
// clip pass
// ---------------------------------------------------------------------------

struct RobustClipArgs {
  float* replicas;           // [R, P]
  const float* global;       // [K, P]
  const int* mod_off;        // [K+1] pair ranges, grouped by model
  const long long* pr_row;   // [U] replica row
  const int* pr_model;       // [U]
  const float* pr_w;         // [U] aggregation weight
  double* nsq;               // [U, C] partial squared norms
  float* scale;              // [U]
  int* counts;               // [K, 2] (clipped, seen), accumulated
  float* out;                // [S, K, L] slabs, or nullptr (clip only)
  float bound;
  long long P;
  int U, K, S, C;            // pairs, models, pair slices per model, chunks
  int TQ, tq_shift;          // element quads per block row (power of two)
  int iters;                 // quads per thread in the norm pass
};

// grid (element chunk, pair group). A block is TQ quads wide and 256/TQ
// pairs tall, every thread sums `iters` quads TQ apart: at CNN size a block
// is one pair over 4096 elements, at MLP size (a row is a few quads) the
// lanes a row cannot fill take further pairs. One double per (pair, chunk).
extern "C" __global__ __launch_bounds__(RB_THREADS)
void robust_norm_kernel(RobustClipArgs a) {
  __shared__ double red[RB_THREADS / RB_WAVE];
  const int tx = threadIdx.x & (a.TQ - 1);
  const int ty = threadIdx.x >> a.tq_shift;
  const int TY = RB_THREADS >> a.tq_shift;
  const int u = blockIdx.y * TY + ty;
  const bool live = u < a.U;
  float s = 0.f;
  if (live) {
    const float* th = a.replicas + a.pr_row[u] * a.P;
    const float* g = a.global + (long long)a.pr_model[u] * a.P;
    for (int it = 0; it < a.iters; ++it) {
      const long long e0 =
          (((long long)blockIdx.x * a.iters + it) * a.TQ + tx) * RB_ELEMS;
      if (e0 + RB_ELEMS <= a.P) {
        const f4u t = *(const f4u*)(th + e0);
        const f4u q = *(const f4u*)(g + e0);
#pragma unroll
        for (int i = 0; i < RB_ELEMS; ++i) {
          const float d = t[i] - q[i];
          s = fmaf(d, d, s);
        }
      } else {
        for (int i = 0; i < RB_ELEMS; ++i)
          if (e0 + i < a.P) {
            const float d = th[e0 + i] - g[e0 + i];
            s = fmaf(d, d, s);
          }
      }
    }
  }
  double acc = (double)s;
  // the TQ threads of one pair: inside a wave by shuffles, across waves
  // (TQ = 128 or 256) through LDS in wave order
  const int w = a.TQ < RB_WAVE ? a.TQ : RB_WAVE;
  for (int o = w >> 1; o > 0; o >>= 1) acc += __shfl_xor(acc, o, RB_WAVE);
  if (a.TQ <= RB_WAVE) {
    if (live && tx == 0) a.nsq[(long long)u * a.C + blockIdx.x] = acc;
    return;
  }
  if ((threadIdx.x & (RB_WAVE - 1)) == 0) red[threadIdx.x / RB_WAVE] = acc;
  __syncthreads();
  if (live && tx == 0) {
    const int w0 = threadIdx.x / RB_WAVE, nw = a.TQ / RB_WAVE;
    double t = 0.0;
    for (int k = 0; k < nw; ++k) t += red[w0 + k];
    a.nsq[(long long)u * a.C + blockIdx.x] = t;
  }
}

// one wave per pair: chunk sums in a fixed order, then the factor
// min(1, bound / (norm + 1e-12)) and the model's counts
extern "C" __global__ __launch_bounds__(RB_WAVE)
void robust_scale_kernel(RobustClipArgs a) {
  const int u = blockIdx.x;
  double acc = 0.0;
  for (int c = threadIdx.x; c < a.C; c += RB_WAVE)
    acc += a.nsq[(long long)u * a.C + c];
  for (int o = RB_WAVE >> 1; o > 0; o >>= 1)
    acc += __shfl_xor(acc, o, RB_WAVE);
  if (threadIdx.x == 0) {
    const float norm = (float)sqrt(acc);
    const float sc = fminf(1.0f, a.bound / (norm + 1e-12f));
    a.scale[u] = sc;
    const int m = a.pr_model[u];
    atomicAdd(a.counts + 2 * m + 1, 1);
    if (sc < 1.0f) atomicAdd(a.counts + 2 * m, 1);
  }
}

// grid (element chunk, model x slice group), the shape of the secure-
// aggregation mask kernel: every thread owns 4 consecutive elements of one
// model and one slice of that model's pairs, writes each clipped row quad
// back, keeps the weighted sum in registers and stores it once. Slot P of a
// model's row takes the weights. Each (pair, element) belongs to exactly
// one thread, so the write-back needs no ordering.
extern "C" __global__ __launch_bounds__(RB_THREADS)
void robust_accum_kernel(RobustClipArgs a) {
  const long long L = a.P + 1;
  const int tx = threadIdx.x & (a.TQ - 1);
  const int ty = threadIdx.x >> a.tq_shift;
  const int TY = RB_THREADS >> a.tq_shift;
  const int SB = (a.S + TY - 1) / TY;          // blocks per model
  const long long e0 = ((long long)blockIdx.x * a.TQ + tx) * RB_ELEMS;
  const int m = blockIdx.y / SB;
  const int slice = (blockIdx.y - m * SB) * TY + ty;
  if (slice >= a.S || e0 >= L) return;
  const int u_lo = a.mod_off[m], u_hi = a.mod_off[m + 1];
  const int per = (u_hi - u_lo + a.S - 1) / a.S;
  const int u0 = u_lo + slice * per;
  const int u1 = min(u0 + per, u_hi);
  const float* g = a.global + (long long)m * a.P;
  const bool full = e0 + RB_ELEMS <= a.P;
  float q[RB_ELEMS];
#pragma unroll
  for (int i = 0; i < RB_ELEMS; ++i)
    q[i] = e0 + i < a.P ? g[e0 + i] : 0.f;

  float acc[RB_ELEMS] = {0.f, 0.f, 0.f, 0.f};
  for (int u = u0; u < u1; ++u) {
    const float n = a.pr_w[u];
    const float sc = a.scale[u];
    float* th = a.replicas + a.pr_row[u] * a.P;
    float v[RB_ELEMS];
    if (full) {
      const f4u t = *(const f4u*)(th + e0);
#pragma unroll
      for (int i = 0; i < RB_ELEMS; ++i) v[i] = t[i];
    } else {
#pragma unroll
      for (int i = 0; i < RB_ELEMS; ++i)
        v[i] = e0 + i < a.P ? th[e0 + i] : 0.f;
    }
    if (sc < 1.0f) {
#pragma unroll
      for (int i = 0; i < RB_ELEMS; ++i)
        v[i] = __fadd_rn(q[i], __fmul_rn(v[i] - q[i], sc));
      if (full) {
        f4u t;
#pragma unroll
        for (int i = 0; i < RB_ELEMS; ++i) t[i] = v[i];
        *(f4u*)(th + e0) = t;
      } else {
#pragma unroll
        for (int i = 0; i < RB_ELEMS; ++i)
          if (e0 + i < a.P) th[e0 + i] = v[i];
      }
    }
    if (n > 0.f) {
#pragma unroll
      for (int i = 0; i < RB_ELEMS; ++i) {
        const long long e = e0 + i;
        acc[i] += e < a.P ? __fmul_rn(n, v[i]) : (e == a.P ? n : 0.f);
      }
    }
  }
  if (a.out == nullptr) return;
  float* dst = a.out + ((long long)slice * a.K + m) * L;
#pragma unroll
  for (int i = 0; i < RB_ELEMS; ++i)
    if (e0 + i < L) dst[e0 + i] = acc[i];
}

// partial[i] += slab_0[i] + slab_1[i] + ... in slice order
extern "C" __global__ __launch_bounds__(RB_THREADS)
void robust_reduce_kernel(const float* slabs, float* partial, long long n,
                          int S) {
  const long long i = (long long)blockIdx.x * RB_THREADS + threadIdx.x;
  if (i >= n) return;
  float s = slabs[i];
  for (int k = 1; k < S; ++k) s += slabs[(long long)k * n + i];
  partial[i] += s;
}

// ---------------------------------------------------------------------------
// apply pass
// ---------------------------------------------------------------------------

enum { RB_AVG = 0, RB_SGD = 1, RB_ADAM = 2, RB_ADAGRAD = 3 };

struct RobustApplyArgs {
  float* global;             // [K, P]
  float* partial;            // [K, P+1], drained to zero
  const unsigned char* mask; // [K] or nullptr
  const float* totals;       // [K], filled BEFORE this launch
  float* s0;                 // adam m / sgd momentum buffer / adagrad sum
  float* s1;                 // adam v
  long long P;
  int K, kind, first;        // first: the momentum buffer starts as g
  int QB;                    // quads per slab
  float lr, momentum;
  float step_size, inv_sqrt_bc2;   // adam: lr / (1 - b1^t), 1 / sqrt(1 - b2^t)
  float noise_std;           // 0: no noise
  u32 key0, key1, ctr0, ctr1;
};

static __device__ __forceinline__ void philox4(u32 c0, u32 c1, u32 c2, u32 c3,
                                               u32 k0, u32 k1, u32* x) {
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
  x[0] = c0; x[1] = c1; x[2] = c2; x[3] = c3;
}

// Box-Muller on u = (x + 0.5) 2^-32, accurate libm calls
static __device__ __forceinline__ void box_muller(u32 xa, u32 xb, float& z0,
                                                  float& z1) {
  const float ua = ((float)xa + 0.5f) * 2.3283064365386963e-10f;
  const float ub = ((float)xb + 0.5f) * 2.3283064365386963e-10f;
  const float r = sqrtf(-2.0f * logf(ua));
  float sn, cs;
  sincosf(6.2831853071795865f * ub, &sn, &cs);
  z0 = r * cs;
  z1 = r * sn;
}

extern "C" __global__ __launch_bounds__(RB_THREADS)
void robust_totals_kernel(const float* partial, float* totals, int K,
                          long long P) {
  const int m = blockIdx.x * RB_THREADS + threadIdx.x;
  if (m < K) totals[m] = partial[(long long)m * (P + 1) + P];
}

// grid (model, slab). The total comes from `totals`, which no block of this
// launch writes; block (m, 0) alone clears partial[m, P].
extern "C" __global__ __launch_bounds__(RB_THREADS)
void robust_apply_kernel(RobustApplyArgs a) {
  const int m = blockIdx.x;
  const float tot = a.totals[m];
  const bool upd = tot > 0.f && !(a.mask && !a.mask[m]);
  const float inv = upd ? 1.0f / tot : 0.f;
  float* gl = a.global + (long long)m * a.P;
  float* pa = a.partial + (long long)m * (a.P + 1);
  float* s0 = a.s0 ? a.s0 + (long long)m * a.P : nullptr;
  float* s1 = a.s1 ? a.s1 + (long long)m * a.P : nullptr;
  if (blockIdx.y == 0 && threadIdx.x == 0) pa[a.P] = 0.f;
  const long long quads = (a.P + RB_ELEMS - 1) / RB_ELEMS;
  const long long q_lo = (long long)blockIdx.y * a.QB;
  const long long q_hi = min(q_lo + a.QB, quads);
  // a non-updated row moves only through optimizer state
  if (!upd && a.kind == RB_AVG) {
    for (long long j = q_lo + threadIdx.x; j < q_hi; j += RB_THREADS)
      for (int i = 0; i < RB_ELEMS; ++i)
        if (j * RB_ELEMS + i < a.P) pa[j * RB_ELEMS + i] = 0.f;
    return;
  }
  for (long long j = q_lo + threadIdx.x; j < q_hi; j += RB_THREADS) {
    const long long e0 = j * RB_ELEMS;
    float z[RB_ELEMS] = {0.f, 0.f, 0.f, 0.f};
    if (upd && a.noise_std > 0.f) {
      u32 x[4];
      philox4((u32)j, (u32)m, a.ctr0, a.ctr1, a.key0, a.key1, x);
      box_muller(x[0], x[1], z[0], z[1]);
      box_muller(x[2], x[3], z[2], z[3]);
    }
#pragma unroll
    for (int i = 0; i < RB_ELEMS; ++i) {
      const long long e = e0 + i;
      if (e >= a.P) break;
      const float p = gl[e];
      float g = 0.f, avg = p;
      if (upd) {
        avg = __fmul_rn(pa[e], inv);
        if (a.noise_std > 0.f) avg = __fadd_rn(avg, __fmul_rn(a.noise_std, z[i]));
        g = p - avg;
      }
      pa[e] = 0.f;
      float np_;
      if (a.kind == RB_AVG) {
        np_ = avg;
      } else if (a.kind == RB_SGD) {
        float d = g;
        if (s0) {
          d = a.first ? g : __fadd_rn(__fmul_rn(a.momentum, s0[e]), g);
          s0[e] = d;
        }
        np_ = __fsub_rn(p, __fmul_rn(a.lr, d));
      } else if (a.kind == RB_ADAM) {
        const float mm = __fadd_rn(s0[e], __fmul_rn(g - s0[e], 0.1f));
        const float vv = __fadd_rn(__fmul_rn(0.999f, s1[e]),
                                   __fmul_rn(__fmul_rn(g, g), 0.001f));
        s0[e] = mm;
        s1[e] = vv;
        const float den = __fadd_rn(__fmul_rn(sqrtf(vv), a.inv_sqrt_bc2), 1e-8f);
        np_ = __fsub_rn(p, __fmul_rn(a.step_size, mm / den));
      } else {
        const float ss = __fadd_rn(s0[e], __fmul_rn(g, g));
        s0[e] = ss;
        np_ = __fsub_rn(p, __fmul_rn(a.lr, g / __fadd_rn(sqrtf(ss), 1e-10f)));
      }
      gl[e] = np_;
    }
  }
}

// ---------------------------------------------------------------------------
// host wrappers
// ---------------------------------------------------------------------------

static void rb_check(const torch::Tensor& t, c10::ScalarType dt,
                     const char* name) {
  TORCH_CHECK(t.is_cuda() && t.dtype() == dt && t.is_contiguous(), name,
              " must be a contiguous CUDA tensor of the expected dtype");
}

// Clip the listed pairs' replica rows in place; with `partial`, add the
// weighted sums of the clipped rows into it. `slices` = pair slices per
// model (>= 1). counts [K, 2] int32 accumulates (clipped, seen).
static void robust_clip_impl(
    torch::Tensor replicas, torch::Tensor global_params, torch::Tensor mod_off,
    torch::Tensor pr_row, torch::Tensor pr_model, torch::Tensor pr_w,
    c10::optional<torch::Tensor> partial, torch::Tensor counts, double bound,
    int64_t slices) {
  rb_check(replicas, torch::kFloat32, "replicas");
  rb_check(global_params, torch::kFloat32, "global_params");
  rb_check(mod_off, torch::kInt32, "mod_off");
  rb_check(pr_row, torch::kInt64, "pr_row");
  rb_check(pr_model, torch::kInt32, "pr_model");
  rb_check(pr_w, torch::kFloat32, "pr_w");
  rb_check(counts, torch::kInt32, "counts");
  TORCH_CHECK(replicas.dim() == 2 && global_params.dim() == 2 &&
              replicas.size(1) == global_params.size(1),
              "robust_clip: replicas / global_params shapes differ");
  const int64_t K = global_params.size(0), P = global_params.size(1);
  const int64_t U = pr_row.size(0), L = P + 1;
  TORCH_CHECK(mod_off.size(0) == K + 1 && pr_model.size(0) == U &&
              pr_w.size(0) == U && counts.numel() == 2 * K,
              "robust_clip: pair / model arrays differ in size");
  TORCH_CHECK(bound > 0.0, "robust_clip: bound must be positive");
  TORCH_CHECK(slices >= 1, "robust_clip: slices must be >= 1");
  if (partial.has_value()) {
    rb_check(*partial, torch::kFloat32, "partial");
    TORCH_CHECK(partial->dim() == 2 && partial->size(0) == K &&
                partial->size(1) == L, "robust_clip: partial must be [K, P+1]");
  }
  if (U == 0 || P == 0) return;
  const int64_t quads = (L + RB_ELEMS - 1) / RB_ELEMS;
  int tq_shift = 0;
  while ((1 << tq_shift) < RB_THREADS && (1 << tq_shift) < quads) ++tq_shift;
  const int TQ = 1 << tq_shift, TY = RB_THREADS / TQ;
  const int64_t SB = (slices + TY - 1) / TY;
  TORCH_CHECK(K >= 1 && K * SB <= 65535 && (U + TY - 1) / TY <= 65535,
              "robust_clip: grid y range exceeded");
  const int iters = (int)std::min<int64_t>(RB_NORM_ITERS,
                                           (quads + TQ - 1) / TQ);
  const int64_t C = (quads + (int64_t)TQ * iters - 1) / ((int64_t)TQ * iters);
  auto dev = replicas.device();
  auto nsq = torch::empty({U, C}, torch::TensorOptions().dtype(torch::kFloat64)
                                      .device(dev));
  auto scale = torch::empty({U}, torch::TensorOptions().dtype(torch::kFloat32)
                                     .device(dev));
  torch::Tensor slabs;
  auto stream = c10::hip::getCurrentHIPStream();

  RobustClipArgs a;
  a.replicas = replicas.data_ptr<float>();
  a.global = global_params.data_ptr<float>();
  a.mod_off = mod_off.data_ptr<int>();
  a.pr_row = (const long long*)pr_row.data_ptr<int64_t>();
  a.pr_model = pr_model.data_ptr<int>();
  a.pr_w = pr_w.data_ptr<float>();
  a.nsq = nsq.data_ptr<double>();
  a.scale = scale.data_ptr<float>();
  a.counts = counts.data_ptr<int>();
  a.out = nullptr;
  if (partial.has_value()) {
    slabs = torch::empty({slices, K, L},
                         torch::TensorOptions().dtype(torch::kFloat32)
                             .device(dev));
    a.out = slabs.data_ptr<float>();
  }
  a.bound = (float)bound;
  a.P = P;
  a.U = (int)U; a.K = (int)K; a.S = (int)slices; a.C = (int)C;
  a.TQ = TQ; a.tq_shift = tq_shift; a.iters = iters;

  hipLaunchKernelGGL(robust_norm_kernel,
                     dim3((unsigned)C, (unsigned)((U + TY - 1) / TY)),
                     dim3(RB_THREADS), 0, stream, a);
  TORCH_CHECK(hipGetLastError() == hipSuccess, "robust_norm_kernel launch");
  hipLaunchKernelGGL(robust_scale_kernel, dim3((unsigned)U), dim3(RB_WAVE), 0,
                     stream, a);
  TORCH_CHECK(hipGetLastError() == hipSuccess, "robust_scale_kernel launch");
  const unsigned gx = (unsigned)((quads + TQ - 1) / TQ);
  hipLaunchKernelGGL(robust_accum_kernel, dim3(gx, (unsigned)(K * SB)),
                     dim3(RB_THREADS), 0, stream, a);
  TORCH_CHECK(hipGetLastError() == hipSuccess, "robust_accum_kernel launch");
  if (partial.has_value()) {
    const long long n = K * L;
    hipLaunchKernelGGL(robust_reduce_kernel,
                       dim3((unsigned)((n + RB_THREADS - 1) / RB_THREADS)),
                       dim3(RB_THREADS), 0, stream,
                       (const float*)slabs.data_ptr<float>(),
                       partial->data_ptr<float>(), n, (int)slices);
    TORCH_CHECK(hipGetLastError() == hipSuccess,
                "robust_reduce_kernel launch");
  }
}

// apply_aggregate's contract (skip rules, mask, totals_out, zero-drain of
// all of partial) + noise on updated rows + the optimizer step. `step` is
// the 1-based count of this step; s0 / s1 are the [K, P] state tensors the
// kind needs. slabs <= 0 picks the slab count.
static void robust_apply_impl(
    torch::Tensor global_params, torch::Tensor partial,
    c10::optional<torch::Tensor> mask, torch::Tensor totals_out, int64_t kind,
    c10::optional<torch::Tensor> s0, c10::optional<torch::Tensor> s1,
    int64_t step, double lr, double momentum, double noise_std, int64_t key,
    int64_t ctr, int64_t slabs) {
  rb_check(global_params, torch::kFloat32, "global_params");
  rb_check(partial, torch::kFloat32, "partial");
  rb_check(totals_out, torch::kFloat32, "totals_out");
  TORCH_CHECK(global_params.dim() == 2, "global_params must be [K, P]");
  const int64_t K = global_params.size(0), P = global_params.size(1);
  TORCH_CHECK(partial.dim() == 2 && partial.size(0) == K &&
              partial.size(1) == P + 1 && totals_out.numel() == K,
              "robust_apply: partial must be [K, P+1] and totals_out [K]");
  TORCH_CHECK(kind >= RB_AVG && kind <= RB_ADAGRAD, "robust_apply: bad kind");
  TORCH_CHECK(kind == RB_AVG || step >= 1, "robust_apply: step must be >= 1");
  if (mask.has_value()) {
    rb_check(*mask, torch::kUInt8, "mask");
    TORCH_CHECK(mask->numel() == K, "robust_apply: mask must be [K]");
  }
  const bool need0 = kind == RB_ADAM || kind == RB_ADAGRAD ||
                     (kind == RB_SGD && momentum != 0.0);
  TORCH_CHECK(!need0 || s0.has_value(), "robust_apply: state tensor missing");
  TORCH_CHECK(kind != RB_ADAM || s1.has_value(),
              "robust_apply: second state tensor missing");
  for (auto* s : {&s0, &s1})
    if (s->has_value()) {
      rb_check(**s, torch::kFloat32, "optimizer state");
      TORCH_CHECK((*s)->numel() == K * P, "optimizer state must be [K, P]");
    }
  TORCH_CHECK(K >= 1 && K <= 2147483647 / 2, "robust_apply: K out of range");
  const int64_t quads = (P + RB_ELEMS - 1) / RB_ELEMS;
  TORCH_CHECK(quads < (1ll << 32), "robust_apply: P exceeds the Philox counter");
  if (slabs <= 0) {
    // about 2048 blocks in all, each with at least one quad per thread
    const int64_t fit = (quads + RB_THREADS - 1) / RB_THREADS;
    slabs = std::max<int64_t>(1, std::min<int64_t>(fit, (2048 + K - 1) / K));
  }
  slabs = std::max<int64_t>(1, std::min<int64_t>(slabs,
                                                 std::max<int64_t>(quads, 1)));
  TORCH_CHECK(slabs <= 65535, "robust_apply: too many slabs");
  auto stream = c10::hip::getCurrentHIPStream();

  RobustApplyArgs a;
  a.global = global_params.data_ptr<float>();
  a.partial = partial.data_ptr<float>();
  a.mask = mask.has_value() ? mask->data_ptr<unsigned char>() : nullptr;
  a.totals = totals_out.data_ptr<float>();
  a.s0 = need0 ? s0->data_ptr<float>() : nullptr;
  a.s1 = kind == RB_ADAM ? s1->data_ptr<float>() : nullptr;
  a.P = P;
  a.K = (int)K; a.kind = (int)kind; a.first = step <= 1 ? 1 : 0;
  a.QB = (int)((quads + slabs - 1) / slabs);
  a.lr = (float)lr; a.momentum = (float)momentum;
  a.step_size = (float)(lr / (1.0 - pow(0.9, (double)step)));
  a.inv_sqrt_bc2 = (float)(1.0 / sqrt(1.0 - pow(0.999, (double)step)));
  a.noise_std = (float)noise_std;
  a.key0 = (u32)((u64)key & 0xffffffffull);
  a.key1 = (u32)((u64)key >> 32);
  a.ctr0 = (u32)((u64)ctr & 0xffffffffull);
  a.ctr1 = (u32)((u64)ctr >> 32);

  hipLaunchKernelGGL(robust_totals_kernel,
                     dim3((unsigned)((K + RB_THREADS - 1) / RB_THREADS)),
                     dim3(RB_THREADS), 0, stream,
                     (const float*)partial.data_ptr<float>(),
                     totals_out.data_ptr<float>(), (int)K, (long long)P);
  TORCH_CHECK(hipGetLastError() == hipSuccess, "robust_totals_kernel launch");
  hipLaunchKernelGGL(robust_apply_kernel, dim3((unsigned)K, (unsigned)slabs),
                     dim3(RB_THREADS), 0, stream, a);
  TORCH_CHECK(hipGetLastError() == hipSuccess, "robust_apply_kernel launch");
}

void register_robust(pybind11::module_& mod) {
  mod.def("robust_clip", &robust_clip_impl,
          "norm clipping of replica rows + weighted sums per model");
  mod.def("robust_apply", &robust_apply_impl,
          "average + noise + server-optimizer step, draining partial");
  mod.def("robust_span", []() { return (int64_t)RB_SPAN; },
          "elements one block of the accumulate kernel covers");
}
