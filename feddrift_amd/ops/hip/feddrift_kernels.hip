// feddrift MI355X (gfx950 / CDNA4) kernels
//
// Fused batched local training + evaluation sweeps for the MLP model family
// (FeedForwardNN / LogisticRegression of the drift path).
//
// Design (not a port: the reference, microsoft/FedDrift, runs these loops as
// per-model Python/torch eager code with CPU<->GPU model movement every
// round — fedml_api/distributed/fedavg_ens/FedAvgEnsTrainer.py:47-95):
//
//  * mlp_train_kernel: ONE launch trains every (client, model) pair of the
//    round. One workgroup per pair; the pair's weights and the gradient
//    accumulator live in LDS for the entire E-step optimizer loop; each
//    step stages its minibatch chunk through LDS, computes forward +
//    backward with per-thread sample parallelism, reduces gradients with a
//    per-thread ownership partition (no atomics: shared entries add
//    their partial sums in a fixed order), and applies the
//    SGD/Adam(amsgrad, wd) update in-place. Adam state stays in HBM.
//  * mlp_train_small_kernel: the same launch for the five compile-time
//    shapes of the drift path (the flagship). Samples, activations and the
//    gradient accumulators live in registers; a wave reduce-scatter leaves
//    each parameter entry's gradient total in one owner lane, which keeps
//    the entry's weight and Adam state in registers for the whole E-step
//    loop and steps it there. LDS holds only the weights the sample
//    pipeline reads; nothing is accumulated through LDS atomics.
//  * mlp_eval_kernel: ONE launch per accuracy/loss sweep (the K-models x
//    C-clients matrices, prequential testing). One workgroup per data
//    window; per-thread sample loop + LDS tree reduction; one global
//    float64 atomicAdd per output slot.
//
// fp32 everywhere (the reference trains fp32; dtype parity is required for
// the accuracy metric). Wavefront = 64; block = 256 threads.
//
// Why no MFMA here (a decision, not an omission): the drift-path models
// are 3->6->2 / 2->4->2 MLPs — per pair the "GEMMs" are [batch,3]x[3,6]
// and the K=batch gradient reductions produce [6,3] tiles. An
// mfma_f32_16x16x4_f32 tile would be >90% padding on M=6/N=3 fragments
// and the f32 MFMA rate equals the f32 VALU rate on gfx950, so matrix
// cores buy nothing at these shapes; PMC shows the kernel is
// LATENCY-bound (SQ_WAIT dominated), not FLOP-bound (profiles/README.md).
// Where genuinely MFMA-shaped work exists — CNN/ResNet convolutions and
// FEMNIST-scale tower GEMMs — the engine uses MIOpen / rocBLAS batched
// GEMMs, which are the MFMA paths for library-shaped matmuls.

#include <hip/hip_runtime.h>
#include <torch/extension.h>
#include <c10/hip/HIPStream.h>

#include <cmath>
#include <vector>

#define THREADS 256
#define LDS_BUDGET_FLOATS (150 * 1024 / 4)

#define KIND_FNN 0
#define KIND_LR 1

#define OPT_SGD 0
#define OPT_ADAM 1

// ---------------------------------------------------------------------------
// training kernel
// ---------------------------------------------------------------------------

struct TrainArgs {
  float* __restrict__ params;        // [R, P] replicas (out)
  const float* __restrict__ in_params;  // [K, P] global models (in), or null
  const int* __restrict__ model_of;  // [G] model per pair (with in_params)
  const float* __restrict__ sample_w;   // [G] aggregation weight, or null
  float* __restrict__ partial;       // [K, P+1] weighted sums, or null
  const int64_t* __restrict__ rows;  // [G]
  const float* __restrict__ x;       // [N, D]
  const int64_t* __restrict__ y;     // [N]
  const int64_t* __restrict__ step_off;  // [G, E]
  const int64_t* __restrict__ step_len;  // [G, E]
  const float* __restrict__ x_mask;  // [G, D] or nullptr
  float* __restrict__ m;             // [R, P] (adam) or nullptr
  float* __restrict__ v;
  float* __restrict__ vmax;
  int* __restrict__ t;               // [R]
  const float* __restrict__ lr;      // [R]
  float wd;
  float mu;                          // FedProx coefficient, 0 = off
  int E, D, H, O, P, kind, opt, BC;
};

// FedProx anchor w0 of pair g: the row the weights were staged from
// (stage_weights). Nothing writes either source before write_back, so the
// anchor is re-read from global memory at each step and costs no LDS.
__device__ __forceinline__ const float* prox_anchor(const TrainArgs& a, int g,
                                                    int64_t row) {
  return a.in_params ? a.in_params + (int64_t)a.model_of[g] * a.P
                     : a.params + row * a.P;
}

__device__ __forceinline__ float block_reduce_sum(float val, float* scratch) {
  // wave shuffle reduce then cross-wave via LDS (4 waves / 256 threads)
  for (int off = 32; off > 0; off >>= 1)
    val += __shfl_down(val, off, 64);
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  if (lane == 0) scratch[wave] = val;
  __syncthreads();
  if (wave == 0) {
    val = (lane < (blockDim.x >> 6)) ? scratch[lane] : 0.f;
    for (int off = 2; off > 0; off >>= 1)
      val += __shfl_down(val, off, 64);
  }
  __syncthreads();
  return val;  // valid in thread 0
}

__device__ __forceinline__ void stage_weights(const TrainArgs& a, int g,
                                              int64_t row, float* w) {
  // strided by blockDim.x: the templated small kernel also launches with
  // 64-thread (single-wave) blocks
  if (a.in_params) {
    const int64_t src = (int64_t)a.model_of[g] * a.P;
    for (int p = threadIdx.x; p < a.P; p += blockDim.x)
      w[p] = a.in_params[src + p];
  } else {
    for (int p = threadIdx.x; p < a.P; p += blockDim.x)
      w[p] = a.params[row * a.P + p];
  }
  __syncthreads();
}

__device__ __forceinline__ void opt_update(const TrainArgs& a, int g,
                                           int64_t row, float* w,
                                           float* grad) {
  const int tid = threadIdx.x;
  if (a.mu != 0.f) {
    // proximal pull, folded into the gradient by the thread that consumes
    // entry p below (same p -> tid mapping: no barrier in between)
    const float* w0 = prox_anchor(a, g, row);
    for (int p = tid; p < a.P; p += THREADS)
      grad[p] += a.mu * (w[p] - w0[p]);
  }
  if (a.opt == OPT_SGD) {
    const float lr_ = a.lr[row];
    for (int p = tid; p < a.P; p += THREADS) w[p] -= lr_ * grad[p];
    return;
  }
  if (tid == 0) a.t[row] += 1;
  __syncthreads();
  const int tnew = a.t[row];
  const float b1 = 0.9f, b2 = 0.999f, eps = 1e-8f;
  // 1 - beta as torch rounds it (from double): 1.f - 0.999f is 1.3e-5 short
  const float omb1 = 0.1f, omb2 = 0.001f;
  const float bc1 = 1.f - powf(b1, (float)tnew);
  const float bc2 = 1.f - powf(b2, (float)tnew);
  const float lr_ = a.lr[row];
  for (int p = tid; p < a.P; p += THREADS) {
    const int64_t gp = row * a.P + p;
    const float gr = grad[p] + a.wd * w[p];
    const float mn = b1 * a.m[gp] + omb1 * gr;
    const float vn = b2 * a.v[gp] + omb2 * gr * gr;
    a.m[gp] = mn;
    a.v[gp] = vn;
    const float vm = fmaxf(a.vmax[gp], vn);
    a.vmax[gp] = vm;
    const float denom = sqrtf(vm / bc2) + eps;
    w[p] -= lr_ * (mn / bc1) / denom;
  }
}

__device__ __forceinline__ void write_back(const TrainArgs& a, int g,
                                           int64_t row, const float* w) {
  const int tid = threadIdx.x;
  for (int p = tid; p < a.P; p += blockDim.x) a.params[row * a.P + p] = w[p];
  if (a.partial && a.sample_w) {
    const float sw = a.sample_w[g];
    if (sw > 0.f) {
      const int64_t pbase = (int64_t)a.model_of[g] * (a.P + 1);
      for (int p = tid; p < a.P; p += blockDim.x)
        atomicAdd(&a.partial[pbase + p], sw * w[p]);
      if (tid == 0) atomicAdd(&a.partial[pbase + a.P], sw);
    }
  }
}

extern "C" __global__ __launch_bounds__(THREADS)
void mlp_train_kernel(TrainArgs a) {
  const int g = blockIdx.x;
  const int64_t row = a.rows[g];
  const int tid = threadIdx.x;

  extern __shared__ __attribute__((aligned(16))) float lds[];
  // per-entry partial gradient sums of phase E (2 KB beside the 150 KB
  // dynamic budget; the 160 KB of a CU hold both)
  __shared__ float gpart[2 * THREADS];
  float* w = lds;              // [P]
  float* grad = w + a.P;       // [P]
  float* xb = grad + a.P;      // [BC, D]
  float* act = xb + a.BC * a.D;      // [BC, H] (fnn activations)
  float* dza = act + (a.kind == KIND_FNN ? a.BC * a.H : 0);  // [BC, H] dz1
  float* dzo = dza + (a.kind == KIND_FNN ? a.BC * a.H : 0);  // [BC, O]

  // stage weights: straight from the GLOBAL model row (replaces the
  // reference's server->client model broadcast and the engine's
  // replica-sync copy — the round starts here)
  stage_weights(a, g, row, w);

  const int HD = a.H * a.D;
  const int OH = a.O * a.H;
  const int OD = a.O * a.D;

  for (int e = 0; e < a.E; ++e) {
    const int64_t off = a.step_off[(int64_t)g * a.E + e];
    const int n = (int)a.step_len[(int64_t)g * a.E + e];
    if (n == 0) continue;  // reference skips the step entirely
    const float inv_n = 1.0f / (float)n;

    // zero gradient accumulator
    for (int p = tid; p < a.P; p += THREADS) grad[p] = 0.f;
    __syncthreads();

    for (int c0 = 0; c0 < n; c0 += a.BC) {
      const int bc = (a.BC < n - c0) ? a.BC : (n - c0);

      // phase A: stage input chunk (optionally feature-masked: KUE)
      for (int q = tid; q < bc * a.D; q += THREADS) {
        const int i = q / a.D;
        const int d = q - i * a.D;
        float xv = a.x[(off + c0 + i) * a.D + d];
        if (a.x_mask) xv *= a.x_mask[(int64_t)g * a.D + d];
        xb[q] = xv;
      }
      __syncthreads();

      if (a.kind == KIND_FNN) {
        // phase B: z1/act, one work item per (sample, hidden unit) —
        // keeps all 256 threads busy and the dependent chains short
        // (the original sample-serial h-loop left the workgroup
        // latency-bound at ~10 active threads for SEA-sized models)
        for (int q = tid; q < bc * a.H; q += THREADS) {
          const int i = q / a.H;
          const int h = q - i * a.H;
          float z = w[HD + h];
          for (int d = 0; d < a.D; ++d)
            z += w[h * a.D + d] * xb[i * a.D + d];
          act[q] = z > 0.f ? z : 0.f;
        }
        __syncthreads();

        // phase C: z2 + softmax + dz2 per sample (O is small)
        for (int i = tid; i < bc; i += THREADS) {
          const int yi = (int)a.y[off + c0 + i];
          float z2[64];
          float zmax = -1e30f;
          for (int o = 0; o < a.O; ++o) {
            float z = w[HD + a.H + OH + o];
            for (int h = 0; h < a.H; ++h)
              z += w[HD + a.H + o * a.H + h] * act[i * a.H + h];
            z2[o] = z;
            zmax = fmaxf(zmax, z);
          }
          float zsum = 0.f;
          for (int o = 0; o < a.O; ++o) {
            z2[o] = __expf(z2[o] - zmax);
            zsum += z2[o];
          }
          for (int o = 0; o < a.O; ++o) {
            float sm = z2[o] / zsum;
            if (o == yi) sm -= 1.f;
            dzo[i * a.O + o] = sm * inv_n;
          }
        }
        __syncthreads();

        // phase D: dz1 per (sample, hidden unit)
        for (int q = tid; q < bc * a.H; q += THREADS) {
          const int i = q / a.H;
          const int h = q - i * a.H;
          float s = 0.f;
          for (int o = 0; o < a.O; ++o)
            s += dzo[i * a.O + o] * w[HD + a.H + o * a.H + h];
          dza[q] = act[q] > 0.f ? s : 0.f;
        }
        __syncthreads();
      } else {  // LR: out = sigmoid(Wx+b); CE applied to the sigmoid
        for (int i = tid; i < bc; i += THREADS) {
          const int yi = (int)a.y[off + c0 + i];
          float p_[64];  // O <= 64 for the LR path
          float pmax = -1e30f;
          for (int o = 0; o < a.O; ++o) {
            float z = w[OD + o];
            for (int d = 0; d < a.D; ++d)
              z += w[o * a.D + d] * xb[i * a.D + d];
            const float pv = 1.f / (1.f + __expf(-z));
            p_[o] = pv;
            pmax = fmaxf(pmax, pv);
          }
          float psum = 0.f;
          for (int o = 0; o < a.O; ++o) psum += __expf(p_[o] - pmax);
          for (int o = 0; o < a.O; ++o) {
            float sm = __expf(p_[o] - pmax) / psum;
            if (o == yi) sm -= 1.f;
            // dz = dp * sigmoid' = dp * p (1-p)
            dzo[i * a.O + o] = sm * inv_n * p_[o] * (1.f - p_[o]);
          }
        }
        __syncthreads();
      }

      // phase E: gradient accumulation. NSUB threads share each parameter
      // entry, each summing a sample stride; the NSUB partial sums then
      // meet in sub order (below) — P*NSUB work items keep the block busy
      // for small P
      {
        int nsub = (2 * THREADS) / (a.P > 0 ? a.P : 1);
        nsub = nsub < 1 ? 1 : (nsub > 32 ? 32 : nsub);
        for (int q = tid; q < a.P * nsub; q += THREADS) {
          const int p = q % a.P;
          const int sub = q / a.P;
          float acc = 0.f;
          if (a.kind == KIND_FNN) {
            if (p < HD) {
              const int h = p / a.D, d = p - (p / a.D) * a.D;
              for (int i = sub; i < bc; i += nsub)
                acc += dza[i * a.H + h] * xb[i * a.D + d];
            } else if (p < HD + a.H) {
              const int h = p - HD;
              for (int i = sub; i < bc; i += nsub) acc += dza[i * a.H + h];
            } else if (p < HD + a.H + OH) {
              const int qq = p - HD - a.H;
              const int o = qq / a.H, h = qq - (qq / a.H) * a.H;
              for (int i = sub; i < bc; i += nsub)
                acc += dzo[i * a.O + o] * act[i * a.H + h];
            } else {
              const int o = p - HD - a.H - OH;
              for (int i = sub; i < bc; i += nsub) acc += dzo[i * a.O + o];
            }
          } else {
            if (p < OD) {
              const int o = p / a.D, d = p - (p / a.D) * a.D;
              for (int i = sub; i < bc; i += nsub)
                acc += dzo[i * a.O + o] * xb[i * a.D + d];
            } else {
              const int o = p - OD;
              for (int i = sub; i < bc; i += nsub) acc += dzo[i * a.O + o];
            }
          }
          // nsub == 1: this thread owns entry p. Otherwise the partial
          // sums wait in gpart (q = sub * P + p < P * nsub <= 2 * THREADS)
          // and are added in sub order below: LDS atomics would land in
          // whatever order the waves arrive, and a launch would not
          // repeat bit for bit
          if (nsub == 1) grad[p] += acc;
          else gpart[q] = acc;
        }
        if (nsub > 1) {
          __syncthreads();
          for (int p = tid; p < a.P; p += THREADS) {
            float gsum = grad[p];
            for (int s = 0; s < nsub; ++s) gsum += gpart[s * a.P + p];
            grad[p] = gsum;
          }
        }
      }
      __syncthreads();
    }

    // optimizer update (matches torch.optim exactly; see ops/mlp_torch.py)
    opt_update(a, g, row, w, grad);
    __syncthreads();
  }

  write_back(a, g, row, w);
}

// ---------------------------------------------------------------------------
// specialized small-MLP training kernel: the whole per-sample pipeline and
// the per-thread gradient accumulators live in REGISTERS (compile-time
// D/H/O, fully unrolled). The gradients meet in a wave reduce-SCATTER:
// entry p's total ends in lane bitrev6(p) and nowhere else, and that owner
// lane keeps w[p] and the entry's Adam state in registers from the first
// load to the last store and steps the entry itself. LDS holds only the
// weights the sample pipeline reads (and, for 256-thread blocks, the
// waves' sums, which wave 0's owner lanes add in wave order). This is the
// SEA/SINE/CIRCLE flagship path: about ten one-wave blocks per launch, so
// the length of one wave's dependent chain per step is all that counts.
// ---------------------------------------------------------------------------

// one sample's forward + backward, added into this lane's accumulators.
// Which products fuse into an FMA is written out here, not left to the
// compiler's contraction (it moves with the surrounding code, and the
// round's results with it): the roundings are the ones this pipeline has
// always had. Hidden layer, dz1 and the weight gradients are FMA chains;
// the output dot products add rounded products (after a fused first term
// where the input width is odd); the output-bias gradient fuses the last
// product of dz with its own sum.
template <int TD, int TH, int TO, int KIND, int TP>
__device__ __forceinline__ void small_sample_grad(const float (&x)[TD],
                                                  const int yi,
                                                  const float* w,
                                                  const float inv_n,
                                                  float (&gacc)[TP]) {
#pragma clang fp contract(off)
  constexpr int HD = TH * TD;
  constexpr int OH = TO * TH;
  if constexpr (KIND == KIND_FNN) {
    float act[TH], dzo[TO];
#pragma unroll
    for (int h = 0; h < TH; ++h) {
      float z = w[HD + h];
#pragma unroll
      for (int d = 0; d < TD; ++d) z = __builtin_fmaf(w[h * TD + d], x[d], z);
      act[h] = z > 0.f ? z : 0.f;
    }
    float zmax = -1e30f;
#pragma unroll
    for (int o = 0; o < TO; ++o) {
      float z = w[HD + TH + OH + o];
#pragma unroll
      for (int h = 0; h < TH; ++h) z += w[HD + TH + o * TH + h] * act[h];
      dzo[o] = z;
      zmax = fmaxf(zmax, z);
    }
    float zsum = 0.f;
#pragma unroll
    for (int o = 0; o < TO; ++o) {
      dzo[o] = __expf(dzo[o] - zmax);
      zsum += dzo[o];
    }
#pragma unroll
    for (int o = 0; o < TO; ++o) {
      float sm = dzo[o] / zsum;
      if (o == yi) sm -= 1.f;
      dzo[o] = sm * inv_n;
      gacc[HD + TH + OH + o] =
          __builtin_fmaf(sm, inv_n, gacc[HD + TH + OH + o]);
    }
    float dza[TH];
#pragma unroll
    for (int h = 0; h < TH; ++h) {
      float s = 0.f;
#pragma unroll
      for (int o = 0; o < TO; ++o)
        s = __builtin_fmaf(dzo[o], w[HD + TH + o * TH + h], s);
      dza[h] = act[h] > 0.f ? s : 0.f;
    }
#pragma unroll
    for (int h = 0; h < TH; ++h) {
#pragma unroll
      for (int d = 0; d < TD; ++d)
        gacc[h * TD + d] = __builtin_fmaf(dza[h], x[d], gacc[h * TD + d]);
      gacc[HD + h] += dza[h];
    }
#pragma unroll
    for (int o = 0; o < TO; ++o) {
#pragma unroll
      for (int h = 0; h < TH; ++h)
        gacc[HD + TH + o * TH + h] =
            __builtin_fmaf(dzo[o], act[h], gacc[HD + TH + o * TH + h]);
    }
  } else {  // LR
    float p_[TO], dzo[TO];
    float pmax = -1e30f;
#pragma unroll
    for (int o = 0; o < TO; ++o) {
      float z = w[TO * TD + o];
#pragma unroll
      for (int d = 0; d < TD; ++d) {
        if (d < (TD & 1)) z = __builtin_fmaf(w[o * TD + d], x[d], z);
        else z += w[o * TD + d] * x[d];
      }
      p_[o] = 1.f / (1.f + __expf(-z));
      pmax = fmaxf(pmax, p_[o]);
    }
    float psum = 0.f;
#pragma unroll
    for (int o = 0; o < TO; ++o) psum += __expf(p_[o] - pmax);
#pragma unroll
    for (int o = 0; o < TO; ++o) {
      float sm = __expf(p_[o] - pmax) / psum;
      if (o == yi) sm -= 1.f;
      // dz = dp * sigmoid' = dp * p (1-p)
      const float dp = sm * inv_n * p_[o];
      dzo[o] = dp * (1.f - p_[o]);
      gacc[TO * TD + o] =
          __builtin_fmaf(dp, 1.f - p_[o], gacc[TO * TD + o]);
    }
#pragma unroll
    for (int o = 0; o < TO; ++o) {
#pragma unroll
      for (int d = 0; d < TD; ++d)
        gacc[o * TD + d] = __builtin_fmaf(dzo[o], x[d], gacc[o * TD + d]);
    }
  }
}

// Lane that ends up holding entry p of the wave reduce-scatter below.
__device__ __forceinline__ int bitrev6(int p) {
  return (int)(__brev((unsigned)p) >> 26);
}

// One exchange of the reduce-scatter at lane distance S. Lanes with bit S
// clear keep entry `a`, lanes with bit S set keep entry `b`; each lane adds
// its partner's (lane ^ S) partial of the entry it keeps to its own.
template <int S>
__device__ __forceinline__ float scatter_exchange_add(const float a,
                                                      const float b,
                                                      const int lane) {
  if constexpr (S == 32) {
    // half-wave swap: lanes 32..63 of the first operand trade places with
    // lanes 0..31 of the second, so both operands then hold (own partial,
    // partner's partial) of the kept entry: one swap, one add, no select,
    // nothing on the LDS pipe
    const auto r = __builtin_amdgcn_permlane32_swap(
        __float_as_uint(a), __float_as_uint(b), false, false);
    return __uint_as_float(r[0]) + __uint_as_float(r[1]);
  } else if constexpr (S == 16) {
    // the same between the odd 16-lane rows of the first operand and the
    // even rows of the second
    const auto r = __builtin_amdgcn_permlane16_swap(
        __float_as_uint(a), __float_as_uint(b), false, false);
    return __uint_as_float(r[0]) + __uint_as_float(r[1]);
  } else {
    const bool hi = (lane & S) != 0;
    const float keep = hi ? b : a;
    const float send = hi ? a : b;
    return keep + __shfl_xor(send, S, 64);
  }
}

// Wave reduce-scatter of N per-lane partials, levels S = 32, 16, ..., 1.
// Level S pairs the entries still held two by two (split on the lowest
// entry bit not yet used) and halves their number; an odd one out pairs
// with a zero nobody reads. Entry p's total ends in lane bitrev6(p): that
// lane's return value. For TP = 38 the levels move 19+10+5+3+2+1 = 40
// registers, where an all-reduce tree moves 6 x 38.
//
// The sum of an entry has the order of the shuffle-down tree
// (v[i] + v[i + S] for i < S at level S) bit for bit: every lane that
// keeps the entry adds the same two values, commuted in half of them.
// All register indices are compile-time, so nothing spills.
template <int N, int S>
struct ScatterReduce {
  static __device__ __forceinline__ float run(const float (&r)[N],
                                              const int lane) {
    constexpr int M = (N + 1) / 2;
    float o[M];
#pragma unroll
    for (int k = 0; k < M; ++k)
      o[k] = scatter_exchange_add<S>(r[2 * k],
                                     2 * k + 1 < N ? r[2 * k + 1] : 0.f,
                                     lane);
    if constexpr (S == 1) {
      static_assert(M == 1, "reduce-scatter holds at most 64 entries");
      return o[0];
    } else {
      return ScatterReduce<M, S / 2>::run(o, lane);
    }
  }
};

// Step windows of a small fleet travel in the launch packet: G*E (off, len)
// pairs as int32, 2 KB of the 4 KB kernel-argument segment. A block's index
// g*E + e is uniform, so the reads are scalar loads from that segment and
// the launch needs no upload before it. Larger fleets pass the device arrays
// (a.step_off != nullptr) and the struct is not read.
#define INLINE_STEPS 256
struct StepWin {
  int2 w[INLINE_STEPS];              // (off, len) of step g*E + e
};

template <int TD, int TH, int TO, int KIND, int BS>
__global__ __launch_bounds__(BS)
void mlp_train_small_kernel(TrainArgs a, StepWin win) {
  constexpr int TP = (KIND == KIND_FNN)
                         ? (TH * TD + TH + TO * TH + TO)
                         : (TO * TD + TO);
  static_assert(TP <= 64, "one owner lane per parameter entry");
  constexpr int NW = BS / 64;
  // a step of up to PF trips of the sample loop loads all its samples up
  // front (one wave per SIMD may hold 512 VGPRs; see ops/hip/README.md)
  constexpr int PF = 8;
  const int g = blockIdx.x;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int p_own = bitrev6(lane);
  // the lane that holds entry p_own's total after the reduce and steps it
  const bool owner = tid < 64 && p_own < TP;
  const bool adam = (a.opt == OPT_ADAM);

  __shared__ __attribute__((aligned(16))) float w[TP];
  __shared__ float wsum[NW > 1 ? NW : 1][NW > 1 ? TP : 1];

  // every load that depends on nothing, or only on rows[g], issues here
  const int64_t row = a.rows[g];
  const int64_t e0 = (int64_t)g * a.E;
  const bool inl = a.step_off == nullptr;  // windows in the launch packet
  int64_t off_nx = 0;
  int n_nx = 0;
  if (a.E > 0) {
    if (inl) {
      const int2 sw0 = win.w[e0];
      off_nx = sw0.x;
      n_nx = sw0.y;
    } else {
      off_nx = a.step_off[e0];
      n_nx = (int)a.step_len[e0];
    }
  }
  float mk[TD];
#pragma unroll
  for (int d = 0; d < TD; ++d)
    mk[d] = a.x_mask ? a.x_mask[(int64_t)g * TD + d] : 1.f;
  const bool fuse_partial = a.partial && a.sample_w;
  const float sw = fuse_partial ? a.sample_w[g] : 0.f;
  const int64_t pbase =
      fuse_partial ? (int64_t)a.model_of[g] * (TP + 1) : 0;
  const float lr_ = a.lr[row];
  float wreg = 0.f, mreg = 0.f, vreg = 0.f, vmreg = 0.f;
  if (owner) {
    // straight from the GLOBAL model row when the broadcast is fused
    wreg = a.in_params
               ? a.in_params[(int64_t)a.model_of[g] * TP + p_own]
               : a.params[row * TP + p_own];
    if (adam) {
      mreg = a.m[row * TP + p_own];
      vreg = a.v[row * TP + p_own];
      vmreg = a.vmax[row * TP + p_own];
    }
  }
  // every lane keeps its own step count and beta^t (incrementally)
  int tstep = adam ? a.t[row] : 0;
  float b1pow = 1.f, b2pow = 1.f;
  if (adam) {
    b1pow = powf(0.9f, (float)tstep);
    b2pow = powf(0.999f, (float)tstep);
  }
  // FedProx anchor: the value the entry was staged with
  const float w0 = wreg;
  if (owner) w[p_own] = wreg;
  __syncthreads();

  for (int e = 0; e < a.E; ++e) {
    const int64_t off = off_nx;
    const int n = n_nx;
    if (e + 1 < a.E) {  // next step's window, ahead of this step's work
      if (inl) {
        const int2 swn = win.w[e0 + e + 1];
        off_nx = swn.x;
        n_nx = swn.y;
      } else {
        off_nx = a.step_off[e0 + e + 1];
        n_nx = (int)a.step_len[e0 + e + 1];
      }
    }
    if (n == 0) continue;
    const float inv_n = 1.0f / (float)n;

    float gacc[TP];
#pragma unroll
    for (int p = 0; p < TP; ++p) gacc[p] = 0.f;

    if (n <= PF * BS) {
      // all of the step's samples in flight at once, then the same
      // per-lane order of accumulation (i = tid, tid + BS, ...)
      float xr[PF][TD];
      int yr[PF];
#pragma unroll
      for (int k = 0; k < PF; ++k) {
        const int i = tid + k * BS;
        const bool on = i < n;
#pragma unroll
        for (int d = 0; d < TD; ++d)
          xr[k][d] = on ? a.x[(off + i) * TD + d] : 0.f;
        yr[k] = on ? (int)a.y[off + i] : 0;
      }
#pragma unroll
      for (int k = 0; k < PF; ++k) {
        if (tid + k * BS < n) {
          if (a.x_mask) {
#pragma unroll
            for (int d = 0; d < TD; ++d) xr[k][d] *= mk[d];
          }
          small_sample_grad<TD, TH, TO, KIND, TP>(xr[k], yr[k], w, inv_n,
                                                  gacc);
        }
      }
    } else {
      for (int i = tid; i < n; i += BS) {
        float x[TD];
#pragma unroll
        for (int d = 0; d < TD; ++d) {
          x[d] = a.x[(off + i) * TD + d];
          if (a.x_mask) x[d] *= mk[d];
        }
        const int yi = (int)a.y[off + i];
        small_sample_grad<TD, TH, TO, KIND, TP>(x, yi, w, inv_n, gacc);
      }
    }

    float tot = ScatterReduce<TP, 32>::run(gacc, lane);
    if constexpr (NW == 1) {
      // the total used to land in a zeroed LDS slot by an atomic add;
      // 0 + total keeps that result where the total is -0
      tot = 0.f + tot;
    } else {
      // several waves: their sums meet in wave order, so a launch repeats
      // bit for bit
      if (p_own < TP) wsum[tid >> 6][p_own] = tot;
      __syncthreads();
      if (owner) {
        tot = wsum[0][p_own];
#pragma unroll
        for (int wv = 1; wv < NW; ++wv) tot += wsum[wv][p_own];
      }
    }

    // optimizer step in the owner lane's registers (numerics match
    // ops/mlp_torch.py)
    if (adam) {
      tstep += 1;
      b1pow *= 0.9f;
      b2pow *= 0.999f;
    }
    if (owner) {
      // Which products fuse into an FMA is written out, not left to the
      // compiler's contraction: the roundings below are the ones this
      // step has always had (m adds two rounded products), so results do
      // not move when the code around them does.
#pragma clang fp contract(off)
      float gr = tot;
      if (a.mu != 0.f) gr = __builtin_fmaf(a.mu, wreg - w0, gr);  // FedProx
      if (!adam) {
        wreg = __builtin_fmaf(-lr_, gr, wreg);
      } else {
        const float b1 = 0.9f, b2 = 0.999f, eps = 1e-8f;
        const float bc1 = 1.f - b1pow;
        const float bc2 = 1.f - b2pow;
        gr = __builtin_fmaf(a.wd, wreg, gr);
        const float mn = b1 * mreg + (1.f - b1) * gr;
        const float vn = __builtin_fmaf((1.f - b2) * gr, gr, b2 * vreg);
        mreg = mn;
        vreg = vn;
        const float vm = fmaxf(vmreg, vn);
        vmreg = vm;
        const float denom = sqrtf(vm / bc2) + eps;
        wreg -= lr_ * (mn / bc1) / denom;
      }
      w[p_own] = wreg;
    }
    // the next step's samples read the new weights (and, with several
    // waves, wsum is free again)
    __syncthreads();
  }

  if (owner) {
    if (adam) {
      a.m[row * TP + p_own] = mreg;
      a.v[row * TP + p_own] = vreg;
      a.vmax[row * TP + p_own] = vmreg;
      if (tid == 0) a.t[row] = tstep;
    }
    a.params[row * TP + p_own] = wreg;
    if (fuse_partial && sw > 0.f) {
      atomicAdd(&a.partial[pbase + p_own], sw * wreg);
      if (tid == 0) atomicAdd(&a.partial[pbase + TP], sw);
    }
  }
}

// test-only: the train kernel's reduce-scatter on one wave. vals is
// [64, TP] (lane-major); out[p] is entry p's total as its owner lane holds it
template <int TP>
__global__ __launch_bounds__(64)
void train_reduce_probe_kernel(const float* __restrict__ vals,
                               float* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  float r[TP];
#pragma unroll
  for (int p = 0; p < TP; ++p) r[p] = vals[lane * TP + p];
  const float tot = ScatterReduce<TP, 32>::run(r, lane);
  const int p_own = bitrev6(lane);
  if (p_own < TP) out[p_own] = tot;
}

#define SMALL_SHAPE_LIST(X)      \
  X(3, 6, 2, KIND_FNN)           \
  X(2, 4, 2, KIND_FNN)           \
  X(4, 8, 2, KIND_FNN)           \
  X(3, 0, 2, KIND_LR)            \
  X(2, 0, 2, KIND_LR)

static bool small_shape(int D, int H, int O, int kind) {
#define IS_SHAPE(SD, SH, SO, SK) \
  if (kind == SK && D == SD && H == SH && O == SO) return true;
  SMALL_SHAPE_LIST(IS_SHAPE)
#undef IS_SHAPE
  return false;
}

// Whether a launch of G pairs x E steps on this shape may carry its step
// windows in the launch packet (the values must also fit int32: pack_steps)
bool inline_steps_ok(int64_t D, int64_t H, int64_t O, int64_t kind,
                     int64_t G, int64_t E) {
  return G >= 0 && E >= 0 && G * E <= INLINE_STEPS &&
         small_shape((int)D, (int)H, (int)O, (int)kind);
}

// [G, E] CPU int64 windows -> win; false where an off or off + len leaves
// int32 (the caller then uploads the arrays instead)
static bool pack_steps(const torch::Tensor& step_off,
                       const torch::Tensor& step_len, StepWin* win) {
  const int64_t n = step_off.numel();
  if (n > INLINE_STEPS) return false;
  const int64_t* po = step_off.data_ptr<int64_t>();
  const int64_t* pl = step_len.data_ptr<int64_t>();
  const int64_t lim = 2147483647LL;
  for (int64_t i = 0; i < n; ++i) {
    if (po[i] < 0 || pl[i] < 0 || po[i] > lim || pl[i] > lim ||
        po[i] + pl[i] > lim)
      return false;
    win->w[i] = make_int2((int)po[i], (int)pl[i]);
  }
  return true;
}

// test hook of pack_steps' range rule
bool steps_fit_inline(torch::Tensor step_off, torch::Tensor step_len) {
  TORCH_CHECK(!step_off.is_cuda() && !step_len.is_cuda() &&
              step_off.dtype() == torch::kInt64 &&
              step_len.dtype() == torch::kInt64 &&
              step_off.sizes() == step_len.sizes(),
              "steps_fit_inline: CPU int64 tensors of one shape");
  StepWin win;
  return pack_steps(step_off.contiguous(), step_len.contiguous(), &win);
}

static bool launch_small(const TrainArgs& args, const StepWin& win, int G,
                         hipStream_t stream) {
  // Block-size choice: every wave of a block redundantly executes the
  // TP x 6-level shuffle reduction, so single-wave (64-thread) blocks cut
  // the total reduction work 4x. Measured same-box across grid sizes
  // (profiles/README.md): +41% at G=3400, +52% at G=10000, and never
  // slower even at G=100 (the per-pair critical path is the same serial
  // E-step chain either way). Default BS=64 everywhere; the env knob
  // remains as the benchmarking escape hatch (set huge to force 256).
  static const int bs64_min = [] {
    const char* e = getenv("FEDDRIFT_TRAIN_BS64_MIN_G");
    return e ? atoi(e) : 0;
  }();
  const bool bs64 = G >= bs64_min;
#define TRY_SHAPE(SD, SH, SO, SK)                                          \
  if (args.kind == SK && args.D == SD && args.H == SH && args.O == SO) {   \
    if (bs64) {                                                            \
      hipLaunchKernelGGL((mlp_train_small_kernel<SD, SH, SO, SK, 64>),     \
                         dim3(G), dim3(64), 0, stream, args, win);         \
    } else {                                                               \
      hipLaunchKernelGGL((mlp_train_small_kernel<SD, SH, SO, SK, THREADS>),\
                         dim3(G), dim3(THREADS), 0, stream, args, win);    \
    }                                                                      \
    return true;                                                           \
  }
  SMALL_SHAPE_LIST(TRY_SHAPE)
#undef TRY_SHAPE
  return false;
}

// apply the aggregated average: models with positive total weight get
// partial/total, others keep their parameters (skip rules:
// FedAvgEnsAggregatorSoftCluster.py:151-169). The kernel also drains
// the partial buffer to zero for the next round's fused accumulation
// (saves a separate fill launch per round) and parks the per-model
// totals in `totals` for the host-side weight checks.
extern "C" __global__ __launch_bounds__(THREADS)
void apply_aggregate_kernel(float* __restrict__ global_params,
                            float* __restrict__ partial,
                            const unsigned char* __restrict__ mask,
                            float* __restrict__ totals,
                            int K, int P) {
  // ONE block per model: every thread reads the weight total before
  // anything zeroes it (a multi-block grid would race the drain of the
  // [m, P] slot against sibling blocks' read of it)
  const int m = blockIdx.x;
  const float tot = partial[(int64_t)m * (P + 1) + P];
  const bool upd = tot > 0.f && !(mask && !mask[m]);
  // every wave must have loaded `tot` before thread 0 drains the slot;
  // a wave arriving after the store would otherwise see 0 and skip its
  // slice of the model while still zeroing its slice of `partial`
  __syncthreads();
  if (threadIdx.x == 0) {
    totals[m] = tot;
    partial[(int64_t)m * (P + 1) + P] = 0.f;
  }
  const float inv = upd ? 1.0f / tot : 0.f;
  for (int p = threadIdx.x; p < P; p += THREADS) {
    if (upd)
      global_params[(int64_t)m * P + p] =
          partial[(int64_t)m * (P + 1) + p] * inv;
    partial[(int64_t)m * (P + 1) + p] = 0.f;
  }
}

// ---------------------------------------------------------------------------
// evaluation kernel
// ---------------------------------------------------------------------------

struct EvalArgs {
  const float* __restrict__ params;     // [M, P]
  const int64_t* __restrict__ task_row; // [W]
  const int64_t* __restrict__ task_id;  // [W]
  const int64_t* __restrict__ off;      // [W]
  const int64_t* __restrict__ len;      // [W]
  const float* __restrict__ x;          // [N, D]
  const int64_t* __restrict__ y;        // [N]
  const float* __restrict__ x_mask;     // [W, D] or nullptr
  double* __restrict__ correct;         // [T]
  double* __restrict__ total;           // [T]
  double* __restrict__ loss;            // [T]
  double* __restrict__ mse;             // [T] or nullptr
  int D, H, O, P, kind;
};

extern "C" __global__ __launch_bounds__(THREADS)
void mlp_eval_kernel(EvalArgs a) {
  const int wdx = blockIdx.x;
  const int tid = threadIdx.x;
  const int64_t row = a.task_row[wdx];
  const int64_t tsk = a.task_id[wdx];
  const int64_t off = a.off[wdx];
  const int n = (int)a.len[wdx];

  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* w = lds;              // [P] (P fits: MLP family)
  float* red = w + a.P;        // [8] reduction scratch

  for (int p = tid; p < a.P; p += THREADS) w[p] = a.params[row * a.P + p];
  __syncthreads();

  const int HD = a.H * a.D;
  const int OH = a.O * a.H;
  const int OD = a.O * a.D;

  float c_acc = 0.f, l_acc = 0.f, e_acc = 0.f;
  for (int i = tid; i < n; i += THREADS) {
    const int yi = (int)a.y[off + i];
    float logits[64];
    if (a.kind == KIND_FNN) {
      // activations computed per-h on the fly (no [H] storage needed);
      // x is read from global — the window is L1/L2 resident
      for (int o = 0; o < a.O; ++o) logits[o] = w[HD + a.H + OH + o];
      for (int h = 0; h < a.H; ++h) {
        float z = w[HD + h];
        for (int d = 0; d < a.D; ++d) {
          float xd = a.x[(off + i) * a.D + d];
          if (a.x_mask) xd *= a.x_mask[(int64_t)wdx * a.D + d];
          z += w[h * a.D + d] * xd;
        }
        if (z > 0.f)
          for (int o = 0; o < a.O; ++o)
            logits[o] += w[HD + a.H + o * a.H + h] * z;
      }
    } else {
      for (int o = 0; o < a.O; ++o) {
        float z = w[OD + o];
        for (int d = 0; d < a.D; ++d) {
          float xd = a.x[(off + i) * a.D + d];
          if (a.x_mask) xd *= a.x_mask[(int64_t)wdx * a.D + d];
          z += w[o * a.D + d] * xd;
        }
        logits[o] = 1.f / (1.f + __expf(-z));
      }
    }
    // argmax + CE(logits, y) + optional AUE mse
    int best = 0;
    float zmax = logits[0];
    for (int o = 1; o < a.O; ++o)
      if (logits[o] > zmax) { zmax = logits[o]; best = o; }
    float zsum = 0.f;
    for (int o = 0; o < a.O; ++o) zsum += __expf(logits[o] - zmax);
    const float lse = logf(zsum) + zmax;
    c_acc += (best == yi) ? 1.f : 0.f;
    l_acc += lse - logits[yi];
    if (a.mse) {
      const float ptrue = __expf(logits[yi] - lse);
      e_acc += (1.f - ptrue) * (1.f - ptrue);
    }
  }

  float cs = block_reduce_sum(c_acc, red);
  float ls = block_reduce_sum(l_acc, red);
  float es = a.mse ? block_reduce_sum(e_acc, red) : 0.f;
  if (tid == 0) {
    atomicAdd(&a.correct[tsk], (double)cs);
    atomicAdd(&a.total[tsk], (double)n);
    atomicAdd(&a.loss[tsk], (double)ls);
    if (a.mse) atomicAdd(&a.mse[tsk], (double)es);
  }
}

// specialized small-model eval kernel: fully unrolled per-sample pipeline,
// x cached in registers (the generic kernel re-reads x[d] from global for
// every hidden unit; at SEA shapes that is D*H loads per sample and the
// kernel measures 87% SQ_WAIT) — same dispatch list as the train kernel
template <int TD, int TH, int TO, int KIND, int BS>
__global__ __launch_bounds__(BS)
void mlp_eval_small_kernel(EvalArgs a) {
  constexpr int TP = (KIND == KIND_FNN)
                         ? (TH * TD + TH + TO * TH + TO)
                         : (TO * TD + TO);
  constexpr int HD = TH * TD;
  constexpr int OH = TO * TH;
  const int wdx = blockIdx.x;
  const int tid = threadIdx.x;
  const int64_t row = a.task_row[wdx];
  const int64_t tsk = a.task_id[wdx];
  const int64_t off = a.off[wdx];
  const int n = (int)a.len[wdx];

  __shared__ __attribute__((aligned(16))) float w[TP];
  __shared__ float red[8];
  __shared__ float msk[TD];
  for (int p = tid; p < TP; p += BS) w[p] = a.params[row * TP + p];
  if (a.x_mask && tid < TD) msk[tid] = a.x_mask[(int64_t)wdx * TD + tid];
  __syncthreads();

  float c_acc = 0.f, l_acc = 0.f, e_acc = 0.f;
  for (int i = tid; i < n; i += BS) {
    float x[TD];
#pragma unroll
    for (int d = 0; d < TD; ++d) {
      x[d] = a.x[(off + i) * TD + d];
      if (a.x_mask) x[d] *= msk[d];
    }
    const int yi = (int)a.y[off + i];
    float logits[TO];
    if constexpr (KIND == KIND_FNN) {
#pragma unroll
      for (int o = 0; o < TO; ++o) logits[o] = w[HD + TH + OH + o];
#pragma unroll
      for (int h = 0; h < TH; ++h) {
        float z = w[HD + h];
#pragma unroll
        for (int d = 0; d < TD; ++d) z += w[h * TD + d] * x[d];
        z = z > 0.f ? z : 0.f;
#pragma unroll
        for (int o = 0; o < TO; ++o) logits[o] += w[HD + TH + o * TH + h] * z;
      }
    } else {
#pragma unroll
      for (int o = 0; o < TO; ++o) {
        float z = w[TO * TD + o];
#pragma unroll
        for (int d = 0; d < TD; ++d) z += w[o * TD + d] * x[d];
        logits[o] = 1.f / (1.f + __expf(-z));
      }
    }
    int best = 0;
    float zmax = logits[0];
#pragma unroll
    for (int o = 1; o < TO; ++o)
      if (logits[o] > zmax) { zmax = logits[o]; best = o; }
    float zsum = 0.f;
#pragma unroll
    for (int o = 0; o < TO; ++o) zsum += __expf(logits[o] - zmax);
    const float lse = logf(zsum) + zmax;
    c_acc += (best == yi) ? 1.f : 0.f;
    l_acc += lse - logits[yi];
    if (a.mse) {
      const float ptrue = __expf(logits[yi] - lse);
      e_acc += (1.f - ptrue) * (1.f - ptrue);
    }
  }

  float cs = block_reduce_sum(c_acc, red);
  float ls = block_reduce_sum(l_acc, red);
  float es = a.mse ? block_reduce_sum(e_acc, red) : 0.f;
  if (tid == 0) {
    atomicAdd(&a.correct[tsk], (double)cs);
    atomicAdd(&a.total[tsk], (double)n);
    atomicAdd(&a.loss[tsk], (double)ls);
    if (a.mse) atomicAdd(&a.mse[tsk], (double)es);
  }
}

static bool launch_small_eval(const EvalArgs& args, int W,
                              hipStream_t stream) {
  // A/B escape hatches for benchmarking the generic vs templated eval path
  // on the same box (FEDDRIFT_NO_SMALL_EVAL=1 forces the generic kernel,
  // FEDDRIFT_FORCE_SMALL_EVAL=1 ignores the grid-size gate — used by the
  // GPU numerics tests, which run tiny grids).
  static const bool disabled = [] {
    const char* e = getenv("FEDDRIFT_NO_SMALL_EVAL");
    return e && e[0] == '1';
  }();
  static const bool forced = [] {
    const char* e = getenv("FEDDRIFT_FORCE_SMALL_EVAL");
    return e && e[0] == '1';
  }();
  if (disabled) return false;
  // Same-box A/B (profiles/README.md): the register-pipelined kernel has
  // longer per-thread dependent chains than the generic unit-parallel one,
  // so it only wins once the grid saturates the 256 CUs with enough waves.
  // Measured (bench eval = 8 window-blocks/client): -6% at W=1600, tie at
  // W=3200, +5% at W=6400 rising to +16% at W=27k -> gate at 4096.
  if (W < 4096 && !forced) return false;
  // 64-thread (single-wave) blocks: windows are capped at 128 samples
  // (TaskList.CHUNK), so 256-thread blocks leave half the lanes idle and
  // run the block reduction across 4 waves; the gate above guarantees the
  // grid is large enough to fill the CUs with single-wave blocks.
#define TRY_ESHAPE(SD, SH, SO, SK)                                          \
  if (args.kind == SK && args.D == SD && args.H == SH && args.O == SO) {    \
    hipLaunchKernelGGL((mlp_eval_small_kernel<SD, SH, SO, SK, 64>),         \
                       dim3(W), dim3(64), 0, stream, args);                 \
    return true;                                                            \
  }
  SMALL_SHAPE_LIST(TRY_ESHAPE)
#undef TRY_ESHAPE
  return false;
}

// ---------------------------------------------------------------------------
// ensemble-vote + confusion kernels (AUE/AUE-PC/KUE server paths):
// the reference runs _infer_ens / _confusion_matrix as per-client torch
// loops on the server (FedAvgEnsAggregatorAue.py:256-283,
// FedAvgEnsAggregatorKue.py:234-303); here ONE launch covers every
// (task, window) with per-task ensemble weights and per-model masks.
// ---------------------------------------------------------------------------

#define VOTE_HARD 0
#define VOTE_SOFT 1

struct VoteArgs {
  const float* __restrict__ params;     // [M, P]
  const float* __restrict__ weights;    // [W, M]
  const int64_t* __restrict__ task_id;  // [W]
  const int64_t* __restrict__ off;      // [W]
  const int64_t* __restrict__ len;      // [W]
  const float* __restrict__ x;
  const int64_t* __restrict__ y;
  const float* __restrict__ masks;      // [M, D] or null
  double* __restrict__ correct;         // [T]
  double* __restrict__ total;           // [T]
  double* __restrict__ conf;            // [T, O, O] (confusion kernel)
  const int64_t* __restrict__ task_row; // [W] (confusion kernel)
  int M, D, H, O, P, kind, mode;
  int mask_bcast;                       // confusion: masks is [D], not [W, D]
};

__device__ __forceinline__ void mlp_logits_for(
    const float* __restrict__ w, const float* __restrict__ xrow,
    const float* __restrict__ msk, int D, int H, int O, int kind,
    float* logits) {
  if (kind == KIND_FNN) {
    const int HD = H * D;
    const int OH = O * H;
    for (int o = 0; o < O; ++o) logits[o] = w[HD + H + OH + o];
    for (int h = 0; h < H; ++h) {
      float z = w[HD + h];
      for (int d = 0; d < D; ++d) {
        float xd = xrow[d];
        if (msk) xd *= msk[d];
        z += w[h * D + d] * xd;
      }
      if (z > 0.f)
        for (int o = 0; o < O; ++o) logits[o] += w[HD + H + o * H + h] * z;
    }
  } else {
    const int OD = O * D;
    for (int o = 0; o < O; ++o) {
      float z = w[OD + o];
      for (int d = 0; d < D; ++d) {
        float xd = xrow[d];
        if (msk) xd *= msk[d];
        z += w[o * D + d] * xd;
      }
      logits[o] = 1.f / (1.f + __expf(-z));
    }
  }
}

extern "C" __global__ __launch_bounds__(THREADS)
void mlp_vote_kernel(VoteArgs a) {
  const int wdx = blockIdx.x;
  const int n = (int)a.len[wdx];
  const long long tsk = a.task_id[wdx];
  const long long off = a.off[wdx];
  const int tid = threadIdx.x;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* wt = lds;            // [M] this task's ensemble weights
  float* red = wt + a.M;      // [8]
  for (int m = tid; m < a.M; m += THREADS)
    wt[m] = a.weights[(long long)wdx * a.M + m];
  __syncthreads();
  float c_acc = 0.f;
  for (int i = tid; i < n; i += THREADS) {
    const float* xrow = a.x + (off + i) * a.D;
    const int yi = (int)a.y[off + i];
    float votes[64];
    for (int o = 0; o < a.O; ++o) votes[o] = 0.f;
    for (int m = 0; m < a.M; ++m) {
      const float wm = wt[m];
      if (wm == 0.f) continue;
      const float* msk = a.masks ? a.masks + (long long)m * a.D : nullptr;
      float logits[64];
      mlp_logits_for(a.params + (long long)m * a.P, xrow, msk,
                     a.D, a.H, a.O, a.kind, logits);
      if (a.mode == VOTE_HARD) {
        int best = 0;
        float bv = logits[0];
        for (int o = 1; o < a.O; ++o)
          if (logits[o] > bv) { bv = logits[o]; best = o; }
        votes[best] += wm;
      } else {
        float zmax = -1e30f;
        for (int o = 0; o < a.O; ++o) zmax = fmaxf(zmax, logits[o]);
        float zsum = 0.f;
        for (int o = 0; o < a.O; ++o) {
          logits[o] = __expf(logits[o] - zmax);
          zsum += logits[o];
        }
        for (int o = 0; o < a.O; ++o) votes[o] += wm * logits[o] / zsum;
      }
    }
    int best = 0;
    float bv = votes[0];
    for (int o = 1; o < a.O; ++o)
      if (votes[o] > bv) { bv = votes[o]; best = o; }
    c_acc += (best == yi) ? 1.f : 0.f;
  }
  const float cs = block_reduce_sum(c_acc, red);
  if (tid == 0) {
    atomicAdd(&a.correct[tsk], (double)cs);
    atomicAdd(&a.total[tsk], (double)n);
  }
}

extern "C" __global__ __launch_bounds__(THREADS)
void mlp_confusion_kernel(VoteArgs a) {
  const int wdx = blockIdx.x;
  const int n = (int)a.len[wdx];
  const long long tsk = a.task_id[wdx];
  const long long off = a.off[wdx];
  const long long row = a.task_row[wdx];
  const int tid = threadIdx.x;
  const float* w = a.params + row * a.P;
  const float* msk = a.masks
      ? a.masks + (a.mask_bcast ? 0 : (long long)wdx * a.D) : nullptr;
  for (int i = tid; i < n; i += THREADS) {
    const float* xrow = a.x + (off + i) * a.D;
    const int yi = (int)a.y[off + i];
    float logits[64];
    mlp_logits_for(w, xrow, msk, a.D, a.H, a.O, a.kind, logits);
    int best = 0;
    float bv = logits[0];
    for (int o = 1; o < a.O; ++o)
      if (logits[o] > bv) { bv = logits[o]; best = o; }
    atomicAdd(&a.conf[(tsk * a.O + yi) * a.O + best], 1.0);
  }
}

// ---------------------------------------------------------------------------
// host wrappers
// ---------------------------------------------------------------------------

static void check_f32_2d(const torch::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.dtype() == torch::kFloat32 &&
              t.is_contiguous(), name, " must be contiguous f32 CUDA");
}

void train_fused_hip(torch::Tensor params, torch::Tensor rows,
                     torch::Tensor x, torch::Tensor y,
                     torch::Tensor step_off, torch::Tensor step_len,
                     int64_t D, int64_t H, int64_t O, int64_t kind,
                     c10::optional<torch::Tensor> x_mask,
                     c10::optional<torch::Tensor> m,
                     c10::optional<torch::Tensor> v,
                     c10::optional<torch::Tensor> vmax,
                     c10::optional<torch::Tensor> t,
                     torch::Tensor lr, double wd,
                     c10::optional<torch::Tensor> in_params,
                     c10::optional<torch::Tensor> model_of,
                     c10::optional<torch::Tensor> sample_w,
                     c10::optional<torch::Tensor> partial, double mu) {
  const int G = rows.size(0);
  if (G == 0) return;
  TORCH_CHECK(O >= 1 && O <= 64,
              "train_fused: O=", O, " outside the per-sample float[64] logits");
  TORCH_CHECK(mu >= 0.0 && std::isfinite(mu),
              "train_fused: fedprox mu=", mu, " must be finite and >= 0");
  check_f32_2d(params, "params");
  const int P = params.size(1);
  const int E = step_off.size(1);
  const bool adam = m.has_value();

  // CPU step windows: into the launch packet where they fit, else this
  // call uploads them itself (correct, but a blocking pageable copy: the
  // engine asks inline_steps_ok first and keeps its pinned path otherwise)
  StepWin win;  // the launch copies it; entries past G*E are never read
  bool inl = false;
  if (!step_off.is_cuda()) {
    TORCH_CHECK(!step_len.is_cuda() && step_off.dtype() == torch::kInt64 &&
                step_len.dtype() == torch::kInt64 &&
                step_off.sizes() == step_len.sizes(),
                "train_fused: CPU step windows must be int64 of one shape");
    step_off = step_off.contiguous();
    step_len = step_len.contiguous();
    inl = inline_steps_ok(D, H, O, kind, G, E) &&
          step_off.numel() == (int64_t)G * E &&
          pack_steps(step_off, step_len, &win);
    if (!inl) {
      step_off = step_off.to(params.device());
      step_len = step_len.to(params.device());
    }
  }

  // chunk size: fit 2P + BC*(D + 2H + O | D + O) in the LDS budget
  const int per_sample = (kind == KIND_FNN) ? (D + 2 * H + O) : (D + O);
  int BC = (LDS_BUDGET_FLOATS - 2 * P) / per_sample;
  TORCH_CHECK(BC >= 1, "model too large for LDS-resident training path");
  BC = std::min<int>(BC, 512);

  const size_t lds_bytes =
      (size_t)(2 * P + (size_t)BC * per_sample) * sizeof(float);

  TrainArgs args;
  args.params = params.data_ptr<float>();
  args.in_params = in_params.has_value() ? in_params->data_ptr<float>()
                                         : nullptr;
  args.model_of = model_of.has_value() ? model_of->data_ptr<int>() : nullptr;
  args.sample_w = sample_w.has_value() ? sample_w->data_ptr<float>()
                                       : nullptr;
  args.partial = partial.has_value() ? partial->data_ptr<float>() : nullptr;
  args.rows = rows.data_ptr<int64_t>();
  args.x = x.data_ptr<float>();
  args.y = y.data_ptr<int64_t>();
  args.step_off = inl ? nullptr : step_off.data_ptr<int64_t>();
  args.step_len = inl ? nullptr : step_len.data_ptr<int64_t>();
  args.x_mask = x_mask.has_value() ? x_mask->data_ptr<float>() : nullptr;
  args.m = adam ? m->data_ptr<float>() : nullptr;
  args.v = adam ? v->data_ptr<float>() : nullptr;
  args.vmax = adam ? vmax->data_ptr<float>() : nullptr;
  args.t = adam ? t->data_ptr<int>() : nullptr;
  args.lr = lr.data_ptr<float>();
  args.wd = (float)wd;
  args.mu = (float)mu;
  args.E = E; args.D = (int)D; args.H = (int)H; args.O = (int)O;
  args.P = P; args.kind = (int)kind; args.opt = adam ? OPT_ADAM : OPT_SGD;
  args.BC = BC;

  if (!launch_small(args, win, G, c10::hip::getCurrentHIPStream())) {
    TORCH_CHECK(!inl, "train_fused: inline steps without a small kernel");
    hipLaunchKernelGGL(mlp_train_kernel, dim3(G), dim3(THREADS), lds_bytes,
                       c10::hip::getCurrentHIPStream(), args);
  }
  TORCH_CHECK(hipGetLastError() == hipSuccess, "mlp_train_kernel launch");
}

// test-only: the small train kernel's wave reduce-scatter on vals [64, TP]
torch::Tensor train_reduce_probe_hip(torch::Tensor vals) {
  check_f32_2d(vals, "vals");
  TORCH_CHECK(vals.dim() == 2 && vals.size(0) == 64,
              "train_reduce_probe: vals must be [64, TP]");
  const int TP = vals.size(1);
  auto out = torch::zeros({TP}, vals.options());
  auto stream = c10::hip::getCurrentHIPStream();
  bool found = false;
#define TRY_PROBE(SD, SH, SO, SK)                                          \
  if (!found && TP == (SK == KIND_FNN ? SH * SD + SH + SO * SH + SO        \
                                      : SO * SD + SO)) {                   \
    hipLaunchKernelGGL((train_reduce_probe_kernel<(                        \
                           SK == KIND_FNN ? SH * SD + SH + SO * SH + SO    \
                                          : SO * SD + SO)>),               \
                       dim3(1), dim3(64), 0, stream,                       \
                       vals.data_ptr<float>(), out.data_ptr<float>());     \
    found = true;                                                          \
  }
  SMALL_SHAPE_LIST(TRY_PROBE)
#undef TRY_PROBE
  TORCH_CHECK(found, "train_reduce_probe: no small train kernel has TP=", TP);
  TORCH_CHECK(hipGetLastError() == hipSuccess, "train_reduce_probe launch");
  return out;
}

torch::Tensor eval_tasks_hip(
    torch::Tensor params, torch::Tensor x, torch::Tensor y,
    torch::Tensor task_row, torch::Tensor task_id, torch::Tensor off,
    torch::Tensor len, int64_t n_tasks, int64_t D, int64_t H, int64_t O,
    int64_t kind, bool want_mse, c10::optional<torch::Tensor> x_mask) {
  TORCH_CHECK(O >= 1 && O <= 64,
              "eval_tasks: O=", O, " outside the per-sample float[64] logits");
  const int W = task_row.size(0);
  auto optd = torch::TensorOptions().dtype(torch::kFloat64)
                  .device(params.device());
  // one [rows, n_tasks] output buffer: correct/total/loss(/mse) are its
  // contiguous rows — no post-hoc stack/cat
  auto out = torch::zeros({want_mse ? 4 : 3, n_tasks}, optd);
  if (W == 0)
    return out;
  const int P = params.size(1);

  EvalArgs args;
  args.params = params.data_ptr<float>();
  args.task_row = task_row.data_ptr<int64_t>();
  args.task_id = task_id.data_ptr<int64_t>();
  args.off = off.data_ptr<int64_t>();
  args.len = len.data_ptr<int64_t>();
  args.x = x.data_ptr<float>();
  args.y = y.data_ptr<int64_t>();
  args.x_mask = x_mask.has_value() ? x_mask->data_ptr<float>() : nullptr;
  double* base = out.data_ptr<double>();
  args.correct = base;
  args.total = base + n_tasks;
  args.loss = base + 2 * n_tasks;
  args.mse = want_mse ? base + 3 * n_tasks : nullptr;
  args.D = (int)D; args.H = (int)H; args.O = (int)O; args.P = P;
  args.kind = (int)kind;

  const size_t lds_bytes = (size_t)(P + 8) * sizeof(float);
  TORCH_CHECK(lds_bytes <= 150 * 1024, "model too large for eval LDS path");
  if (!launch_small_eval(args, W, c10::hip::getCurrentHIPStream())) {
    hipLaunchKernelGGL(mlp_eval_kernel, dim3(W), dim3(THREADS), lds_bytes,
                       c10::hip::getCurrentHIPStream(), args);
  }
  TORCH_CHECK(hipGetLastError() == hipSuccess, "mlp_eval_kernel launch");
  return out;
}

void apply_aggregate_hip(torch::Tensor global_params, torch::Tensor partial,
                         c10::optional<torch::Tensor> mask,
                         torch::Tensor totals) {
  const int K = global_params.size(0);
  const int P = global_params.size(1);
  hipLaunchKernelGGL(apply_aggregate_kernel, dim3(K), dim3(THREADS), 0,
                     c10::hip::getCurrentHIPStream(),
                     global_params.data_ptr<float>(),
                     partial.data_ptr<float>(),
                     mask.has_value() ? mask->data_ptr<unsigned char>()
                                      : nullptr,
                     totals.data_ptr<float>(),
                     K, P);
  TORCH_CHECK(hipGetLastError() == hipSuccess, "apply_aggregate launch");
}

void register_cnn(pybind11::module_& mod);  // cnn_kernels.hip
void register_secagg(pybind11::module_& mod);  // secagg_kernels.hip
void register_robust(pybind11::module_& mod);  // robust_kernels.hip
void register_orderstat(pybind11::module_& mod);  // orderstat_kernels.hip
void register_krum(pybind11::module_& mod);  // krum_kernels.hip
void register_compress(pybind11::module_& mod);  // compress_kernels.hip

torch::Tensor ens_vote_multi_hip(
    torch::Tensor params, torch::Tensor weights, torch::Tensor x,
    torch::Tensor y, torch::Tensor task_id, torch::Tensor off,
    torch::Tensor len, int64_t n_tasks, int64_t D, int64_t H, int64_t O,
    int64_t kind, int64_t mode, c10::optional<torch::Tensor> masks) {
  TORCH_CHECK(O >= 1 && O <= 64,
              "ens_vote_multi: O=", O, " outside the per-sample float[64] logits");
  const int W = task_id.size(0);
  auto optd = torch::TensorOptions().dtype(torch::kFloat64)
                  .device(params.device());
  auto out = torch::zeros({2, n_tasks}, optd);
  if (W == 0) return out;
  VoteArgs a;
  a.params = params.data_ptr<float>();
  a.weights = weights.data_ptr<float>();
  a.task_id = task_id.data_ptr<int64_t>();
  a.off = off.data_ptr<int64_t>();
  a.len = len.data_ptr<int64_t>();
  a.x = x.data_ptr<float>();
  a.y = y.data_ptr<int64_t>();
  a.masks = masks.has_value() ? masks->data_ptr<float>() : nullptr;
  double* base = out.data_ptr<double>();
  a.correct = base;
  a.total = base + n_tasks;
  a.conf = nullptr;
  a.task_row = nullptr;
  a.M = (int)params.size(0);
  a.D = (int)D; a.H = (int)H; a.O = (int)O; a.P = (int)params.size(1);
  a.kind = (int)kind; a.mode = (int)mode; a.mask_bcast = 0;
  const size_t lds = (size_t)(a.M + 8) * sizeof(float);
  hipLaunchKernelGGL(mlp_vote_kernel, dim3(W), dim3(THREADS), lds,
                     c10::hip::getCurrentHIPStream(), a);
  TORCH_CHECK(hipGetLastError() == hipSuccess, "mlp_vote_kernel launch");
  return out;
}

torch::Tensor confusion_tasks_hip(
    torch::Tensor params, torch::Tensor x, torch::Tensor y,
    torch::Tensor task_row, torch::Tensor task_id, torch::Tensor off,
    torch::Tensor len, int64_t n_tasks, int64_t n_classes, int64_t D,
    int64_t H, int64_t O, int64_t kind,
    c10::optional<torch::Tensor> masks) {
  TORCH_CHECK(O >= 1 && O <= 64,
              "confusion_tasks: O=", O, " outside the per-sample float[64] logits");
  const int W = task_row.size(0);
  auto optd = torch::TensorOptions().dtype(torch::kFloat64)
                  .device(params.device());
  auto out = torch::zeros({n_tasks, n_classes, n_classes}, optd);
  if (W == 0) return out;
  VoteArgs a;
  a.params = params.data_ptr<float>();
  a.weights = nullptr;
  a.task_id = task_id.data_ptr<int64_t>();
  a.off = off.data_ptr<int64_t>();
  a.len = len.data_ptr<int64_t>();
  a.x = x.data_ptr<float>();
  a.y = y.data_ptr<int64_t>();
  a.masks = masks.has_value() ? masks->data_ptr<float>() : nullptr;
  a.correct = nullptr;
  a.total = nullptr;
  a.conf = out.data_ptr<double>();
  a.task_row = task_row.data_ptr<int64_t>();
  a.M = (int)params.size(0);
  a.D = (int)D; a.H = (int)H; a.O = (int)O; a.P = (int)params.size(1);
  a.kind = (int)kind; a.mode = 0;
  a.mask_bcast = (masks.has_value() && masks->dim() == 1) ? 1 : 0;
  hipLaunchKernelGGL(mlp_confusion_kernel, dim3(W), dim3(THREADS), 0,
                     c10::hip::getCurrentHIPStream(), a);
  TORCH_CHECK(hipGetLastError() == hipSuccess, "mlp_confusion launch");
  return out;
}

PYBIND11_MODULE(TORCH_EXTENSION_NAME, mod) {
  mod.def("train_fused", &train_fused_hip, "fused batched MLP local training");
  mod.def("train_reduce_probe", &train_reduce_probe_hip,
          "test-only: the small train kernel's wave reduce-scatter");
  mod.def("eval_tasks", &eval_tasks_hip, "batched MLP accuracy/loss sweep");
  mod.def("inline_steps_ok", &inline_steps_ok,
          "may a (d, h, o, kind) launch of G x E steps carry them inline");
  mod.def("steps_fit_inline", &steps_fit_inline,
          "test hook: do these CPU step windows pack into int32 pairs");
  mod.attr("INLINE_STEPS") = INLINE_STEPS;
  mod.def("apply_aggregate", &apply_aggregate_hip,
          "masked weighted-average model update");
  mod.def("ens_vote_multi", &ens_vote_multi_hip,
          "batched weighted ensemble vote (AUE/KUE)");
  mod.def("confusion_tasks", &confusion_tasks_hip,
          "batched per-task confusion matrices (KUE)");
  register_cnn(mod);
  register_secagg(mod);
  register_robust(mod);
  register_orderstat(mod);
  register_krum(mod);
  register_compress(mod);
}
