// feddrift MI355X (gfx950 / CDNA4) kernels — CNN_DropOut training + eval.
//
// Hand-written CDNA4 pipeline for the reference's MNIST/FEMNIST CNN
// (fedml_api/model/cv/cnn.py:113-135: 784 -> 28x28 -> conv3x3(32) ->
// conv3x3(64) [NO activation after either conv] -> maxpool2x2 ->
// dropout(.25) -> flatten(9216) -> relu(fc 128) -> dropout(.5) -> fc O ->
// in-graph Softmax; the training loss is CE applied to that softmax output
// — the double-softmax quirk, FedAvgEnsTrainer.py:73 — and the optimizer
// is SGD or Adam(amsgrad, wd), FedAvgEnsTrainer.py:23-33).
//
// Design (not a port — the reference runs this as per-(client, model)
// eager torch with CPU<->GPU model movement every round):
//   * ONE epoch = one fused multi-kernel launch sequence batched over ALL
//     (client, model) pairs of the round; per-pair weights stay resident
//     in flat HBM rows the whole time.
//   * gradient buffers use exclusive-owner writes (each block owns a
//     disjoint grad slice and loops the batch internally) — no grad
//     zeroing pass and no atomics on the wgrad paths.
//   * dropout masks are counter-based hashes of (seed, element id), so the
//     backward pass recomputes them instead of storing them.
//   * the softmax+CE tail computes dL/dz2 in the forward head kernel
//     (one kernel fuses fc2 forward, both softmaxes, and the CE gradient).
//   * fp32 everywhere: dtype parity with the reference's training, and
//     f32-input MFMA on gfx950 is bit-exact against an fmaf chain.
//
// Conv shapes (28x28 in): conv1 -> [32, 26, 26], conv2 -> [64, 24, 24],
// pool -> [64, 12, 12] = 9216 = fc1 input. fc1 -> 128, fc2 -> O (10/62).

#include <hip/hip_runtime.h>
#include <torch/extension.h>
#include <c10/hip/HIPStream.h>

#include <cmath>

#define WG 256

// fixed geometry of CNN_DropOut
#define IN_W 28
#define C1 32
#define S1 26           // conv1 output side
#define C2 64
#define S2 24           // conv2 output side
#define SP 12           // pooled side
#define NF 9216         // C2*SP*SP
#define NH 128
#define X1N (C1 * S1 * S1)   // 21632
#define Z2N (C2 * S2 * S2)   // 36864
#define D_IN 784

// flat parameter offsets (state_dict order; models/generic_packer.py)
#define OFF_W1C 0
#define OFF_B1C 288
#define OFF_W2C 320
#define OFF_B2C 18752
#define OFF_W1F 18816
#define OFF_B1F 1198464
#define OFF_W2F 1198592
// OFF_B2F = OFF_W2F + O*NH (runtime O)

struct CnnArgs {
  float* __restrict__ work;          // [G, P] live weights
  float* __restrict__ grad;          // [G, P]
  const int64_t* __restrict__ rows;  // [G] replica rows (opt state index)
  const float* __restrict__ x;       // arena [N, 784]
  const int64_t* __restrict__ y;     // arena [N]
  const int64_t* __restrict__ step_off;  // [G, E]
  const int64_t* __restrict__ step_len;  // [G, E]
  const float* __restrict__ x_mask;  // [G, 784] or null
  // workspace
  float* __restrict__ x1;            // [G, B, X1N]
  float* __restrict__ a2;            // [G, B, NF]  pooled+dropout1
  unsigned char* __restrict__ pidx;  // [G, B, NF]  pool argmax 0..3
  float* __restrict__ z1;            // [G, B, NH]  fc1 pre-activation
  float* __restrict__ a1;            // [G, B, NH]  relu+dropout2
  float* __restrict__ dz2;           // [G, B, O]   dL/d(fc2 out)
  float* __restrict__ dz1;           // [G, B, NH]
  float* __restrict__ da2;           // [G, B, NF]
  float* __restrict__ zz2;           // [G, B, Z2N] z2 (fwd) / dz2 (bwd),
                                     //   channels-last
  float* __restrict__ dx1;           // [G, B, X1N] channels-last
  float* __restrict__ c1part;        // [G, B, 320] conv1-wgrad partials
  float* __restrict__ wtf;           // [G, 9, 32, 64] conv2 W (fwd)
  float* __restrict__ wtd;           // [G, 9, 64, 32] conv2 W (dgrad)
  float* __restrict__ z1part;        // [G, FC1_KS, B, NH]
  float* __restrict__ w2part;        // [G, 9, W2_KS, 32, 64]
  float* __restrict__ b2part;        // [G, B, 64] conv2 bias partials
  // optimizer state (indexed by rows[g])
  float* __restrict__ m;
  float* __restrict__ v;
  float* __restrict__ vmax;
  int* __restrict__ t;
  const float* __restrict__ lr;      // [n_rows]
  float wd;
  // FedProx: mu > 0 pulls every executed step towards the pair's round
  // start, row rows[g] % K of the global bank (never written by a round)
  const float* __restrict__ anchor;  // [K, P] global models, or null
  float mu;
  int K;
  float p1, p2;                      // dropout probs
  unsigned long long seed;           // per (round, epoch)
  long long g0;                      // global pair-index base (mask hash)
  int G, B, E, e, O, P, opt, w2ms;
};

#define OPT_SGD 0
#define OPT_ADAM 1

typedef float f32x4 __attribute__((ext_vector_type(4)));
#define FC1_BK 32       // fc1 GEMM K-tile depth
#define FC1_KS 8        // fc1 K-split count (train z1part and eval z1pe)

__device__ __forceinline__ float hash_u01(unsigned long long s,
                                          unsigned long long id) {
  unsigned long long x = s + id * 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  x ^= x >> 31;
  return (float)(x >> 40) * (1.f / 16777216.f);
}

// dropout keep-scale for element id (1/(1-p) when kept, 0 when dropped)
__device__ __forceinline__ float drop_scale(const CnnArgs& a, int which,
                                            long long g, int b,
                                            long long j) {
  const float p = which == 0 ? a.p1 : a.p2;
  if (p <= 0.f) return 1.f;
  const long long nj = which == 0 ? NF : NH;
  const unsigned long long id =
      (unsigned long long)(((a.g0 + g) * (long long)a.E + a.e) *
                               (long long)a.B + b) * (2 * NF) +
      which * nj + j;
  return hash_u01(a.seed, id) >= p ? 1.f / (1.f - p) : 0.f;
}

__device__ __forceinline__ int step_n(const CnnArgs& a, int g) {
  return (int)a.step_len[(long long)g * a.E + a.e];
}
__device__ __forceinline__ long long step_o(const CnnArgs& a, int g) {
  return (long long)a.step_off[(long long)g * a.E + a.e];
}

// ---------------------------------------------------------------------------
// forward tile bodies, shared by the training kernels (block per (g, b),
// weights in work[g]) and the eval kernels (block per slot, weights in
// params[srow[slot]]). A kernel resolves its sample and its pointers and
// calls the body; the arithmetic exists once.
// ---------------------------------------------------------------------------

// masked 784-float input row -> LDS (the caller barriers)
__device__ __forceinline__ void stage_masked_input(float* xin,
                                                   const float* xs,
                                                   const float* xm) {
  for (int d = threadIdx.x; d < D_IN; d += WG)
    xin[d] = xm ? xs[d] * xm[d] : xs[d];
}

// conv1 forward for one sample: the masked input and the conv1 weights
// (w = the model's flat parameter row) stage in LDS once; each thread
// emits channels-last x1 elements (9 fused MACs each). x1 is
// CHANNELS-LAST [676, 32] so the conv2 MFMA stagers read contiguous ci
// slices.
__device__ __forceinline__ void conv1_fwd_body(const float* xs,
                                               const float* xm,
                                               const float* w, float* out) {
  const int tid = threadIdx.x;
  __shared__ __attribute__((aligned(16))) float xin[D_IN];
  __shared__ __attribute__((aligned(16))) float wc[288 + C1];
  stage_masked_input(xin, xs, xm);
  for (int i = tid; i < 288 + C1; i += WG) wc[i] = w[OFF_W1C + i];
  __syncthreads();
  for (int e = tid; e < X1N; e += WG) {
    const int pp = e / C1;
    const int c = e - pp * C1;
    const int oy = pp / S1, ox = pp - (pp / S1) * S1;
    float z = wc[288 + c];
#pragma unroll
    for (int ky = 0; ky < 3; ++ky)
#pragma unroll
      for (int kx = 0; kx < 3; ++kx)
        z = fmaf(xin[(oy + ky) * IN_W + ox + kx],
                 wc[c * 9 + ky * 3 + kx], z);
    out[e] = z;
  }
}

// conv2 forward as implicit GEMM on f32 MFMA: one tile of 64 * MF output
// pixels x 64 channels of one sample, K = 9 taps x 32 ci; each wave owns
// MF 16-pixel M-fragments. The x1 REGION feeding all 9 taps (6 or 8
// rows x 26 cols x 32 ci, channels-last) stages once per block — ONE
// barrier, then the MFMAs with the B operand (reshaped weights wt
// [9][32][64], L2-resident: 74 KB per model shared by all its blocks)
// loaded straight to registers. z2 lands CHANNELS-LAST.
//   MF = 1: 64-pixel tiles, 9 per sample, 6-row region.
//   MF = 2: 128-pixel tiles, 5 per sample, 8-row region (27.5 KB LDS):
//           every weight load feeds two MFMAs and each wave runs eight
//           accumulator chains; the last tile is partial (pp < 576).
template <int MF>
__device__ __forceinline__ void conv2_fwd_body(const float* x1_sample,
                                               const float* wt,
                                               const float* bias,
                                               float* z2, int pt) {
  constexpr int ROWS = MF == 1 ? 6 : 8;
  const int tid = threadIdx.x;
  const int wv = tid >> 6;
  const int l = tid & 63;
  const int li = l & 15, lk = l >> 4;
  // region: x1 rows [r0, r0+ROWS) x 26 cols, channels-last, +1 padded
  __shared__ __attribute__((aligned(16))) float sR[ROWS * S1][C1 + 1];
  const int p0 = pt * (64 * MF);
  const int r0 = p0 / S2;
  const float* x1 = x1_sample + (long long)r0 * S1 * C1;
  {
    // last tile: x1 only has rows r0..25 — rows past it are never read
    // by the compute (oy <= 25) but must not be FETCHED (OOB)
    const int nrow = min(ROWS * S1, (S1 - r0) * S1);
    const int r8 = tid >> 5, kk = tid & 31;
    for (int rr = r8; rr < ROWS * S1; rr += 8)
      sR[rr][kk] = (rr < nrow) ? x1[(long long)rr * C1 + kk] : 0.f;
  }
  __syncthreads();
  f32x4 acc[MF][4];
#pragma unroll
  for (int mf = 0; mf < MF; ++mf)
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[mf][t] = {0.f, 0.f, 0.f, 0.f};
  // this lane's A rows: output pixel p_a (M-fragment 0) and p_b (1).
  // Per-fragment values are named scalars, not MF-sized arrays: small
  // private arrays in the tap loop change how the compiler unrolls it
  // and the weight loads lose their scalar-base addressing.
  const int p_a = p0 + wv * (16 * MF) + li;
  const int p_b = p_a + 16;
  const int arow_a = (p_a / S2 - r0) * S1 + (p_a - (p_a / S2) * S2);
  const int arow_b = (p_b / S2 - r0) * S1 + (p_b - (p_b / S2) * S2);
  for (int kyx = 0; kyx < 9; ++kyx) {
    const int ky = kyx / 3, kx = kyx - (kyx / 3) * 3;
    const int offa = arow_a + ky * S1 + kx;
    const int offb = arow_b + ky * S1 + kx;
    const float* wk = wt + kyx * 2048;
#pragma unroll
    for (int ks = 0; ks < C1 / 4; ++ks) {
      const float av0 = sR[offa][ks * 4 + lk];
      float av1 = 0.f;
      if constexpr (MF == 2) av1 = sR[offb][ks * 4 + lk];
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) {
        const float bv = wk[(ks * 4 + lk) * C2 + ct * 16 + li];
        acc[0][ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(
            av0, bv, acc[0][ct], 0, 0, 0);
        if constexpr (MF == 2)
          acc[1][ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(
              av1, bv, acc[1][ct], 0, 0, 0);
      }
    }
  }
#pragma unroll
  for (int ct = 0; ct < 4; ++ct) {
    const int co = ct * 16 + li;
    const float bb = bias[co];
#pragma unroll
    for (int mf = 0; mf < MF; ++mf)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int pp = p0 + (wv * MF + mf) * 16 + lk * 4 + r;
        if (MF == 1 || pp < Z2N / C2)
          z2[(long long)pp * C2 + co] = acc[mf][ct][r] + bb;
      }
  }
}

// 2x2 maxpool of one sample's channels-last z2 into sa2 (LDS, [NF] in
// the torch-flatten [c][py][px] layout): z2 row pairs stage through LDS
// double-buffered (coalesced channels-last reads) — the next pooled
// row's loads issue before this row's max pass, land after it. TRAIN
// also records the argmax (first maximum wins: strict >) in spidx; eval
// keeps the max only. Returns after the barrier that publishes sa2.
template <bool TRAIN>
__device__ __forceinline__ void pool_rows_body(const float* z2, float* sa2,
                                               unsigned char* spidx) {
  const int tid = threadIdx.x;
  __shared__ __attribute__((aligned(16))) float srow[2][2 * S2 * C2];
  float rst[12];
#define PF_LOAD(py)                                                     \
  _Pragma("unroll") for (int jj = 0; jj < 12; ++jj)                      \
    rst[jj] = z2[(long long)(2 * (py)) * S2 * C2 + tid + jj * WG];
#define PF_WRITE(buf)                                                   \
  _Pragma("unroll") for (int jj = 0; jj < 12; ++jj)                      \
    srow[buf][tid + jj * WG] = rst[jj];
  PF_LOAD(0);
  PF_WRITE(0);
  __syncthreads();
  int cur = 0;
  for (int py = 0; py < SP; ++py) {
    if (py + 1 < SP) { PF_LOAD(py + 1); }
    for (int q = tid; q < C2 * SP; q += WG) {
      const int c = q / SP;
      const int px = q - c * SP;
      float best = -1e30f;
      int arg = 0;
#pragma unroll
      for (int dy = 0; dy < 2; ++dy)
#pragma unroll
        for (int dx = 0; dx < 2; ++dx) {
          const float z = srow[cur][(dy * S2 + 2 * px + dx) * C2 + c];
          if (TRAIN) {
            if (z > best) { best = z; arg = dy * 2 + dx; }
          } else {
            best = fmaxf(best, z);
          }
        }
      sa2[c * (SP * SP) + py * SP + px] = best;
      if (TRAIN) spidx[c * (SP * SP) + py * SP + px] = (unsigned char)arg;
    }
    if (py + 1 < SP) { PF_WRITE(cur ^ 1); }
    __syncthreads();
    cur ^= 1;
  }
#undef PF_LOAD
#undef PF_WRITE
}

// fc1 as an MFMA tile GEMM with K split over blocks (fills the chip at
// small fleets and small eval sweeps): partial z1 for up to 64 rows of A
// (mlen live, row stride NF) x 128 h over K-range [k_lo, k_hi) against
// the fc1 weight wp [128][NF]. 4 waves x 16 rows x 128 cols, f32-input
// MFMA, BK = 32 double-buffered register-staged LDS tiles with +1
// padding (issue the next tile's loads before the MFMAs, write after).
// Row r of the partial lands at out + r * out_stride.
__device__ __forceinline__ void fc1_tile_body(const float* A_rows, int mlen,
                                              const float* wp, int k_lo,
                                              int k_hi, float* out,
                                              long long out_stride) {
  const int tid = threadIdx.x;
  const int wv = tid >> 6;
  const int l = tid & 63;
  const int li = l & 15, lk = l >> 4;
  __shared__ __attribute__((aligned(16))) float sA[2][64][FC1_BK + 1];
  __shared__ __attribute__((aligned(16))) float sB[2][FC1_BK][NH + 1];
  f32x4 acc[8];
#pragma unroll
  for (int t = 0; t < 8; ++t) acc[t] = {0.f, 0.f, 0.f, 0.f};
  const int r8 = tid >> 5, kk = tid & 31;
  // register staging: 8 A rows + 16 B rows per thread per tile
  float ra[8], rb[16];
#define FC_LOAD(k0)                                                     \
  _Pragma("unroll") for (int j = 0; j < 8; ++j) {                        \
    const int rr = r8 + j * 8;                                           \
    ra[j] = (rr < mlen) ? A_rows[(long long)rr * NF + (k0) + kk] : 0.f;  \
  }                                                                      \
  _Pragma("unroll") for (int j = 0; j < 16; ++j)                         \
    rb[j] = wp[(long long)(r8 + j * 8) * NF + (k0) + kk];
#define FC_WRITE(buf)                                                   \
  _Pragma("unroll") for (int j = 0; j < 8; ++j)                          \
    sA[buf][r8 + j * 8][kk] = ra[j];                                     \
  _Pragma("unroll") for (int j = 0; j < 16; ++j)                         \
    sB[buf][kk][r8 + j * 8] = rb[j];
  FC_LOAD(k_lo);
  FC_WRITE(0);
  __syncthreads();
  int cur = 0;
  for (int k0 = k_lo; k0 < k_hi; k0 += FC1_BK) {
    if (k0 + FC1_BK < k_hi) { FC_LOAD(k0 + FC1_BK); }
#pragma unroll
    for (int kq = 0; kq < FC1_BK / 4; ++kq) {
      const float av = sA[cur][wv * 16 + li][kq * 4 + lk];
#pragma unroll
      for (int ct = 0; ct < 8; ++ct)
        acc[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(
            av, sB[cur][kq * 4 + lk][ct * 16 + li], acc[ct], 0, 0, 0);
    }
    if (k0 + FC1_BK < k_hi) { FC_WRITE(cur ^ 1); }
    __syncthreads();
    cur ^= 1;
  }
#undef FC_LOAD
#undef FC_WRITE
#pragma unroll
  for (int ct = 0; ct < 8; ++ct) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int mrow = wv * 16 + lk * 4 + r;
      if (mrow < mlen)
        out[mrow * out_stride + ct * 16 + li] = acc[ct][r];
    }
  }
}

// fold the FC1_KS fc1 partials of one (row, h) onto the bias: part
// points at the ks = 0 partial, consecutive partials lie ks_stride apart
__device__ __forceinline__ float fc1_fold(float bias, const float* part,
                                          long long ks_stride) {
  float z = bias;
#pragma unroll
  for (int ks = 0; ks < FC1_KS; ++ks) z += part[ks * ks_stride];
  return z;
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) v += __shfl_xor(v, m, 64);
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) v = fmaxf(v, __shfl_xor(v, m, 64));
  return v;
}

// fc2 + in-graph softmax for one sample on ONE WAVE: from the 128-float
// activation row a1 and the model's flat parameter row w, returns the
// model output s[l] in lane l (0 in lanes l >= O). Lane l collects logit
// l (O <= 64 always): the a1 row loads once into two coalesced registers
// per lane, each o-round is two coalesced weight loads + two fmas + a
// wave reduce, and the softmax runs as 6-step shuffle reductions — no
// per-thread O-arrays (the thread-per-sample form kept z2/s/ds[64] in
// scratch: 133 us/dispatch of spill traffic at the config-3 probe shape).
__device__ __forceinline__ float head_softmax(const float* a1,
                                              const float* w, int O,
                                              int l) {
  const float r0 = a1[l], r1 = a1[64 + l];
  float zlane = 0.f;
  for (int o = 0; o < O; ++o) {
    const float* wo = w + OFF_W2F + (long long)o * NH;
    const float v = wave_sum(fmaf(r0, wo[l], r1 * wo[64 + l]));
    if (l == o) zlane = v;
  }
  const bool live = l < O;
  const float z = live ? zlane + w[OFF_W2F + (long long)O * NH + l]
                       : -1e30f;
  const float zmax = wave_max(z);
  const float e = live ? __expf(z - zmax) : 0.f;
  return e / wave_sum(e);
}

// ---------------------------------------------------------------------------
// forward (training)
// ---------------------------------------------------------------------------

// conv1 forward, block per (g, b) -> x1 [G, B, 676, 32]
extern "C" __global__ __launch_bounds__(WG)
void cnn_conv1_fwd(CnnArgs a) {
  const int g = blockIdx.x / a.B;
  const int b = blockIdx.x - g * a.B;
  if (b >= step_n(a, g)) return;
  conv1_fwd_body(a.x + (step_o(a, g) + b) * D_IN,
                 a.x_mask ? a.x_mask + (long long)g * D_IN : nullptr,
                 a.work + (long long)g * a.P,
                 a.x1 + ((long long)g * a.B + b) * X1N);
}

// reshape conv2 weights for the MFMA stagers (per pair, per epoch):
// wtf[g][kyx][ci][co] (fwd B-operand) and wtd[g][kyx][co][ci] (dgrad)
extern "C" __global__ __launch_bounds__(WG)
void cnn_w2_reshape(CnnArgs a) {
  const long long total = (long long)a.G * C2 * C1 * 9;
  for (long long q = (long long)blockIdx.x * WG + threadIdx.x; q < total;
       q += (long long)gridDim.x * WG) {
    const int g = (int)(q / (C2 * C1 * 9));
    const int r = (int)(q - (long long)g * C2 * C1 * 9);
    const int co = r / (C1 * 9);
    const int t = r - co * C1 * 9;
    const int ci = t / 9;
    const int kyx = t - ci * 9;
    const float wv = a.work[(long long)g * a.P + OFF_W2C + r];
    a.wtf[((long long)g * 9 + kyx) * 2048 + ci * C2 + co] = wv;
    a.wtd[((long long)g * 9 + kyx) * 2048 + co * C1 + ci] = wv;
  }
}

// conv2 forward, block per (g, b, ptile): z2 lands in zz2. The 64-pixel
// kernel is the default; the 128-pixel one (FEDDRIFT_CONV2FWD=2) applies
// the dgrad-v3 trick to fwd (fwd was issue-stalled 0.65 with one global
// load per MFMA) and measured slower.
template <int MF>
__device__ __forceinline__ void conv2_fwd_train(const CnnArgs& a) {
  constexpr int TILES = MF == 1 ? 9 : 5;      // ceil(576 / (64 * MF))
  const int pt = blockIdx.x % TILES;
  const int gb = blockIdx.x / TILES;
  const int g = gb / a.B;
  const int b = gb - g * a.B;
  if (b >= step_n(a, g)) return;
  conv2_fwd_body<MF>(a.x1 + ((long long)g * a.B + b) * X1N,
                     a.wtf + (long long)g * 9 * 2048,
                     a.work + (long long)g * a.P + OFF_B2C,
                     a.zz2 + ((long long)g * a.B + b) * Z2N, pt);
}
extern "C" __global__ __launch_bounds__(WG)
void cnn_conv2_fwd_mfma(CnnArgs a) { conv2_fwd_train<1>(a); }
extern "C" __global__ __launch_bounds__(WG)
void cnn_conv2_fwd_mfma2(CnnArgs a) { conv2_fwd_train<2>(a); }

// maxpool + dropout1 over the channels-last z2, block per (g, b): the
// pooled a2/pidx tiles assemble in LDS and store with one coalesced pass
// in the torch-flatten [c][py][px] layout
extern "C" __global__ __launch_bounds__(WG)
void cnn_pool_fwd(CnnArgs a) {
  const int g = blockIdx.x / a.B;
  const int b = blockIdx.x - g * a.B;
  if (b >= step_n(a, g)) return;
  __shared__ __attribute__((aligned(16))) float sa2[NF];
  __shared__ unsigned char spidx[NF];
  pool_rows_body<true>(a.zz2 + ((long long)g * a.B + b) * Z2N, sa2, spidx);
  float* a2o = a.a2 + ((long long)g * a.B + b) * NF;
  unsigned char* po = a.pidx + ((long long)g * a.B + b) * NF;
  for (int e = threadIdx.x; e < NF; e += WG) {
    a2o[e] = sa2[e] * drop_scale(a, 0, g, b, e);
    po[e] = spidx[e];
  }
}

// fc1 forward: block (g, mtile, ks) computes partial z1 for 64 batch
// rows x 128 h over K-range [ks*NF/KS, ...). Partials land in z1part
// [G, FC1_KS, B, NH].
extern "C" __global__ __launch_bounds__(WG)
void cnn_fc1_fwd_mfma(CnnArgs a) {
  const int mtiles = (a.B + 63) / 64;
  const int ks = blockIdx.x % FC1_KS;
  const int rest = blockIdx.x / FC1_KS;
  const int mt = rest % mtiles;
  const int g = rest / mtiles;
  const int n = step_n(a, g);
  if (mt * 64 >= n) return;
  fc1_tile_body(
      a.a2 + ((long long)g * a.B + (long long)mt * 64) * NF,
      min(64, n - mt * 64), a.work + (long long)g * a.P + OFF_W1F,
      ks * (NF / FC1_KS), (ks + 1) * (NF / FC1_KS),
      a.z1part + (((long long)g * FC1_KS + ks) * a.B + (long long)mt * 64)
                     * NH,
      NH);
}

// combine fc1 K-split partials + bias, apply relu + dropout2
extern "C" __global__ __launch_bounds__(WG)
void cnn_fc1_act(CnnArgs a) {
  const long long total = (long long)a.G * a.B * NH;
  for (long long q = (long long)blockIdx.x * WG + threadIdx.x; q < total;
       q += (long long)gridDim.x * WG) {
    const int g = (int)(q / ((long long)a.B * NH));
    const long long r = q - (long long)g * a.B * NH;
    const int b = (int)(r / NH);
    if (b >= step_n(a, g)) continue;
    const int h = (int)(r - (long long)b * NH);
    const float z = fc1_fold(
        a.work[(long long)g * a.P + OFF_B1F + h],
        a.z1part + ((long long)g * FC1_KS * a.B + b) * NH + h,
        (long long)a.B * NH);
    a.z1[q] = z;
    const float rl = z > 0.f ? z : 0.f;
    a.a1[q] = rl * drop_scale(a, 1, g, b, h);
  }
}

// fc2 + softmax (in-graph model output s) + CE-on-s gradient -> dz2
// dL/ds = (softmax(s) - onehot(y)) / n; dL/dz2 = s*(dL/ds - sum(dL/ds*s))
// ONE WAVE per sample (head_softmax); the second softmax and the
// gradient run as the same shuffle reductions.
extern "C" __global__ __launch_bounds__(WG)
void cnn_head_fwd(CnnArgs a) {
  const long long total = (long long)a.G * a.B;
  const int l = threadIdx.x & 63;
  for (long long q = (long long)blockIdx.x * (WG / 64) + (threadIdx.x >> 6);
       q < total; q += (long long)gridDim.x * (WG / 64)) {
    const int g = (int)(q / a.B);
    const int b = (int)(q - (long long)g * a.B);
    const int n = step_n(a, g);
    if (b >= n) continue;
    const float inv_n = 1.f / (float)n;
    const int yi = (int)a.y[step_o(a, g) + b];
    const bool live = l < a.O;
    const float s = head_softmax(a.a1 + q * NH,
                                 a.work + (long long)g * a.P, a.O, l);
    // CE(log_softmax(s), y): q2 = softmax(s)
    const float smax = wave_max(live ? s : -1e30f);
    float e2 = live ? __expf(s - smax) : 0.f;
    float q2 = e2 / wave_sum(e2);
    if (l == yi) q2 -= 1.f;
    const float ds = q2 * inv_n;
    const float dot = wave_sum(live ? ds * s : 0.f);
    if (live) a.dz2[q * a.O + l] = s * (ds - dot);
  }
}

// ---------------------------------------------------------------------------
// backward
// ---------------------------------------------------------------------------

// fc2 wgrad + bias grad: thread per (g, o, h) (+ o for bias when h == 0)
extern "C" __global__ __launch_bounds__(WG)
void cnn_fc2_wgrad(CnnArgs a) {
  const long long total = (long long)a.G * a.O * NH;
  for (long long q = (long long)blockIdx.x * WG + threadIdx.x; q < total;
       q += (long long)gridDim.x * WG) {
    const int g = (int)(q / ((long long)a.O * NH));
    const long long r = q - (long long)g * a.O * NH;
    const int o = (int)(r / NH);
    const int h = (int)(r - (long long)o * NH);
    const int n = step_n(a, g);
    if (n == 0) continue;
    float acc = 0.f, accb = 0.f;
    for (int b = 0; b < n; ++b) {
      const float d = a.dz2[((long long)g * a.B + b) * a.O + o];
      acc = fmaf(d, a.a1[((long long)g * a.B + b) * NH + h], acc);
      if (h == 0) accb += d;
    }
    float* gr = a.grad + (long long)g * a.P;
    gr[OFF_W2F + (long long)o * NH + h] = acc;
    if (h == 0) gr[OFF_W2F + (long long)a.O * NH + o] = accb;
  }
}

// fc2 dgrad -> through dropout2 + relu -> dz1: thread per (g, b, h)
extern "C" __global__ __launch_bounds__(WG)
void cnn_fc2_dgrad(CnnArgs a) {
  const long long total = (long long)a.G * a.B * NH;
  for (long long q = (long long)blockIdx.x * WG + threadIdx.x; q < total;
       q += (long long)gridDim.x * WG) {
    const int g = (int)(q / ((long long)a.B * NH));
    const long long r = q - (long long)g * a.B * NH;
    const int b = (int)(r / NH);
    if (b >= step_n(a, g)) continue;
    const int h = (int)(r - (long long)b * NH);
    const float* w = a.work + (long long)g * a.P + OFF_W2F;
    float acc = 0.f;
    for (int o = 0; o < a.O; ++o)
      acc = fmaf(a.dz2[((long long)g * a.B + b) * a.O + o],
                 w[(long long)o * NH + h], acc);
    const float zv = a.z1[q];
    a.dz1[q] = zv > 0.f ? acc * drop_scale(a, 1, g, b, h) : 0.f;
  }
}

// fc1 wgrad as MFMA GEMM: dW1f[h][j] = sum_b dz1[b][h] a2[b][j] —
// block per (g, jtile of 128 columns), 64 (h-tile, j-tile) outputs
// split over 4 waves, K = batch staged in 16-sample chunks (both
// operands come in [b][.] layout, so the A fragment reads the staged
// dz1 tile transposed in place). Exclusive-owner writes.
extern "C" __global__ __launch_bounds__(WG)
void cnn_fc1_wgrad(CnnArgs a) {
  const int jt = blockIdx.x % (NF / 128);
  const int g = blockIdx.x / (NF / 128);
  const int n = step_n(a, g);
  if (n == 0) return;
  const int tid = threadIdx.x;
  const int wv = tid >> 6;
  const int l = tid & 63;
  const int li = l & 15, lk = l >> 4;
  __shared__ __attribute__((aligned(16))) float sDZ[16][NH + 1];
  __shared__ __attribute__((aligned(16))) float sA2[16][129];
  f32x4 acc[16];
#pragma unroll
  for (int t = 0; t < 16; ++t) acc[t] = {0.f, 0.f, 0.f, 0.f};
  const float* dz1 = a.dz1 + (long long)g * a.B * NH;
  const float* a2 = a.a2 + (long long)g * a.B * NF + jt * 128;
  const int j = tid & 127;
  const int b2 = tid >> 7;                // 2 stager rows per pass
  for (int b0 = 0; b0 < n; b0 += 16) {
    for (int bb = b2; bb < 16; bb += 2) {
      const bool ok = b0 + bb < n;
      sDZ[bb][j] = ok ? dz1[(long long)(b0 + bb) * NH + j] : 0.f;
      sA2[bb][j] = ok ? a2[(long long)(b0 + bb) * NF + j] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
#pragma unroll
      for (int t = 0; t < 16; ++t) {
        const int tile = wv * 16 + t;
        const int rt = tile >> 3, ct = tile & 7;
        acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(
            sDZ[ks * 4 + lk][rt * 16 + li],
            sA2[ks * 4 + lk][ct * 16 + li], acc[t], 0, 0, 0);
      }
    }
    __syncthreads();
  }
  float* gr = a.grad + (long long)g * a.P + OFF_W1F;
#pragma unroll
  for (int t = 0; t < 16; ++t) {
    const int tile = wv * 16 + t;
    const int rt = tile >> 3, ct = tile & 7;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int h = rt * 16 + lk * 4 + r;
      gr[(long long)h * NF + jt * 128 + ct * 16 + li] = acc[t][r];
    }
  }
}

// fc1 bias grad: thread per (g, h)
extern "C" __global__ __launch_bounds__(WG)
void cnn_fc1_bias_grad(CnnArgs a) {
  const long long total = (long long)a.G * NH;
  for (long long q = (long long)blockIdx.x * WG + threadIdx.x; q < total;
       q += (long long)gridDim.x * WG) {
    const int g = (int)(q / NH);
    const int h = (int)(q - (long long)g * NH);
    const int n = step_n(a, g);
    if (n == 0) continue;
    float s = 0.f;
    for (int b = 0; b < n; ++b)
      s += a.dz1[((long long)g * a.B + b) * NH + h];
    a.grad[(long long)g * a.P + OFF_B1F + h] = s;
  }
}

// fc1 dgrad as MFMA GEMM: da2[b][j] = sum_h dz1[b][h] W1f[h][j] —
// block per (g, b-tile of 64, jtile of 128), K = 128 in 32-deep chunks
extern "C" __global__ __launch_bounds__(WG)
void cnn_fc1_dgrad(CnnArgs a) {
  const int jt = blockIdx.x % (NF / 128);
  const int rest = blockIdx.x / (NF / 128);
  const int mtiles = (a.B + 63) / 64;
  const int mt = rest % mtiles;
  const int g = rest / mtiles;
  const int n = step_n(a, g);
  if (mt * 64 >= n) return;
  const int tid = threadIdx.x;
  const int wv = tid >> 6;
  const int l = tid & 63;
  const int li = l & 15, lk = l >> 4;
  __shared__ __attribute__((aligned(16))) float sA[64][33];
  __shared__ __attribute__((aligned(16))) float sB[32][129];
  f32x4 acc[8];
#pragma unroll
  for (int t = 0; t < 8; ++t) acc[t] = {0.f, 0.f, 0.f, 0.f};
  const int mlen = min(64, n - mt * 64);
  const float* dz1 = a.dz1 + ((long long)g * a.B + mt * 64) * NH;
  const float* w = a.work + (long long)g * a.P + OFF_W1F + jt * 128;
  const int r8 = tid >> 5, kk = tid & 31;
  const int j = tid & 127, h2 = tid >> 7;
  for (int k0 = 0; k0 < NH; k0 += 32) {
    for (int rr = r8; rr < 64; rr += 8)
      sA[rr][kk] = (rr < mlen)
          ? dz1[(long long)rr * NH + k0 + kk] : 0.f;
    for (int hh = h2; hh < 32; hh += 2)
      sB[hh][j] = w[(long long)(k0 + hh) * NF + j];
    __syncthreads();
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) {
      const float av = sA[wv * 16 + li][ks * 4 + lk];
#pragma unroll
      for (int ct = 0; ct < 8; ++ct)
        acc[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(
            av, sB[ks * 4 + lk][ct * 16 + li], acc[ct], 0, 0, 0);
    }
    __syncthreads();
  }
  float* da2 = a.da2 + ((long long)g * a.B + mt * 64) * NF + jt * 128;
#pragma unroll
  for (int ct = 0; ct < 8; ++ct) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = wv * 16 + lk * 4 + r;
      if (row < mlen)
        da2[(long long)row * NF + ct * 16 + li] = acc[ct][r];
    }
  }
}

// pool backward, block per (g, b): da2 reads coalesced (flatten layout,
// dropout reapplied), routed dz2 writes coalesced channels-last via an
// LDS-staged transpose; the conv2 bias grad (sum of routed dz) emits a
// per-sample partial (b2part) that the wgrad reduce sums deterministically
extern "C" __global__ __launch_bounds__(WG)
void cnn_pool_bwd(CnnArgs a) {
  const int g = blockIdx.x / a.B;
  const int b = blockIdx.x - g * a.B;
  if (b >= step_n(a, g)) return;
  const int tid = threadIdx.x;
  __shared__ __attribute__((aligned(16))) float sda[NF];
  __shared__ float sbias[C2];
  const float* da2 = a.da2 + ((long long)g * a.B + b) * NF;
  for (int e = tid; e < NF; e += WG)
    sda[e] = da2[e] * drop_scale(a, 0, g, b, e);
  if (tid < C2) sbias[tid] = 0.f;
  __syncthreads();
  const unsigned char* pidx = a.pidx + ((long long)g * a.B + b) * NF;
  float* dzc = a.zz2 + ((long long)g * a.B + b) * Z2N;
  float bacc = 0.f;
  const int c = tid & 63;            // fixed per thread (WG % 64 == 0)
  for (int q = tid; q < Z2N; q += WG) {
    const int p2 = q >> 6;           // z2 pixel
    const int oy = p2 / S2, ox = p2 - (p2 / S2) * S2;
    const int e = c * (SP * SP) + (oy >> 1) * SP + (ox >> 1);
    const int arg = (oy & 1) * 2 + (ox & 1);
    const float v = ((int)pidx[e] == arg) ? sda[e] : 0.f;
    dzc[q] = v;
    bacc += v;
  }
  // per-channel reduce (4 threads share each c), then a per-sample
  // partial into the dz2 scratch ([G, B, 64], free after fc2 backward);
  // cnn_conv2_wgrad_reduce sums it deterministically
  for (int off = 192; off > 0; off -= 64) {
    __syncthreads();
    if (tid >= off && tid < off + 64) sbias[c] += bacc;
  }
  __syncthreads();
  if (tid < C2)
    a.b2part[((long long)g * a.B + b) * C2 + tid] = sbias[tid] + bacc;
}

// conv2 wgrad as MFMA GEMM: dW[(kyx, ci)][co] = sum_m A[m, ci] dz[m, co]
// with m = (b, pixel). Block per (g, ms): for each owned 64-pixel
// m-tile, the x1 REGION (feeds all 9 taps) and the dz tile stage ONCE;
// each wave accumulates 18 of the 72 (kyx, ci-tile, co-tile) outputs
// (acc stays in registers across the whole m-range). Partials land in
// w2part[g][ms] and reduce deterministically. The m-split count is a
// runtime knob (a.w2ms) so small fleets still fill 256 CUs.
#define W2_FLUSH 16    // tiles per first-level accumulation chain

// waves_per_eu(2, 2): LDS already limits this kernel to 2 blocks/CU; the
// cap keeps both accumulator sets in 193 VGPRs with no scratch (left to
// itself the allocator takes 260 registers and halves the occupancy)
extern "C" __global__ __launch_bounds__(WG)
__attribute__((amdgpu_waves_per_eu(2, 2)))
void cnn_conv2_wgrad_mfma(CnnArgs a) {
  const int ms = blockIdx.x % a.w2ms;
  const int g = blockIdx.x / a.w2ms;
  const int n = step_n(a, g);
  float* part = a.w2part + ((long long)g * a.w2ms + ms) * (9 * 2048);
  const int tid = threadIdx.x;
  const int wv = tid >> 6;
  const int l = tid & 63;
  const int li = l & 15, lk = l >> 4;
  // all staging by async DMA (global_load_lds): both operands are read
  // stride-1 per lane group, so LINEAR LDS images need no padding or
  // swizzle. Region [160 rows x 32 ci] (rows 156..159 are never read),
  // dz tile [64 m x 64 co]; both double-buffered with counted waits +
  // raw barriers so the next m-tile streams under this tile's MFMAs.
  // ONE shared object (a second __shared__ makes hipcc drain vmcnt(0)
  // before every ds_read beside an in-flight glds — guide §5 trap (a))
  __shared__ __attribute__((aligned(16))) float ldsw[2 * 160 * C1
                                                     + 2 * 64 * C2];
  float (*sR)[160 * C1] = (float (*)[160 * C1])ldsw;
  float (*sD)[64 * C2] = (float (*)[64 * C2])(ldsw + 2 * 160 * C1);
  // Two-level accumulation: `acc` takes the MFMA chain of at most
  // W2_FLUSH tiles (1024 terms), then folds into `tot`. At w2ms = 1 one
  // block owns all 9 * n tiles; a single fp32 chain over those (37,440
  // terms at n = 65) measured 4.2e-6 of max|dW| against float64, ten
  // times the error of the 64-way split. Register-only: the fold is 72
  // adds per 16 tiles of 288 MFMAs each.
  f32x4 acc[18], tot[18];
#pragma unroll
  for (int t = 0; t < 18; ++t) {
    acc[t] = {0.f, 0.f, 0.f, 0.f};
    tot[t] = {0.f, 0.f, 0.f, 0.f};
  }
  int chain = 0;
  const long long mtiles = ((long long)n * (S2 * S2) + 63) / 64;
  // per wave per tile: 5 region glds + 4 dz glds (1 KiB each)
#define WG_ISSUE(MT, BUF)                                                \
  {                                                                      \
    const long long m0_ = (MT) * 64;                                     \
    const int b_ = (int)(m0_ / (S2 * S2));                               \
    const int p0_ = (int)(m0_ - (long long)b_ * (S2 * S2));              \
    const int r0_ = p0_ / S2;                                            \
    const int nrow_ = (S1 - r0_) * S1;                                   \
    const long long gb_ = (long long)g * a.B + b_;                       \
    const float* x1_ = a.x1 + (gb_ * 676 + (long long)r0_ * S1) * C1;    \
    const float* dz_ = a.zz2 + (gb_ * 576 + p0_) * C2;                   \
    _Pragma("unroll") for (int gq = 0; gq < 5; ++gq) {                   \
      const int f0_ = (wv * 5 + gq) * 256;      /* region floats */      \
      int srow_ = (f0_ + l * 4) / C1;           /* source arow */        \
      srow_ = srow_ < nrow_ ? srow_ : nrow_ - 1;                         \
      const int sch_ = (f0_ + l * 4) & 31;                               \
      __builtin_amdgcn_global_load_lds(                                  \
          (const __attribute__((address_space(1))) unsigned int*)        \
              (x1_ + (long long)srow_ * C1 + sch_),                      \
          (__attribute__((address_space(3))) unsigned int*)              \
              (&sR[BUF][f0_]),                                           \
          16, 0, 0);                                                     \
    }                                                                    \
    _Pragma("unroll") for (int gq = 0; gq < 4; ++gq) {                   \
      const int f0_ = (wv * 4 + gq) * 256;                               \
      __builtin_amdgcn_global_load_lds(                                  \
          (const __attribute__((address_space(1))) unsigned int*)        \
              (dz_ + f0_ + l * 4),                                       \
          (__attribute__((address_space(3))) unsigned int*)              \
              (&sD[BUF][f0_]),                                           \
          16, 0, 0);                                                     \
    }                                                                    \
  }
  int cur = 0;
  if (ms < mtiles) { WG_ISSUE(ms, 0); }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  for (long long mt = ms; mt < mtiles; mt += a.w2ms) {
    const int p0 = (int)((mt * 64) % (S2 * S2));
    const int r0 = p0 / S2;
    if (mt + a.w2ms < mtiles) { WG_ISSUE(mt + a.w2ms, cur ^ 1); }
    int parow[16];
#pragma unroll
    for (int km = 0; km < 16; ++km) {
      const int q = p0 + km * 4 + lk;
      parow[km] = (q / S2 - r0) * S1 + (q - (q / S2) * S2);
    }
    const float* bR = sR[cur];
    const float* bD = sD[cur];
#pragma unroll
    for (int kyx = 0; kyx < 9; ++kyx) {
      const int kyoff = (kyx / 3) * S1 + (kyx - (kyx / 3) * 3);
#pragma unroll
      for (int tt = 0; tt < 8; ++tt) {
        if ((kyx * 8 + tt) % 4 != wv) continue;
        const int slot = (kyx * 8 + tt) / 4;
        const int rt = tt >> 2, ct = tt & 3;
#pragma unroll
        for (int km = 0; km < 16; ++km) {
          acc[slot] = __builtin_amdgcn_mfma_f32_16x16x4f32(
              bR[(parow[km] + kyoff) * C1 + rt * 16 + li],
              bD[(km * 4 + lk) * C2 + ct * 16 + li], acc[slot],
              0, 0, 0);
        }
      }
    }
    if (mt + a.w2ms < mtiles) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __builtin_amdgcn_s_barrier();
    cur ^= 1;
    if (++chain == W2_FLUSH) {
      chain = 0;
#pragma unroll
      for (int t = 0; t < 18; ++t) {
        tot[t] += acc[t];
        acc[t] = {0.f, 0.f, 0.f, 0.f};
      }
    }
  }
#undef WG_ISSUE
#pragma unroll
  for (int t = 0; t < 18; ++t) acc[t] += tot[t];
#pragma unroll
  for (int slot = 0; slot < 18; ++slot) {
    const int kyx = (slot * 4 + wv) / 8;
    const int tt = (slot * 4 + wv) % 8;
    const int rt = tt >> 2, ct = tt & 3;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int ci = rt * 16 + lk * 4 + r;
      part[kyx * 2048 + ci * C2 + ct * 16 + li] = acc[slot][r];
    }
  }
}

// reduce the conv2 wgrad msplit partials into the (co, ci, ky, kx) grad;
// the tail entries (one per (g, co)) reduce the bias partials from
// pool_bwd over the batch — all deterministic
extern "C" __global__ __launch_bounds__(WG)
void cnn_conv2_wgrad_reduce(CnnArgs a) {
  const long long per_g = 9 * 2048 + C2;
  const long long total = (long long)a.G * per_g;
  for (long long q = (long long)blockIdx.x * WG + threadIdx.x; q < total;
       q += (long long)gridDim.x * WG) {
    const int g = (int)(q / per_g);
    const int r = (int)(q - (long long)g * per_g);
    const int n = step_n(a, g);
    if (n == 0) continue;
    if (r >= 9 * 2048) {
      const int co = r - 9 * 2048;
      float s = 0.f;
      for (int b = 0; b < n; ++b)
        s += a.b2part[((long long)g * a.B + b) * C2 + co];
      a.grad[(long long)g * a.P + OFF_B2C + co] = s;
      continue;
    }
    const int kyx = r / 2048;
    const int t = r - kyx * 2048;
    const int ci = t / C2, co = t - (t / C2) * C2;
    const float* part = a.w2part + (long long)g * a.w2ms * 9 * 2048
                        + kyx * 2048 + t;
    float s = 0.f;
    for (int ms = 0; ms < a.w2ms; ++ms)
      s += part[(long long)ms * 9 * 2048];
    a.grad[(long long)g * a.P + OFF_W2C + (co * C1 + ci) * 9 + kyx] = s;
  }
}

// conv2 dgrad as MFMA GEMM: dx1[m=(b,y,x)][ci] over K = (kyx, co).
// ONE block per (g, b) walks all 11 64-pixel tiles with EVERYTHING
// LDS-resident via global_load_lds (async DMA): the full 74 KB weight
// tensor stages once in the prologue, and the 37 KB dz region
// double-buffers so the next tile streams while the current tile's
// 288 MFMAs issue (counted-wait + raw barriers; __syncthreads or any
// ordinary global load in the loop would drain the DMA queue — guide
// T3/T4 and the §5 mixing-load-kinds trap). The region image is linear
// (glds requirement): bank spread comes from a 4-float channel
// rotation keyed on the row-col index, applied identically at the DMA
// source address and at read time; out-of-bounds taps resolve by
// operand predication instead of staged zero borders.
#define DG_RC (6 * S2)              // 144 row-cols per tile region

extern "C" __global__ __launch_bounds__(WG)
void cnn_conv2_dgrad_mfma(CnnArgs a) {
  const int gb = blockIdx.x;
  const int g = gb / a.B;
  const int b = gb - g * a.B;
  if (b >= step_n(a, g)) return;
  const int tid = threadIdx.x;
  const int wv = tid >> 6;
  const int l = tid & 63;
  const int li = l & 15, lk = l >> 4;
  // carve: sB [9*2048] then sD [2][DG_RC][64]
  extern __shared__ __attribute__((aligned(16))) float lds_[];
  float* sB = lds_;
  float* sD = lds_ + 9 * 2048;
  const float* dz = a.zz2 + ((long long)g * a.B + b) * Z2N;
  const float* wt = a.wtd + (long long)g * 9 * 2048;
  float* dx1 = a.dx1 + ((long long)g * a.B + b) * X1N;

  // prologue: the whole wtd[9][64][32] tensor -> LDS (18 glds per wave)
  {
    const int base = wv * (18 * 256);       // floats
#pragma unroll
    for (int gq = 0; gq < 18; ++gq)
      __builtin_amdgcn_global_load_lds(
          (const __attribute__((address_space(1))) unsigned int*)
              (wt + base + gq * 256 + l * 4),
          (__attribute__((address_space(3))) unsigned int*)
              (sB + base + gq * 256),
          16, 0, 0);
  }

  // each wave DMAs rows {wv, wv + 4 partial} of the 6-row region: the
  // 144 row-cols split as 36 glds (4 arows each) -> 9 per wave; invalid
  // rows load from a clamped source row and are masked at use
#define DG_ISSUE(mt, buf)                                                \
  {                                                                      \
    const int y0_ = (mt) * 64 / S1;                                      \
    _Pragma("unroll") for (int gq = 0; gq < 9; ++gq) {                   \
      const int arow0_ = (wv * 9 + gq) * 4;                              \
      const int arow_l = arow0_ + (l >> 4);                              \
      const int row_ = arow_l / S2;                                      \
      const int col_ = arow_l - row_ * S2;                               \
      int dzrow_ = y0_ - 2 + row_;  /* region = dz rows [y0-2, y0+4) */  \
      dzrow_ = dzrow_ < 0 ? 0 : (dzrow_ > S2 - 1 ? S2 - 1 : dzrow_);     \
      const int chp_ = (l & 15) * 4;                                     \
      const int chs_ = (chp_ - 4 * arow_l) & 63;                         \
      __builtin_amdgcn_global_load_lds(                                  \
          (const __attribute__((address_space(1))) unsigned int*)        \
              (dz + ((long long)dzrow_ * S2 + col_) * C2 + chs_),        \
          (__attribute__((address_space(3))) unsigned int*)              \
              (sD + (buf) * (DG_RC * 64) + arow0_ * 64),                 \
          16, 0, 0);                                                     \
    }                                                                    \
  }

  DG_ISSUE(0, 0);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  int cur = 0;
  for (int mt = 0; mt < 11; ++mt) {
    if (mt + 1 < 11) { DG_ISSUE(mt + 1, cur ^ 1); }
    const int p0 = mt * 64;
    const int y0 = p0 / S1;
    const int p = p0 + wv * 16 + li;        // this lane's x1 pixel
    const int y = p / S1, x = p - (p / S1) * S1;
    f32x4 acc[2];
    acc[0] = f32x4{0.f, 0.f, 0.f, 0.f};
    acc[1] = f32x4{0.f, 0.f, 0.f, 0.f};
    const float* base = sD + cur * (DG_RC * 64);
    for (int kyx = 0; kyx < 9; ++kyx) {
      const int ky = kyx / 3, kx = kyx - (kyx / 3) * 3;
      const float* wk = sB + kyx * 2048;
      const int oy = y - ky, ox = x - kx;
      // region = dz rows [y0-2, y0+4): every VALID tap of this tile's
      // pixels lands inside (oy in [y-2, y], y in [y0, y0+2])
      const bool ok = oy >= 0 && oy < S2 && ox >= 0 && ox < S2;
      const int arow = ok ? (oy - y0 + 2) * S2 + ox : 0;
      const int rot = 4 * arow;
      const float* rowp = base + arow * 64;
#pragma unroll
      for (int ks = 0; ks < C2 / 4; ++ks) {
        const int co = ks * 4 + lk;
        float av = rowp[(co + rot) & 63];
        av = ok ? av : 0.f;
#pragma unroll
        for (int ct = 0; ct < 2; ++ct)
          acc[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(
              av, wk[co * C1 + ct * 16 + li], acc[ct], 0, 0, 0);
      }
    }
#pragma unroll
    for (int ct = 0; ct < 2; ++ct)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int pix = p0 + wv * 16 + lk * 4 + r;
        if (pix < 676)
          dx1[(long long)pix * C1 + ct * 16 + li] = acc[ct][r];
      }
    if (mt + 1 < 11) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __builtin_amdgcn_s_barrier();
    cur ^= 1;
  }
#undef DG_ISSUE
}

// conv2 dgrad v2/v3 — the fwd-shaped decomposition: ONE block per
// (g, b, mtile), mirroring conv2_fwd_body; each wave owns MF 16-pixel
// M-fragments. The block's dz region (zero-bordered, +4-padded) stages
// once with ordinary loads and ONE barrier; the B operand (wtd, 74 KB
// per pair) reads straight from L2 inside the MFMA loop exactly like
// fwd's wtf. v1 keeps everything (weights + region) LDS-resident via
// the glds DMA pipeline, which is elegant but needs 144 KB of LDS ->
// ONE block (4 waves) per CU, and its inter-tile barrier + vmcnt waits
// run unhidden (PMC: 57% parked, profiles/pmc5_summary.json). These
// shapes fit several blocks per CU, so parked time overlaps across
// blocks.
//   MF = 1 (v2): 64-pixel tiles, 11 per sample, 6-row region (37 KB,
//                4 blocks/CU).
//   MF = 2 (v3): 128-pixel tiles, 6 per sample, 8-row region (52 KB,
//                3 blocks/CU): every weight load feeds two MFMAs (the B
//                operand is the per-MFMA global-issue cost in v2) and
//                each wave runs four independent accumulator chains.
template <int MF>
__device__ __forceinline__ void conv2_dgrad_body(const CnnArgs& a) {
  constexpr int TILES = MF == 1 ? 11 : 6;     // ceil(676 / (64 * MF))
  constexpr int ROWS = MF == 1 ? 6 : 8;
  const int mt = blockIdx.x % TILES;
  const int gb = blockIdx.x / TILES;
  const int g = gb / a.B;
  const int b = gb - g * a.B;
  if (b >= step_n(a, g)) return;
  const int tid = threadIdx.x;
  const int wv = tid >> 6;
  const int l = tid & 63;
  const int li = l & 15, lk = l >> 4;
  // row stride C2+4 = 68 === 4 (mod 32): the MFMA-loop read
  // sD[arow][ks*4+lk] with arow consecutive in li then hits bank
  // 4*li + lk -- an exact 2-way spread (the 64-lane minimum)
  __shared__ __attribute__((aligned(16))) float sD[ROWS * S2][C2 + 4];
  const float* dz = a.zz2 + ((long long)g * a.B + b) * Z2N;
  const float* wt = a.wtd + (long long)g * 9 * 2048;
  float* dx1 = a.dx1 + ((long long)g * a.B + b) * X1N;
  const int p0 = mt * (64 * MF);
  const int y0 = p0 / S1;          // first dx1 pixel row of this tile
  // region = dz rows [y0-2, y0-2+ROWS): the tile's pixels span rows
  // [y0, y0+2] (MF = 1) or [y0, y0+5] (MF = 2) and taps reach two rows
  // up, so every valid tap lands inside; rows outside [0, S2) stage as
  // zeros
  for (int e = tid; e < ROWS * S2 * C2; e += WG) {
    const int rr = e / (S2 * C2);
    const int rem = e - rr * S2 * C2;
    const int cc = rem / C2;
    const int ch = rem - cc * C2;
    const int dzrow = y0 - 2 + rr;
    sD[rr * S2 + cc][ch] =
        (dzrow >= 0 && dzrow < S2)
            ? dz[((long long)dzrow * S2 + cc) * C2 + ch] : 0.f;
  }
  __syncthreads();
  // this lane's dx1 pixels: p_a (M-fragment 0) and p_b (1); named
  // scalars, not MF-sized arrays (see conv2_fwd_body)
  const int p_a = p0 + wv * (16 * MF) + li;
  const int p_b = p_a + 16;
  const int ya = p_a / S1, xa = p_a - ya * S1;
  const int yb = p_b / S1, xb = p_b - yb * S1;
  f32x4 acc[MF][2];
#pragma unroll
  for (int mf = 0; mf < MF; ++mf)
#pragma unroll
    for (int ct = 0; ct < 2; ++ct) acc[mf][ct] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int kyx = 0; kyx < 9; ++kyx) {
    const int ky = kyx / 3, kx = kyx - (kyx / 3) * 3;
    // x borders (S1=26 > S2=24) still need operand predication; the
    // staged y borders are already zero
    const int oya = ya - ky, oxa = xa - kx;
    const bool oka = oya >= 0 && oya < S2 && oxa >= 0 && oxa < S2;
    const int ra = oka ? (oya - y0 + 2) * S2 + oxa : 0;
    bool okb = false;
    int rb = 0;
    if constexpr (MF == 2) {
      const int oyb = yb - ky, oxb = xb - kx;
      okb = oyb >= 0 && oyb < S2 && oxb >= 0 && oxb < S2;
      rb = okb ? (oyb - y0 + 2) * S2 + oxb : 0;
    }
    const float* wk = wt + kyx * 2048;
#pragma unroll
    for (int ks = 0; ks < C2 / 4; ++ks) {
      const int co = ks * 4 + lk;
      float av0 = sD[ra][co];
      av0 = oka ? av0 : 0.f;
      float av1 = 0.f;
      if constexpr (MF == 2) {
        av1 = sD[rb][co];
        av1 = okb ? av1 : 0.f;
      }
#pragma unroll
      for (int ct = 0; ct < 2; ++ct) {
        const float bv = wk[co * C1 + ct * 16 + li];
        acc[0][ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(
            av0, bv, acc[0][ct], 0, 0, 0);
        if constexpr (MF == 2)
          acc[1][ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(
              av1, bv, acc[1][ct], 0, 0, 0);
      }
    }
  }
#pragma unroll
  for (int mf = 0; mf < MF; ++mf)
#pragma unroll
    for (int ct = 0; ct < 2; ++ct)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int pix = p0 + (wv * MF + mf) * 16 + lk * 4 + r;
        if (pix < 676)
          dx1[(long long)pix * C1 + ct * 16 + li] = acc[mf][ct][r];
      }
}
extern "C" __global__ __launch_bounds__(WG)
void cnn_conv2_dgrad_mfma2(CnnArgs a) { conv2_dgrad_body<1>(a); }
extern "C" __global__ __launch_bounds__(WG)
void cnn_conv2_dgrad_mfma3(CnnArgs a) { conv2_dgrad_body<2>(a); }

// conv1 wgrad, stage 1: per-(g, b) partials into the dz2 scratch region
// (reused: dz2 is [G, B, 64] and conv1 has 288+32=320 grad entries, so
// partials use their own ws buffer c1part [G, B, 320]). Deterministic
// two-stage reduce (no atomics).
extern "C" __global__ __launch_bounds__(WG)
void cnn_conv1_wgrad_part(CnnArgs a) {
  const int g = blockIdx.x / a.B;
  const int b = blockIdx.x - g * a.B;
  if (b >= step_n(a, g)) return;
  const int tid = threadIdx.x;
  __shared__ __attribute__((aligned(16))) float xin[D_IN];
  stage_masked_input(xin, a.x + (step_o(a, g) + b) * D_IN,
                     a.x_mask ? a.x_mask + (long long)g * D_IN : nullptr);
  __syncthreads();
  const float* dx = a.dx1 + ((long long)g * a.B + b) * X1N;  // chans-last
  float* out = a.c1part + ((long long)g * a.B + b) * 320;
  for (int tap = tid; tap < 320; tap += WG) {
    float s = 0.f;
    if (tap < 288) {
      const int c = tap / 9;
      const int k = tap - c * 9;
      const int ky = k / 3, kx = k - (k / 3) * 3;
      for (int y = 0; y < S1; ++y) {
        const float* xr = xin + (y + ky) * IN_W + kx;
        const float* dr = dx + (long long)y * S1 * C1 + c;
        for (int x = 0; x < S1; ++x)
          s = fmaf(xr[x], dr[(long long)x * C1], s);
      }
    } else {
      const int c = tap - 288;
      for (int p = 0; p < S1 * S1; ++p) s += dx[(long long)p * C1 + c];
    }
    out[tap] = s;
  }
}

// conv1 wgrad, stage 2: reduce partials over the batch
extern "C" __global__ __launch_bounds__(WG)
void cnn_conv1_wgrad_reduce(CnnArgs a) {
  const long long total = (long long)a.G * 320;
  for (long long q = (long long)blockIdx.x * WG + threadIdx.x; q < total;
       q += (long long)gridDim.x * WG) {
    const int g = (int)(q / 320);
    const int tap = (int)(q - (long long)g * 320);
    const int n = step_n(a, g);
    if (n == 0) continue;
    const float* part = a.c1part + (long long)g * a.B * 320 + tap;
    float s = 0.f;
    for (int b = 0; b < n; ++b) s += part[(long long)b * 320];
    float* gr = a.grad + (long long)g * a.P;
    if (tap < 288) gr[OFF_W1C + tap] = s;
    else gr[OFF_B1C + tap - 288] = s;
  }
}

// optimizer update: vector grid-stride over (g, p/4) with a scalar
// tail. The SGD/Adam branch is hoisted OUT of the element loop and the
// state rows use alignment-4 float4s (rows are only dword-aligned at
// odd P), so the compiler emits merged dwordx4 traffic instead of the
// 28 scalar loads the per-element branch produced.
typedef float f4u __attribute__((ext_vector_type(4), aligned(4)));

// PROX (FedProx, mu != 0) adds mu * (w - w0) to the gradient, w0 the
// pair's row of the global bank. It is a template parameter, not a runtime
// test: the four anchor registers cost cnn_opt_step a wave of occupancy
// (76 VGPRs against 72), which the mu = 0 kernel does not pay.
template <bool PROX>
__device__ __forceinline__ void cnn_opt_step_body(const CnnArgs& a) {
  const float b1 = 0.9f, b2 = 0.999f, eps = 1e-8f;
  const long long pv = a.P / 4;          // float4 body; tail scalar
  const long long total = (long long)a.G * pv;
  for (long long qv = (long long)blockIdx.x * WG + threadIdx.x;
       qv < total; qv += (long long)gridDim.x * WG) {
    const int g = (int)(qv / pv);
    if (step_n(a, g) == 0) continue;
    const long long row = a.rows[g];
    const float lr_ = a.lr[row];
    const long long pp = (qv - (long long)g * pv) * 4;
    const long long q0 = (long long)g * a.P + pp;
    const bool tail = (qv - (long long)g * pv == pv - 1);
    const float* __restrict__ w0 =
        PROX ? a.anchor + (row % a.K) * (long long)a.P : nullptr;
    if (a.opt == OPT_SGD) {
      f4u wv = *(const f4u*)(a.work + q0);
      f4u gr = *(const f4u*)(a.grad + q0);
      if constexpr (PROX) {
        const f4u av = *(const f4u*)(w0 + pp);
#pragma unroll
        for (int j = 0; j < 4; ++j) gr[j] += a.mu * (wv[j] - av[j]);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) wv[j] -= lr_ * gr[j];
      *(f4u*)(a.work + q0) = wv;
      if (tail)
        for (long long q = q0 + 4; q < (long long)(g + 1) * a.P; ++q) {
          float gs = a.grad[q];
          if constexpr (PROX)
            gs += a.mu * (a.work[q] - w0[q - (long long)g * a.P]);
          a.work[q] -= lr_ * gs;
        }
      continue;
    }
    const int tnew = a.t[row] + 1;       // tick kernel commits after
    const float bc1 = 1.f - powf(b1, (float)tnew);
    const float bc2 = 1.f - powf(b2, (float)tnew);
    const long long s0 = row * a.P + pp;
    f4u wv = *(const f4u*)(a.work + q0);
    f4u gr0 = *(const f4u*)(a.grad + q0);
    if constexpr (PROX) {
      const f4u av = *(const f4u*)(w0 + pp);
#pragma unroll
      for (int j = 0; j < 4; ++j) gr0[j] += a.mu * (wv[j] - av[j]);
    }
    f4u mo = *(const f4u*)(a.m + s0);
    f4u vo = *(const f4u*)(a.v + s0);
    f4u vm = *(const f4u*)(a.vmax + s0);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float gr = gr0[j] + a.wd * wv[j];
      const float mn = b1 * mo[j] + (1.f - b1) * gr;
      const float vn = b2 * vo[j] + (1.f - b2) * gr * gr;
      mo[j] = mn;
      vo[j] = vn;
      const float v2 = fmaxf(vm[j], vn);
      vm[j] = v2;
      wv[j] -= lr_ * (mn / bc1) / (sqrtf(v2 / bc2) + eps);
    }
    *(f4u*)(a.m + s0) = mo;
    *(f4u*)(a.v + s0) = vo;
    *(f4u*)(a.vmax + s0) = vm;
    *(f4u*)(a.work + q0) = wv;
    if (tail) {
      for (long long q = q0 + 4; q < (long long)(g + 1) * a.P; ++q) {
        const long long gp = row * a.P + (q - (long long)g * a.P);
        float gs = a.grad[q];
        if constexpr (PROX)
          gs += a.mu * (a.work[q] - w0[q - (long long)g * a.P]);
        const float gr = gs + a.wd * a.work[q];
        const float mn = b1 * a.m[gp] + (1.f - b1) * gr;
        const float vn = b2 * a.v[gp] + (1.f - b2) * gr * gr;
        a.m[gp] = mn;
        a.v[gp] = vn;
        const float v2 = fmaxf(a.vmax[gp], vn);
        a.vmax[gp] = v2;
        a.work[q] -= lr_ * (mn / bc1) / (sqrtf(v2 / bc2) + eps);
      }
    }
  }
}

extern "C" __global__ __launch_bounds__(WG)
void cnn_opt_step(CnnArgs a) { cnn_opt_step_body<false>(a); }
extern "C" __global__ __launch_bounds__(WG)
void cnn_opt_step_prox(CnnArgs a) { cnn_opt_step_body<true>(a); }

extern "C" __global__ void cnn_opt_tick(CnnArgs a) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g < a.G && a.opt == OPT_ADAM && step_n(a, g) > 0)
    a.t[a.rows[g]] += 1;
}

// ---------------------------------------------------------------------------
// evaluation: conv stage (per-sample block, x1 in LDS) + fc stage
// (per-window block, amortizes the fc1 weight stream over the window)
// ---------------------------------------------------------------------------

#define EV_ACC 0
#define EV_CONF 1
#define EV_DUMP 2

struct CnnEvalArgs {
  const float* __restrict__ params;     // [M, P]
  const float* __restrict__ x;
  const float* __restrict__ x_mask;     // [W, 784] or [784] or null
  int xm_per_task;
  float* __restrict__ a2e;              // [slots, NF]
  float* __restrict__ z1e;              // [slots, NH] (fc1 output)
  float* __restrict__ z1pe;             // [slots, FC1_KS, NH] fc1 partials
  // fc1 GEMM block metadata (slots grouped by model row, <=64 per block)
  const int64_t* __restrict__ blk_row;
  const int64_t* __restrict__ blk_s0;
  const int64_t* __restrict__ blk_len;
  // per-slot metadata
  const int64_t* __restrict__ srow;     // model row per slot
  const int64_t* __restrict__ stid;     // task id per slot
  const int64_t* __restrict__ sy;       // label per slot
  const int64_t* __restrict__ soff;     // arena sample index per slot
  const int64_t* __restrict__ swin;     // window index per slot (masks)
  float* __restrict__ x1e;              // [slots, X1N] channels-last
  float* __restrict__ z2e;              // [slots, Z2N] channels-last
  const float* __restrict__ wtf_e;      // [M, 9, 32, 64] reshaped conv2 W
  long long n_slots;
  // mode EV_ACC
  double* __restrict__ correct;         // [T]
  double* __restrict__ total;
  double* __restrict__ loss;
  double* __restrict__ mse;             // or null
  // mode EV_CONF: conf [T, O, O]; mode EV_DUMP: outp [slots, O]
  double* __restrict__ conf;
  float* __restrict__ outp;
  int O, P, mode;
};

// eval conv1, block per slot -> x1e [slots, 676, 32]
extern "C" __global__ __launch_bounds__(WG)
void cnn_eval_conv1(CnnEvalArgs a) {
  const long long slot = blockIdx.x;
  if (slot >= a.n_slots) return;
  conv1_fwd_body(
      a.x + a.soff[slot] * D_IN,
      a.x_mask ? a.x_mask + (a.xm_per_task ? a.swin[slot] * D_IN : 0)
               : nullptr,
      a.params + a.srow[slot] * (long long)a.P, a.x1e + slot * X1N);
}

// eval conv2, block per (slot, ptile), per-slot model rows; 64-pixel
// tiles by default, 128-pixel under FEDDRIFT_CONV2FWD=2
template <int MF>
__device__ __forceinline__ void conv2_fwd_eval(const CnnEvalArgs& a) {
  constexpr int TILES = MF == 1 ? 9 : 5;
  const int pt = blockIdx.x % TILES;
  const long long slot = blockIdx.x / TILES;
  if (slot >= a.n_slots) return;
  const long long row = a.srow[slot];
  conv2_fwd_body<MF>(a.x1e + slot * X1N, a.wtf_e + row * (9 * 2048),
                     a.params + row * (long long)a.P + OFF_B2C,
                     a.z2e + slot * Z2N, pt);
}
extern "C" __global__ __launch_bounds__(WG)
void cnn_eval_conv2_mfma(CnnEvalArgs a) { conv2_fwd_eval<1>(a); }
extern "C" __global__ __launch_bounds__(WG)
void cnn_eval_conv2_mfma2(CnnEvalArgs a) { conv2_fwd_eval<2>(a); }

// eval maxpool, block per slot: pooled a2e assembled in LDS and stored
// in one coalesced pass (torch-flatten layout; no dropout, no argmax)
extern "C" __global__ __launch_bounds__(WG)
void cnn_eval_pool(CnnEvalArgs a) {
  const long long slot = blockIdx.x;
  if (slot >= a.n_slots) return;
  __shared__ __attribute__((aligned(16))) float sa2[NF];
  pool_rows_body<false>(a.z2e + slot * Z2N, sa2, nullptr);
  float* out = a.a2e + slot * (long long)NF;
  for (int e = threadIdx.x; e < NF; e += WG) out[e] = sa2[e];
}

// eval fc1 with the training K-split (the eval grid is otherwise tiny:
// ~4000 slots = 63 blocks for 256 CUs — per-wave PMC showed healthy 37%
// MFMA busy but only a quarter of the chip occupied): block (blk, ks)
// computes the partial z1 for up to 64 consecutive same-row slots;
// partials land in z1pe [slots, FC1_KS, NH]
extern "C" __global__ __launch_bounds__(WG)
void cnn_eval_fc1_mfma(CnnEvalArgs a) {
  const int ks = blockIdx.x % FC1_KS;
  const int blk = blockIdx.x / FC1_KS;
  const long long s0 = a.blk_s0[blk];
  fc1_tile_body(a.a2e + s0 * (long long)NF, (int)a.blk_len[blk],
                a.params + a.blk_row[blk] * (long long)a.P + OFF_W1F,
                ks * (NF / FC1_KS), (ks + 1) * (NF / FC1_KS),
                a.z1pe + (s0 * FC1_KS + ks) * (long long)NH,
                (long long)FC1_KS * NH);
}

// fold the eval fc1 K-split partials + bias, apply relu -> z1e
extern "C" __global__ __launch_bounds__(WG)
void cnn_eval_fc1_act(CnnEvalArgs a) {
  const long long total = a.n_slots * NH;
  for (long long q = (long long)blockIdx.x * WG + threadIdx.x; q < total;
       q += (long long)gridDim.x * WG) {
    const long long slot = q / NH;
    const int h = (int)(q - slot * NH);
    const float z = fc1_fold(
        a.params[a.srow[slot] * (long long)a.P + OFF_B1F + h],
        a.z1pe + slot * FC1_KS * (long long)NH + h, NH);
    a.z1e[q] = z > 0.f ? z : 0.f;
  }
}

// head: per-slot fc2 + in-graph softmax (head_softmax, ONE WAVE per
// slot) + mode tail: argmax runs as a shuffle reduction, atomic tails
// issue from lane 0.
extern "C" __global__ __launch_bounds__(WG)
void cnn_eval_head(CnnEvalArgs a) {
  const int l = threadIdx.x & 63;
  for (long long slot = (long long)blockIdx.x * (WG / 64)
                        + (threadIdx.x >> 6);
       slot < a.n_slots; slot += (long long)gridDim.x * (WG / 64)) {
    const bool live = l < a.O;
    // the model OUTPUT (in-graph softmax)
    const float s = head_softmax(a.z1e + slot * NH,
                                 a.params + a.srow[slot] * (long long)a.P,
                                 a.O, l);
    // argmax, LOWEST index on ties (the sequential scan used strict >)
    float bv = live ? s : -1e30f;
    int bi = live ? l : 64;
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
      const float ov = __shfl_xor(bv, m, 64);
      const int oi = __shfl_xor(bi, m, 64);
      if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
    }
    const int best = bi;
    const long long tsk = a.stid[slot];
    const int yi = (int)a.sy[slot];
    if (a.mode == EV_DUMP) {
      if (live) a.outp[slot * (long long)a.O + l] = s;
    } else if (a.mode == EV_CONF) {
      if (l == 0) atomicAdd(&a.conf[(tsk * a.O + yi) * a.O + best], 1.0);
    } else {
      // CE / mse on the softmax OUTPUT (double-softmax quirk)
      const float smax = wave_max(live ? s : -1e30f);
      const float ssum = wave_sum(live ? __expf(s - smax) : 0.f);
      const float lse = logf(ssum) + smax;
      const float syi = __shfl(s, yi, 64);
      if (l == 0) {
        atomicAdd(&a.correct[tsk], (double)((best == yi) ? 1.f : 0.f));
        atomicAdd(&a.total[tsk], 1.0);
        atomicAdd(&a.loss[tsk], (double)(lse - syi));
        if (a.mse) {
          const float pt = __expf(syi - lse);
          atomicAdd(&a.mse[tsk], (double)((1.f - pt) * (1.f - pt)));
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------

// conv2 fwd/eval variant: 64-pixel tiles (1) vs 128-pixel shared-load
// tiles (2); FEDDRIFT_CONV2FWD overrides
static bool fwd_v2() {
  static const int v = [] {
    const char* e = getenv("FEDDRIFT_CONV2FWD");
    return e ? atoi(e) : 1;
  }();
  return v == 2;
}

static int grid_for(long long total) {
  long long b = (total + WG - 1) / WG;
  if (b > 16384) b = 16384;          // grid-stride beyond
  return (int)(b < 1 ? 1 : b);
}

// Launch macros of the two host functions below. They capture two
// locals of the function they are used in: `s`, the current HIP stream,
// and `a`, its kernel-argument struct (CnnArgs in cnn_train_epoch_impl,
// CnnEvalArgs in cnn_eval). LB takes an explicit block count, L sizes a
// grid-stride grid from a thread total; both launch WG threads per block.
#define LB(kern, blocks) \
  hipLaunchKernelGGL(kern, dim3((int)(blocks)), dim3(WG), 0, s, a)
#define L(kern, total) LB(kern, grid_for(total))

void cnn_train_epoch_impl(
    torch::Tensor work, torch::Tensor grad, torch::Tensor rows,
    torch::Tensor x, torch::Tensor y,
    torch::Tensor step_off, torch::Tensor step_len, int64_t e,
    c10::optional<torch::Tensor> x_mask,
    torch::Tensor ws_x1, torch::Tensor ws_a2, torch::Tensor ws_pidx,
    torch::Tensor ws_z1, torch::Tensor ws_a1, torch::Tensor ws_dz2,
    torch::Tensor ws_dz1, torch::Tensor ws_da2, torch::Tensor ws_zz2,
    torch::Tensor ws_dx1, torch::Tensor ws_c1part, torch::Tensor ws_wtf,
    torch::Tensor ws_wtd, torch::Tensor ws_z1part, torch::Tensor ws_w2part,
    torch::Tensor ws_b2part,
    c10::optional<torch::Tensor> m, c10::optional<torch::Tensor> v,
    c10::optional<torch::Tensor> vmax, c10::optional<torch::Tensor> t,
    torch::Tensor lr, double wd, double p1, double p2,
    int64_t seed, int64_t g0, int64_t B, int64_t O, int64_t w2ms,
    double mu, c10::optional<torch::Tensor> anchor) {
  const int G = rows.size(0);
  if (G == 0) return;
  TORCH_CHECK(mu >= 0.0 && std::isfinite(mu),
              "cnn_train_epoch: fedprox mu=", mu,
              " must be finite and >= 0");
  CnnArgs a;
  a.mu = (float)mu;
  a.anchor = nullptr;
  a.K = 1;
  if (a.mu != 0.f) {
    TORCH_CHECK(anchor.has_value() && anchor->is_cuda() &&
                anchor->dtype() == torch::kFloat32 &&
                anchor->is_contiguous() && anchor->dim() == 2 &&
                anchor->size(1) == work.size(1) && anchor->size(0) >= 1,
                "cnn_train_epoch: fedprox needs the contiguous f32 [K, P] "
                "global bank as anchor");
    a.anchor = anchor->data_ptr<float>();
    a.K = (int)anchor->size(0);
  }
  a.work = work.data_ptr<float>();
  a.grad = grad.data_ptr<float>();
  a.rows = rows.data_ptr<int64_t>();
  a.x = x.data_ptr<float>();
  a.y = y.data_ptr<int64_t>();
  a.step_off = step_off.data_ptr<int64_t>();
  a.step_len = step_len.data_ptr<int64_t>();
  a.x_mask = x_mask.has_value() ? x_mask->data_ptr<float>() : nullptr;
  a.x1 = ws_x1.data_ptr<float>();
  a.a2 = ws_a2.data_ptr<float>();
  a.pidx = ws_pidx.data_ptr<unsigned char>();
  a.z1 = ws_z1.data_ptr<float>();
  a.a1 = ws_a1.data_ptr<float>();
  a.dz2 = ws_dz2.data_ptr<float>();
  a.dz1 = ws_dz1.data_ptr<float>();
  a.da2 = ws_da2.data_ptr<float>();
  a.zz2 = ws_zz2.data_ptr<float>();
  a.dx1 = ws_dx1.data_ptr<float>();
  a.c1part = ws_c1part.data_ptr<float>();
  a.wtf = ws_wtf.data_ptr<float>();
  a.wtd = ws_wtd.data_ptr<float>();
  a.z1part = ws_z1part.data_ptr<float>();
  a.w2part = ws_w2part.data_ptr<float>();
  a.b2part = ws_b2part.data_ptr<float>();
  const bool adam = m.has_value();
  a.m = adam ? m->data_ptr<float>() : nullptr;
  a.v = adam ? v->data_ptr<float>() : nullptr;
  a.vmax = adam ? vmax->data_ptr<float>() : nullptr;
  a.t = adam ? t->data_ptr<int>() : nullptr;
  a.lr = lr.data_ptr<float>();
  a.wd = (float)wd;
  a.p1 = (float)p1;
  a.p2 = (float)p2;
  a.seed = (unsigned long long)seed;
  a.g0 = g0;
  a.G = G;
  a.B = (int)B;
  a.E = (int)step_off.size(1);
  a.e = (int)e;
  a.O = (int)O;
  a.P = (int)work.size(1);
  a.opt = adam ? OPT_ADAM : OPT_SGD;
  a.w2ms = (int)w2ms;

  auto s = c10::hip::getCurrentHIPStream();
  const long long GB = (long long)G * B;
  const int mtiles = (a.B + 63) / 64;
  // forward
  L(cnn_w2_reshape, (long long)G * C2 * C1 * 9);
  LB(cnn_conv1_fwd, GB);
  if (fwd_v2())
    LB(cnn_conv2_fwd_mfma2, GB * 5);
  else
    LB(cnn_conv2_fwd_mfma, GB * 9);
  LB(cnn_pool_fwd, GB);
  LB(cnn_fc1_fwd_mfma, G * mtiles * FC1_KS);
  L(cnn_fc1_act, GB * NH);
  L(cnn_head_fwd, GB * 64);   // one wave per sample
  // backward
  L(cnn_fc2_wgrad, (long long)G * O * NH);
  L(cnn_fc2_dgrad, GB * NH);
  LB(cnn_fc1_wgrad, G * (NF / 128));
  L(cnn_fc1_bias_grad, (long long)G * NH);
  LB(cnn_fc1_dgrad, G * mtiles * (NF / 128));
  LB(cnn_pool_bwd, GB);
  LB(cnn_conv2_wgrad_mfma, G * a.w2ms);
  L(cnn_conv2_wgrad_reduce, (long long)G * (9 * 2048 + C2));
  // dgrad variant switch, A/B-measured at both ends of the fleet-size
  // axis (FEDDRIFT_DGRAD=1|2|3 forces one): v3 (128-pixel tiles, every
  // weight load shared by two M-fragments, 4 MFMA chains/wave) matches
  // v2 at small fleets (config-3 train 8.0 ms/round both) and beats
  // both the fwd-shaped v2 (5.97) and the all-LDS glds pipeline v1
  // (5.6-5.7) at 3400-client scale: 5.2 s/round -> default everywhere.
  static const int dgrad_env = [] {
    const char* e = getenv("FEDDRIFT_DGRAD");
    return e ? atoi(e) : 0;
  }();
  const int dgrad_v = dgrad_env ? dgrad_env : 3;
  if (dgrad_v == 1)
    hipLaunchKernelGGL(cnn_conv2_dgrad_mfma, dim3((int)GB), dim3(WG),
                       (9 * 2048 + 2 * DG_RC * 64) * sizeof(float), s, a);
  else if (dgrad_v == 3)
    LB(cnn_conv2_dgrad_mfma3, GB * 6);
  else
    LB(cnn_conv2_dgrad_mfma2, GB * 11);
  LB(cnn_conv1_wgrad_part, GB);
  L(cnn_conv1_wgrad_reduce, (long long)G * 320);
  // optimizer
  if (a.mu != 0.f)
    L(cnn_opt_step_prox, (long long)G * a.P);
  else
    L(cnn_opt_step, (long long)G * a.P);
  LB(cnn_opt_tick, (G + WG - 1) / WG);
  TORCH_CHECK(hipGetLastError() == hipSuccess, "cnn_train_epoch launch");
}

torch::Tensor cnn_eval(
    torch::Tensor params, torch::Tensor x, torch::Tensor a2e,
    torch::Tensor z1e, torch::Tensor z1pe,
    torch::Tensor x1e, torch::Tensor z2e, torch::Tensor wtf_e,
    torch::Tensor blk_row, torch::Tensor blk_s0, torch::Tensor blk_len,
    torch::Tensor srow, torch::Tensor stid, torch::Tensor sy,
    torch::Tensor soff, torch::Tensor swin,
    c10::optional<torch::Tensor> x_mask, int64_t n_tasks, int64_t O,
    int64_t mode, bool want_mse, int64_t n_slots,
    c10::optional<torch::Tensor> outp) {
  auto optd = torch::TensorOptions().dtype(torch::kFloat64)
                  .device(params.device());
  torch::Tensor out;
  if (mode == EV_ACC)
    out = torch::zeros({want_mse ? 4 : 3, n_tasks}, optd);
  else if (mode == EV_CONF)
    out = torch::zeros({n_tasks, O, O}, optd);
  else
    out = torch::zeros({0}, optd);
  if (n_slots == 0) return out;

  CnnEvalArgs a;
  a.params = params.data_ptr<float>();
  a.x = x.data_ptr<float>();
  a.x_mask = x_mask.has_value() ? x_mask->data_ptr<float>() : nullptr;
  a.xm_per_task = x_mask.has_value() && x_mask->dim() == 2 ? 1 : 0;
  a.a2e = a2e.data_ptr<float>();
  a.z1e = z1e.data_ptr<float>();
  a.z1pe = z1pe.data_ptr<float>();
  a.blk_row = blk_row.data_ptr<int64_t>();
  a.blk_s0 = blk_s0.data_ptr<int64_t>();
  a.blk_len = blk_len.data_ptr<int64_t>();
  a.srow = srow.data_ptr<int64_t>();
  a.stid = stid.data_ptr<int64_t>();
  a.sy = sy.data_ptr<int64_t>();
  a.soff = soff.data_ptr<int64_t>();
  a.swin = swin.data_ptr<int64_t>();
  a.x1e = x1e.data_ptr<float>();
  a.z2e = z2e.data_ptr<float>();
  a.wtf_e = wtf_e.data_ptr<float>();
  a.n_slots = (long long)n_slots;
  double* base = (mode == EV_ACC) ? out.data_ptr<double>() : nullptr;
  a.correct = base;
  a.total = base ? base + n_tasks : nullptr;
  a.loss = base ? base + 2 * n_tasks : nullptr;
  a.mse = (base && want_mse) ? base + 3 * n_tasks : nullptr;
  a.conf = (mode == EV_CONF) ? out.data_ptr<double>() : nullptr;
  a.outp = outp.has_value() ? outp->data_ptr<float>() : nullptr;
  a.O = (int)O;
  a.P = (int)params.size(1);
  a.mode = (int)mode;

  auto s = c10::hip::getCurrentHIPStream();
  LB(cnn_eval_conv1, n_slots);
  if (fwd_v2())
    LB(cnn_eval_conv2_mfma2, n_slots * 5);
  else
    LB(cnn_eval_conv2_mfma, n_slots * 9);
  LB(cnn_eval_pool, n_slots);
  LB(cnn_eval_fc1_mfma, blk_row.size(0) * FC1_KS);
  L(cnn_eval_fc1_act, n_slots * NH);
  L(cnn_eval_head, n_slots * 64);   // one wave per slot
  TORCH_CHECK(hipGetLastError() == hipSuccess, "cnn_eval launch");
  return out;
}
#undef L
#undef LB

void register_cnn(pybind11::module_& mod) {
  mod.def("cnn_train_epoch", &cnn_train_epoch_impl,
          "one fused CNN training epoch over all (client, model) pairs");
  mod.def("cnn_eval", &cnn_eval, "batched CNN eval sweep (acc/conf/dump)");
  // geometry and mode constants the Python engine sizes its buffers by
  mod.attr("X1N") = X1N;
  mod.attr("Z2N") = Z2N;
  mod.attr("NF") = NF;
  mod.attr("NH") = NH;
  mod.attr("D_IN") = D_IN;
  mod.attr("FC1_KS") = FC1_KS;
  mod.attr("EV_ACC") = EV_ACC;
  mod.attr("EV_CONF") = EV_CONF;
  mod.attr("EV_DUMP") = EV_DUMP;
}
