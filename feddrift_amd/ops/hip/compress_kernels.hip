// Top-k upload sparsification with error feedback (upload_compress = topk)
// for gfx950: per (replica row, model) pair, the k coordinates of largest
// magnitude of a = (theta - g) + e travel, the rest stays in the residual e.
//
// Row kernels, rows of at most CP_ROW_MAX coordinates:
// compress_wave_kernel    P <= CP_WAVE_MAX (the SEA rows): one wave per pair,
//                         four pairs per block, a in registers. tau, the k-th
//                         largest magnitude key, by bisection on the 31 key
//                         bits; a pass counts with ballot + popcount, so the
//                         kernel has no LDS and no barrier.
// compress_block_kernel   one block per pair, a staged once in LDS, the same
//                         bisection with the four wave counts combined
//                         through LDS (one barrier per pass).
//
// Long path, several blocks per row (a block covers CP_CHUNK coordinates),
// rows in slabs of at most `slab` pairs so the histogram scratch is bounded:
// compress_hist_kernel    MSB-first radix over the key, 11 + 10 + 10 bits:
//                         a block histograms the digit of the keys that match
//                         the prefix found so far in LDS and merges it into
//                         the row's global histogram with integer atomics
//                         (order-independent). Pass 0 forms a and, with error
//                         feedback, parks it in the residual row, so passes 1,
//                         2 and the write pass read one array.
// compress_pick_kernel    one block per row: walks the histogram from the top
//                         bin, fixes the next digit of tau, leaves the count
//                         still wanted inside that bin, clears the bins.
// compress_write_kernel   writes the replica and the residual.
//
// Stochastic quantisation (upload_compress = quant, topk_quant): quant_*
// kernels beside the ones above, sharing their bisection and radix bodies.
// The row kernels add the row's scale S, the largest finite key, by a u32
// wave shuffle (+ LDS) max, and quantise in the emit step; a lane draws a
// whole Philox block for its coordinate. On the long path pass 0 of the
// histogram kernel (topk_quant) or quant_form_kernel (quant) folds the finite
// keys into smax[slab] with integer atomicMax, and quant_write_kernel gives
// every thread four consecutive coordinates, one Philox block.
//
// a and the outputs are formed with __fsub_rn / __fadd_rn (no contraction).
// No float atomics. The sent counts take one 64-bit integer atomic per pair
// (row kernels) or per block (long path).
//
// The specification is comm/compress.py.
#include <hip/hip_runtime.h>
#include <torch/extension.h>
#include <c10/hip/HIPStream.h>

constexpr int CP_THREADS = 256;
constexpr int CP_WAVE = 64;
constexpr int CP_WAVES = CP_THREADS / CP_WAVE;
constexpr int CP_WAVE_ELEMS = 4;                       // per lane
constexpr int CP_WAVE_MAX = CP_WAVE * CP_WAVE_ELEMS;   // 256
constexpr int CP_ROW_MAX = 8192;                       // 32 KiB of LDS
constexpr int CP_ITEMS = 16;
constexpr int CP_CHUNK = CP_THREADS * CP_ITEMS;        // 4096 per block
constexpr int CP_BINS0 = 2048;                         // bits 30..20
constexpr int CP_BINS = 1024;                          // bits 19..10, 9..0
constexpr int CP_SLAB_ROWS = 1024;                     // 8 MiB of histograms

typedef unsigned int u32;
typedef unsigned long long u64;

struct CompressArgs {
  float* replicas;           // [R, P]
  const float* global;       // [K, P]
  float* resid;              // [R, P] or null (no error feedback)
  const long long* rows;     // [U] replica row of every pair
  const int* models;         // [U]
  u64* counts;               // [K, 2]; slot 0 takes the sent coordinates
  long long P;
  long long U;
  int k;
  // long path
  u32* hist;                 // [slab, CP_BINS0]
  u32* tau;                  // [slab]
  u32* krem;                 // [slab]
  long long u0;              // first pair of the slab
};

static __device__ __forceinline__ u32 cp_key(float a) {
  return __float_as_uint(a) & 0x7fffffffu;
}

static __device__ __forceinline__ float cp_form(float th, float g,
                                                const float* e, long long j) {
  const float d = __fsub_rn(th, g);
  return e ? __fadd_rn(d, e[j]) : d;
}

// returns whether the coordinate was sent
static __device__ __forceinline__ bool cp_emit(float a, u32 tau, float g,
                                               float* th, float* e,
                                               long long j) {
  const u32 key = cp_key(a);
  const bool sent = key >= tau && key > 0u;
  th[j] = sent ? __fadd_rn(g, a) : g;
  if (e) e[j] = (sent || key >= 0x7f800000u) ? 0.f : a;
  return sent;
}

// tau = the largest t with count(key >= t) >= k, keys in a wave's registers
static __device__ __forceinline__ u32 cp_wave_tau(
    const u32 (&key)[CP_WAVE_ELEMS], int P, int k) {
  u32 tau = 0u;
  for (int b = 30; b >= 0; --b) {
    const u32 t = tau | (1u << b);
    int c = 0;
#pragma unroll
    for (int i = 0; i < CP_WAVE_ELEMS; ++i)
      if (CP_WAVE * i < P) c += __popcll(__ballot(key[i] >= t));
    if (c >= k) tau = t;
  }
  return tau;
}

// the same over a row staged in LDS by the whole block; leaves cnt[0] as
// the last buffer written
static __device__ __forceinline__ u32 cp_block_tau(
    const float* sa, int (*cnt)[CP_WAVES], int P, int k) {
  const int tid = threadIdx.x;
  const int lane = tid & (CP_WAVE - 1), wave = tid / CP_WAVE;
  u32 tau = 0u;
  for (int b = 30; b >= 0; --b) {
    const u32 t = tau | (1u << b);
    int c = 0;
    for (int j0 = 0; j0 < P; j0 += CP_THREADS) {
      const int j = j0 + tid;
      c += __popcll(__ballot(j < P && cp_key(sa[j < P ? j : 0]) >= t));
    }
    // the buffers alternate, so one barrier per pass is enough
    if (lane == 0) cnt[b & 1][wave] = c;
    __syncthreads();
    int tot = 0;
#pragma unroll
    for (int w = 0; w < CP_WAVES; ++w) tot += cnt[b & 1][w];
    if (tot >= k) tau = t;
  }
  return tau;
}

// ---- stochastic quantisation ------------------------------------------------

struct QuantArgs {
  CompressArgs c;            // c.k = 0: quant, every non-zero travels
  const int* workers;        // [U] global worker id of every pair
  u32* smax;                 // [slab] largest finite key (long path)
  u32 key0, key1, ctr;       // Philox key halves, compress-pass counter
  float L;                   // 2^(bits - 1) - 1 magnitude levels
};

// Philox4x32-10, the layout of comm/secure_agg.py:philox4x32
static __device__ __forceinline__ void cp_philox(u32 c0, u32 c1, u32 c2,
                                                 u32 c3, u32 k0, u32 k1,
                                                 u32* x) {
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

// max over the wave, integers: no float compare, no order
static __device__ __forceinline__ u32 cp_wave_max(u32 v) {
#pragma unroll
  for (int off = CP_WAVE / 2; off; off >>= 1) {
    const u32 o = (u32)__shfl_xor((int)v, off, CP_WAVE);
    v = o > v ? o : v;
  }
  return v;
}

static __device__ __forceinline__ u32 cp_finite_key(u32 key) {
  return key < 0x7f800000u ? key : 0u;
}

// Writes the coordinate; x is its Philox word, s the row's scale. Returns
// whether the replica value was written from g + ... . The products feed
// adds, so contraction is switched off for the whole body.
static __device__ __forceinline__ bool cp_emit_quant(float a, u32 tau, float s,
                                                     float L, u32 x, float g,
                                                     float* th, float* e,
                                                     long long j) {
#pragma clang fp contract(off)
  const u32 key = cp_key(a);
  const bool travel = key >= tau && key > 0u;
  const bool finite = key < 0x7f800000u;
  float out = g, res = finite ? a : 0.f;
  bool written = false;
  if (travel) {
    if (finite) {
      // u = (x >> 8) 2^-24: 24 bits, exact
      const float u = __fmul_rn((float)(x >> 8), 5.9604644775390625e-08f);
      const float xj = __fmul_rn(__fdiv_rn(fabsf(a), s), L);
      const float q = fminf(L, floorf(__fadd_rn(xj, u)));
      const float v = copysignf(__fmul_rn(__fdiv_rn(q, L), s), a);
      written = q > 0.f;
      if (written) out = __fadd_rn(g, v);
      res = __fsub_rn(a, v);
    } else {
      out = __fadd_rn(g, a);
      res = 0.f;
      written = true;
    }
  }
  th[j] = out;
  if (e) e[j] = res;
  return written;
}

extern "C" __global__ __launch_bounds__(CP_THREADS)
void compress_wave_kernel(CompressArgs a) {
  const int lane = threadIdx.x & (CP_WAVE - 1);
  const long long u =
      (long long)blockIdx.x * CP_WAVES + (threadIdx.x / CP_WAVE);
  if (u >= a.U) return;                          // the whole wave leaves
  const int P = (int)a.P;
  const int m = a.models[u];
  const long long base = a.rows[u] * a.P;
  float* th = a.replicas + base;
  float* e = a.resid ? a.resid + base : nullptr;
  const float* g = a.global + (long long)m * a.P;

  float av[CP_WAVE_ELEMS], gv[CP_WAVE_ELEMS];
  u32 key[CP_WAVE_ELEMS];
#pragma unroll
  for (int i = 0; i < CP_WAVE_ELEMS; ++i) {
    const int j = lane + CP_WAVE * i;
    av[i] = 0.f; gv[i] = 0.f;
    if (j < P) {
      gv[i] = g[j];
      av[i] = cp_form(th[j], gv[i], e, j);
    }
    key[i] = cp_key(av[i]);                      // 0 past the end: never >= t
  }
  const u32 tau = cp_wave_tau(key, P, a.k);
  int sent = 0;
#pragma unroll
  for (int i = 0; i < CP_WAVE_ELEMS; ++i) {
    const int j = lane + CP_WAVE * i;
    bool s = false;
    if (j < P) s = cp_emit(av[i], tau, gv[i], th, e, j);
    sent += __popcll(__ballot(s));
  }
  if (lane == 0 && sent) atomicAdd(a.counts + 2 * m, (u64)sent);
}

extern "C" __global__ __launch_bounds__(CP_THREADS)
void compress_block_kernel(CompressArgs a) {
  __shared__ float sa[CP_ROW_MAX];
  __shared__ int cnt[2][CP_WAVES];
  const int tid = threadIdx.x;
  const int lane = tid & (CP_WAVE - 1), wave = tid / CP_WAVE;
  const long long u = blockIdx.x;
  const int P = (int)a.P;                        // <= CP_ROW_MAX
  const int m = a.models[u];
  const long long base = a.rows[u] * a.P;
  float* th = a.replicas + base;
  float* e = a.resid ? a.resid + base : nullptr;
  const float* g = a.global + (long long)m * a.P;

  for (int j = tid; j < P; j += CP_THREADS) sa[j] = cp_form(th[j], g[j], e, j);
  __syncthreads();

  const u32 tau = cp_block_tau(sa, cnt, P, a.k);
  int sent = 0;
  for (int j0 = 0; j0 < P; j0 += CP_THREADS) {
    const int j = j0 + tid;
    bool s = false;
    if (j < P) s = cp_emit(sa[j], tau, g[j], th, e, j);
    sent += __popcll(__ballot(s));
  }
  if (lane == 0) cnt[1][wave] = sent;            // pass 0 used cnt[0]
  __syncthreads();
  if (tid == 0) {
    int tot = 0;
#pragma unroll
    for (int w = 0; w < CP_WAVES; ++w) tot += cnt[1][w];
    if (tot) atomicAdd(a.counts + 2 * m, (u64)tot);
  }
}

extern "C" __global__ __launch_bounds__(CP_THREADS)
void quant_wave_kernel(QuantArgs q) {
  const CompressArgs& a = q.c;
  const int lane = threadIdx.x & (CP_WAVE - 1);
  const long long u =
      (long long)blockIdx.x * CP_WAVES + (threadIdx.x / CP_WAVE);
  if (u >= a.U) return;                          // the whole wave leaves
  const int P = (int)a.P;
  const int m = a.models[u];
  const u32 w = (u32)q.workers[u];
  const long long base = a.rows[u] * a.P;
  float* th = a.replicas + base;
  float* e = a.resid ? a.resid + base : nullptr;
  const float* g = a.global + (long long)m * a.P;

  float av[CP_WAVE_ELEMS], gv[CP_WAVE_ELEMS];
  u32 key[CP_WAVE_ELEMS];
  u32 top = 0u;
#pragma unroll
  for (int i = 0; i < CP_WAVE_ELEMS; ++i) {
    const int j = lane + CP_WAVE * i;
    av[i] = 0.f; gv[i] = 0.f;
    if (j < P) {
      gv[i] = g[j];
      av[i] = cp_form(th[j], gv[i], e, j);
    }
    key[i] = cp_key(av[i]);
    const u32 f = cp_finite_key(key[i]);
    top = f > top ? f : top;
  }
  const float s = __uint_as_float(cp_wave_max(top));
  const u32 tau = a.k ? cp_wave_tau(key, P, a.k) : 0u;
  int sent = 0;
#pragma unroll
  for (int i = 0; i < CP_WAVE_ELEMS; ++i) {
    const int j = lane + CP_WAVE * i;
    bool wr = false;
    if (j < P) {
      u32 x[4];
      cp_philox((u32)(j >> 2), w, (u32)m, q.ctr, q.key0, q.key1, x);
      const int r = j & 3;
      const u32 xs = r == 0 ? x[0] : (r == 1 ? x[1] : (r == 2 ? x[2] : x[3]));
      wr = cp_emit_quant(av[i], tau, s, q.L, xs, gv[i], th, e, j);
    }
    sent += __popcll(__ballot(wr));
  }
  if (lane == 0 && sent) atomicAdd(a.counts + 2 * m, (u64)sent);
}

extern "C" __global__ __launch_bounds__(CP_THREADS)
void quant_block_kernel(QuantArgs q) {
  __shared__ float sa[CP_ROW_MAX];
  __shared__ int cnt[2][CP_WAVES];
  __shared__ u32 smx[CP_WAVES];
  const CompressArgs& a = q.c;
  const int tid = threadIdx.x;
  const int lane = tid & (CP_WAVE - 1), wave = tid / CP_WAVE;
  const long long u = blockIdx.x;
  const int P = (int)a.P;                        // <= CP_ROW_MAX
  const int m = a.models[u];
  const u32 w = (u32)q.workers[u];
  const long long base = a.rows[u] * a.P;
  float* th = a.replicas + base;
  float* e = a.resid ? a.resid + base : nullptr;
  const float* g = a.global + (long long)m * a.P;

  u32 top = 0u;
  for (int j = tid; j < P; j += CP_THREADS) {
    const float av = cp_form(th[j], g[j], e, j);
    sa[j] = av;
    const u32 f = cp_finite_key(cp_key(av));
    top = f > top ? f : top;
  }
  top = cp_wave_max(top);
  if (lane == 0) smx[wave] = top;
  __syncthreads();
#pragma unroll
  for (int v = 0; v < CP_WAVES; ++v) top = smx[v] > top ? smx[v] : top;
  const float s = __uint_as_float(top);

  const u32 tau = a.k ? cp_block_tau(sa, cnt, P, a.k) : 0u;
  int sent = 0;
  for (int j0 = 0; j0 < P; j0 += CP_THREADS) {
    const int j = j0 + tid;
    bool wr = false;
    if (j < P) {
      u32 x[4];
      cp_philox((u32)(j >> 2), w, (u32)m, q.ctr, q.key0, q.key1, x);
      const int r = j & 3;
      const u32 xs = r == 0 ? x[0] : (r == 1 ? x[1] : (r == 2 ? x[2] : x[3]));
      wr = cp_emit_quant(sa[j], tau, s, q.L, xs, g[j], th, e, j);
    }
    sent += __popcll(__ballot(wr));
  }
  if (lane == 0) cnt[1][wave] = sent;            // pass 0 used cnt[0]
  __syncthreads();
  if (tid == 0) {
    int tot = 0;
#pragma unroll
    for (int v = 0; v < CP_WAVES; ++v) tot += cnt[1][v];
    if (tot) atomicAdd(a.counts + 2 * m, (u64)tot);
  }
}

// pass 0: digit = key bits 30..20; pass 1: bits 19..10 of the keys whose
// bits 30..20 match tau; pass 2: bits 9..0 of those whose bits 30..10 match
// HIST: the radix histogram; QMAX: pass 0 also folds the finite keys into
// smax[s] (one LDS and one global integer atomicMax per wave / block)
template <bool HIST, bool QMAX>
static __device__ __forceinline__ void cp_hist_body(const CompressArgs& a,
                                                    int pass, u32* smax) {
  __shared__ u32 h[HIST ? CP_BINS0 : 1];
  __shared__ u32 bmax;
  const int tid = threadIdx.x;
  const int s = blockIdx.y;
  const long long u = a.u0 + s;
  const int bins = pass == 0 ? CP_BINS0 : CP_BINS;
  if (HIST)
    for (int b = tid; b < bins; b += CP_THREADS) h[b] = 0u;
  if (QMAX && tid == 0) bmax = 0u;
  u32 top = 0u;
  __syncthreads();
  const int m = a.models[u];
  const long long base = a.rows[u] * a.P;
  float* th = a.replicas + base;
  float* e = a.resid ? a.resid + base : nullptr;
  const float* g = a.global + (long long)m * a.P;
  const int shift = pass == 0 ? 20 : (pass == 1 ? 10 : 0);
  const int fixed = pass == 1 ? 20 : 10;         // low bits not fixed yet
  const u32 want = (HIST && pass) ? (a.tau[s] >> fixed) : 0u;
  const long long j0 = (long long)blockIdx.x * CP_CHUNK + tid;
#pragma unroll 4
  for (int i = 0; i < CP_ITEMS; ++i) {
    const long long j = j0 + (long long)i * CP_THREADS;
    if (j >= a.P) break;
    float av;
    if (pass == 0) {
      av = cp_form(th[j], g[j], e, j);
      if (e) e[j] = av;
    } else {
      av = e ? e[j] : __fsub_rn(th[j], g[j]);
    }
    const u32 key = cp_key(av);
    if (QMAX && pass == 0) {
      const u32 f = cp_finite_key(key);
      top = f > top ? f : top;
    }
    if (HIST) {
      if (pass == 0) atomicAdd(&h[key >> 20], 1u);
      else if ((key >> fixed) == want)
        atomicAdd(&h[(key >> shift) & 1023u], 1u);
    }
  }
  if (QMAX && pass == 0) {
    top = cp_wave_max(top);
    if ((tid & (CP_WAVE - 1)) == 0 && top) atomicMax(&bmax, top);
  }
  __syncthreads();
  if (QMAX && pass == 0 && tid == 0 && bmax) atomicMax(smax + s, bmax);
  if (HIST) {
    u32* gh = a.hist + (long long)s * CP_BINS0;
    for (int b = tid; b < bins; b += CP_THREADS)
      if (h[b]) atomicAdd(gh + b, h[b]);
  }
}

extern "C" __global__ __launch_bounds__(CP_THREADS)
void compress_hist_kernel(CompressArgs a, int pass) {
  cp_hist_body<true, false>(a, pass, nullptr);
}

// topk_quant: the same passes; pass 0 also takes the row's scale
extern "C" __global__ __launch_bounds__(CP_THREADS)
void quant_hist_kernel(CompressArgs a, int pass, u32* smax) {
  cp_hist_body<true, true>(a, pass, smax);
}

// quant: forms a, parks it in the residual row, takes the row's scale
extern "C" __global__ __launch_bounds__(CP_THREADS)
void quant_form_kernel(CompressArgs a, u32* smax) {
  cp_hist_body<false, true>(a, 0, smax);
}

// Thread t owns the `per` bins below bins - t * per, walked downwards. The
// one thread whose range holds the wanted rank fixes the digit.
extern "C" __global__ __launch_bounds__(CP_THREADS)
void compress_pick_kernel(CompressArgs a, int pass) {
  __shared__ u32 part[CP_THREADS];
  const int tid = threadIdx.x;
  const int s = blockIdx.x;
  const int bins = pass == 0 ? CP_BINS0 : CP_BINS;
  const int per = bins / CP_THREADS;             // 8 or 4
  const int shift = pass == 0 ? 20 : (pass == 1 ? 10 : 0);
  u32* gh = a.hist + (long long)s * CP_BINS0;
  u32 loc[CP_BINS0 / CP_THREADS];
  u32 sum = 0u;
#pragma unroll
  for (int i = 0; i < CP_BINS0 / CP_THREADS; ++i) {
    loc[i] = 0u;
    if (i < per) {
      const int bin = bins - 1 - (tid * per + i);
      loc[i] = gh[bin];
      gh[bin] = 0u;                              // clean for the next pass
      sum += loc[i];
    }
  }
  part[tid] = sum;
  __syncthreads();
  u32 above = 0u;
  for (int i = 0; i < tid; ++i) above += part[i];
  const u32 need = pass == 0 ? (u32)a.k : a.krem[s];
  if (above < need && need <= above + sum) {
#pragma unroll
    for (int i = 0; i < CP_BINS0 / CP_THREADS; ++i) {
      if (i < per) {
        if (need <= above + loc[i]) {
          const u32 bin = (u32)(bins - 1 - (tid * per + i));
          a.tau[s] = (pass ? a.tau[s] : 0u) | (bin << shift);
          a.krem[s] = need - above;
          break;
        }
        above += loc[i];
      }
    }
  }
}

extern "C" __global__ __launch_bounds__(CP_THREADS)
void compress_write_kernel(CompressArgs a) {
  __shared__ int cnt[CP_WAVES];
  const int tid = threadIdx.x;
  const int lane = tid & (CP_WAVE - 1), wave = tid / CP_WAVE;
  const int s = blockIdx.y;
  const long long u = a.u0 + s;
  const int m = a.models[u];
  const long long base = a.rows[u] * a.P;
  float* th = a.replicas + base;
  float* e = a.resid ? a.resid + base : nullptr;
  const float* g = a.global + (long long)m * a.P;
  const u32 tau = a.tau[s];
  const long long j0 = (long long)blockIdx.x * CP_CHUNK + tid;
  int sent = 0;
#pragma unroll 4
  for (int i = 0; i < CP_ITEMS; ++i) {
    const long long j = j0 + (long long)i * CP_THREADS;
    bool snt = false;
    if (j < a.P) {
      const float gj = g[j];
      const float av = e ? e[j] : __fsub_rn(th[j], gj);
      snt = cp_emit(av, tau, gj, th, e, j);
    }
    sent += __popcll(__ballot(snt));
  }
  if (lane == 0) cnt[wave] = sent;
  __syncthreads();
  if (tid == 0) {
    int tot = 0;
#pragma unroll
    for (int w = 0; w < CP_WAVES; ++w) tot += cnt[w];
    if (tot) atomicAdd(a.counts + 2 * m, (u64)tot);
  }
}

// Thread t of a block takes the four consecutive coordinates of Philox
// block (chunk start) / 4 + i * CP_THREADS + t, i < CP_ITEMS / 4.
extern "C" __global__ __launch_bounds__(CP_THREADS)
void quant_write_kernel(QuantArgs q) {
  __shared__ int cnt[CP_WAVES];
  const CompressArgs& a = q.c;
  const int tid = threadIdx.x;
  const int lane = tid & (CP_WAVE - 1), wave = tid / CP_WAVE;
  const int sl = blockIdx.y;
  const long long u = a.u0 + sl;
  const int m = a.models[u];
  const u32 w = (u32)q.workers[u];
  const long long base = a.rows[u] * a.P;
  float* th = a.replicas + base;
  float* e = a.resid ? a.resid + base : nullptr;
  const float* g = a.global + (long long)m * a.P;
  const u32 tau = a.k ? a.tau[sl] : 0u;
  const float s = __uint_as_float(q.smax[sl]);
  int sent = 0;
#pragma unroll 1
  for (int i = 0; i < CP_ITEMS / 4; ++i) {
    const long long jb = (long long)blockIdx.x * CP_CHUNK +
                         ((long long)i * CP_THREADS + tid) * 4;
    u32 x[4] = {0u, 0u, 0u, 0u};
    if (jb < a.P)
      cp_philox((u32)(jb >> 2), w, (u32)m, q.ctr, q.key0, q.key1, x);
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const long long j = jb + t;
      bool wr = false;
      if (j < a.P) {
        const float gj = g[j];
        const float av = e ? e[j] : __fsub_rn(th[j], gj);
        wr = cp_emit_quant(av, tau, s, q.L, x[t], gj, th, e, j);
      }
      sent += __popcll(__ballot(wr));
    }
  }
  if (lane == 0) cnt[wave] = sent;
  __syncthreads();
  if (tid == 0) {
    int tot = 0;
#pragma unroll
    for (int v = 0; v < CP_WAVES; ++v) tot += cnt[v];
    if (tot) atomicAdd(a.counts + 2 * m, (u64)tot);
  }
}

// ---------------------------------------------------------------------------
// host wrapper
// ---------------------------------------------------------------------------

static void cp_check(const torch::Tensor& t, c10::ScalarType dt,
                     const char* name) {
  TORCH_CHECK(t.is_cuda() && t.dtype() == dt && t.is_contiguous(), name,
              " must be a contiguous CUDA tensor of the expected dtype");
}

// Checks shared by both entry points; fills the row-kernel part of the
// arguments. k lies in [kmin, P].
static CompressArgs cp_args(const torch::Tensor& replicas,
                            const torch::Tensor& global,
                            const c10::optional<torch::Tensor>& resid,
                            const torch::Tensor& rows,
                            const torch::Tensor& models,
                            const torch::Tensor& counts, int64_t k,
                            int64_t kmin, int64_t row_max,
                            const torch::Tensor& hist,
                            const torch::Tensor& tau,
                            const torch::Tensor& krem) {
  cp_check(replicas, torch::kFloat32, "replicas");
  cp_check(global, torch::kFloat32, "global");
  cp_check(rows, torch::kInt64, "rows");
  cp_check(models, torch::kInt32, "models");
  cp_check(counts, torch::kInt64, "counts");
  cp_check(hist, torch::kInt32, "hist");
  cp_check(tau, torch::kInt32, "tau");
  cp_check(krem, torch::kInt32, "krem");
  TORCH_CHECK(replicas.dim() == 2 && global.dim() == 2 &&
              replicas.size(1) == global.size(1),
              "compress: replicas [R, P] and global [K, P] differ in P");
  const int64_t P = replicas.size(1), K = global.size(0), U = rows.size(0);
  TORCH_CHECK(counts.dim() == 2 && counts.size(0) == K && counts.size(1) == 2,
              "compress: counts must be [K, 2]");
  TORCH_CHECK(models.size(0) == U, "compress: pair arrays differ in size");
  if (resid.has_value()) {
    cp_check(*resid, torch::kFloat32, "residual");
    TORCH_CHECK(resid->sizes() == replicas.sizes(),
                "compress: the residual bank must have the replicas' shape");
  }
  CompressArgs a;
  a.replicas = replicas.data_ptr<float>();
  a.global = global.data_ptr<float>();
  a.resid = resid.has_value() ? resid->data_ptr<float>() : nullptr;
  a.rows = (const long long*)rows.data_ptr<int64_t>();
  a.models = models.data_ptr<int>();
  a.counts = (u64*)counts.data_ptr<int64_t>();
  a.P = P;
  a.U = U;
  a.k = (int)k;
  a.hist = nullptr;
  a.tau = nullptr;
  a.krem = nullptr;
  a.u0 = 0;
  if (U == 0 || P == 0) return a;
  TORCH_CHECK(P <= 2147483647 && k >= kmin && k <= P,
              "compress: k must lie in [", kmin, ", P]");
  TORCH_CHECK(row_max >= 0 && row_max <= CP_ROW_MAX,
              "compress: row_max above the row kernel's LDS bound");
  TORCH_CHECK(U <= 2147483647, "compress: too many pairs");
  return a;
}

// the long path's scratch behind the arguments
static void cp_long_args(CompressArgs& a, const torch::Tensor& hist,
                         const torch::Tensor& tau, const torch::Tensor& krem,
                         int64_t slab) {
  TORCH_CHECK(slab >= 1 && slab <= 65535, "compress: slab out of range");
  TORCH_CHECK(hist.numel() >= slab * CP_BINS0 && tau.numel() >= slab &&
              krem.numel() >= slab,
              "compress: scratch too small for the slab");
  a.hist = (u32*)hist.data_ptr<int>();
  a.tau = (u32*)tau.data_ptr<int>();
  a.krem = (u32*)krem.data_ptr<int>();
}

// Compress replicas[rows[i]] around global[models[i]] in place, keeping the
// k largest magnitudes (ties included); resid, when given, is read and
// rewritten on the same rows; counts[m, 0] gains the sent coordinates. Rows
// of at most row_max (<= CP_ROW_MAX) coordinates take a row kernel, longer
// ones the radix path in slabs of `slab` pairs over hist / tau / krem. The
// caller (ops/compress_hip.py) has checked rows against the bank and models
// against K on the host.
static void compress_topk_impl(torch::Tensor replicas, torch::Tensor global,
                               c10::optional<torch::Tensor> resid,
                               torch::Tensor rows, torch::Tensor models,
                               torch::Tensor counts, int64_t k,
                               int64_t row_max, torch::Tensor hist,
                               torch::Tensor tau, torch::Tensor krem,
                               int64_t slab) {
  CompressArgs a = cp_args(replicas, global, resid, rows, models, counts, k,
                           1, row_max, hist, tau, krem);
  const int64_t P = a.P, U = a.U;
  if (U == 0 || P == 0) return;
  auto stream = c10::hip::getCurrentHIPStream();

  if (P <= row_max) {
    if (P <= CP_WAVE_MAX) {
      hipLaunchKernelGGL(compress_wave_kernel,
                         dim3((unsigned)((U + CP_WAVES - 1) / CP_WAVES)),
                         dim3(CP_THREADS), 0, stream, a);
      TORCH_CHECK(hipGetLastError() == hipSuccess,
                  "compress_wave_kernel launch");
    } else {
      hipLaunchKernelGGL(compress_block_kernel, dim3((unsigned)U),
                         dim3(CP_THREADS), 0, stream, a);
      TORCH_CHECK(hipGetLastError() == hipSuccess,
                  "compress_block_kernel launch");
    }
    return;
  }

  cp_long_args(a, hist, tau, krem, slab);
  const int64_t chunks = (P + CP_CHUNK - 1) / CP_CHUNK;
  TORCH_CHECK(hipMemsetAsync(a.hist, 0, (size_t)slab * CP_BINS0 * sizeof(u32),
                             stream) == hipSuccess,
              "compress: histogram clear");
  for (int64_t u0 = 0; u0 < U; u0 += slab) {
    const unsigned n = (unsigned)std::min<int64_t>(slab, U - u0);
    a.u0 = u0;
    for (int pass = 0; pass < 3; ++pass) {
      hipLaunchKernelGGL(compress_hist_kernel, dim3((unsigned)chunks, n),
                         dim3(CP_THREADS), 0, stream, a, pass);
      TORCH_CHECK(hipGetLastError() == hipSuccess,
                  "compress_hist_kernel launch");
      hipLaunchKernelGGL(compress_pick_kernel, dim3(n), dim3(CP_THREADS), 0,
                         stream, a, pass);
      TORCH_CHECK(hipGetLastError() == hipSuccess,
                  "compress_pick_kernel launch");
    }
    hipLaunchKernelGGL(compress_write_kernel, dim3((unsigned)chunks, n),
                       dim3(CP_THREADS), 0, stream, a);
    TORCH_CHECK(hipGetLastError() == hipSuccess,
                "compress_write_kernel launch");
  }
}

// compress_topk with stochastic quantisation to `bits` bits of what travels;
// k = 0: every non-zero coordinate travels (quant), else the top k
// (topk_quant). workers[i] is pair i's global worker id, (key, ctr) the
// Philox key and the compress-pass counter, smax [slab] the long path's
// scale scratch.
static void compress_quant_impl(torch::Tensor replicas, torch::Tensor global,
                                c10::optional<torch::Tensor> resid,
                                torch::Tensor rows, torch::Tensor models,
                                torch::Tensor workers, torch::Tensor counts,
                                int64_t k, int64_t bits, uint64_t key,
                                int64_t ctr, int64_t row_max,
                                torch::Tensor hist, torch::Tensor tau,
                                torch::Tensor krem, torch::Tensor smax,
                                int64_t slab) {
  QuantArgs q;
  q.c = cp_args(replicas, global, resid, rows, models, counts, k, 0, row_max,
                hist, tau, krem);
  CompressArgs& a = q.c;
  const int64_t P = a.P, U = a.U;
  cp_check(workers, torch::kInt32, "workers");
  cp_check(smax, torch::kInt32, "smax");
  TORCH_CHECK(workers.size(0) == U, "compress: pair arrays differ in size");
  TORCH_CHECK(bits >= 2 && bits <= 16, "compress: bits must lie in [2, 16]");
  if (U == 0 || P == 0) return;
  q.workers = workers.data_ptr<int>();
  q.smax = nullptr;
  q.key0 = (u32)(key & 0xffffffffull);
  q.key1 = (u32)(key >> 32);
  q.ctr = (u32)((uint64_t)ctr & 0xffffffffull);
  q.L = (float)((1 << (bits - 1)) - 1);
  auto stream = c10::hip::getCurrentHIPStream();

  if (P <= row_max) {
    if (P <= CP_WAVE_MAX) {
      hipLaunchKernelGGL(quant_wave_kernel,
                         dim3((unsigned)((U + CP_WAVES - 1) / CP_WAVES)),
                         dim3(CP_THREADS), 0, stream, q);
      TORCH_CHECK(hipGetLastError() == hipSuccess,
                  "quant_wave_kernel launch");
    } else {
      hipLaunchKernelGGL(quant_block_kernel, dim3((unsigned)U),
                         dim3(CP_THREADS), 0, stream, q);
      TORCH_CHECK(hipGetLastError() == hipSuccess,
                  "quant_block_kernel launch");
    }
    return;
  }

  cp_long_args(a, hist, tau, krem, slab);
  TORCH_CHECK(smax.numel() >= slab, "compress: scratch too small for the slab");
  q.smax = (u32*)smax.data_ptr<int>();
  const int64_t chunks = (P + CP_CHUNK - 1) / CP_CHUNK;
  if (k)
    TORCH_CHECK(hipMemsetAsync(a.hist, 0,
                               (size_t)slab * CP_BINS0 * sizeof(u32),
                               stream) == hipSuccess,
                "compress: histogram clear");
  for (int64_t u0 = 0; u0 < U; u0 += slab) {
    const unsigned n = (unsigned)std::min<int64_t>(slab, U - u0);
    a.u0 = u0;
    TORCH_CHECK(hipMemsetAsync(q.smax, 0, (size_t)n * sizeof(u32), stream) ==
                    hipSuccess,
                "compress: scale clear");
    if (k) {
      for (int pass = 0; pass < 3; ++pass) {
        hipLaunchKernelGGL(quant_hist_kernel, dim3((unsigned)chunks, n),
                           dim3(CP_THREADS), 0, stream, a, pass, q.smax);
        TORCH_CHECK(hipGetLastError() == hipSuccess,
                    "quant_hist_kernel launch");
        hipLaunchKernelGGL(compress_pick_kernel, dim3(n), dim3(CP_THREADS), 0,
                           stream, a, pass);
        TORCH_CHECK(hipGetLastError() == hipSuccess,
                    "compress_pick_kernel launch");
      }
    } else {
      hipLaunchKernelGGL(quant_form_kernel, dim3((unsigned)chunks, n),
                         dim3(CP_THREADS), 0, stream, a, q.smax);
      TORCH_CHECK(hipGetLastError() == hipSuccess,
                  "quant_form_kernel launch");
    }
    hipLaunchKernelGGL(quant_write_kernel, dim3((unsigned)chunks, n),
                       dim3(CP_THREADS), 0, stream, q);
    TORCH_CHECK(hipGetLastError() == hipSuccess,
                "quant_write_kernel launch");
  }
}

void register_compress(pybind11::module_& mod) {
  mod.def("compress_topk", &compress_topk_impl,
          "top-k upload sparsification with error feedback, in place");
  mod.def("compress_quant", &compress_quant_impl,
          "stochastic quantisation of all (k = 0) or the top-k coordinates, "
          "with error feedback, in place");
  mod.def("compress_wave_max", []() { return (int64_t)CP_WAVE_MAX; },
          "row length up to which one wave takes a pair");
  mod.def("compress_row_max", []() { return (int64_t)CP_ROW_MAX; },
          "row length up to which a row kernel takes a pair");
  mod.def("compress_chunk", []() { return (int64_t)CP_CHUNK; },
          "coordinates one block of the long path covers");
  mod.def("compress_slab_rows", []() { return (int64_t)CP_SLAB_ROWS; },
          "default bound on the pairs of the long path held at once");
  mod.def("compress_bins", []() { return (int64_t)CP_BINS0; },
          "histogram bins a pair of the long path owns in the scratch");
}
