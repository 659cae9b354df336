// ga3c_dmlp.hip -- the discrete-action vector-state network of reference NetworkVP_discrate.py:39-130 (GAME = 'CartPole-v0')
// on gfx950, and its C ABI (ga3c_dmlp_*, include/ga3c_abi.h).  DESIGN.md 8g.
//
//   x[B,S] -> dense1_<i>_p (w_i, sigmoid), i = 1..L -> logits_v (1, linear) | logits_p (A, linear) -> softmax
//
// The layer list is data (1..8 layers of 1..256 units) and has two wirings.  chained = 0 is the reference as written
// (:52-56): every layer reads x, only the last one reaches the heads, the others are variables that nothing reads.
// chained = 1: layer i reads layer i - 1.
//
// Kernels (all f32, one workgroup of 256 threads per 16-row tile where rows are involved):
//   dmlp_tile_kernel<PREDICT>  forward of one tile, activations in LDS ([width][16]); thread j owns output column j.
//   dmlp_tile_kernel<TRAIN>    the same forward, the softmax head's loss row and dz / dv, and the deltas back through the
//                              live layers; activations and deltas go to HBM for the weight gradients.  <EVAL>: forward + loss.
//   dmlp_wgrad_kernel<FUSED>   one thread per arena element sums its gradient over the rows in row order (no atomics: the
//                              same call gives the same bits); FUSED (no clipping) applies RMSProp to the element at once.
//                              An element of a dead variable gets gradient 0 and no step.  Threads 0..2 of block 0: the
//                              three loss sums, in row order.
//   dmlp_update_kernel<CLIP>   one block per live variable: tf.clip_by_average_norm's norm (fixed-order tree), then RMSProp.
// A train step is 2 launches without USE_GRAD_CLIP and 3 with it; a prediction is 1; an evaluation 2.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <condition_variable>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <map>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "../../include/ga3c_abi.h"
#include "ga3c_checkpoint.hpp"

void ga3c_set_last_error(const char* msg);   // ga3c_engine.hip: the thread's ga3c_last_error() message

namespace ga3c_dvec {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int TILE = 16;                  // rows per workgroup
constexpr int THREADS = 256;
constexpr int MAX_S = 64;
constexpr int MAX_A = 32;
constexpr int MAX_L = GA3C_DMLP_MAX_LAYERS;
constexpr int WIDE = 256;                 // widest layer (LDS buffers)
constexpr int MAX_NL = MAX_L + 2;         // trunk layers, logits_v, logits_p
constexpr int MAX_NV = 2 * MAX_NL;

struct Layout {                // layers 0..L-1 the trunk, L logits_v, L+1 logits_p; variables w then b per layer, TF creation order
  int S, A, L, chained;
  int in[MAX_NL], out[MAX_NL];
  int live[MAX_NL];            // 0: a layer nothing reads (chained = 0, layers 0..L-2): no gradient, no optimizer step
  int64_t off[MAX_NV + 1];     // off[2 (L + 2)] = parameter count
};

inline Layout make_layout(int S, int A, int L, const int* widths, int chained) {
  Layout Y;
  memset(&Y, 0, sizeof Y);
  Y.S = S; Y.A = A; Y.L = L; Y.chained = chained;
  for (int l = 0; l < L; ++l) {
    Y.in[l] = (chained && l > 0) ? widths[l - 1] : S;
    Y.out[l] = widths[l];
    Y.live[l] = (chained || l == L - 1) ? 1 : 0;
  }
  Y.in[L] = Y.in[L + 1] = widths[L - 1];
  Y.out[L] = 1;
  Y.out[L + 1] = A;
  Y.live[L] = Y.live[L + 1] = 1;
  int64_t o = 0;
  for (int l = 0; l < L + 2; ++l) {
    Y.off[2 * l] = o;
    o += (int64_t)Y.in[l] * Y.out[l];
    Y.off[2 * l + 1] = o;
    o += Y.out[l];
  }
  for (int v = 2 * (L + 2); v <= MAX_NV; ++v) Y.off[v] = o;
  return Y;
}

// Per-row buffers of the train workspace, row-major [B][width].
struct Work {
  float* x;            // [B,S] the rows the step read
  float* act[MAX_L];   // [B,w_l] outputs of the live trunk layers
  float* del[MAX_L];   // the deltas at the same layers' pre-activations
  float* v;            // [B]
  float* z;            // [B,A] logits
  float* p;            // [B,A]
  float* dv;           // [B]
  float* dz;           // [B,A]
  float* lossrow;      // [B,3]
  float* losses;       // [3]
};

struct Input {         // row r of the batch: S floats at base + (off ? off[r] : r * stride) bytes
  const char* base;
  const int64_t* off;
  int64_t stride;
};

struct Head {          // the loss of NetworkVP_discrate.py:61-85
  float beta, log_eps, min_policy;
  int log_softmax;
};

struct Opt {           // TF-1 ApplyRMSProp: ms += (g*g - ms)(1-rho); mom = mom*mu + g*lr/sqrt(eps+ms); theta -= mom
  float* theta; float* ms; float* mom; float* grad;
  float lr, omr, mu, eps, clip;
};

enum { PREDICT = 0, EVAL = 1, TRAIN = 2 };

__device__ __forceinline__ float sigm(float h) { return 1.0f / (1.0f + expf(-h)); }

// out[j][r] = sigmoid(b[j] + sum_k in[k][r] W[k][j]) for the tile; thread j owns column j (coalesced weight reads).
// gout (may be null): the same values, row-major [B][N], rows < nrows only.
__device__ void dense_fwd(const float* __restrict__ W, const float* __restrict__ bias, int K, int N, const float* in, float* out,
                          float* gout, int row0, int nrows) {
  for (int j = threadIdx.x; j < N; j += THREADS) {
    float acc[TILE];
    const float b = bias[j];
#pragma unroll
    for (int r = 0; r < TILE; ++r) acc[r] = b;
    for (int k = 0; k < K; ++k) {
      const float w = W[(size_t)k * N + j];
      const f32x4* col = reinterpret_cast<const f32x4*>(in + k * TILE);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const f32x4 c = col[q];
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[4 * q + i] = fmaf(c[i], w, acc[4 * q + i]);
      }
    }
#pragma unroll
    for (int r = 0; r < TILE; ++r) {
      const float h = sigm(acc[r]);
      out[j * TILE + r] = h;
      if (gout && r < nrows) gout[(size_t)(row0 + r) * N + j] = h;
    }
  }
  __syncthreads();
}

// gin[k][r] = s (1 - s) sum_j W(k, j) gout[j][r] for k < K <= 256, s = gact[row][k] the layer's sigmoid output as this
// workgroup wrote it to HBM in the forward pass.  P threads share a k (the largest power of two with P K <= 256), each
// summing the strided slice j = p, p + P, ...; the P partials meet in `scratch` (P K 16 floats) and are added in p order.
template <class WF>
__device__ void dense_bwd(WF W, int K, int N, const float* gout, const float* gact, float* gin_lds, float* gin_glob, int row0,
                          int nrows, float* scratch) {
  int P = 1;
  while (P * 2 * K <= THREADS) P *= 2;
  const int t = threadIdx.x;
  auto finish = [&](int k, int r, float s) {
    float g = 0.f;
    if (r < nrows) {
      const float h = gact[(size_t)(row0 + r) * K + k];
      g = s * (h * (1.0f - h));
      gin_glob[(size_t)(row0 + r) * K + k] = g;
    }
    if (gin_lds) gin_lds[k * TILE + r] = g;
  };
  if (t < P * K) {
    const int k = t / P, p = t % P;
    float acc[TILE];
#pragma unroll
    for (int r = 0; r < TILE; ++r) acc[r] = 0.f;
    for (int j = p; j < N; j += P) {
      const float w = W(k, j);
      const f32x4* col = reinterpret_cast<const f32x4*>(gout + j * TILE);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const f32x4 c = col[q];
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[4 * q + i] = fmaf(c[i], w, acc[4 * q + i]);
      }
    }
    if (P == 1) {
#pragma unroll
      for (int r = 0; r < TILE; ++r) finish(k, r, acc[r]);
    } else {
#pragma unroll
      for (int r = 0; r < TILE; ++r) scratch[(p * K + k) * TILE + r] = acc[r];
    }
  }
  if (P > 1) {
    __syncthreads();
    for (int e = t; e < K * TILE; e += THREADS) {
      const int k = e / TILE, r = e % TILE;
      float s = 0.f;
      for (int p = 0; p < P; ++p) s += scratch[(p * K + k) * TILE + r];
      finish(k, r, s);
    }
  }
  __syncthreads();
}

// One 16-row tile: forward (all modes), loss rows (EVAL, TRAIN), deltas (TRAIN).  Outputs p[B,A], v[B], z[B,A] always.
template <int MODE>
__global__ __launch_bounds__(THREADS) void dmlp_tile_kernel(const Layout* __restrict__ layout, const float* __restrict__ theta,
                                                            Input in, const float* __restrict__ y, const float* __restrict__ a,
                                                            int B, Head hd, const Work* __restrict__ work,
                                                            float* __restrict__ p_out, float* __restrict__ v_out,
                                                            float* __restrict__ z_out) {
  // the layer table and the row buffers' addresses are read from HBM where they are needed (scalar loads): as kernel
  // arguments they were live across the layer loops and the TRAIN kernel spilled 64 SGPRs and asked for a private segment
  const Layout& L = *layout;
  const Work& w = *work;
  // LDS, [width][16] each (56.1 KB).  bufA / bufB alternate as a layer's input and output, forward and backward; bufC holds
  // the partial sums of dense_bwd.
  __shared__ __attribute__((aligned(16))) float xin[MAX_S * TILE];
  __shared__ __attribute__((aligned(16))) float bufA[WIDE * TILE];
  __shared__ __attribute__((aligned(16))) float bufB[WIDE * TILE];
  __shared__ __attribute__((aligned(16))) float bufC[WIDE * TILE];
  __shared__ __attribute__((aligned(16))) float zh[(1 + MAX_A) * TILE];
  __shared__ __attribute__((aligned(16))) float sm[MAX_A * TILE];

  const int S = L.S, A = L.A, NL = L.L, NH = 1 + A;
  const int row0 = blockIdx.x * TILE, nrows = min(TILE, B - row0);
  constexpr bool KEEP = MODE != PREDICT;

  for (int e = threadIdx.x; e < S * TILE; e += THREADS) {
    const int r = e / S, s = e % S;
    float xv = 0.f;
    if (r < nrows) {
      const int64_t ob = in.off ? in.off[row0 + r] : (int64_t)(row0 + r) * in.stride;
      xv = reinterpret_cast<const float*>(in.base + ob)[s];
      if (KEEP) w.x[(size_t)(row0 + r) * S + s] = xv;
    }
    xin[s * TILE + r] = xv;
  }
  __syncthreads();

  // the trunk: every layer when chained, else the last one alone, which reads x as all of them do
  const float* cur = xin;
  bool into_a = true;
  for (int l = L.chained ? 0 : NL - 1; l < NL; ++l) {
    float* out = into_a ? bufA : bufB;
    dense_fwd(theta + L.off[2 * l], theta + L.off[2 * l + 1], L.in[l], L.out[l], cur, out, KEEP ? w.act[l] : nullptr, row0,
              nrows);
    cur = out;
    into_a = !into_a;
  }
  const int H = L.out[NL - 1];
  const int64_t ovw = L.off[2 * NL], ovb = L.off[2 * NL + 1], opw = L.off[2 * NL + 2], opb = L.off[2 * NL + 3];

  // the two heads as one [H, 1 + A] layer: column 0 logits_v, 1..A logits_p
  for (int j = threadIdx.x; j < NH; j += THREADS) {
    float acc[TILE];
    const float b = j == 0 ? theta[ovb] : theta[opb + j - 1];
#pragma unroll
    for (int r = 0; r < TILE; ++r) acc[r] = b;
    for (int k = 0; k < H; ++k) {
      const float wk = j == 0 ? theta[ovw + k] : theta[opw + (int64_t)k * A + j - 1];
      const f32x4* col = reinterpret_cast<const f32x4*>(cur + k * TILE);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const f32x4 cc = col[q];
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[4 * q + i] = fmaf(cc[i], wk, acc[4 * q + i]);
      }
    }
#pragma unroll
    for (int r = 0; r < TILE; ++r) zh[j * TILE + r] = acc[r];
  }
  __syncthreads();

  // per row: softmax, the loss terms and the head deltas -- the arithmetic of heads_rows (ga3c_kernels.hpp) with the wave's
  // reductions as loops over the A actions in index order
  float* gz = into_a ? bufA : bufB;   // [1 + A][16]: dv, dz (the buffer the last layer did not write)
  if (threadIdx.x < TILE) {
    const int r = threadIdx.x;
    const bool ok = r < nrows;
    const int row = row0 + r;
    const float v = zh[r];
    float zmax = -INFINITY;
    for (int i = 0; i < A; ++i) zmax = fmaxf(zmax, zh[(1 + i) * TILE + r]);
    float esum = 0.f;
    for (int i = 0; i < A; ++i) {
      const float e = expf(zh[(1 + i) * TILE + r] - zmax);
      sm[i * TILE + r] = e;
      esum += e;
    }
    const float denom = 1.0f + hd.min_policy * (float)A;
    for (int i = 0; i < A; ++i) {
      const float s = sm[i * TILE + r] / esum;
      sm[i * TILE + r] = s;
      if (ok) {
        p_out[(size_t)row * A + i] = hd.log_softmax ? s : (s + hd.min_policy) / denom;
        z_out[(size_t)row * A + i] = zh[(1 + i) * TILE + r];
      }
    }
    if (ok) v_out[row] = v;
    if (MODE != PREDICT) {
      const float yy = ok ? y[row] : 0.f;
      const float adv = yy - v;
      float c1, c2;
      if (hd.log_softmax) {
        const float lse = logf(esum);
        float lsel = 0.f, ent = 0.f, asum = 0.f;
        for (int i = 0; i < A; ++i) {
          const float aa = ok ? a[(size_t)row * A + i] : 0.f;
          const float ls = (zh[(1 + i) * TILE + r] - zmax) - lse;
          lsel += ls * aa;
          ent += sm[i * TILE + r] * ls;
          asum += aa;
        }
        c1 = lsel * adv;
        c2 = -hd.beta * ent;
        if (MODE == TRAIN)
          for (int i = 0; i < A; ++i) {
            const float aa = ok ? a[(size_t)row * A + i] : 0.f;
            const float s = sm[i * TILE + r];
            const float ls = (zh[(1 + i) * TILE + r] - zmax) - lse;
            const float dz = ok ? -adv * (aa - s * asum) + hd.beta * s * (ls - ent) : 0.f;
            gz[(1 + i) * TILE + r] = dz;
            if (ok) w.dz[(size_t)row * A + i] = dz;
          }
      } else {
        float sel = 0.f, plogp = 0.f;
        for (int i = 0; i < A; ++i) {
          const float aa = ok ? a[(size_t)row * A + i] : 0.f;
          const float p = (sm[i * TILE + r] + hd.min_policy) / denom;
          sel += p * aa;
          plogp += logf(fmaxf(p, hd.log_eps)) * p;
        }
        c1 = logf(fmaxf(sel, hd.log_eps)) * adv;
        c2 = -hd.beta * plogp;
        if (MODE == TRAIN) {
          const float gsel = sel >= hd.log_eps ? 1.0f / sel : 0.f;
          auto gs_of = [&](int i) {
            const float aa = ok ? a[(size_t)row * A + i] : 0.f;
            const float p = (sm[i * TILE + r] + hd.min_policy) / denom;
            const float gp = -(adv * gsel) * aa + hd.beta * (logf(fmaxf(p, hd.log_eps)) + (p >= hd.log_eps ? 1.0f : 0.f));
            return gp / denom;
          };
          float dot = 0.f;
          for (int i = 0; i < A; ++i) dot += gs_of(i) * sm[i * TILE + r];
          for (int i = 0; i < A; ++i) {
            const float dz = ok ? sm[i * TILE + r] * (gs_of(i) - dot) : 0.f;
            gz[(1 + i) * TILE + r] = dz;
            if (ok) w.dz[(size_t)row * A + i] = dz;
          }
        }
      }
      if (ok) {
        w.lossrow[(size_t)row * 3 + 0] = c1;
        w.lossrow[(size_t)row * 3 + 1] = c2;
        w.lossrow[(size_t)row * 3 + 2] = 0.5f * (yy - v) * (yy - v);
      }
      if (MODE == TRAIN) {
        const float dv = ok ? v - yy : 0.f;
        gz[r] = dv;
        if (ok) w.dv[row] = dv;
      }
    }
  }
  __syncthreads();
  if (MODE != TRAIN) return;

  // backward through the live layers; rows >= nrows carry zero deltas
  const float* th = theta;
  float* dcur = into_a ? bufB : bufA;   // the last layer's activations: read from HBM from here on
  dense_bwd([=](int k, int j) { return j == 0 ? th[ovw + k] : th[opw + (int64_t)k * A + j - 1]; }, H, NH, gz, w.act[NL - 1],
            dcur, w.del[NL - 1], row0, nrows, bufC);
  if (L.chained)
    for (int l = NL - 1; l > 0; --l) {
      const float* Wl = theta + L.off[2 * l];
      const int K = L.out[l - 1], N = L.out[l];
      float* dnext = dcur == bufA ? bufB : bufA;
      dense_bwd([=](int k, int j) { return Wl[(size_t)k * N + j]; }, K, N, dcur, w.act[l - 1], l > 1 ? dnext : nullptr,
                w.del[l - 1], row0, nrows, bufC);
      dcur = dnext;
    }
}

// Where the weight gradient of each layer comes from: its input rows (ld K) and its output deltas (ld N).
struct GradSrc {
  const float* in[MAX_NL];
  const float* d[MAX_NL];
};

__device__ __forceinline__ float rms_step(const Opt& o, int64_t i, float g) {
  float m = o.ms[i];
  m += (g * g - m) * o.omr;
  o.ms[i] = m;
  float step = (g * o.lr) / sqrtf(o.eps + m);
  if (o.mu != 0.f) {
    step = o.mom[i] * o.mu + step;
    o.mom[i] = step;
  }
  o.theta[i] -= step;
  return step;
}

// Sums over the batch rows, in row order.  The loads of ROWS_AHEAD rows are issued together and the additions stay one chain:
// the bits of the plain loop at the latency of B / ROWS_AHEAD round trips to L2 instead of B.
constexpr int ROWS_AHEAD = 16;

__device__ __forceinline__ float sum_rows(const float* __restrict__ d, int ld, int B) {
  float g = 0.f;
  int r = 0;
  for (; r + ROWS_AHEAD <= B; r += ROWS_AHEAD) {
    float t[ROWS_AHEAD];
#pragma unroll
    for (int i = 0; i < ROWS_AHEAD; ++i) t[i] = d[(size_t)(r + i) * ld];
#pragma unroll
    for (int i = 0; i < ROWS_AHEAD; ++i) g += t[i];
  }
  for (; r < B; ++r) g += d[(size_t)r * ld];
  return g;
}

__device__ __forceinline__ float dot_rows(const float* __restrict__ x, int ldx, const float* __restrict__ d, int ldd, int B) {
  float g = 0.f;
  int r = 0;
  for (; r + ROWS_AHEAD <= B; r += ROWS_AHEAD) {
    float tx[ROWS_AHEAD], td[ROWS_AHEAD];
#pragma unroll
    for (int i = 0; i < ROWS_AHEAD; ++i) {
      tx[i] = x[(size_t)(r + i) * ldx];
      td[i] = d[(size_t)(r + i) * ldd];
    }
#pragma unroll
    for (int i = 0; i < ROWS_AHEAD; ++i) g = fmaf(tx[i], td[i], g);
  }
  for (; r < B; ++r) g = fmaf(x[(size_t)r * ldx], d[(size_t)r * ldd], g);
  return g;
}

template <bool FUSED>
__global__ __launch_bounds__(THREADS) void dmlp_wgrad_kernel(Layout L, GradSrc src, int B, Opt o, Work w) {
  const int NV = 2 * (L.L + 2);
  const int64_t e = (int64_t)blockIdx.x * THREADS + threadIdx.x;
  if (e < L.off[NV]) {
    int v = NV - 1;
    while (e < L.off[v]) --v;
    const int l = v / 2;
    if (!L.live[l]) {
      o.grad[e] = 0.f;           // a variable nothing reads: no gradient, and the optimizer leaves it and its slots alone
    } else {
      const int N = L.out[l], K = L.in[l];
      const float* d = src.d[l];
      float g;
      if (v & 1) {
        g = sum_rows(d + (e - L.off[v]), N, B);
      } else {
        const int64_t loc = e - L.off[v];
        const int k = (int)(loc / N), j = (int)(loc % N);
        g = dot_rows(src.in[l] + k, K, d + j, N, B);
      }
      o.grad[e] = g;
      if (FUSED) rms_step(o, e, g);
    }
  }
  if (blockIdx.x == 0 && threadIdx.x < 3) w.losses[threadIdx.x] = sum_rows(w.lossrow + threadIdx.x, 3, B);
}

// One block per variable; a dead variable's block returns at once.  CLIP: scale = clip / max(||g||_2 / n, clip)
// (tf.clip_by_average_norm), the sum of squares in a fixed order (strided partials, then a tree in LDS).
template <bool CLIP>
__global__ __launch_bounds__(THREADS) void dmlp_update_kernel(Layout L, Opt o) {
  __shared__ float sh[THREADS];
  if (!L.live[blockIdx.x / 2]) return;
  const int64_t lo = L.off[blockIdx.x], hi = L.off[blockIdx.x + 1];
  float scale = 1.f;
  if (CLIP) {
    float s = 0.f;
    for (int64_t i = lo + threadIdx.x; i < hi; i += THREADS) s += o.grad[i] * o.grad[i];
    sh[threadIdx.x] = s;
    __syncthreads();
    for (int h = THREADS / 2; h > 0; h >>= 1) {
      if (threadIdx.x < h) sh[threadIdx.x] += sh[threadIdx.x + h];
      __syncthreads();
    }
    scale = o.clip / fmaxf(sqrtf(sh[0]) / (float)(hi - lo), o.clip);
  }
  for (int64_t i = lo + threadIdx.x; i < hi; i += THREADS) {
    float g = o.grad[i];
    if (CLIP) g *= scale;
    rms_step(o, i, g);
  }
}

__global__ void dmlp_loss_kernel(Work w, int B) {
  if (threadIdx.x < 3) w.losses[threadIdx.x] = sum_rows(w.lossrow + threadIdx.x, 3, B);
}

// ------------------------------------------------------------------ host side

int fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  ga3c_set_last_error(buf);
  return code;
}

#define HIPCHK(expr)                                                                                  \
  do {                                                                                                \
    hipError_t _e = (expr);                                                                           \
    if (_e != hipSuccess) {                                                                           \
      (void)hipGetLastError();                                                                        \
      return fail(GA3C_EHIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
    }                                                                                                 \
  } while (0)
#define CHK(expr)                 \
  do {                            \
    int _r = (expr);              \
    if (_r != GA3C_OK) return _r; \
  } while (0)

struct PLane {                    // one prediction in flight: pinned staging + device outputs + completion event
  int64_t* h_off = nullptr; float* h_x = nullptr; float* h_p = nullptr; float* h_v = nullptr; float* h_z = nullptr;
  int64_t* d_off = nullptr; float* d_x = nullptr; float* d_p = nullptr; float* d_v = nullptr; float* d_z = nullptr;
  hipEvent_t ev = nullptr;
  bool busy = false;
  int B = 0;
};

}  // namespace ga3c_dvec

using namespace ga3c_dvec;

struct ga3c_dmlp {
  ga3c_dmlp_config cfg;
  Layout L;
  int nv = 0;                     // variables: 2 L + 4
  std::vector<std::string> names; // dense1_<i>_p/w, /b, ..., logits_v/w, /b, logits_p/w, /b
  int64_t n = 0;
  bool clip = false;
  Head head{};
  hipStream_t st = nullptr;       // every kernel and copy of the network: a prediction sees the weights before or after a
                                  // train step, never a mix, and needs no second buffer
  std::mutex mu;                  // enqueue order on `st` and the lanes' bookkeeping
  std::condition_variable lane_cv;
  std::mutex train_mu;            // one train / evaluate / arena call at a time (they share the staging below)
  std::vector<PLane> lanes;
  float* arena[4] = {nullptr, nullptr, nullptr, nullptr};   // theta, ms, mom, grad
  Work w{};
  float* work_base = nullptr;
  Layout* d_layout = nullptr;     // L and w as the row kernel reads them
  Work* d_work = nullptr;
  // train staging: pinned host + device
  float* h_x = nullptr; float* h_y = nullptr; float* h_a = nullptr; int64_t* h_off = nullptr; float* h_loss = nullptr;
  float* d_x = nullptr; float* d_y = nullptr; float* d_a = nullptr; int64_t* d_off = nullptr;
  hipEvent_t tev = nullptr, t0 = nullptr, t1 = nullptr;
  int last_B = 0;                 // rows of the last train / evaluate / resident step (fetch)
  int res_B = 0;                  // rows uploaded for the resident path
  std::atomic<int64_t> step{0};
  const char* reg_host = nullptr;
  const char* reg_dev = nullptr;
  int64_t reg_bytes = 0;
};

namespace {

// "x", "h<i>" / "dh<i>" (layer i = 1..L: its output and the delta at its pre-activation), "v", "z", "p", "dv", "dz", "lossrow"
float* work_ptr(ga3c_dmlp* m, const std::string& name, int64_t* width) {
  const int A = m->L.A;
  if (name == "x") { *width = m->L.S; return m->w.x; }
  if (name == "v") { *width = 1; return m->w.v; }
  if (name == "p") { *width = A; return m->w.p; }
  if (name == "z") { *width = A; return m->w.z; }
  if (name == "dv") { *width = 1; return m->w.dv; }
  if (name == "dz") { *width = A; return m->w.dz; }
  if (name == "lossrow") { *width = 3; return m->w.lossrow; }
  const bool delta = name.size() > 1 && name[0] == 'd' && name[1] == 'h';
  const size_t at = delta ? 2 : 1;
  if (name.size() != at + 1 || (!delta && name[0] != 'h')) return nullptr;
  const int l = name[at] - '1';
  if (l < 0 || l >= m->L.L || !m->L.live[l]) return nullptr;
  *width = m->L.out[l];
  return delta ? m->w.del[l] : m->w.act[l];
}

GradSrc grad_src(ga3c_dmlp* m) {
  GradSrc g;
  memset(&g, 0, sizeof g);
  const int NL = m->L.L;
  for (int l = 0; l < NL; ++l) {
    g.in[l] = (m->L.chained && l > 0) ? m->w.act[l - 1] : m->w.x;
    g.d[l] = m->w.del[l];
  }
  g.in[NL] = g.in[NL + 1] = m->w.act[NL - 1];
  g.d[NL] = m->w.dv;
  g.d[NL + 1] = m->w.dz;
  return g;
}

Opt make_opt(ga3c_dmlp* m, float lr) {
  Opt o;
  o.theta = m->arena[0]; o.ms = m->arena[1]; o.mom = m->arena[2]; o.grad = m->arena[3];
  o.lr = lr;
  o.omr = 1.0f - m->cfg.rmsprop_decay;
  o.mu = m->cfg.rmsprop_momentum;
  o.eps = m->cfg.rmsprop_epsilon;
  o.clip = m->cfg.grad_clip_norm;
  return o;
}

Head make_head(ga3c_dmlp* m, float beta) {
  Head h = m->head;
  h.beta = beta;
  return h;
}

int tiles(int B) { return (B + TILE - 1) / TILE; }

// Enqueue the row kernel on `in` (caller holds mu).  TRAIN: + the weight gradients and, apply != 0, the update.
int enqueue_train(ga3c_dmlp* m, const Input& in, int B, float beta, bool apply, float lr) {
  hipLaunchKernelGGL(dmlp_tile_kernel<TRAIN>, dim3(tiles(B)), dim3(THREADS), 0, m->st, (const Layout*)m->d_layout, (const float*)m->arena[0], in,
                     (const float*)m->d_y, (const float*)m->d_a, B, make_head(m, beta), (const Work*)m->d_work, m->w.p, m->w.v, m->w.z);
  const Opt o = make_opt(m, lr);
  const int gblocks = (int)((m->n + THREADS - 1) / THREADS);
  if (apply && !m->clip)
    hipLaunchKernelGGL(dmlp_wgrad_kernel<true>, dim3(gblocks), dim3(THREADS), 0, m->st, m->L, grad_src(m), B, o, m->w);
  else
    hipLaunchKernelGGL(dmlp_wgrad_kernel<false>, dim3(gblocks), dim3(THREADS), 0, m->st, m->L, grad_src(m), B, o, m->w);
  if (apply && m->clip) hipLaunchKernelGGL(dmlp_update_kernel<true>, dim3(m->nv), dim3(THREADS), 0, m->st, m->L, o);
  HIPCHK(hipGetLastError());
  return GA3C_OK;
}

int enqueue_apply(ga3c_dmlp* m, float lr) {
  const Opt o = make_opt(m, lr);
  if (m->clip) hipLaunchKernelGGL(dmlp_update_kernel<true>, dim3(m->nv), dim3(THREADS), 0, m->st, m->L, o);
  else hipLaunchKernelGGL(dmlp_update_kernel<false>, dim3(m->nv), dim3(THREADS), 0, m->st, m->L, o);
  HIPCHK(hipGetLastError());
  return GA3C_OK;
}

int check_batch(ga3c_dmlp* m, int B) {
  if (B < 1 || B > m->cfg.max_batch) return fail(GA3C_EINVAL, "batch %d outside [1,%d]", B, m->cfg.max_batch);
  return GA3C_OK;
}

// offsets of rows in the registered segment: each must hold S whole floats inside it
int check_offsets(ga3c_dmlp* m, const int64_t* off, int B) {
  if (!m->reg_dev) return fail(GA3C_ESTATE, "no host segment registered");
  const int64_t row = 4 * (int64_t)m->L.S;
  for (int i = 0; i < B; ++i)
    if (off[i] < 0 || off[i] % 4 != 0 || off[i] > m->reg_bytes - row)
      return fail(GA3C_EINVAL, "offset %lld of row %d is not a 4-byte aligned row of %lld bytes inside the %lld-byte segment",
                  (long long)off[i], i, (long long)row, (long long)m->reg_bytes);
  return GA3C_OK;
}

// Stages y_r / a and the states (x: host rows, or offsets into the registered segment) of a train-type call; caller holds
// train_mu.  Returns the Input the row kernel reads.
int stage_train(ga3c_dmlp* m, const float* x, const int64_t* off, const float* y, const float* a, int B, Input* in) {
  const int S = m->L.S, A = m->L.A;
  if (off) CHK(check_offsets(m, off, B));
  memcpy(m->h_y, y, sizeof(float) * B);
  memcpy(m->h_a, a, sizeof(float) * B * A);
  HIPCHK(hipMemcpyAsync(m->d_y, m->h_y, sizeof(float) * B, hipMemcpyHostToDevice, m->st));
  HIPCHK(hipMemcpyAsync(m->d_a, m->h_a, sizeof(float) * B * A, hipMemcpyHostToDevice, m->st));
  if (off) {
    memcpy(m->h_off, off, sizeof(int64_t) * B);
    HIPCHK(hipMemcpyAsync(m->d_off, m->h_off, sizeof(int64_t) * B, hipMemcpyHostToDevice, m->st));
    *in = Input{m->reg_dev, m->d_off, 0};
  } else {
    memcpy(m->h_x, x, sizeof(float) * B * S);
    HIPCHK(hipMemcpyAsync(m->d_x, m->h_x, sizeof(float) * B * S, hipMemcpyHostToDevice, m->st));
    *in = Input{reinterpret_cast<const char*>(m->d_x), nullptr, 4 * (int64_t)S};
  }
  return GA3C_OK;
}

int finish_train(ga3c_dmlp* m) {
  HIPCHK(hipMemcpyAsync(m->h_loss, m->w.losses, 3 * sizeof(float), hipMemcpyDeviceToHost, m->st));
  HIPCHK(hipEventRecord(m->tev, m->st));
  return GA3C_OK;
}

int wait_train(ga3c_dmlp* m, float* losses) {
  HIPCHK(hipEventSynchronize(m->tev));
  if (losses) memcpy(losses, m->h_loss, 3 * sizeof(float));
  return GA3C_OK;
}

// train / compute_grads on host rows or on offsets
int train_common(ga3c_dmlp* m, const float* x, const int64_t* off, const float* y, const float* a, int B, bool apply, float lr,
                 float beta, float* losses) {
  if (!m || (!x && !off) || !y || !a) return fail(GA3C_EINVAL, "null argument");
  CHK(check_batch(m, B));
  HIPCHK(hipSetDevice(m->cfg.device));
  std::lock_guard<std::mutex> tl(m->train_mu);
  {
    std::lock_guard<std::mutex> lk(m->mu);
    Input in;
    CHK(stage_train(m, x, off, y, a, B, &in));
    CHK(enqueue_train(m, in, B, beta, apply, lr));
    CHK(finish_train(m));
    m->last_B = B;
  }
  CHK(wait_train(m, losses));
  if (apply) m->step.fetch_add(1);
  return GA3C_OK;
}

PLane* take_lane(ga3c_dmlp* m, std::unique_lock<std::mutex>& lk, int* ticket) {
  for (;;) {
    for (size_t i = 0; i < m->lanes.size(); ++i)
      if (!m->lanes[i].busy) {
        m->lanes[i].busy = true;
        *ticket = (int)i;
        return &m->lanes[i];
      }
    m->lane_cv.wait(lk);
  }
}

void give_lane(ga3c_dmlp* m, PLane* P) {
  {
    std::lock_guard<std::mutex> lk(m->mu);
    P->busy = false;
  }
  m->lane_cv.notify_one();
}

// Enqueues one prediction on a lane of its own (x: host rows; off: rows of the registered segment).
int predict_begin(ga3c_dmlp* m, const float* x, const int64_t* off, int B, int* ticket) {
  CHK(check_batch(m, B));
  HIPCHK(hipSetDevice(m->cfg.device));
  if (off) {
    CHK(check_offsets(m, off, B));
  }
  std::unique_lock<std::mutex> lk(m->mu);
  PLane* P = take_lane(m, lk, ticket);
  const int S = m->L.S, A = m->L.A;
  Input in;
  hipError_t e = hipSuccess;
  if (off) {
    memcpy(P->h_off, off, sizeof(int64_t) * B);
    e = hipMemcpyAsync(P->d_off, P->h_off, sizeof(int64_t) * B, hipMemcpyHostToDevice, m->st);
    in = Input{m->reg_dev, P->d_off, 0};
  } else {
    memcpy(P->h_x, x, sizeof(float) * B * S);
    e = hipMemcpyAsync(P->d_x, P->h_x, sizeof(float) * B * S, hipMemcpyHostToDevice, m->st);
    in = Input{reinterpret_cast<const char*>(P->d_x), nullptr, 4 * (int64_t)S};
  }
  if (e == hipSuccess) {
    hipLaunchKernelGGL(dmlp_tile_kernel<PREDICT>, dim3(tiles(B)), dim3(THREADS), 0, m->st, (const Layout*)m->d_layout, (const float*)m->arena[0], in,
                       (const float*)nullptr, (const float*)nullptr, B, make_head(m, 0.f), (const Work*)m->d_work, P->d_p, P->d_v, P->d_z);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(P->h_p, P->d_p, sizeof(float) * B * A, hipMemcpyDeviceToHost, m->st);
  if (e == hipSuccess) e = hipMemcpyAsync(P->h_v, P->d_v, sizeof(float) * B, hipMemcpyDeviceToHost, m->st);
  if (e == hipSuccess) e = hipMemcpyAsync(P->h_z, P->d_z, sizeof(float) * B * A, hipMemcpyDeviceToHost, m->st);
  if (e == hipSuccess) e = hipEventRecord(P->ev, m->st);
  if (e != hipSuccess) {
    P->busy = false;
    lk.unlock();
    m->lane_cv.notify_one();
    (void)hipGetLastError();
    return fail(GA3C_EHIP, "prediction enqueue failed: %s", hipGetErrorString(e));
  }
  P->B = B;
  return GA3C_OK;
}

int predict_end(ga3c_dmlp* m, int ticket, int B, float* p, float* v, float* z) {
  if (ticket < 0 || ticket >= (int)m->lanes.size()) return fail(GA3C_ESTATE, "no prediction begun under ticket %d", ticket);
  PLane* P = &m->lanes[ticket];
  {
    std::lock_guard<std::mutex> lk(m->mu);
    if (!P->busy) return fail(GA3C_ESTATE, "no prediction begun under ticket %d", ticket);
  }
  const hipError_t e = hipEventSynchronize(P->ev);     // the lane's staging is free for the next begin only after this
  if (e == hipSuccess && B != P->B) {
    give_lane(m, P);
    return fail(GA3C_EINVAL, "batch %d, begun with %d", B, P->B);
  }
  if (e == hipSuccess) {
    const int A = m->L.A;
    if (p) memcpy(p, P->h_p, sizeof(float) * B * A);
    if (v) memcpy(v, P->h_v, sizeof(float) * B);
    if (z) memcpy(z, P->h_z, sizeof(float) * B * A);
  }
  give_lane(m, P);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    return fail(GA3C_EHIP, "prediction failed: %s", hipGetErrorString(e));
  }
  return GA3C_OK;
}

int param_index(const ga3c_dmlp* m, const char* name) {
  if (!name) return -1;
  std::string s(name);
  if (s.size() > 2 && s.compare(s.size() - 2, 2, ":0") == 0) s.resize(s.size() - 2);
  for (int i = 0; i < m->nv; ++i)
    if (s == m->names[i]) return i;
  return -1;
}

void param_shape(const ga3c_dmlp* m, int i, int32_t* ndim, int64_t shape[4]) {
  const int l = i / 2;
  if (i & 1) {
    *ndim = 1;
    shape[0] = m->L.out[l];
  } else {
    *ndim = 2;
    shape[0] = m->L.in[l];
    shape[1] = m->L.out[l];
  }
}

int arena_copy(ga3c_dmlp* m, int which, int64_t off, int64_t count, float* out, const float* in) {
  if (which < 0 || which > 3 || (in && which > 2)) return fail(GA3C_EINVAL, "arena selector %d not in [0,%d]", which, in ? 2 : 3);
  HIPCHK(hipSetDevice(m->cfg.device));
  std::lock_guard<std::mutex> tl(m->train_mu);
  std::lock_guard<std::mutex> lk(m->mu);
  HIPCHK(hipStreamSynchronize(m->st));
  if (out) HIPCHK(hipMemcpy(out, m->arena[which] + off, sizeof(float) * count, hipMemcpyDeviceToHost));
  else HIPCHK(hipMemcpy(m->arena[which] + off, in, sizeof(float) * count, hipMemcpyHostToDevice));
  return GA3C_OK;
}

void free_all(ga3c_dmlp* m) {
  if (m->st) (void)hipStreamSynchronize(m->st);
  for (PLane& P : m->lanes) {
    (void)hipHostFree(P.h_off); (void)hipHostFree(P.h_x); (void)hipHostFree(P.h_p); (void)hipHostFree(P.h_v);
    (void)hipHostFree(P.h_z);
    (void)hipFree(P.d_off); (void)hipFree(P.d_x); (void)hipFree(P.d_p); (void)hipFree(P.d_v); (void)hipFree(P.d_z);
    if (P.ev) (void)hipEventDestroy(P.ev);
  }
  for (float*& a : m->arena) (void)hipFree(a);
  (void)hipFree(m->work_base);
  (void)hipFree(m->d_layout);
  (void)hipFree(m->d_work);
  (void)hipHostFree(m->h_x); (void)hipHostFree(m->h_y); (void)hipHostFree(m->h_a); (void)hipHostFree(m->h_off);
  (void)hipHostFree(m->h_loss);
  (void)hipFree(m->d_x); (void)hipFree(m->d_y); (void)hipFree(m->d_a); (void)hipFree(m->d_off);
  for (hipEvent_t e : {m->tev, m->t0, m->t1})
    if (e) (void)hipEventDestroy(e);
  if (m->reg_host) (void)hipHostUnregister((void*)m->reg_host);
  if (m->st) (void)hipStreamDestroy(m->st);
  (void)hipGetLastError();
}

template <class T>
int dalloc(T** p, size_t n) {
  HIPCHK(hipMalloc((void**)p, n * sizeof(T) + 16));
  return GA3C_OK;
}
template <class T>
int halloc(T** p, size_t n) {
  HIPCHK(hipHostMalloc((void**)p, n * sizeof(T) + 16, hipHostMallocDefault));
  return GA3C_OK;
}

int create(ga3c_dmlp* m) {
  const ga3c_dmlp_config& c = m->cfg;
  const size_t B = (size_t)c.max_batch, S = c.state_dim, A = c.num_actions;
  const int NL = m->L.L;
  HIPCHK(hipStreamCreateWithFlags(&m->st, hipStreamNonBlocking));
  for (int i = 0; i < 4; ++i) {
    CHK(dalloc(&m->arena[i], (size_t)m->n));
    HIPCHK(hipMemset(m->arena[i], 0, sizeof(float) * m->n));
  }
  std::vector<float> ones((size_t)m->n, 1.0f);     // the RMSProp ms slot starts at 1 (TF-1 RMSPropOptimizer)
  HIPCHK(hipMemcpy(m->arena[1], ones.data(), sizeof(float) * m->n, hipMemcpyHostToDevice));
  // per-row workspace, one block; the dead layers of chained = 0 get no rows
  std::vector<size_t> widths = {S, 1, A, A, 1, A, 3};
  std::vector<float**> dst = {&m->w.x, &m->w.v, &m->w.z, &m->w.p, &m->w.dv, &m->w.dz, &m->w.lossrow};
  for (int l = 0; l < NL; ++l)
    if (m->L.live[l]) {
      widths.push_back((size_t)m->L.out[l]); dst.push_back(&m->w.act[l]);
      widths.push_back((size_t)m->L.out[l]); dst.push_back(&m->w.del[l]);
    }
  size_t total = 0;
  for (size_t wd : widths) total += (B * wd + 3) / 4 * 4;
  CHK(dalloc(&m->work_base, total + 4));
  HIPCHK(hipMemset(m->work_base, 0, sizeof(float) * (total + 4)));
  float* q = m->work_base;
  for (size_t i = 0; i < widths.size(); ++i) {
    *dst[i] = q;
    q += (B * widths[i] + 3) / 4 * 4;
  }
  m->w.losses = q;
  CHK(dalloc(&m->d_layout, 1));
  CHK(dalloc(&m->d_work, 1));
  HIPCHK(hipMemcpy(m->d_layout, &m->L, sizeof(Layout), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(m->d_work, &m->w, sizeof(Work), hipMemcpyHostToDevice));
  CHK(halloc(&m->h_x, B * S)); CHK(halloc(&m->h_y, B)); CHK(halloc(&m->h_a, B * A)); CHK(halloc(&m->h_off, B));
  CHK(halloc(&m->h_loss, 4));
  CHK(dalloc(&m->d_x, B * S)); CHK(dalloc(&m->d_y, B)); CHK(dalloc(&m->d_a, B * A)); CHK(dalloc(&m->d_off, B));
  HIPCHK(hipEventCreateWithFlags(&m->tev, hipEventDisableTiming));
  HIPCHK(hipEventCreate(&m->t0));
  HIPCHK(hipEventCreate(&m->t1));
  m->lanes.resize((size_t)(c.predict_lanes > 0 ? c.predict_lanes : 4));
  for (PLane& P : m->lanes) {
    CHK(halloc(&P.h_off, B)); CHK(halloc(&P.h_x, B * S)); CHK(halloc(&P.h_p, B * A)); CHK(halloc(&P.h_v, B));
    CHK(halloc(&P.h_z, B * A));
    CHK(dalloc(&P.d_off, B)); CHK(dalloc(&P.d_x, B * S)); CHK(dalloc(&P.d_p, B * A)); CHK(dalloc(&P.d_v, B));
    CHK(dalloc(&P.d_z, B * A));
    HIPCHK(hipEventCreateWithFlags(&P.ev, hipEventDisableTiming));
  }
  return GA3C_OK;
}

std::string layer_name(int i) { return "dense1_" + std::to_string(i + 1) + "_p"; }

}  // namespace

extern "C" {

int ga3c_dmlp_create(const ga3c_dmlp_config* cfg, ga3c_dmlp** out) {
  if (!cfg || !out) return fail(GA3C_EINVAL, "null argument");
  *out = nullptr;
  if (cfg->state_dim < 1 || cfg->state_dim > MAX_S) return fail(GA3C_EINVAL, "state_dim %d outside [1,%d]", cfg->state_dim, MAX_S);
  if (cfg->num_actions < 1 || cfg->num_actions > MAX_A)
    return fail(GA3C_EINVAL, "num_actions %d outside [1,%d]", cfg->num_actions, MAX_A);
  if (cfg->max_batch < 1 || cfg->max_batch > 65536) return fail(GA3C_EINVAL, "max_batch %d outside [1,65536]", cfg->max_batch);
  if (cfg->num_layers < 1 || cfg->num_layers > MAX_L) return fail(GA3C_EINVAL, "num_layers %d outside [1,%d]", cfg->num_layers, MAX_L);
  for (int l = 0; l < cfg->num_layers; ++l)
    if (cfg->widths[l] < 1 || cfg->widths[l] > WIDE)
      return fail(GA3C_EINVAL, "width %d of layer %d outside [1,%d]", cfg->widths[l], l + 1, WIDE);
  if (cfg->chained != 0 && cfg->chained != 1) return fail(GA3C_EINVAL, "chained %d is neither 0 nor 1", cfg->chained);
  if (cfg->flags & ~(uint32_t)(GA3C_FLAG_LOG_SOFTMAX | GA3C_FLAG_GRAD_CLIP))
    return fail(GA3C_EINVAL, "flags 0x%x: only GA3C_FLAG_LOG_SOFTMAX and GA3C_FLAG_GRAD_CLIP apply to the discrete vector-state "
                             "network", cfg->flags);
  if (cfg->predict_lanes < 0 || cfg->predict_lanes > 64) return fail(GA3C_EINVAL, "predict_lanes %d outside [0,64]", cfg->predict_lanes);
  int ndev = 0;
  HIPCHK(hipGetDeviceCount(&ndev));
  if (cfg->device < 0 || cfg->device >= ndev) return fail(GA3C_EINVAL, "device %d not in [0,%d)", cfg->device, ndev);
  HIPCHK(hipSetDevice(cfg->device));
  hipDeviceProp_t prop;
  HIPCHK(hipGetDeviceProperties(&prop, cfg->device));
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return fail(GA3C_ESTATE, "device %d is %s; this library is built for gfx950 only", cfg->device, prop.gcnArchName);
  ga3c_dmlp* m = new (std::nothrow) ga3c_dmlp();
  if (!m) return fail(GA3C_EINVAL, "out of host memory");
  m->cfg = *cfg;
  m->L = make_layout(cfg->state_dim, cfg->num_actions, cfg->num_layers, cfg->widths, cfg->chained);
  m->nv = 2 * (cfg->num_layers + 2);
  for (int l = 0; l < cfg->num_layers + 2; ++l) {
    const std::string base = l < cfg->num_layers ? layer_name(l) : (l == cfg->num_layers ? "logits_v" : "logits_p");
    m->names.push_back(base + "/w");
    m->names.push_back(base + "/b");
  }
  m->n = m->L.off[m->nv];
  m->clip = (cfg->flags & GA3C_FLAG_GRAD_CLIP) != 0;
  m->head.beta = 0.f;
  m->head.log_eps = cfg->log_epsilon;
  m->head.min_policy = cfg->min_policy;
  m->head.log_softmax = (cfg->flags & GA3C_FLAG_LOG_SOFTMAX) != 0;
  const int rc = create(m);
  if (rc != GA3C_OK) {
    free_all(m);
    delete m;
    return rc;
  }
  *out = m;
  return GA3C_OK;
}

int ga3c_dmlp_destroy(ga3c_dmlp* m) {
  if (!m) return fail(GA3C_EINVAL, "null argument");
  (void)hipSetDevice(m->cfg.device);
  free_all(m);
  delete m;
  return GA3C_OK;
}

int ga3c_dmlp_param_count(ga3c_dmlp* m, int64_t* count) {
  if (!m || !count) return fail(GA3C_EINVAL, "null argument");
  *count = m->n;
  return GA3C_OK;
}

int ga3c_dmlp_get_arena(ga3c_dmlp* m, int32_t which, float* out, int64_t count) {
  if (!m || !out) return fail(GA3C_EINVAL, "null argument");
  if (count != m->n) return fail(GA3C_EINVAL, "count %lld != arena size %lld", (long long)count, (long long)m->n);
  return arena_copy(m, which, 0, count, out, nullptr);
}

int ga3c_dmlp_set_arena(ga3c_dmlp* m, int32_t which, const float* in, int64_t count) {
  if (!m || !in) return fail(GA3C_EINVAL, "null argument");
  if (count != m->n) return fail(GA3C_EINVAL, "count %lld != arena size %lld", (long long)count, (long long)m->n);
  return arena_copy(m, which, 0, count, nullptr, in);
}

int ga3c_dmlp_get_step(ga3c_dmlp* m, int64_t* step) {
  if (!m || !step) return fail(GA3C_EINVAL, "null argument");
  *step = m->step.load();
  return GA3C_OK;
}

int ga3c_dmlp_set_step(ga3c_dmlp* m, int64_t step) {
  if (!m) return fail(GA3C_EINVAL, "null argument");
  m->step.store(step);
  return GA3C_OK;
}

int32_t ga3c_dmlp_num_params(ga3c_dmlp* m) { return m ? m->nv : 0; }

const char* ga3c_dmlp_param_name(ga3c_dmlp* m, int32_t index) {
  return (m && index >= 0 && index < m->nv) ? m->names[index].c_str() : nullptr;
}

int ga3c_dmlp_param_info(ga3c_dmlp* m, const char* name, int64_t* offset, int64_t* count, int32_t* ndim, int64_t shape[4]) {
  if (!m || !name) return fail(GA3C_EINVAL, "null argument");
  const int i = param_index(m, name);
  if (i < 0) return fail(GA3C_EINVAL, "no variable named %s", name);
  if (offset) *offset = m->L.off[i];
  if (count) *count = m->L.off[i + 1] - m->L.off[i];
  int32_t nd;
  int64_t sh[4] = {0, 0, 0, 0};
  param_shape(m, i, &nd, sh);
  if (ndim) *ndim = nd;
  if (shape) memcpy(shape, sh, sizeof sh);
  return GA3C_OK;
}

int ga3c_dmlp_get_param(ga3c_dmlp* m, const char* name, int32_t which, float* out, int64_t count) {
  if (!m || !name || !out) return fail(GA3C_EINVAL, "null argument");
  const int i = param_index(m, name);
  if (i < 0) return fail(GA3C_EINVAL, "no variable named %s", name);
  if (count != m->L.off[i + 1] - m->L.off[i]) return fail(GA3C_EINVAL, "%s has %lld elements, not %lld", name,
                                                          (long long)(m->L.off[i + 1] - m->L.off[i]), (long long)count);
  return arena_copy(m, which, m->L.off[i], count, out, nullptr);
}

int ga3c_dmlp_set_param(ga3c_dmlp* m, const char* name, int32_t which, const float* in, int64_t count) {
  if (!m || !name || !in) return fail(GA3C_EINVAL, "null argument");
  const int i = param_index(m, name);
  if (i < 0) return fail(GA3C_EINVAL, "no variable named %s", name);
  if (count != m->L.off[i + 1] - m->L.off[i]) return fail(GA3C_EINVAL, "%s has %lld elements, not %lld", name,
                                                          (long long)(m->L.off[i + 1] - m->L.off[i]), (long long)count);
  return arena_copy(m, which, m->L.off[i], count, nullptr, in);
}

int ga3c_dmlp_save(ga3c_dmlp* m, const char* path) {
  if (!m || !path) return fail(GA3C_EINVAL, "null argument");
  std::vector<float> arena[3];
  for (int w = 0; w < 3; ++w) {
    arena[w].resize((size_t)m->n);
    CHK(ga3c_dmlp_get_arena(m, w, arena[w].data(), m->n));
  }
  const char* suffix[3] = {":0", "/RMSProp:0", "/RMSProp_1:0"};
  std::vector<ga3c_ckpt::Member> members;
  ga3c_ckpt::Member st;
  st.name = "step";
  st.descr = "<i8";
  const int64_t step = m->step.load();
  st.bytes.assign(reinterpret_cast<const uint8_t*>(&step), reinterpret_cast<const uint8_t*>(&step) + 8);
  members.push_back(st);
  for (int i = 0; i < m->nv; ++i) {
    int32_t nd;
    int64_t sh[4];
    param_shape(m, i, &nd, sh);
    for (int w = 0; w < 3; ++w) {
      ga3c_ckpt::Member mb;
      mb.name = m->names[i] + suffix[w];
      mb.descr = "<f4";
      mb.shape.assign(sh, sh + nd);
      const uint8_t* src = reinterpret_cast<const uint8_t*>(arena[w].data() + m->L.off[i]);
      mb.bytes.assign(src, src + (size_t)(m->L.off[i + 1] - m->L.off[i]) * sizeof(float));
      members.push_back(std::move(mb));
    }
  }
  std::string err;
  if (!ga3c_ckpt::write_npz(path, members, &err)) return fail(GA3C_ESTATE, "%s", err.c_str());
  return GA3C_OK;
}

int ga3c_dmlp_load(ga3c_dmlp* m, const char* path) {
  if (!m || !path) return fail(GA3C_EINVAL, "null argument");
  std::map<std::string, ga3c_ckpt::Member> members;
  std::string err;
  if (!ga3c_ckpt::read_npz(path, &members, &err)) return fail(GA3C_ESTATE, "%s", err.c_str());
  // a file of another network kind holds no dense1_1_p/w; one of this kind with more layers holds dense1_<L+1>_p/w:
  // both refused before anything is written
  if (members.count(layer_name(m->L.L) + "/w:0"))
    return fail(GA3C_ESTATE, "%s holds %s/w: a network of more than this one's %d layers", path, layer_name(m->L.L).c_str(), m->L.L);
  const char* suffix[3] = {":0", "/RMSProp:0", "/RMSProp_1:0"};
  std::vector<float> arena[3];
  for (int w = 0; w < 3; ++w) arena[w].resize((size_t)m->n);
  for (int i = 0; i < m->nv; ++i) {
    const int64_t cnt = m->L.off[i + 1] - m->L.off[i];
    int32_t nd;
    int64_t sh[4];
    param_shape(m, i, &nd, sh);
    for (int w = 0; w < 3; ++w) {
      const std::string key = m->names[i] + suffix[w];
      auto it = members.find(key);
      if (it == members.end())
        return fail(GA3C_ESTATE, "%s holds no %s: not a checkpoint of this discrete vector-state network", path, key.c_str());
      const ga3c_ckpt::Member& mb = it->second;
      const bool shape_ok = mb.shape.size() == (size_t)nd && std::equal(mb.shape.begin(), mb.shape.end(), sh);
      if (mb.descr != "<f4" || !shape_ok || mb.bytes.size() != (size_t)cnt * sizeof(float))
        return fail(GA3C_ESTATE, "%s: %s is not <f4 of this network's shape (%lld elements)", path, key.c_str(), (long long)cnt);
      memcpy(arena[w].data() + m->L.off[i], mb.bytes.data(), mb.bytes.size());
    }
  }
  auto st = members.find("step");
  if (st == members.end() || st->second.descr != "<i8" || st->second.bytes.size() != 8)
    return fail(GA3C_ESTATE, "%s holds no int64 step", path);
  int64_t step = 0;
  memcpy(&step, st->second.bytes.data(), 8);
  for (int w = 0; w < 3; ++w) CHK(ga3c_dmlp_set_arena(m, w, arena[w].data(), m->n));
  m->step.store(step);
  return GA3C_OK;
}

int ga3c_dmlp_predict(ga3c_dmlp* m, const float* x, int32_t batch, float* p, float* v, float* z) {
  if (!m || !x || !p || !v) return fail(GA3C_EINVAL, "null argument");
  int ticket;
  CHK(predict_begin(m, x, nullptr, batch, &ticket));
  return predict_end(m, ticket, batch, p, v, z);
}

int ga3c_dmlp_train(ga3c_dmlp* m, const float* x, const float* y_r, const float* a, int32_t batch, float learning_rate,
                    float beta, float* losses) {
  return train_common(m, x, nullptr, y_r, a, batch, true, learning_rate, beta, losses);
}

int ga3c_dmlp_compute_grads(ga3c_dmlp* m, const float* x, const float* y_r, const float* a, int32_t batch, float beta,
                            float* losses) {
  return train_common(m, x, nullptr, y_r, a, batch, false, 0.f, beta, losses);
}

int ga3c_dmlp_apply_grads(ga3c_dmlp* m, float learning_rate) {
  if (!m) return fail(GA3C_EINVAL, "null argument");
  HIPCHK(hipSetDevice(m->cfg.device));
  std::lock_guard<std::mutex> tl(m->train_mu);
  {
    std::lock_guard<std::mutex> lk(m->mu);
    CHK(enqueue_apply(m, learning_rate));
    HIPCHK(hipEventRecord(m->tev, m->st));
  }
  HIPCHK(hipEventSynchronize(m->tev));
  m->step.fetch_add(1);
  return GA3C_OK;
}

int ga3c_dmlp_evaluate(ga3c_dmlp* m, const float* x, const int64_t* offsets, const float* y_r, const float* a, int32_t batch,
                       float beta, float* losses, float* lastdense, float* v, float* p) {
  if (!m || (!x && !offsets) || (x && offsets) || !y_r || !a) return fail(GA3C_EINVAL, "bad argument");
  CHK(check_batch(m, batch));
  HIPCHK(hipSetDevice(m->cfg.device));
  std::lock_guard<std::mutex> tl(m->train_mu);
  {
    std::lock_guard<std::mutex> lk(m->mu);
    Input in;
    CHK(stage_train(m, x, offsets, y_r, a, batch, &in));
    hipLaunchKernelGGL(dmlp_tile_kernel<EVAL>, dim3(tiles(batch)), dim3(THREADS), 0, m->st, (const Layout*)m->d_layout, (const float*)m->arena[0], in,
                       (const float*)m->d_y, (const float*)m->d_a, batch, make_head(m, beta), (const Work*)m->d_work, m->w.p, m->w.v, m->w.z);
    hipLaunchKernelGGL(dmlp_loss_kernel, dim3(1), dim3(64), 0, m->st, m->w, batch);
    HIPCHK(hipGetLastError());
    CHK(finish_train(m));
    m->last_B = batch;
  }
  CHK(wait_train(m, losses));
  const size_t B = (size_t)batch;
  const int last = m->L.L - 1;
  if (lastdense) HIPCHK(hipMemcpy(lastdense, m->w.act[last], B * m->L.out[last] * sizeof(float), hipMemcpyDeviceToHost));
  if (v) HIPCHK(hipMemcpy(v, m->w.v, B * sizeof(float), hipMemcpyDeviceToHost));
  if (p) HIPCHK(hipMemcpy(p, m->w.p, B * m->L.A * sizeof(float), hipMemcpyDeviceToHost));
  return GA3C_OK;
}

int ga3c_dmlp_register_host(ga3c_dmlp* m, void* base, int64_t bytes) {
  if (!m || !base || bytes < 16) return fail(GA3C_EINVAL, "bad argument");
  if (m->reg_host) return fail(GA3C_ESTATE, "a host segment is already registered");
  HIPCHK(hipSetDevice(m->cfg.device));
  HIPCHK(hipHostRegister(base, (size_t)bytes, hipHostRegisterMapped));
  void* dev = nullptr;
  hipError_t e = hipHostGetDevicePointer(&dev, base, 0);
  if (e != hipSuccess) {
    (void)hipHostUnregister(base);
    return fail(GA3C_EHIP, "hipHostGetDevicePointer failed: %s", hipGetErrorString(e));
  }
  std::lock_guard<std::mutex> tl(m->train_mu);
  std::lock_guard<std::mutex> lk(m->mu);
  m->reg_host = static_cast<const char*>(base);
  m->reg_dev = static_cast<const char*>(dev);
  m->reg_bytes = bytes;
  return GA3C_OK;
}

int ga3c_dmlp_unregister_host(ga3c_dmlp* m) {
  if (!m) return fail(GA3C_EINVAL, "null argument");
  if (!m->reg_host) return GA3C_OK;
  HIPCHK(hipSetDevice(m->cfg.device));
  std::lock_guard<std::mutex> tl(m->train_mu);
  std::lock_guard<std::mutex> lk(m->mu);
  HIPCHK(hipStreamSynchronize(m->st));
  HIPCHK(hipHostUnregister((void*)m->reg_host));
  m->reg_host = m->reg_dev = nullptr;
  m->reg_bytes = 0;
  return GA3C_OK;
}

int ga3c_dmlp_predict_gather(void* net, const int64_t* offsets, int32_t batch, int32_t u8, float* p, float* v, float* z) {
  ga3c_dmlp* m = static_cast<ga3c_dmlp*>(net);
  int ticket;
  CHK(ga3c_dmlp_predict_gather_begin(net, offsets, batch, u8, &ticket));
  return predict_end(m, ticket, batch, p, v, z);
}

int ga3c_dmlp_predict_gather_begin(void* net, const int64_t* offsets, int32_t batch, int32_t u8, int32_t* ticket) {
  ga3c_dmlp* m = static_cast<ga3c_dmlp*>(net);
  if (!m || !offsets || !ticket) return fail(GA3C_EINVAL, "null argument");
  if (u8) return fail(GA3C_EINVAL, "the vector-state network reads f32 rows (u8 = 0)");
  return predict_begin(m, nullptr, offsets, batch, ticket);
}

int ga3c_dmlp_predict_gather_end(void* net, int32_t ticket, int32_t batch, float* p, float* v) {
  ga3c_dmlp* m = static_cast<ga3c_dmlp*>(net);
  if (!m || !p || !v) return fail(GA3C_EINVAL, "null argument");
  return predict_end(m, ticket, batch, p, v, nullptr);
}

int ga3c_dmlp_train_gather(ga3c_dmlp* m, const int64_t* offsets, int32_t u8, const float* y_r, const float* a, int32_t batch,
                           float learning_rate, float beta, float* losses) {
  if (u8) return fail(GA3C_EINVAL, "the vector-state network reads f32 rows (u8 = 0)");
  if (!offsets) return fail(GA3C_EINVAL, "null argument");
  return train_common(m, nullptr, offsets, y_r, a, batch, true, learning_rate, beta, losses);
}

int ga3c_dmlp_upload(ga3c_dmlp* m, const float* x, const float* y_r, const float* a, int32_t batch) {
  if (!m || !x || !y_r || !a) return fail(GA3C_EINVAL, "null argument");
  CHK(check_batch(m, batch));
  HIPCHK(hipSetDevice(m->cfg.device));
  std::lock_guard<std::mutex> tl(m->train_mu);
  std::lock_guard<std::mutex> lk(m->mu);
  Input in;
  CHK(stage_train(m, x, nullptr, y_r, a, batch, &in));
  HIPCHK(hipStreamSynchronize(m->st));
  m->res_B = batch;
  return GA3C_OK;
}

int ga3c_dmlp_time_resident(ga3c_dmlp* m, int32_t mode, int32_t batch, int32_t iters, float learning_rate, float beta,
                            float* elapsed_ms) {
  if (!m || !elapsed_ms || iters < 1 || (mode != 0 && mode != 1)) return fail(GA3C_EINVAL, "bad argument");
  if (batch < 1 || batch > m->res_B) return fail(GA3C_ESTATE, "batch %d: %d rows uploaded", batch, m->res_B);
  HIPCHK(hipSetDevice(m->cfg.device));
  std::lock_guard<std::mutex> tl(m->train_mu);
  {
    std::lock_guard<std::mutex> lk(m->mu);
    const Input in{reinterpret_cast<const char*>(m->d_x), nullptr, 4 * (int64_t)m->L.S};
    HIPCHK(hipEventRecord(m->t0, m->st));
    for (int i = 0; i < iters; ++i) {
      if (mode == 0)
        hipLaunchKernelGGL(dmlp_tile_kernel<PREDICT>, dim3(tiles(batch)), dim3(THREADS), 0, m->st, (const Layout*)m->d_layout,
                           (const float*)m->arena[0], in, (const float*)nullptr, (const float*)nullptr, batch,
                           make_head(m, 0.f), (const Work*)m->d_work, m->w.p, m->w.v, m->w.z);
      else
        CHK(enqueue_train(m, in, batch, beta, true, learning_rate));
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(m->t1, m->st));
    m->last_B = batch;
  }
  HIPCHK(hipEventSynchronize(m->t1));
  HIPCHK(hipEventElapsedTime(elapsed_ms, m->t0, m->t1));
  if (mode == 1) m->step.fetch_add(iters);
  return GA3C_OK;
}

int ga3c_dmlp_fetch(ga3c_dmlp* m, const char* name, float* out, int64_t count) {
  if (!m || !name || !out) return fail(GA3C_EINVAL, "null argument");
  int64_t wd = -1;
  float* src = work_ptr(m, name, &wd);
  if (!src) return fail(GA3C_EINVAL, "no activation named %s (a layer nothing reads has none)", name);
  if (count != wd * m->last_B)
    return fail(GA3C_EINVAL, "%s of the last step is %lld floats, not %lld", name, (long long)(wd * m->last_B), (long long)count);
  HIPCHK(hipSetDevice(m->cfg.device));
  std::lock_guard<std::mutex> tl(m->train_mu);
  std::lock_guard<std::mutex> lk(m->mu);
  HIPCHK(hipStreamSynchronize(m->st));
  HIPCHK(hipMemcpy(out, src, sizeof(float) * count, hipMemcpyDeviceToHost));
  return GA3C_OK;
}

}  // extern "C"
