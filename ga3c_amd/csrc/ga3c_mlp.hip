// ga3c_mlp.hip -- the vector-state network of reference NetworkVP.py:67-105,175-210 (GAME = 'Pendulum-v0') on gfx950, and
// its C ABI (ga3c_mlp_*, include/ga3c_abi.h).  DESIGN.md 8e.
//
//   x[B,S] -> dense11_p (4, linear) -> dense12_p (256, linear) -> dense13_p (256, linear) -> dense14_p (100, sigmoid)
//          -> dense1 (64, sigmoid) -> logits_v (1, linear) | logits_p/out_x, out_y (A each, sigmoid; angle output)
//
// Kernels (all f32, one workgroup of 256 threads per 16-row tile where rows are involved).  The tile's layout in LDS, who
// owns which sum and the order of its additions are ga3c_tile.hpp's; here are the layer table and the head.
//   mlp_tile_kernel<PREDICT>  forward of one tile (load_input_tile, dense_fwd); weights are read through L2 (0.4 MB), one
//                             column per thread, the 256x256 layer streamed k by k.
//   mlp_tile_kernel<TRAIN>    the same forward, the per-row loss, and the per-row deltas back through all seven layers
//                             (dense_bwd_split); activations and deltas go to HBM for the weight gradients.  <EVAL>:
//                             forward + loss only.
//   mlp_wgrad_kernel<FUSED>   one thread per arena element sums its gradient over the rows in row order (elem_grad);
//                             FUSED (no clipping) applies rms_step to the element at once.  Block 0 also: loss_sums.
//   mlp_update_kernel<CLIP>   one block per variable: clip_and_step (tf.clip_by_average_norm, RMSProp).
// A train step is 2 launches without USE_GRAD_CLIP and 3 with it; a prediction is 1.
//
// GA3C_FLAG_DUAL_RMSPROP (one RMSProp optimizer per cost) swaps the three train kernels, launch for launch:
//   mlp_tile_kernel             TRAIN's forward, loss rows, dv and dz, then the trunk backward twice on the same weights:
//   <TRAIN_DUAL, WorkDual>      from (dv = 0, dz) into Work::del (cost_p) and from (dv, dz = 0) into WorkDual::del_v (cost_v).
//   mlp_wgrad_dual_kernel<FUSED>  both costs' sums per arena element, the layer input read once per row; arenas 3 and 6;
//                               FUSED: the value step, then the policy step, each only where its optimizer has a slot.
//   mlp_update_dual_kernel<CLIP>  one block per variable: both norms, tf.clip_by_norm each, the value step, the policy step.
#include <hip/hip_runtime.h>

#include <cmath>
#include <map>
#include <new>
#include <string>
#include <vector>

#include "ga3c_actors.hpp"
#include "ga3c_tile.hpp"
#include "ga3c_vecnet.hpp"

namespace ga3c_vec {

using namespace ga3c_vecnet;   // Input, Opt, PREDICT / EVAL / TRAIN and the host half
using namespace ga3c_tile;     // TILE and the device half

constexpr int THREADS = 256;
constexpr int MAX_S = 64;
constexpr int MAX_A = 32;
constexpr float PI_F = 3.14159265358979f;
constexpr int TRAIN_DUAL = 3;             // a row-kernel mode of this file: TRAIN with one trunk backward per cost

// The layer table.  Trunk layers 0..4 (reference dense_layer calls, NetworkVP.py:78-85), then the three heads, each of
// which reads the last trunk layer: logits_v (linear) and logits_p/out_x, out_y (sigmoid, then the angle).
enum { LIN = 0, SIG = 1 };
constexpr int NTRUNK = 5;
constexpr int TRUNK_OUT[NTRUNK] = {4, 256, 256, 100, 64};
constexpr int TRUNK_ACT[NTRUNK] = {LIN, LIN, LIN, SIG, SIG};
constexpr int HID = 64;                   // width of dense1, the layer the heads read
constexpr int NLAYERS = NTRUNK + 3;
constexpr int NVARS = 2 * NLAYERS;
constexpr int WIDE = 256;                 // widest layer (LDS ping-pong buffers)

const char* const VAR_NAMES[NVARS] = {
    "dense11_p/w", "dense11_p/b", "dense12_p/w", "dense12_p/b", "dense13_p/w", "dense13_p/b", "dense14_p/w", "dense14_p/b",
    "dense1/w", "dense1/b", "logits_v/w", "logits_v/b", "logits_p/out_x/w", "logits_p/out_x/b", "logits_p/out_y/w",
    "logits_p/out_y/b"};

struct Layout {                // arena offsets of every variable, TF creation order (w then b per layer)
  int S, A;
  int in[NLAYERS], out[NLAYERS];
  int64_t off[NVARS + 1];      // off[NVARS] = parameter count = 4 S + 99,305 + 130 A
};

inline Layout make_layout(int S, int A) {
  Layout L;
  L.S = S;
  L.A = A;
  int w = S;
  for (int l = 0; l < NTRUNK; ++l) {
    L.in[l] = w;
    L.out[l] = TRUNK_OUT[l];
    w = TRUNK_OUT[l];
  }
  L.in[5] = L.in[6] = L.in[7] = HID;
  L.out[5] = 1;
  L.out[6] = L.out[7] = A;
  int64_t o = 0;
  for (int l = 0; l < NLAYERS; ++l) {
    L.off[2 * l] = o;
    o += (int64_t)L.in[l] * L.out[l];
    L.off[2 * l + 1] = o;
    o += L.out[l];
  }
  L.off[NVARS] = o;
  return L;
}

// Per-row buffers of the train workspace, row-major [B][width].
struct Work {
  float* x;            // [B,S] the rows the step read
  float* act[NTRUNK];  // [B,4] [B,256] [B,256] [B,100] [B,64]: pd1, pd2, pd3, pd4, d1
  float* del[NTRUNK];  // the deltas at the same layers' pre-activations
  float* v;            // [B]
  float* z;            // [B,2A] = [hx | hy]
  float* p;            // [B,A]
  float* dv;           // [B]
  float* dz;           // [B,2A] = [dhx | dhy]
  float* lossrow;      // [B,3]
  float* losses;       // [3]
};

struct WorkDual : Work {       // DUAL_RMSPROP: del holds the policy cost's deltas, del_v the value cost's
  float* del_v[NTRUNK];
};

// out[j][r] = act(b[j] + sum_k in[k][r] W[k][j]) for the tile (dense_fwd, ga3c_tile.hpp).
// gout (may be null): the same values, row-major [B][N], rows < nrows only.
template <int ACT>
__device__ void dense_fwd(const float* __restrict__ W, const float* __restrict__ bias, int K, int N, const float* in,
                          float* out, float* __restrict__ gout, int row0, int nrows) {
  ga3c_tile::dense_fwd<THREADS>(W, bias, K, N, in, nullptr, 0, nullptr, [&](int j, int r, float acc) {
    const float h = ACT == SIG ? sigm(acc) : acc;
    out[j * TILE + r] = h;
    if (gout && r < nrows) gout[(size_t)(row0 + r) * N + j] = h;
  });
}

// gin[k][r] = act'(k, r) * sum_j W(k, j) gout[j][r] for k < K <= 256 (dense_bwd_split, ga3c_tile.hpp, whose partials `scratch` holds).
// `act`: the layer's outputs in LDS, for the sigmoid's derivative.  gin_lds / gin_glob may be null.
template <int ACT, class WF>
__device__ void dense_bwd(WF W, int K, int N, const float* gout, const float* act, float* gin_lds, float* __restrict__ gin_glob,
                          int row0, int nrows, float* scratch) {
  dense_bwd_split<THREADS>(W, K, N, gout, scratch, [&](int k, int r, float s) {
    const float g = ACT == SIG ? s * (act[k * TILE + r] * (1.0f - act[k * TILE + r])) : s;
    if (gin_lds) gin_lds[k * TILE + r] = g;
    if (gin_glob && r < nrows) gin_glob[(size_t)(row0 + r) * K + k] = g;
  });
}

// One 16-row tile: forward (all modes), loss rows (EVAL, TRAIN), deltas (TRAIN).  Outputs p[B,A], v[B], z[B,2A] always.
// TRAIN_DUAL: the head deltas stay in zh (its logits are in HBM by then) and the trunk backward runs once per cost from
// them, reusing the same LDS buffers: the policy stream to w.del, the value stream to w.del_v (W = WorkDual).
template <int MODE, class W = Work>
__global__ __launch_bounds__(THREADS) void mlp_tile_kernel(Layout L, const float* __restrict__ theta, Input in,
                                                           const float* __restrict__ y, const float* __restrict__ a, int B,
                                                           float beta, W w, float* __restrict__ p_out,
                                                           float* __restrict__ v_out, float* __restrict__ z_out) {
  // LDS, [width][16] each (51.8 KB).  xin also holds the d1 delta, bufB the head deltas and then the dense14_p delta.
  __shared__ __attribute__((aligned(16))) float xin[MAX_S * TILE];
  __shared__ __attribute__((aligned(16))) float a1[4 * TILE];
  __shared__ __attribute__((aligned(16))) float bufA[WIDE * TILE];
  __shared__ __attribute__((aligned(16))) float bufB[WIDE * TILE];
  __shared__ __attribute__((aligned(16))) float a4[100 * TILE];
  __shared__ __attribute__((aligned(16))) float d1[HID * TILE];
  __shared__ __attribute__((aligned(16))) float zh[(1 + 2 * MAX_A) * TILE];

  const int S = L.S, A = L.A, NH = 1 + 2 * A;
  const int row0 = blockIdx.x * TILE, nrows = min(TILE, B - row0);
  constexpr bool KEEP = MODE != PREDICT;
  constexpr bool DELTAS = MODE == TRAIN || MODE == TRAIN_DUAL;

  load_input_tile<THREADS, KEEP>(in, S, row0, nrows, xin, w.x);
  __syncthreads();

  const float* W0 = theta + L.off[0];
  dense_fwd<LIN>(W0, theta + L.off[1], S, 4, xin, a1, KEEP ? w.act[0] : nullptr, row0, nrows);
  dense_fwd<LIN>(theta + L.off[2], theta + L.off[3], 4, 256, a1, bufA, KEEP ? w.act[1] : nullptr, row0, nrows);
  dense_fwd<LIN>(theta + L.off[4], theta + L.off[5], 256, 256, bufA, bufB, KEEP ? w.act[2] : nullptr, row0, nrows);
  dense_fwd<SIG>(theta + L.off[6], theta + L.off[7], 256, 100, bufB, a4, KEEP ? w.act[3] : nullptr, row0, nrows);
  dense_fwd<SIG>(theta + L.off[8], theta + L.off[9], 100, HID, a4, d1, KEEP ? w.act[4] : nullptr, row0, nrows);

  // the three heads as one [64, 1 + 2A] layer: column 0 logits_v, 1..A out_x, A+1..2A out_y (pre-activation)
  for (int j = threadIdx.x; j < NH; j += THREADS) {
    const int l = j == 0 ? 5 : (j <= A ? 6 : 7);
    const int c = j == 0 ? 0 : (j <= A ? j - 1 : j - 1 - A);
    const int n = L.out[l];
    const float* Wl = theta + L.off[2 * l];
    float acc[TILE];
    const float b = theta[L.off[2 * l + 1] + c];
#pragma unroll
    for (int r = 0; r < TILE; ++r) acc[r] = b;
    for (int k = 0; k < HID; ++k) tile_fma(acc, d1 + k * TILE, Wl[k * n + c]);
#pragma unroll
    for (int r = 0; r < TILE; ++r) zh[j * TILE + r] = acc[r];
  }
  __syncthreads();

  // per row: the angle output, the loss terms and the head deltas (Atan2Grad / pi, then the sigmoids)
  // [1 + 2A][16]: dv, dhx, dhy (bufB's activations are in HBM already).  TRAIN_DUAL: in place of the logits, which each
  // thread below has read for its row before it writes that row's deltas.
  float* gz = MODE == TRAIN_DUAL ? zh : bufB;
  if (threadIdx.x < TILE) {
    const int r = threadIdx.x;
    const bool ok = r < nrows;
    const int row = row0 + r;
    const float v = zh[r];
    const float yy = (MODE != PREDICT && ok) ? y[row] : 0.f;
    const float adv = yy - v;
    float c1 = 0.f, c2 = 0.f;
    for (int i = 0; i < A; ++i) {
      const float hx = zh[(1 + i) * TILE + r], hy = zh[(1 + A + i) * TILE + r];
      const float sx = sigm(hx), sy = sigm(hy);
      const float X = sx - 0.5f, Y = sy - 0.5f;
      const float pc = atan2f(Y, X) / PI_F;
      if (ok) {
        p_out[(size_t)row * A + i] = pc;
        z_out[(size_t)row * 2 * A + i] = hx;
        z_out[(size_t)row * 2 * A + A + i] = hy;
      }
      if (MODE != PREDICT) {
        const float aa = ok ? a[(size_t)row * A + i] : 0.f;
        c1 += pc * aa;
        c2 += pc * pc;
        if (DELTAS) {
          const float g = -aa * adv + 2.0f * beta * pc;
          const float gr = g / (PI_F * (X * X + Y * Y));
          const float dhx = ok ? -Y * gr * (sx * (1.0f - sx)) : 0.f;
          const float dhy = ok ? X * gr * (sy * (1.0f - sy)) : 0.f;
          gz[(1 + i) * TILE + r] = dhx;
          gz[(1 + A + i) * TILE + r] = dhy;
          if (ok) {
            w.dz[(size_t)row * 2 * A + i] = dhx;
            w.dz[(size_t)row * 2 * A + A + i] = dhy;
          }
        }
      }
    }
    if (ok) v_out[row] = v;
    if (MODE != PREDICT && ok) {
      w.lossrow[(size_t)row * 3 + 0] = c1 * adv;
      w.lossrow[(size_t)row * 3 + 1] = -beta * c2;
      w.lossrow[(size_t)row * 3 + 2] = 0.5f * (yy - v) * (yy - v);
    }
    if (DELTAS) {
      const float dv = ok ? v - yy : 0.f;
      gz[r] = dv;
      if (ok) w.dv[row] = dv;
    }
  }
  __syncthreads();
  if (!DELTAS) return;

  // backward through the trunk; rows >= nrows carry zero deltas
  float* g5 = xin;                  // [64][16]
  float* g4 = bufB + NH * TILE;     // [100][16], behind the head deltas
  const float* th = theta;
  const int64_t ov = L.off[10], ox = L.off[12], oy = L.off[14];
  const float* W4 = theta + L.off[8];
  const float* W3 = theta + L.off[6];
  const float* W2 = theta + L.off[4];
  const float* W1 = theta + L.off[2];
  if constexpr (MODE == TRAIN) {
    dense_bwd<SIG>([=](int k, int j) { return j == 0 ? th[ov + k] : (j <= A ? th[ox + k * A + j - 1] : th[oy + k * A + j - 1 - A]); },
                   HID, NH, gz, d1, g5, w.del[4], row0, nrows, bufA);
    dense_bwd<SIG>([=](int k, int j) { return W4[k * HID + j]; }, 100, HID, g5, a4, g4, w.del[3], row0, nrows, bufA);
    dense_bwd<LIN>([=](int k, int j) { return W3[k * 100 + j]; }, 256, 100, g4, nullptr, bufA, w.del[2], row0, nrows, nullptr);
    dense_bwd<LIN>([=](int k, int j) { return W2[k * 256 + j]; }, 256, 256, bufA, nullptr, bufB, w.del[1], row0, nrows, nullptr);
    dense_bwd<LIN>([=](int k, int j) { return W1[k * 256 + j]; }, 4, 256, bufB, nullptr, nullptr, w.del[0], row0, nrows, bufA);
  } else if constexpr (MODE == TRAIN_DUAL) {
    // One pass per cost, the chain above each time (TRAIN's stays written out: routed through this lambda it compiles to
    // other code than it had).  The backward is linear in the head deltas, so a stream is that chain started from the deltas
    // with the other cost's rows zeroed: cost_p from (0, dhx, dhy), then cost_v from (dv, 0, 0).  zh keeps the deltas; bufB,
    // which a pass overwrites, holds the stream's copy.
    auto chain = [&](float* const* del) {
      dense_bwd<SIG>([=](int k, int j) { return j == 0 ? th[ov + k] : (j <= A ? th[ox + k * A + j - 1] : th[oy + k * A + j - 1 - A]); },
                     HID, NH, bufB, d1, g5, del[4], row0, nrows, bufA);
      dense_bwd<SIG>([=](int k, int j) { return W4[k * HID + j]; }, 100, HID, g5, a4, g4, del[3], row0, nrows, bufA);
      dense_bwd<LIN>([=](int k, int j) { return W3[k * 100 + j]; }, 256, 100, g4, nullptr, bufA, del[2], row0, nrows, nullptr);
      dense_bwd<LIN>([=](int k, int j) { return W2[k * 256 + j]; }, 256, 256, bufA, nullptr, bufB, del[1], row0, nrows, nullptr);
      dense_bwd<LIN>([=](int k, int j) { return W1[k * 256 + j]; }, 4, 256, bufB, nullptr, nullptr, del[0], row0, nrows, bufA);
    };
    for (int e = threadIdx.x; e < NH * TILE; e += THREADS) bufB[e] = e < TILE ? 0.f : zh[e];
    __syncthreads();
    chain(w.del);
    for (int e = threadIdx.x; e < NH * TILE; e += THREADS) bufB[e] = e < TILE ? zh[e] : 0.f;
    __syncthreads();
    chain(w.del_v);
  }
}

// Where the weight gradient of each layer comes from: its input rows (ld K) and its output deltas (ld, column offset).
struct GradSrc {
  const float* in[NLAYERS];
  const float* d[NLAYERS];
  int d_ld[NLAYERS];
};

// Element e of variable v (a bias if v is odd): g[c] = its gradient under the deltas d[c], each summed over the rows in row
// order; the NC chains share the row's input and are independent, in double and rounded once (ga3c_tile.hpp's sum_rows has
// the reason).
template <int NC>
__device__ __forceinline__ void elem_grad(const Layout& L, const GradSrc& src, int v, int64_t e, const float* const (&d)[NC], int B,
                                          float (&g)[NC]) {
  const int l = v / 2, N = L.out[l], K = L.in[l], ld = src.d_ld[l];
  double s[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) s[c] = 0.0;
  if (v & 1) {
    const int j = (int)(e - L.off[v]);
    for (int r = 0; r < B; ++r)
#pragma unroll
      for (int c = 0; c < NC; ++c) s[c] += (double)d[c][(size_t)r * ld + j];
  } else {
    const int64_t loc = e - L.off[v];
    const int k = (int)(loc / N), j = (int)(loc % N);
    const float* __restrict__ x = src.in[l];
    for (int r = 0; r < B; ++r) {
      const double xv = (double)x[(size_t)r * K + k];
#pragma unroll
      for (int c = 0; c < NC; ++c) s[c] = fma(xv, (double)d[c][(size_t)r * ld + j], s[c]);
    }
  }
#pragma unroll
  for (int c = 0; c < NC; ++c) g[c] = (float)s[c];
}

template <bool FUSED>
__global__ __launch_bounds__(THREADS) void mlp_wgrad_kernel(Layout L, GradSrc src, int B, Opt o, Work w) {
  const int64_t e = (int64_t)blockIdx.x * THREADS + threadIdx.x;
  if (e < L.off[NVARS]) {
    int v = NVARS - 1;
    while (e < L.off[v]) --v;
    float g[1];
    elem_grad(L, src, v, e, {src.d[v / 2]}, B, g);
    o.grad[e] = g[0];
    if (FUSED) rms_step(o, e, g[0]);
  }
  loss_sums(w.lossrow, w.losses, B, blockIdx.x == 0);
}

// One block per variable: clip_and_step (ga3c_tile.hpp).
template <bool CLIP>
__global__ __launch_bounds__(THREADS) void mlp_update_kernel(Layout L, Opt o) {
  __shared__ float sh[THREADS];
  clip_and_step<THREADS, CLIP>(L.off[blockIdx.x], L.off[blockIdx.x + 1], o, sh);
}

// ------------------------------------------------------------------ two optimizers (GA3C_FLAG_DUAL_RMSPROP)

// Which costs reach variable v: cost_p has no path to logits_v/* (tf.stop_gradient), cost_v none to logits_p/*; TF-1 gives
// an optimizer no slot for a variable without a gradient, so that optimizer neither decays nor applies anything there.
__device__ __forceinline__ bool has_p(int v) { return v != 10 && v != 11; }
__device__ __forceinline__ bool has_v(int v) { return v < 12; }

struct GradSrc2 {              // GradSrc with the deltas of both costs; a head has those of its own cost in both
  GradSrc p;
  const float* dv[NLAYERS];
};

// One thread per arena element: g_p into op.grad (arena 3) and g_v into ov.grad (arena 6), each the sum over the rows in
// row order, exactly 0 where the cost has no path.  On the trunk the two chains share the row's input and are independent.
// A head element takes mlp_wgrad_kernel's single chain (elem_grad<1>): the same products in the same order under its own cost.
// FUSED: the value optimizer's step, then the policy optimizer's, theta' = (theta - D_v) - D_p.
template <bool FUSED>
__global__ __launch_bounds__(THREADS) void mlp_wgrad_dual_kernel(Layout L, GradSrc2 src, int B, Opt op, Opt ov, Work w) {
  const int64_t e = (int64_t)blockIdx.x * THREADS + threadIdx.x;
  if (e < L.off[NVARS]) {
    int v = NVARS - 1;
    while (e < L.off[v]) --v;
    const int l = v / 2;
    const bool hp = has_p(v), hv = has_v(v);
    float gp = 0.f, gv = 0.f;
    if (hp && hv) {
      float g[2];
      elem_grad(L, src.p, v, e, {src.p.d[l], src.dv[l]}, B, g);
      gp = g[0];
      gv = g[1];
    } else {
      float g[1];
      elem_grad(L, src.p, v, e, {src.p.d[l]}, B, g);
      if (hp) gp = g[0];
      else gv = g[0];
    }
    op.grad[e] = gp;
    ov.grad[e] = gv;
    if (FUSED) {
      if (hv) rms_step(ov, e, gv);
      if (hp) rms_step(op, e, gp);
    }
  }
  loss_sums(w.lossrow, w.losses, B, blockIdx.x == 0);
}

// One block per variable.  CLIP: tf.clip_by_norm on each cost's tensor, scale = clip / max(||g||_2, clip), the two sums of
// squares in block_sum's order, walked as one tree.  Then the value step and the policy step, each where its optimizer has a
// slot.  (Two clip_and_step calls, one per optimizer, give the same bits and walk the variable twice: the clipped step took
// 462 us instead of 425, profiles/vecnet_device_half.txt.)
template <bool CLIP>
__global__ __launch_bounds__(THREADS) void mlp_update_dual_kernel(Layout L, Opt op, Opt ov) {
  __shared__ float shp[THREADS];
  __shared__ float shv[THREADS];
  const int var = blockIdx.x;
  const bool hp = has_p(var), hv = has_v(var);
  const int64_t lo = L.off[var], hi = L.off[var + 1];
  float scale_p = 1.f, scale_v = 1.f;
  if (CLIP) {
    float sp = 0.f, sv = 0.f;
    for (int64_t i = lo + threadIdx.x; i < hi; i += THREADS) {
      sp += op.grad[i] * op.grad[i];
      sv += ov.grad[i] * ov.grad[i];
    }
    shp[threadIdx.x] = sp;
    shv[threadIdx.x] = sv;
    __syncthreads();
    for (int h = THREADS / 2; h > 0; h >>= 1) {
      if (threadIdx.x < h) {
        shp[threadIdx.x] += shp[threadIdx.x + h];
        shv[threadIdx.x] += shv[threadIdx.x + h];
      }
      __syncthreads();
    }
    scale_p = op.clip / fmaxf(sqrtf(shp[0]), op.clip);
    scale_v = ov.clip / fmaxf(sqrtf(shv[0]), ov.clip);
  }
  for (int64_t i = lo + threadIdx.x; i < hi; i += THREADS) {
    if (hv) {
      float g = ov.grad[i];
      if (CLIP) g *= scale_v;
      rms_step(ov, i, g);
    }
    if (hp) {
      float g = op.grad[i];
      if (CLIP) g *= scale_p;
      rms_step(op, i, g);
    }
  }
}

__global__ void mlp_loss_kernel(Work w, int B) { loss_sums(w.lossrow, w.losses, B); }

// ------------------------------------------------------------------ host side

}  // namespace ga3c_vec

using namespace ga3c_vec;

struct ga3c_mlp : Net {
  ga3c_mlp_config cfg;
  Layout L;
  WorkDual w{};                   // del_v: dual only
  float* work_base = nullptr;
  ga3c_actors::Actors* actors = nullptr;   // Config.DEVICE_AGENTS with DEVICE_PENDULUM: the environments this handle steps itself (ga3c_actors.hpp)

  int alloc_work(size_t B) {      // per-row workspace, one block
    const size_t S = L.S, A = L.A;
    std::vector<size_t> widths = {S, 4, 256, 256, 100, 64, 4, 256, 256, 100, 64, 1, 2 * A, A, 1, 2 * A, 3};
    std::vector<float**> dst = {&w.x, &w.act[0], &w.act[1], &w.act[2], &w.act[3], &w.act[4], &w.del[0], &w.del[1], &w.del[2],
                                &w.del[3], &w.del[4], &w.v, &w.z, &w.p, &w.dv, &w.dz, &w.lossrow};
    if (dual)
      for (int l = 0; l < NTRUNK; ++l) {
        widths.push_back((size_t)TRUNK_OUT[l]);
        dst.push_back(&w.del_v[l]);
      }
    return carve_rows(B, widths, dst, &work_base, &w.losses);
  }

  void free_work() { (void)hipFree(work_base); }

  GradSrc grad_src() const {
    GradSrc g;
    const int A = L.A;
    g.in[0] = w.x;
    for (int l = 1; l < NTRUNK; ++l) g.in[l] = w.act[l - 1];
    g.in[5] = g.in[6] = g.in[7] = w.act[4];
    for (int l = 0; l < NTRUNK; ++l) {
      g.d[l] = w.del[l];
      g.d_ld[l] = TRUNK_OUT[l];
    }
    g.d[5] = w.dv;       g.d_ld[5] = 1;
    g.d[6] = w.dz;       g.d_ld[6] = 2 * A;
    g.d[7] = w.dz + A;   g.d_ld[7] = 2 * A;
    return g;
  }

  GradSrc2 grad_src2() const {
    GradSrc2 g;
    g.p = grad_src();
    for (int l = 0; l < NLAYERS; ++l) g.dv[l] = l < NTRUNK ? w.del_v[l] : g.p.d[l];
    return g;
  }

  Opt value_opt(const Opt& o) const {   // the value optimizer: the policy optimizer's constants on arenas 4 / 5 / 6
    Opt q = o;
    q.ms = arena[4]; q.mom = arena[5]; q.grad = arena[6];
    return q;
  }

  void rows(int mode, const Input& in, int B, float beta, float* p, float* v, float* z) {
    if (dual && mode == TRAIN) {
      hipLaunchKernelGGL((mlp_tile_kernel<TRAIN_DUAL, WorkDual>), dim3((B + TILE - 1) / TILE), dim3(THREADS), 0, st, L,
                         (const float*)arena[0], in, (const float*)d_y, (const float*)d_a, B, beta, w, p, v, z);
      return;
    }
    const auto kernel = mode == PREDICT ? mlp_tile_kernel<PREDICT> : mode == EVAL ? mlp_tile_kernel<EVAL> : mlp_tile_kernel<TRAIN>;
    const float* y = mode == PREDICT ? nullptr : d_y;
    const float* a = mode == PREDICT ? nullptr : d_a;
    hipLaunchKernelGGL(kernel, dim3((B + TILE - 1) / TILE), dim3(THREADS), 0, st, L, (const float*)arena[0], in, y, a, B, beta,
                       (const Work&)w, p, v, z);
  }

  void wgrad(int B, const Opt& o, bool fused) {
    if (dual) {
      const auto kernel2 = fused ? mlp_wgrad_dual_kernel<true> : mlp_wgrad_dual_kernel<false>;
      hipLaunchKernelGGL(kernel2, dim3((int)((n + THREADS - 1) / THREADS)), dim3(THREADS), 0, st, L, grad_src2(), B, o,
                         value_opt(o), w);
      return;
    }
    const auto kernel = fused ? mlp_wgrad_kernel<true> : mlp_wgrad_kernel<false>;
    hipLaunchKernelGGL(kernel, dim3((int)((n + THREADS - 1) / THREADS)), dim3(THREADS), 0, st, L, grad_src(), B, o, w);
  }

  void update(const Opt& o, bool clipped) {
    if (dual) {
      const auto kernel2 = clipped ? mlp_update_dual_kernel<true> : mlp_update_dual_kernel<false>;
      hipLaunchKernelGGL(kernel2, dim3(NVARS), dim3(THREADS), 0, st, L, o, value_opt(o));
      return;
    }
    const auto kernel = clipped ? mlp_update_kernel<true> : mlp_update_kernel<false>;
    hipLaunchKernelGGL(kernel, dim3(NVARS), dim3(THREADS), 0, st, L, o);
  }

  void loss(int B) { hipLaunchKernelGGL(mlp_loss_kernel, dim3(1), dim3(64), 0, st, w, B); }
};

namespace {

const char* const DEL_NAMES[NTRUNK] = {"dpd1", "dpd2", "dpd3", "dpd4", "dd1"};

int64_t width_of(const ga3c_mlp* m, const std::string& name) {
  const int S = m->L.S, A = m->L.A;
  static const std::map<std::string, int> fixed = {{"pd1", 4}, {"pd2", 256}, {"pd3", 256}, {"pd4", 100}, {"d1", 64},
                                                   {"dpd1", 4}, {"dpd2", 256}, {"dpd3", 256}, {"dpd4", 100}, {"dd1", 64},
                                                   {"v", 1}, {"dv", 1}, {"lossrow", 3}};
  auto it = fixed.find(name);
  if (it != fixed.end()) return it->second;
  for (int l = 0; l < NTRUNK; ++l)                             // dd1_v, dpd4_v ... dpd1_v: the value stream, dual only
    if (m->dual && name == std::string(DEL_NAMES[l]) + "_v") return TRUNK_OUT[l];
  if (name == "x") return S;
  if (name == "p") return A;
  if (name == "z" || name == "dz") return 2 * A;
  return -1;
}

float* work_ptr(ga3c_mlp* m, const std::string& name) {
  const char* acts[NTRUNK] = {"pd1", "pd2", "pd3", "pd4", "d1"};
  for (int l = 0; l < NTRUNK; ++l) {
    if (name == acts[l]) return m->w.act[l];
    if (name == DEL_NAMES[l]) return m->w.del[l];
    if (m->dual && name == std::string(DEL_NAMES[l]) + "_v") return m->w.del_v[l];
  }
  if (name == "x") return m->w.x;
  if (name == "v") return m->w.v;
  if (name == "p") return m->w.p;
  if (name == "z") return m->w.z;
  if (name == "dv") return m->w.dv;
  if (name == "dz") return m->w.dz;
  if (name == "lossrow") return m->w.lossrow;
  return nullptr;
}

}  // namespace

extern "C" {

int ga3c_mlp_create(const ga3c_mlp_config* cfg, ga3c_mlp** out) {
  if (!cfg || !out) return fail(GA3C_EINVAL, "null argument");
  *out = nullptr;
  CHK(check_dims(*cfg, MAX_S, MAX_A, 65536));
  if (!(cfg->flags & GA3C_FLAG_CONTINUOUS))
    return fail(GA3C_EINVAL, "the vector-state network has the angle-output head only: GA3C_FLAG_CONTINUOUS is required");
  if (cfg->flags & ~(uint32_t)(GA3C_FLAG_CONTINUOUS | GA3C_FLAG_GRAD_CLIP | GA3C_FLAG_DUAL_RMSPROP))
    return fail(GA3C_EINVAL,
                "flags 0x%x: only GA3C_FLAG_CONTINUOUS, GA3C_FLAG_GRAD_CLIP and GA3C_FLAG_DUAL_RMSPROP apply to the vector-state "
                "network", cfg->flags);
  CHK(check_device(*cfg));
  ga3c_mlp* m = new (std::nothrow) ga3c_mlp();
  if (!m) return fail(GA3C_EINVAL, "out of host memory");
  m->cfg = *cfg;
  m->kind = "vector-state network";
  m->ZW = 2 * cfg->num_actions;
  m->L = make_layout(cfg->state_dim, cfg->num_actions);
  for (int l = 0; l < NLAYERS; ++l) m->add_dense(VAR_NAMES[2 * l], VAR_NAMES[2 * l + 1], m->L.off[2 * l], m->L.in[l], m->L.out[l]);
  m->dual = (cfg->flags & GA3C_FLAG_DUAL_RMSPROP) != 0;
  if (m->dual) {    // the trunk has both optimizers' slots; the value head (the two variables behind it) and the policy head their own
    const int V0 = 2 * NTRUNK, P0 = V0 + 2;
    for (int v = 0; v < NVARS; ++v) ga3c_ckpt::dual_members(&m->vars[v], v < P0, v < V0 || v >= P0);
  }
  return create(m, out);
}

int ga3c_mlp_destroy(ga3c_mlp* m) {
  if (m) {
    (void)hipSetDevice(m->device);
    ga3c_actors::actors_drop(m);      // whatever state the stream is in: the handle goes on to be destroyed
  }
  return destroy(m);
}

int ga3c_mlp_param_count(ga3c_mlp* m, int64_t* count) { return param_count(m, count); }

int ga3c_mlp_get_arena(ga3c_mlp* m, int32_t which, float* out, int64_t count) { return get_arena(m, which, out, count); }

int ga3c_mlp_set_arena(ga3c_mlp* m, int32_t which, const float* in, int64_t count) { return set_arena(m, which, in, count); }

int ga3c_mlp_get_step(ga3c_mlp* m, int64_t* step) { return get_step(m, step); }

int ga3c_mlp_set_step(ga3c_mlp* m, int64_t step) { return set_step(m, step); }

int32_t ga3c_mlp_num_params(ga3c_mlp* m) { return num_params(m); }

const char* ga3c_mlp_param_name(ga3c_mlp* m, int32_t index) { return param_name(m, index); }

int ga3c_mlp_param_info(ga3c_mlp* m, const char* name, int64_t* offset, int64_t* count, int32_t* ndim, int64_t shape[4]) {
  return param_info(m, name, offset, count, ndim, shape);
}

int ga3c_mlp_get_param(ga3c_mlp* m, const char* name, int32_t which, float* out, int64_t count) {
  return param_copy(m, name, which, out, nullptr, count);
}

int ga3c_mlp_set_param(ga3c_mlp* m, const char* name, int32_t which, const float* in, int64_t count) {
  return param_copy(m, name, which, nullptr, in, count);
}

int ga3c_mlp_save(ga3c_mlp* m, const char* path) { return save(m, path); }

// An image-network file holds no dense11_p/w: refused before anything is written.  A two-optimizer file holds every member
// of a single-optimizer one (the trunk's value slots under the same names), so a single-optimizer network tells it by the
// policy optimizer's first trunk slot; a single-optimizer file lacks that member and a dual network refuses it for that.
int ga3c_mlp_load(ga3c_mlp* m, const char* path) {
  if (!m || !path) return fail(GA3C_EINVAL, "null argument");
  std::map<std::string, ga3c_ckpt::Member> members;
  CHK(read_checkpoint(path, &members));
  if (!m->dual && members.count("dense11_p/w/RMSProp_2:0"))
    return fail(GA3C_ESTATE, "%s is a DUAL_RMSPROP checkpoint; this network has one optimizer", path);
  return load(m, path, members);
}

int ga3c_mlp_predict(ga3c_mlp* m, const float* x, int32_t batch, float* p, float* v, float* z) {
  return predict(m, x, batch, p, v, z);
}

int ga3c_mlp_train(ga3c_mlp* m, const float* x, const float* y_r, const float* a, int32_t batch, float learning_rate,
                   float beta, float* losses) {
  return train_common(m, x, nullptr, y_r, a, batch, true, learning_rate, beta, losses);
}

int ga3c_mlp_compute_grads(ga3c_mlp* m, const float* x, const float* y_r, const float* a, int32_t batch, float beta,
                           float* losses) {
  return train_common(m, x, nullptr, y_r, a, batch, false, 0.f, beta, losses);
}

int ga3c_mlp_apply_grads(ga3c_mlp* m, float learning_rate) { return apply_grads(m, learning_rate); }

int ga3c_mlp_evaluate(ga3c_mlp* m, const float* x, const int64_t* offsets, const float* y_r, const float* a, int32_t batch,
                      float beta, float* losses, float* pd1, float* pd2, float* d1, float* v, float* p) {
  if (!m) return fail(GA3C_EINVAL, "bad argument");
  return evaluate(m, x, offsets, y_r, a, batch, beta, losses, {{pd1, m->w.act[0], 4}, {pd2, m->w.act[1], 256}, {d1, m->w.act[4], HID}},
                  v, p);
}

int ga3c_mlp_register_host(ga3c_mlp* m, void* base, int64_t bytes) { return register_host(m, base, bytes); }

int ga3c_mlp_unregister_host(ga3c_mlp* m) { return unregister_host(m); }

int ga3c_mlp_predict_gather(void* net, const int64_t* offsets, int32_t batch, int32_t u8, float* p, float* v, float* z) {
  return predict_gather(static_cast<ga3c_mlp*>(net), offsets, batch, u8, p, v, z);
}

int ga3c_mlp_predict_gather_begin(void* net, const int64_t* offsets, int32_t batch, int32_t u8, int32_t* ticket) {
  return predict_gather_begin(static_cast<ga3c_mlp*>(net), offsets, batch, u8, ticket);
}

int ga3c_mlp_predict_gather_end(void* net, int32_t ticket, int32_t batch, float* p, float* v) {
  return predict_gather_end(static_cast<ga3c_mlp*>(net), ticket, batch, p, v);
}

int ga3c_mlp_train_gather(ga3c_mlp* m, const int64_t* offsets, int32_t u8, const float* y_r, const float* a, int32_t batch,
                          float learning_rate, float beta, float* losses) {
  return train_gather(m, offsets, u8, y_r, a, batch, learning_rate, beta, losses);
}

int ga3c_mlp_upload(ga3c_mlp* m, const float* x, const float* y_r, const float* a, int32_t batch) {
  return upload(m, x, y_r, a, batch);
}

int ga3c_mlp_time_resident(ga3c_mlp* m, int32_t mode, int32_t batch, int32_t iters, float learning_rate, float beta,
                           float* elapsed_ms) {
  return time_resident(m, mode, batch, iters, learning_rate, beta, elapsed_ms);
}

int ga3c_mlp_fetch(ga3c_mlp* m, const char* name, float* out, int64_t count) {
  if (!m || !name || !out) return fail(GA3C_EINVAL, "null argument");
  const int64_t wd = width_of(m, name);
  const float* src = work_ptr(m, name);
  if (wd < 0 || !src) return fail(GA3C_EINVAL, "no activation named %s", name);
  return fetch(m, name, src, wd, out, count);
}

// ---- device actors: Pendulum environments stepped by this handle, ga3c_actors.hpp

int ga3c_mlp_actors_create(ga3c_mlp* m, int32_t n, int32_t time_max, double discount, int64_t seed) {
  return ga3c_actors::actors_create<ga3c_actors::Pendulum>(m, n, time_max, discount, seed);
}

int ga3c_mlp_actors_destroy(ga3c_mlp* m) { return ga3c_actors::actors_destroy(m); }

int ga3c_mlp_actors_run(ga3c_mlp* m, int32_t steps, float learning_rate, float beta, int32_t train, int64_t* out_stats) {
  return ga3c_actors::actors_run<ga3c_actors::Pendulum>(m, steps, learning_rate, beta, train, out_stats);
}

int ga3c_mlp_actors_episodes(ga3c_mlp* m, double* total_reward, int64_t* total_length, int32_t max, int32_t* count) {
  return ga3c_actors::actors_episodes(m, total_reward, total_length, max, count);
}

int ga3c_mlp_actors_get(ga3c_mlp* m, const char* name, void* out, int64_t bytes) {
  if (!out) return fail(GA3C_EINVAL, "null argument");
  return ga3c_actors::actors_access(m, name, out, nullptr, bytes);
}

int ga3c_mlp_actors_set(ga3c_mlp* m, const char* name, const void* in, int64_t bytes) {
  if (!in) return fail(GA3C_EINVAL, "null argument");
  return ga3c_actors::actors_access(m, name, nullptr, in, bytes);
}

}  // extern "C"
