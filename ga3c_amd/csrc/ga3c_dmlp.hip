// ga3c_dmlp.hip -- the discrete-action vector-state network of reference NetworkVP_discrate.py:39-130 (GAME = 'CartPole-v0')
// on gfx950, and its C ABI (ga3c_dmlp_*, include/ga3c_abi.h).  DESIGN.md 8g.
//
//   x[B,S] -> dense1_<i>_p (w_i, sigmoid), i = 1..L -> logits_v (1, linear) | logits_p (A, linear) -> softmax
//
// The layer list is data (1..8 layers of 1..256 units) and has two wirings.  chained = 0 is the reference as written
// (:52-56): every layer reads x, only the last one reaches the heads, the others are variables that nothing reads.
// chained = 1: layer i reads layer i - 1.
//
// Kernels (all f32, one workgroup of 256 threads per 16-row tile where rows are involved).  The tile's layout in LDS, who
// owns which sum and the order of its additions are ga3c_tile.hpp's; here are the layer list and the head.
//   dmlp_tile_kernel<PREDICT>  forward of one tile (load_input_tile, tile_fma).
//   dmlp_tile_kernel<TRAIN>    the same forward, the softmax head's loss row and dz / dv, and the deltas back through the
//                              live layers (dense_bwd_split); activations and deltas go to HBM for the weight gradients.
//                              <EVAL>: forward + loss.
//   dmlp_wgrad_kernel<FUSED>   one thread per arena element sums its gradient over the rows in row order (sum_rows,
//                              dot_rows); FUSED (no clipping) applies rms_step to the element at once.  An element of a dead
//                              variable gets gradient 0 and no step.  Block 0 also: loss_sums.
//   dmlp_update_kernel<CLIP>   one block per live variable: clip_and_step (tf.clip_by_average_norm, RMSProp).
// A train step is 2 launches without USE_GRAD_CLIP and 3 with it; a prediction is 1; an evaluation 2.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "ga3c_actors.hpp"
#include "ga3c_tile.hpp"
#include "ga3c_vecnet.hpp"

namespace ga3c_dvec {

using namespace ga3c_vecnet;   // Input, Opt, PREDICT / EVAL / TRAIN and the host half
using namespace ga3c_tile;     // TILE and the device half

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

struct Head {          // the loss of NetworkVP_discrate.py:61-85
  float beta, log_eps, min_policy;
  int log_softmax;
};

// out[j][r] = sigmoid(b[j] + sum_k in[k][r] W[k][j]) for the tile; thread j owns column j (coalesced weight reads) and adds
// in k order.  gout (may be null): the same values, row-major [B][N], rows < nrows only.  ga3c_tile.hpp's dense_fwd written
// out: with the sigmoid as that function's epilogue the compiler orders the 16 of them otherwise, and a 128-row prediction
// through two 256-wide layers took 61.0 us instead of 60.1 (profiles/vecnet_device_half.txt).
__device__ void dense_fwd(const float* __restrict__ W, const float* __restrict__ bias, int K, int N, const float* in, float* out,
                          float* gout, int row0, int nrows) {
  for (int j = threadIdx.x; j < N; j += THREADS) {
    float acc[TILE];
    const float b = bias[j];
#pragma unroll
    for (int r = 0; r < TILE; ++r) acc[r] = b;
    for (int k = 0; k < K; ++k) tile_fma(acc, in + k * TILE, W[(size_t)k * N + j]);
#pragma unroll
    for (int r = 0; r < TILE; ++r) {
      const float h = sigm(acc[r]);
      out[j * TILE + r] = h;
      if (gout && r < nrows) gout[(size_t)(row0 + r) * N + j] = h;
    }
  }
  __syncthreads();
}

// gin[k][r] = s (1 - s) sum_j W(k, j) gout[j][r] for k < K <= 256 (dense_bwd_split, ga3c_tile.hpp, whose partials `scratch` holds), s =
// gact[row][k] the layer's sigmoid output as this workgroup wrote it to HBM in the forward pass.  gin_lds may be null.
template <class WF>
__device__ void dense_bwd(WF W, int K, int N, const float* gout, const float* gact, float* gin_lds, float* gin_glob, int row0,
                          int nrows, float* scratch) {
  dense_bwd_split<THREADS>(W, K, N, gout, scratch, [&](int k, int r, float s) {
    float g = 0.f;
    if (r < nrows) {
      const float h = gact[(size_t)(row0 + r) * K + k];
      g = s * (h * (1.0f - h));
      gin_glob[(size_t)(row0 + r) * K + k] = g;
    }
    if (gin_lds) gin_lds[k * TILE + r] = g;
  });
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

  load_input_tile<THREADS, KEEP>(in, S, row0, nrows, xin, w.x);
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
    for (int k = 0; k < H; ++k) tile_fma(acc, cur + k * TILE, j == 0 ? theta[ovw + k] : theta[opw + (int64_t)k * A + j - 1]);
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
  loss_sums(w.lossrow, w.losses, B, blockIdx.x == 0);
}

// One block per variable; a dead variable's block returns at once.  clip_and_step (ga3c_tile.hpp).
template <bool CLIP>
__global__ __launch_bounds__(THREADS) void dmlp_update_kernel(Layout L, Opt o) {
  __shared__ float sh[THREADS];
  if (!L.live[blockIdx.x / 2]) return;
  clip_and_step<THREADS, CLIP>(L.off[blockIdx.x], L.off[blockIdx.x + 1], o, sh);
}

__global__ void dmlp_loss_kernel(Work w, int B) { loss_sums(w.lossrow, w.losses, B); }

// ------------------------------------------------------------------ host side

}  // namespace ga3c_dvec

using namespace ga3c_dvec;

struct ga3c_dmlp : Net {
  ga3c_dmlp_config cfg;
  Layout L;
  Head head{};
  Work w{};
  float* work_base = nullptr;
  Layout* d_layout = nullptr;     // L and w as the row kernel reads them
  Work* d_work = nullptr;
  ga3c_actors::Actors* actors = nullptr;   // Config.DEVICE_AGENTS: the environments this handle steps itself (ga3c_actors.hpp)

  int alloc_work(size_t B) {      // per-row workspace, one block; the dead layers of chained = 0 get no rows
    const size_t S = L.S, A = L.A;
    std::vector<size_t> widths = {S, 1, A, A, 1, A, 3};
    std::vector<float**> dst = {&w.x, &w.v, &w.z, &w.p, &w.dv, &w.dz, &w.lossrow};
    for (int l = 0; l < L.L; ++l)
      if (L.live[l]) {
        widths.push_back((size_t)L.out[l]); dst.push_back(&w.act[l]);
        widths.push_back((size_t)L.out[l]); dst.push_back(&w.del[l]);
      }
    CHK(carve_rows(B, widths, dst, &work_base, &w.losses));
    CHK(dalloc(&d_layout, 1));
    CHK(dalloc(&d_work, 1));
    HIPCHK(hipMemcpy(d_layout, &L, sizeof(Layout), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_work, &w, sizeof(Work), hipMemcpyHostToDevice));
    return GA3C_OK;
  }

  void free_work() {
    (void)hipFree(work_base);
    (void)hipFree(d_layout);
    (void)hipFree(d_work);
  }

  GradSrc grad_src() const {
    GradSrc g;
    memset(&g, 0, sizeof g);
    const int NL = L.L;
    for (int l = 0; l < NL; ++l) {
      g.in[l] = (L.chained && l > 0) ? w.act[l - 1] : w.x;
      g.d[l] = w.del[l];
    }
    g.in[NL] = g.in[NL + 1] = w.act[NL - 1];
    g.d[NL] = w.dv;
    g.d[NL + 1] = w.dz;
    return g;
  }

  void rows(int mode, const Input& in, int B, float beta, float* p, float* v, float* z) {
    const auto kernel = mode == PREDICT ? dmlp_tile_kernel<PREDICT> : mode == EVAL ? dmlp_tile_kernel<EVAL> : dmlp_tile_kernel<TRAIN>;
    const float* y = mode == PREDICT ? nullptr : d_y;
    const float* a = mode == PREDICT ? nullptr : d_a;
    Head hd = head;
    hd.beta = beta;
    hipLaunchKernelGGL(kernel, dim3((B + TILE - 1) / TILE), dim3(THREADS), 0, st, (const Layout*)d_layout, (const float*)arena[0],
                       in, y, a, B, hd, (const Work*)d_work, p, v, z);
  }

  void wgrad(int B, const Opt& o, bool fused) {
    const auto kernel = fused ? dmlp_wgrad_kernel<true> : dmlp_wgrad_kernel<false>;
    hipLaunchKernelGGL(kernel, dim3((int)((n + THREADS - 1) / THREADS)), dim3(THREADS), 0, st, L, grad_src(), B, o, w);
  }

  void update(const Opt& o, bool clipped) {
    const auto kernel = clipped ? dmlp_update_kernel<true> : dmlp_update_kernel<false>;
    hipLaunchKernelGGL(kernel, dim3((int)vars.size()), dim3(THREADS), 0, st, L, o);
  }

  void loss(int B) { hipLaunchKernelGGL(dmlp_loss_kernel, dim3(1), dim3(64), 0, st, w, B); }
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

std::string layer_name(int i) { return "dense1_" + std::to_string(i + 1) + "_p"; }

}  // namespace

extern "C" {

int ga3c_dmlp_create(const ga3c_dmlp_config* cfg, ga3c_dmlp** out) {
  if (!cfg || !out) return fail(GA3C_EINVAL, "null argument");
  *out = nullptr;
  CHK(check_dims(*cfg, MAX_S, MAX_A, 65536));
  if (cfg->num_layers < 1 || cfg->num_layers > MAX_L) return fail(GA3C_EINVAL, "num_layers %d outside [1,%d]", cfg->num_layers, MAX_L);
  for (int l = 0; l < cfg->num_layers; ++l)
    if (cfg->widths[l] < 1 || cfg->widths[l] > WIDE)
      return fail(GA3C_EINVAL, "width %d of layer %d outside [1,%d]", cfg->widths[l], l + 1, WIDE);
  if (cfg->chained != 0 && cfg->chained != 1) return fail(GA3C_EINVAL, "chained %d is neither 0 nor 1", cfg->chained);
  if (cfg->flags & ~(uint32_t)(GA3C_FLAG_LOG_SOFTMAX | GA3C_FLAG_GRAD_CLIP))
    return fail(GA3C_EINVAL, "flags 0x%x: only GA3C_FLAG_LOG_SOFTMAX and GA3C_FLAG_GRAD_CLIP apply to the discrete vector-state "
                             "network", cfg->flags);
  CHK(check_device(*cfg));
  ga3c_dmlp* m = new (std::nothrow) ga3c_dmlp();
  if (!m) return fail(GA3C_EINVAL, "out of host memory");
  m->cfg = *cfg;
  m->kind = "discrete vector-state network";
  m->ZW = cfg->num_actions;
  m->L = make_layout(cfg->state_dim, cfg->num_actions, cfg->num_layers, cfg->widths, cfg->chained);
  for (int l = 0; l < cfg->num_layers + 2; ++l) {
    const std::string base = l < cfg->num_layers ? layer_name(l) : (l == cfg->num_layers ? "logits_v" : "logits_p");
    m->add_dense(base + "/w", base + "/b", m->L.off[2 * l], m->L.in[l], m->L.out[l]);
  }
  m->head.beta = 0.f;
  m->head.log_eps = cfg->log_epsilon;
  m->head.min_policy = cfg->min_policy;
  m->head.log_softmax = (cfg->flags & GA3C_FLAG_LOG_SOFTMAX) != 0;
  return create(m, out);
}

int ga3c_dmlp_destroy(ga3c_dmlp* m) {
  if (m) {
    (void)hipSetDevice(m->device);
    ga3c_actors::actors_drop(m);      // whatever state the stream is in: the handle goes on to be destroyed
  }
  return destroy(m);
}

int ga3c_dmlp_param_count(ga3c_dmlp* m, int64_t* count) { return param_count(m, count); }

int ga3c_dmlp_get_arena(ga3c_dmlp* m, int32_t which, float* out, int64_t count) { return get_arena(m, which, out, count); }

int ga3c_dmlp_set_arena(ga3c_dmlp* m, int32_t which, const float* in, int64_t count) { return set_arena(m, which, in, count); }

int ga3c_dmlp_get_step(ga3c_dmlp* m, int64_t* step) { return get_step(m, step); }

int ga3c_dmlp_set_step(ga3c_dmlp* m, int64_t step) { return set_step(m, step); }

int32_t ga3c_dmlp_num_params(ga3c_dmlp* m) { return num_params(m); }

const char* ga3c_dmlp_param_name(ga3c_dmlp* m, int32_t index) { return param_name(m, index); }

int ga3c_dmlp_param_info(ga3c_dmlp* m, const char* name, int64_t* offset, int64_t* count, int32_t* ndim, int64_t shape[4]) {
  return param_info(m, name, offset, count, ndim, shape);
}

int ga3c_dmlp_get_param(ga3c_dmlp* m, const char* name, int32_t which, float* out, int64_t count) {
  return param_copy(m, name, which, out, nullptr, count);
}

int ga3c_dmlp_set_param(ga3c_dmlp* m, const char* name, int32_t which, const float* in, int64_t count) {
  return param_copy(m, name, which, nullptr, in, count);
}

int ga3c_dmlp_save(ga3c_dmlp* m, const char* path) { return save(m, path); }

int ga3c_dmlp_load(ga3c_dmlp* m, const char* path) {
  if (!m || !path) return fail(GA3C_EINVAL, "null argument");
  std::map<std::string, ga3c_ckpt::Member> members;
  CHK(read_checkpoint(path, &members));
  // a file of another network kind holds no dense1_1_p/w; one of this kind with more layers holds dense1_<L+1>_p/w:
  // both refused before anything is written
  if (members.count(layer_name(m->L.L) + "/w:0"))
    return fail(GA3C_ESTATE, "%s holds %s/w: a network of more than this one's %d layers", path, layer_name(m->L.L).c_str(), m->L.L);
  return load(m, path, members);
}

int ga3c_dmlp_predict(ga3c_dmlp* m, const float* x, int32_t batch, float* p, float* v, float* z) {
  return predict(m, x, batch, p, v, z);
}

int ga3c_dmlp_train(ga3c_dmlp* m, const float* x, const float* y_r, const float* a, int32_t batch, float learning_rate,
                    float beta, float* losses) {
  return train_common(m, x, nullptr, y_r, a, batch, true, learning_rate, beta, losses);
}

int ga3c_dmlp_compute_grads(ga3c_dmlp* m, const float* x, const float* y_r, const float* a, int32_t batch, float beta,
                            float* losses) {
  return train_common(m, x, nullptr, y_r, a, batch, false, 0.f, beta, losses);
}

int ga3c_dmlp_apply_grads(ga3c_dmlp* m, float learning_rate) { return apply_grads(m, learning_rate); }

int ga3c_dmlp_evaluate(ga3c_dmlp* m, const float* x, const int64_t* offsets, const float* y_r, const float* a, int32_t batch,
                       float beta, float* losses, float* lastdense, float* v, float* p) {
  if (!m) return fail(GA3C_EINVAL, "bad argument");
  const int last = m->L.L - 1;
  return evaluate(m, x, offsets, y_r, a, batch, beta, losses, {{lastdense, m->w.act[last], (size_t)m->L.out[last]}}, v, p);
}

int ga3c_dmlp_register_host(ga3c_dmlp* m, void* base, int64_t bytes) { return register_host(m, base, bytes); }

int ga3c_dmlp_unregister_host(ga3c_dmlp* m) { return unregister_host(m); }

int ga3c_dmlp_predict_gather(void* net, const int64_t* offsets, int32_t batch, int32_t u8, float* p, float* v, float* z) {
  return predict_gather(static_cast<ga3c_dmlp*>(net), offsets, batch, u8, p, v, z);
}

int ga3c_dmlp_predict_gather_begin(void* net, const int64_t* offsets, int32_t batch, int32_t u8, int32_t* ticket) {
  return predict_gather_begin(static_cast<ga3c_dmlp*>(net), offsets, batch, u8, ticket);
}

int ga3c_dmlp_predict_gather_end(void* net, int32_t ticket, int32_t batch, float* p, float* v) {
  return predict_gather_end(static_cast<ga3c_dmlp*>(net), ticket, batch, p, v);
}

int ga3c_dmlp_train_gather(ga3c_dmlp* m, const int64_t* offsets, int32_t u8, const float* y_r, const float* a, int32_t batch,
                           float learning_rate, float beta, float* losses) {
  return train_gather(m, offsets, u8, y_r, a, batch, learning_rate, beta, losses);
}

int ga3c_dmlp_upload(ga3c_dmlp* m, const float* x, const float* y_r, const float* a, int32_t batch) {
  return upload(m, x, y_r, a, batch);
}

int ga3c_dmlp_time_resident(ga3c_dmlp* m, int32_t mode, int32_t batch, int32_t iters, float learning_rate, float beta,
                            float* elapsed_ms) {
  return time_resident(m, mode, batch, iters, learning_rate, beta, elapsed_ms);
}

int ga3c_dmlp_fetch(ga3c_dmlp* m, const char* name, float* out, int64_t count) {
  if (!m || !name || !out) return fail(GA3C_EINVAL, "null argument");
  int64_t wd = -1;
  const float* src = work_ptr(m, name, &wd);
  if (!src) return fail(GA3C_EINVAL, "no activation named %s (a layer nothing reads has none)", name);
  return fetch(m, name, src, wd, out, count);
}

// ---- device actors: CartPole environments stepped by this handle, ga3c_actors.hpp

int ga3c_dmlp_actors_create(ga3c_dmlp* m, int32_t n, int32_t time_max, double discount, int64_t seed) {
  return ga3c_actors::actors_create<ga3c_actors::CartPole>(m, n, time_max, discount, seed);
}

int ga3c_dmlp_actors_destroy(ga3c_dmlp* m) { return ga3c_actors::actors_destroy(m); }

int ga3c_dmlp_actors_run(ga3c_dmlp* m, int32_t steps, float learning_rate, float beta, int32_t train, int64_t* out_stats) {
  return ga3c_actors::actors_run<ga3c_actors::CartPole>(m, steps, learning_rate, beta, train, out_stats);
}

int ga3c_dmlp_actors_episodes(ga3c_dmlp* m, double* total_reward, int64_t* total_length, int32_t max, int32_t* count) {
  return ga3c_actors::actors_episodes(m, total_reward, total_length, max, count);
}

int ga3c_dmlp_actors_get(ga3c_dmlp* m, const char* name, void* out, int64_t bytes) {
  if (!out) return fail(GA3C_EINVAL, "null argument");
  return ga3c_actors::actors_access(m, name, out, nullptr, bytes);
}

int ga3c_dmlp_actors_set(ga3c_dmlp* m, const char* name, const void* in, int64_t bytes) {
  if (!in) return fail(GA3C_EINVAL, "null argument");
  return ga3c_actors::actors_access(m, name, nullptr, in, bytes);
}

}  // extern "C"
