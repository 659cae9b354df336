// ga3c_ddpg.hip -- the DDPG networks of reference NetworkDDPG.py (USE_DDPG with CONTINUOUS_INPUT) on gfx950, their train
// step (train_DDPG, :64-98), the replay memory of replay_buffer.py as a ring in HBM, and the C ABI ga3c_ddpg_*
// (include/ga3c_abi.h).  DESIGN.md 8f.
//
//   actor   x[B,S] -> actor_fc1 (400) -> actor_norm1 -> relu -> actor_fc2 (300) -> actor_norm2 -> relu -> actor_output (A, tanh)
//   critic  x -> critic_fc1 (400) -> critic_norm1 -> relu = h;  q = critic_output(relu(h W_fc2 + a W_n2 + b_n2))
//   batch normalisation: gamma (x - moving_mean) / sqrt(moving_variance + 1e-5) + beta (bn_apply below, the one place)
//
// Kernels (all f32, one workgroup of 448 threads per 16-row tile, weights through L2; the tile's layout in LDS, dense_fwd,
// load_input_tile and the fixed-order block_sum are ga3c_tile.hpp's):
// (<NC>: compiled for a handle with one critic and for one with two, below; the critic is blockIdx.y, or blockIdx.x / 10)
//   ddpg_target_kernel<NC>  steps 1-2: actor_target and critic_target on s2, y = r or r + gamma q'
//   ddpg_critic_kernel<NC>  step 3's forward and backward on (s, a): q, dq (either loss form) and the deltas, to HBM
//   ddpg_wgrad_kernel<NC>   one thread per element of a net's trainable variables sums its gradient over the rows in row order
//                           (no atomics); FUSED applies the optimizer step and the soft update of the element's target copy
//   ddpg_update_kernel<NC>  (GA3C_DDPG_GRAD_CLIP) one block per critic variable: tf.clip_by_norm, the step, the soft update
//   ddpg_actor_kernel    steps 4-5: actor(s) + noise, dq/da of the updated critic there, the actor's deltas
//   ddpg_predict_kernel  the online actor alone
//   ddpg_ring_gather_kernel  rows of the registered transport into ring slots
// A train step is 5 launches (6 with clipping); its rows are named by ring slot and read where they lie.
// Prioritised replay (ga3c_ddpg_priorities_create; tests/per_oracle.py is the same statement in numpy):
//   per_fill_kernel       new rows get the largest priority seen
//   per_chunk_sum_kernel  one f64 sum per 1024 slots, in a fixed order
//   per_sample_kernel     one workgroup: scan of the chunk sums, the stratified draw, the importance weights
//   per_update_kernel     one workgroup: pa[slot] = (|y - q| + eps)^alpha from the critic kernel's y and q
// A prioritised step is 8 launches (9 with clipping) and draws its own rows: no host draw, no stamp, nothing to lose.
// Device actors (ga3c_ddpg_actors_create, Config.DEVICE_DDPG; tests/ddpg_actors_oracle.py is the same statement):
//   ddpg_actors_step_kernel<Env, Fork>   one thread per environment: the step (actor_step, the one statement of it) under the
//                                  handle's task, its transition into the ring, the episode record; Fork: the same text compiled
//                                  on the fork's task, for a handle without one
//   ddpg_actors_episodes_kernel    one workgroup: this step's episode records into the episode ring, environment order
//   ddpg_uniform_slots_kernel      a train step's rows without priorities: a stratified draw in integers, on the device
// Twin critics (ga3c_ddpg_twin_create, Config.DDPG_TWIN; tests/td3_oracle.py is the same statement):
//   ddpg_target_kernel<2>      actor_target, the smoothed and clipped target action, both target critics, y from their min
//   ddpg_critic_kernel<2>, ddpg_wgrad_kernel<2>, ddpg_update_kernel<2>      both critics' steps, elements and variables at once
// A twin step is 3 launches (4 with clipping); a policy step, every policy_delay-th, adds ddpg_actor_kernel and the actor's
// ddpg_wgrad_kernel<1>.  Critic 2's variables lie behind the 26 in every arena and are read through a second Layout whose
// critic entries name them (twin_view), so the device functions of one critic serve both; the host's enqueue_step_nc is one
// rule for every handle, a plain step being a twin's at delay 1 and a soft step a twin's with three kernels exchanged.
// An actor step is predict + 2 launches; every launch argument is known to the host, which waits once per actors_run.
// n-step returns (ga3c_ddpg_nstep_create, Config.DDPG_NSTEP; tests/nstep_oracle.py is the same statement):
//   ddpg_actors_nstep_kernel<Env>  actor_step too, the transition into the environment's window of n, and from
//                                  the n-th transition on one ring row per step: the n-step return of the oldest entry, cut at
//                                  an episode's end, and its discount gamma^m into disc[slot]
//   nstep_fill_kernel              disc[slot] = gamma for rows added by hand
// The target kernel reads disc[slot] where a step's rows are ring slots of such a handle, the scalar gamma otherwise.
// Distributional critic (ga3c_ddpg_dist_create, Config.DDPG_DISTRIBUTIONAL; tests/dist_oracle.py is the same statement):
//   ddpg_dist_target_kernel  actor_target and the target critic's atom head on s2, the projection of r + g z onto the support in
//                            gather form (one thread per row and atom, j ascending, no atomics), y and q' as expectations
//   ddpg_dist_critic_kernel  step 3's forward, the softmax, the cross-entropy and its delta (w / B)(p - m), the trunk's backward
//   ddpg_dist_actor_kernel   ddpg_actor_kernel's body with dQ/dlogit_k = p_k (z_k - Q) in the scalar weight's place
// They stand beside the scalar kernels, which compile from the source they had; the launch counts of a step are the same.
// Evaluation episodes (ga3c_ddpg_eval_create, Config.DEVICE_DDPG_EVAL_ENVS; tests/ddpg_eval_oracle.py is the same
// statement):
//   ddpg_eval_kernel<Env, Policy>   one workgroup per 16 evaluation environments walks a whole episode: the policy's forward
//                            without noise (DetPolicy: actor_fwd), the environment's step under the handle's task on the thread's
//                            registers, the f64 sum of the rewards; one launch per evaluation
// Per-environment noise (ga3c_ddpg_envnoise_create, Config.DEVICE_DDPG_NOISE; tests/envnoise_oracle.py is the same
// statement):
//   ddpg_predict_envnoise_kernel  ddpg_predict_kernel's body with every environment's own OU step in its epilogue; launched in
//                                 its place by an actor step under GA3C_DDPG_NOISE_OWN, which stays predict + 2 launches
// PopArt (ga3c_ddpg_popart_create, Config.DDPG_POPART; tests/popart_oracle.py is the same statement):
//   ddpg_popart_kernel   one workgroup between the target and the critic kernel: the f64 sums of y and y^2 in a fixed order, the
//                        new statistics mu, nu (f32 in both arenas, behind the 26 variables), critic_output/W and /b of both
//                        arenas rescaled so that sigma n + mu stays what it was, and yn = (y - mu') / sigma' for the critic step
// The target kernel de-normalises the target critic's output with the statistics it finds; every other kernel runs as it did, on
// yn where y was.  A popart step is 6 launches (7 with clipping, + 3 prioritised).
// The task (ga3c_ddpg_task_create, Config.DEVICE_DDPG_ACTION_BOUND and its four neighbours, DESIGN.md 8t, 8w;
// tests/ddpg_task_oracle.py is the same statement): clip or wrap, the time limit as a truncation, the observation of the reset
// state, the reward's scale and offset.  A PendulumTask in the arguments of the two actor step kernels and of the evaluation
// kernel: a handle without a task passes the fork's values (PendulumTask::fork).  The n-step and the evaluation kernel have no
// other form; the step kernel has a second instantiation that knows those values when it is compiled.
// Soft actor-critic (ga3c_ddpg_soft_create, Config.DDPG_SOFT; tests/sac_oracle.py is the same statement), on a twin
// handle whose actor head is [300, 2A]:
//   ddpg_soft_target_kernel   the ONLINE actor's sample a2, logp2 at s2 (soft_actor_fwd: actor_fwd with the raw head), both target
//                             critics there, y from min q' - alpha logp2
//   ddpg_soft_actor_kernel    the sample a, logp at s, both updated critics one after the other in the same buffers, per row the
//                             smaller one's dq/da, the gradient of (1/B) sum (alpha logp - q) through the sample, the actor's deltas
//   ddpg_soft_wgrad_kernel    the actor's ddpg_wgrad_kernel<1, true> with log_alpha's Adam step riding in it
//   ddpg_soft_predict_kernel  tanh(mu), or the sample under the caller's eps or the counter draws of the row's stream
//   SoftPolicy                ddpg_eval_kernel's policy on such a handle: soft_actor_fwd, a = tanh(mu)
// The critics' kernels are the twin's and the launch counts of a step are the twin's.
// The variables: their names, Layout and twin_view, the table of whatever options a handle carries (make_table),
// the value a variable starts from (initial_value) and the re-lay of an arena from one table to another (relay) are
// ga3c_ddpg_vars.hpp's, host code that knows no device.  The handle keeps its Options; ga3c_ddpg_create and every option's create
// and destroy state the Options they want, and set_table / relay_arenas below are the only code that writes the handle's table
// or replaces its arenas.  Nothing finds a variable by its position: PopArt's statistics and log_alpha are looked up by name at
// their create and kept as offsets.
// The environment, the end of an episode, the episode scan and the host's block, episode queue and fields by name are
// ga3c_actors.hpp's, shared with the rollout actors of ga3c_mlp / ga3c_dmlp; the ring write is this file's.
#include <cmath>
#include <deque>
#include <new>

#include "ga3c_actors.hpp"
#include "ga3c_ddpg_vars.hpp"
#include "ga3c_tile.hpp"
#include "ga3c_uniform.hpp"
#include "ga3c_vecnet.hpp"

namespace ga3c_dd {

using ga3c_vecnet::Input;      // a prediction's row r: S floats at base + (off ? off[r] : r * stride) bytes
using namespace ga3c_tile;     // TILE and the device half

constexpr int THREADS = 448;                 // 7 waves: a 300-wide layer and the 400 rows of a backward pass take one pass each
constexpr int RED = 512;                     // the power of two above it: the leaves of block_sum's tree
constexpr int MAX_S = 64;
constexpr int MAX_A = 32;
constexpr int MAX_B = 4096;                  // rows of a step: per_update_kernel holds their slots in LDS
constexpr float BN_EPS = 1e-5f;
// 1 - beta as the f32 nearest to the real number: 1.0f - 0.999f is off by 1.3e-5 of itself, which Adam's v would carry
constexpr float ADAM_OMB1 = 0.1f, ADAM_OMB2 = 0.001f, ADAM_EPS = 1e-8f;
constexpr double ADAM_B1 = 0.9, ADAM_B2 = 0.999;

// The variables, their names, Layout, make_layout and twin_view: ga3c_ddpg_vars.hpp.

template <class T, int NC>
struct PerCritic { T v[NC]; };     // a kernel argument per critic of a handle with NC of them

// Where a step's rows lie: row i is `rowf` floats at base + (idx ? idx[i] : i) * rowf: s[S] | a[A] | r | done | s2[S].
struct Rows {
  const float* base;
  const int32_t* idx;
  int rowf;
};

struct Noise {         // by value in the kernel arguments: nothing to copy
  float v[MAX_A];
  int wrap;            // GA3C_DDPG_NOISE_NONE: check_bounds(turnaround) on the output
};

// What one critic's step writes.
struct CriticRows {
  float *q, *dq;                               // [B]
  float *xh1, *c1, *dn1, *dh1;                 // [B,400]
  float *c2, *dt;                              // [B,300]
};

// Per-row buffers of the train workspace, row-major [B][width].  Those marked "twin" exist while the handle has twin critics
// (work_table below) and are null otherwise.
struct Work {
  float *y, *qt;                               // [B]
  float *c_x, *c_a;                            // [B,S] [B,A]: the critic step's inputs, kept once for every critic
  CriticRows c[2];                             // c[1] twin: critic 2's
  float *qt1, *qt2;                            // [B] twin: the two target critics' q'
  float *t_eps, *t_a;                          // [B,A] twin: the smoothing noise and the target action it gives
  float *a_xh1, *a_a1, *a_dn1, *a_dh1;         // [B,400]
  float *a_xh2, *a_a2, *a_dn2, *a_dh2;         // [B,300]
  float *a_out, *a_noisy, *g, *dout;           // [B,A]
  float* qstat;                                // {max q, mean q}
};

struct Opt {
  float *theta, *target, *sa, *sb, *grad;
  int adam;                                    // 0: TF-1 ApplyRMSProp on (sa, sb) = (ms, mom); 1: ApplyAdam on (m, v)
  float lr;                                    // RMSProp: the rate; Adam: lr sqrt(1 - b2^t) / (1 - b1^t)
  float omr, mu, eps, clip, tau;
  int apply, soft;
};

// ep(k, r, sum_j W[k][j] gout[j][r]) for k < K; thread k owns row k of W and sums in j order.  (Not dense_bwd_split: that
// would share an A-wide layer's rows among threads and add the partials in another order.)
template <class EP>
__device__ __forceinline__ void dense_bwd(const float* __restrict__ W, int K, int N, const float* gout, EP ep) {
  for (int k = threadIdx.x; k < K; k += THREADS) {
    float acc[TILE];
#pragma unroll
    for (int r = 0; r < TILE; ++r) acc[r] = 0.f;
    const float* __restrict__ wr = W + (size_t)k * N;
    for (int j = 0; j < N; ++j) tile_fma(acc, gout + j * TILE, wr[j]);
#pragma unroll
    for (int r = 0; r < TILE; ++r) ep(k, r, acc[r]);
  }
  __syncthreads();
}

// The reference's batch normalisation (tflearn with its training flag off): -> the normalised value; *n = gamma xhat + beta.
__device__ __forceinline__ float bn_apply(const float* th, const Layout& L, int mm, int mv, int be, int ga, int j, float h, float* n) {
  const float rstd = 1.0f / sqrtf(th[L.off[mv] + j] + BN_EPS);
  const float xh = (h - th[L.off[mm] + j]) * rstd;
  *n = th[L.off[ga] + j] * xh + th[L.off[be] + j];
  return xh;
}
__device__ __forceinline__ float bn_scale(const float* th, const Layout& L, int mv, int ga, int j) {
  return th[L.off[ga] + j] / sqrtf(th[L.off[mv] + j] + BN_EPS);
}

struct ActorKeep { float *xh1, *a1, *xh2, *a2, *out; };    // all null: nothing kept
struct CriticKeep { float *xh1, *c1, *c2; };

// xin [S][16] -> bufA = a1 [400][16], bufB = a2 [300][16], act = tanh output [A][16]
// dact (may be null): 1 - tanh^2 = 4 e / (1 + e)^2 with e = exp(-2 |h|), from h itself: 1 - o * o loses what tanh rounds away
__device__ void actor_fwd(const Layout& L, const float* __restrict__ th, const float* xin, float* bufA, float* bufB, float* act,
                          float* dact, ActorKeep kp, int row0, int nrows) {
  dense_fwd<THREADS>(th + L.off[A_W1], th + L.off[A_B1], L.S, H1, xin, nullptr, 0, nullptr, [&](int j, int r, float h) {
    float n;
    const float xh = bn_apply(th, L, A_MM1, A_MV1, A_BE1, A_GA1, j, h, &n);
    const float a = fmaxf(n, 0.f);
    bufA[j * TILE + r] = a;
    if (kp.a1 && r < nrows) {
      kp.xh1[(size_t)(row0 + r) * H1 + j] = xh;
      kp.a1[(size_t)(row0 + r) * H1 + j] = a;
    }
  });
  dense_fwd<THREADS>(th + L.off[A_W2], th + L.off[A_B2], H1, H2, bufA, nullptr, 0, nullptr, [&](int j, int r, float h) {
    float n;
    const float xh = bn_apply(th, L, A_MM2, A_MV2, A_BE2, A_GA2, j, h, &n);
    const float a = fmaxf(n, 0.f);
    bufB[j * TILE + r] = a;
    if (kp.a2 && r < nrows) {
      kp.xh2[(size_t)(row0 + r) * H2 + j] = xh;
      kp.a2[(size_t)(row0 + r) * H2 + j] = a;
    }
  });
  const int A = L.A;
  dense_fwd<THREADS>(th + L.off[A_WO], th + L.off[A_BO], H2, A, bufB, nullptr, 0, nullptr, [&](int j, int r, float h) {
    const float o = tanhf(h);
    act[j * TILE + r] = o;
    if (dact) {
      const float e = expf(-2.0f * fabsf(h));
      dact[j * TILE + r] = 4.0f * e / ((1.0f + e) * (1.0f + e));
    }
    if (kp.out && r < nrows) kp.out[(size_t)(row0 + r) * A + j] = o;
  });
}

// xin [S][16], act [A][16] -> bufA = c1 [400][16], bufB = c2 [300][16]: the critic below its head
__device__ __forceinline__ void critic_trunk(const Layout& L, const float* __restrict__ th, const float* xin, const float* act,
                                             float* bufA, float* bufB, CriticKeep kp, int row0, int nrows) {
  dense_fwd<THREADS>(th + L.off[C_W1], th + L.off[C_B1], L.S, H1, xin, nullptr, 0, nullptr, [&](int j, int r, float h) {
    float n;
    const float xh = bn_apply(th, L, C_MM1, C_MV1, C_BE1, C_GA1, j, h, &n);
    const float c = fmaxf(n, 0.f);
    bufA[j * TILE + r] = c;
    if (kp.c1 && r < nrows) {
      kp.xh1[(size_t)(row0 + r) * H1 + j] = xh;
      kp.c1[(size_t)(row0 + r) * H1 + j] = c;
    }
  });
  dense_fwd<THREADS>(th + L.off[C_W2], th + L.off[C_BN], H1, H2, bufA, th + L.off[C_WN], L.A, act, [&](int j, int r, float h) {
    const float c = fmaxf(h, 0.f);
    bufB[j * TILE + r] = c;
    if (kp.c2 && r < nrows) kp.c2[(size_t)(row0 + r) * H2 + j] = c;
  });
}

// ... and with the scalar head: -> qv[16] (LDS)
__device__ void critic_fwd(const Layout& L, const float* __restrict__ th, const float* xin, const float* act, float* bufA,
                           float* bufB, float* qv, CriticKeep kp, int row0, int nrows) {
  critic_trunk(L, th, xin, act, bufA, bufB, kp, row0, nrows);
  // q: one thread per row, in j order
  if (threadIdx.x < TILE) {
    const int r = threadIdx.x;
    const float* __restrict__ wo = th + L.off[C_WO];
    float s = th[L.off[C_BO]];
    for (int j = 0; j < H2; ++j) s = fmaf(bufB[j * TILE + r], wo[j], s);
    qv[r] = s;
  }
  __syncthreads();
}

// Loads `width` floats at column offset `col` of the tile's rows into dst [width][16] (zeros beyond nrows).
// a + noise; wrap: the reference's check_bounds(turnaround), which folds what leaves [-1, 1] back in from the other end
__device__ __forceinline__ float wrap_action(float v, int wrap) {
  if (wrap) {
    if (v < -1.f) v = 1.f - fmodf(-1.f - v, 2.f);
    else if (v > 1.f) v = fmodf(v - 1.f, 2.f) - 1.f;
  }
  return v;
}

__device__ __forceinline__ void load_rows(const Rows& src, int col, int width, float* dst, int row0, int nrows, float* keep) {
  for (int e = threadIdx.x; e < width * TILE; e += THREADS) {
    const int r = e / width, c = e % width;
    float v = 0.f;
    if (r < nrows) {
      const int64_t slot = src.idx ? src.idx[row0 + r] : row0 + r;
      v = src.base[slot * src.rowf + col + c];
      if (keep) keep[(size_t)(row0 + r) * width + c] = v;
    }
    dst[c * TILE + r] = v;
  }
}

// disc (null: the scalar gamma for every row): the discount by ring slot of a handle with n-step returns, whose rows are ring
// slots; used (null without n-step): the B discounts this step's target took.
__device__ __forceinline__ float row_discount(const float* __restrict__ disc, float* __restrict__ used, int64_t slot, int row,
                                              float gamma) {
  const float g = disc ? disc[slot] : gamma;
  if (used) used[row] = g;
  return g;
}

// The statistics of a handle with PopArt as the target kernel reads them; stat null: a handle without, whose
// critic's output is the return itself.
struct PopStats {
  const float* stat;         // {mu, nu}, f32, behind the 26 variables of the value arena
  double smin, smax;
};

// sigma = clamp(sqrt(max(nu - mu^2, 0)), smin, smax) in f64 from the stored f32 values (mu^2 is exact in f64)
__device__ __forceinline__ double popart_sigma(float mu, float nu, double smin, double smax) {
  const double m = (double)mu;
  return fmin(fmax(sqrt(fmax((double)nu - m * m, 0.0)), smin), smax);
}

// What the target step writes and, with two critics, what its smoothing draws from.
template <int NC>
struct Target { float *y, *qt; };
template <>
struct Target<2> {
  float *y, *qt, *qt1, *qt2, *t_eps, *t_a;
  float sigma, clip;
  uint64_t seed, number;
};

// Steps 1-2: actor_target and the NC target critics on s2, y = r or r + g q' with q' the smallest of their values.
// NC = 2: the target action of row k = row0 + r, action i is a~ = clip(actor_target(s2) + eps, -1, 1),
// eps = (f32) clip(sigma n, -c, c), n Box-Muller in f64 on uniforms 2j and 2j + 1 of stream `number`, j = k A + i.  Both target
// critics read a~ from `act`, one after the other in the same buffers.
// ps (NC = 1, stat not null: a handle with PopArt): the target critic's output n' is a normalised value and
// q' = fmaf((f32) sigma, n', mu) with the statistics as they stand; "qt" and y are in return units.
template <int NC>
__global__ __launch_bounds__(THREADS) void ddpg_target_kernel(PerCritic<Layout, NC> L, const float* __restrict__ thT, Rows src, int B,
                                                              float gamma, int future, Target<NC> t,
                                                              const float* __restrict__ disc, float* __restrict__ used,
                                                              PopStats ps) {
  __shared__ __attribute__((aligned(16))) float xin[MAX_S * TILE];
  __shared__ __attribute__((aligned(16))) float bufA[H1 * TILE];
  __shared__ __attribute__((aligned(16))) float bufB[H2 * TILE];
  __shared__ __attribute__((aligned(16))) float act[MAX_A * TILE];
  __shared__ float qv[NC][TILE];
  const int S = L.v[0].S, A = L.v[0].A;
  const int row0 = blockIdx.x * TILE, nrows = min(TILE, B - row0);
  if (future) {
    load_rows(src, S + A + 2, S, xin, row0, nrows, nullptr);
    __syncthreads();
    actor_fwd(L.v[0], thT, xin, bufA, bufB, act, nullptr, ActorKeep{nullptr, nullptr, nullptr, nullptr, nullptr}, row0, nrows);
    if constexpr (NC == 2) {
      for (int e = threadIdx.x; e < A * TILE; e += THREADS) {
        const int i = e / TILE, r = e % TILE;
        const uint64_t j = (uint64_t)(row0 + r) * (uint64_t)A + (uint64_t)i;
        const double u1 = 1.0 - ga3c_uniform::actor_uniform(t.seed, t.number, 2 * j);
        const double u2 = ga3c_uniform::actor_uniform(t.seed, t.number, 2 * j + 1);
        const double n = sqrt(-2.0 * log(u1)) * cos(6.283185307179586 * u2);
        const float eps = (float)fmin(fmax((double)t.sigma * n, -(double)t.clip), (double)t.clip);
        const float a = fminf(fmaxf(act[e] + eps, -1.f), 1.f);
        act[e] = a;
        if (r < nrows) {
          t.t_eps[(size_t)(row0 + r) * A + i] = eps;
          t.t_a[(size_t)(row0 + r) * A + i] = a;
        }
      }
      __syncthreads();
    }
#pragma unroll
    for (int c = 0; c < NC; ++c) critic_fwd(L.v[c], thT, xin, act, bufA, bufB, qv[c], CriticKeep{nullptr, nullptr, nullptr}, row0, nrows);
  }
  if (threadIdx.x < nrows) {
    const int r = threadIdx.x;
    const int64_t slot = src.idx ? src.idx[row0 + r] : row0 + r;
    const float rew = src.base[slot * src.rowf + S + A], done = src.base[slot * src.rowf + S + A + 1];
    const float g = row_discount(disc, used, slot, row0 + r, gamma);
    float q[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) q[c] = future ? qv[c][r] : 0.f;
    float qt = q[0];
    if constexpr (NC == 2) qt = fminf(q[0], q[1]);
    if constexpr (NC == 1) {
      if (ps.stat) {
        const float mu = ps.stat[0];
        qt = fmaf((float)popart_sigma(mu, ps.stat[1], ps.smin, ps.smax), qt, mu);
      }
    }
    float y = rew;
    if (future && done == 0.f) y = fmaf(g, qt, rew);
    t.y[row0 + r] = y;
    t.qt[row0 + r] = qt;
    if constexpr (NC == 2) {
      t.qt1[row0 + r] = q[0];
      t.qt2[row0 + r] = q[1];
    }
  }
}

// bufB = the delta at t [300][16], bufA = c1: the delta at critic_norm1's output (in place over c1: thread k reads and writes
// row k alone) and at critic_fc1's, to HBM
__device__ __forceinline__ void critic_bwd1(const Layout& L, const float* __restrict__ th, float* bufA, const float* bufB,
                                            const CriticRows& w, int row0, int nrows) {
  dense_bwd(th + L.off[C_W2], H1, H2, bufB, [&](int k, int r, float s) {
    const float d = bufA[k * TILE + r] > 0.f ? s : 0.f;
    bufA[k * TILE + r] = d;
    if (r < nrows) {
      w.dn1[(size_t)(row0 + r) * H1 + k] = d;
      w.dh1[(size_t)(row0 + r) * H1 + k] = d * bn_scale(th, L, C_MV1, C_GA1, k);
    }
  });
}

// per_w (null without priorities): the rows' importance weights, dq_i = (2/B) w_i (q_i - y_i); keep_x, keep_a (null: not kept):
// where the step's inputs go
__device__ __forceinline__ void critic_step(const Layout& L, const float* __restrict__ th, const Rows& src, int B, int paired,
                                            const float* __restrict__ per_w, const float* __restrict__ y, float* keep_x,
                                            float* keep_a, const CriticRows& w) {
  __shared__ __attribute__((aligned(16))) float xin[MAX_S * TILE];
  __shared__ __attribute__((aligned(16))) float bufA[H1 * TILE];
  __shared__ __attribute__((aligned(16))) float bufB[H2 * TILE];
  __shared__ __attribute__((aligned(16))) float act[MAX_A * TILE];
  __shared__ float qv[TILE];
  __shared__ float dqv[TILE];
  __shared__ float red[RED];
  const int S = L.S, A = L.A;
  const int row0 = blockIdx.x * TILE, nrows = min(TILE, B - row0);
  // mean(y), the same fixed order in every block: strided partials, then block_sum's tree
  float ysum = 0.f;
  for (int i = threadIdx.x; i < B; i += THREADS) ysum += y[i];
  const float ymean = block_sum<THREADS>(ysum, red) / (float)B;
  load_rows(src, 0, S, xin, row0, nrows, keep_x);
  load_rows(src, S, A, act, row0, nrows, keep_a);
  __syncthreads();
  critic_fwd(L, th, xin, act, bufA, bufB, qv, CriticKeep{w.xh1, w.c1, w.c2}, row0, nrows);
  if (threadIdx.x < TILE) {
    const int r = threadIdx.x;
    float dq = 0.f;
    if (r < nrows) {
      const float ref = paired ? y[row0 + r] : ymean;
      dq = (2.0f / (float)B) * (qv[r] - ref);
      if (per_w) dq *= per_w[row0 + r];
      w.q[row0 + r] = qv[r];
      w.dq[row0 + r] = dq;
    }
    dqv[r] = dq;
  }
  __syncthreads();
  // delta at t = h W_fc2 + a W_n2 + b_n2, in place over c2
  const float* __restrict__ wo = th + L.off[C_WO];
  for (int e = threadIdx.x; e < H2 * TILE; e += THREADS) {
    const int j = e / TILE, r = e % TILE;
    const float d = bufB[e] > 0.f ? dqv[r] * wo[j] : 0.f;
    bufB[e] = d;
    if (r < nrows) w.dt[(size_t)(row0 + r) * H2 + j] = d;
  }
  __syncthreads();
  critic_bwd1(L, th, bufA, bufB, w, row0, nrows);
}

// Critic blockIdx.y's step (NC = 1: the one critic's) on the same rows and the same y.  Critic 1 keeps the inputs.
template <int NC>
__global__ __launch_bounds__(THREADS) void ddpg_critic_kernel(PerCritic<Layout, NC> L, const float* __restrict__ th, Rows src, int B,
                                                              int paired, const float* __restrict__ per_w, Work w) {
  const int c = NC == 1 ? 0 : blockIdx.y;
  critic_step(L.v[c], th, src, B, paired, per_w, w.y, c ? nullptr : w.c_x, c ? nullptr : w.c_a, w.c[c]);
}

// ------------------------------------------------------------------ PopArt
struct PopArt {
  float *stat, *stat_t;      // {mu, nu} in the value arena and in the target arena
  float *wo, *bo;            // critic_output/W [300] and /b of the value arena
  float *wo_t, *bo_t;        // ... of the target arena
  const float* y;            // [B] the step's targets, return units
  float* yn;                 // [B] <- (y - mu') / sigma'
  float* out;                // {(f32) mu', (f32) sigma'} for the step's returned stats
  double beta, smin, smax;
};

// One workgroup, between ddpg_target_kernel and ddpg_critic_kernel.  Thread t sums y_i and y_i^2 in f64 over i = t, t + 448, ...
// in that order and the partials fold by block_sum's tree (512 leaves).  Thread 0 then moves the statistics,
// mu' = (1 - beta) mu + beta mean(y) and nu' likewise on mean(y^2) in f64, each rounded to f32 and stored in both arenas, takes
// sigma' from the STORED values, and forms ratio = (f32)(sigma / sigma'), shift = (f32)((mu - mu') / sigma'), muf' = mu' and
// isig' = (f32)(1 / sigma').  All threads: W <- W ratio and b <- fmaf(b, ratio, shift) for critic_output of both arenas, so that
// sigma' n + mu' is what sigma n + mu was, and yn_i = (y_i - muf') isig'.  With beta = 0 on fresh statistics every factor is
// exactly 1 or 0.  No slot and no gradient is touched.
__global__ __launch_bounds__(THREADS) void ddpg_popart_kernel(PopArt p, int B) {
#pragma clang fp contract(off)
  __shared__ double red[2][RED];
  __shared__ float k[4];
  const int t = threadIdx.x;
  double s1 = 0.0, s2 = 0.0;
  for (int i = t; i < B; i += THREADS) {
    const double v = (double)p.y[i];
    s1 += v;
    s2 += v * v;
  }
  red[0][t] = s1;
  red[1][t] = s2;
  if (t + THREADS < RED) red[0][t + THREADS] = red[1][t + THREADS] = 0.0;
  __syncthreads();
  for (int h = RED / 2; h > 0; h >>= 1) {
    if (t < h) {
      red[0][t] += red[0][t + h];
      red[1][t] += red[1][t + h];
    }
    __syncthreads();
  }
  if (t == 0) {
    const float mu = p.stat[0], nu = p.stat[1];
    const double sigma = popart_sigma(mu, nu, p.smin, p.smax);
    const float mu1 = (float)((1.0 - p.beta) * (double)mu + p.beta * (red[0][0] / (double)B));
    const float nu1 = (float)((1.0 - p.beta) * (double)nu + p.beta * (red[1][0] / (double)B));
    const double sigma1 = popart_sigma(mu1, nu1, p.smin, p.smax);
    p.stat[0] = p.stat_t[0] = mu1;
    p.stat[1] = p.stat_t[1] = nu1;
    k[0] = (float)(sigma / sigma1);
    k[1] = (float)(((double)mu - (double)mu1) / sigma1);
    k[2] = mu1;
    k[3] = (float)(1.0 / sigma1);
    p.out[0] = mu1;
    p.out[1] = (float)sigma1;
  }
  __syncthreads();
  const float ratio = k[0], shift = k[1], muf = k[2], isig = k[3];
  for (int j = t; j < H2; j += THREADS) {
    p.wo[j] = p.wo[j] * ratio;
    p.wo_t[j] = p.wo_t[j] * ratio;
  }
  if (t == 0) {
    p.bo[0] = fmaf(p.bo[0], ratio, shift);
    p.bo_t[0] = fmaf(p.bo_t[0], ratio, shift);
  }
  for (int i = t; i < B; i += THREADS) p.yn[i] = (p.y[i] - muf) * isig;
}

// ------------------------------------------------------------------ distributional critic
constexpr int ATOMS_MAX = GA3C_DDPG_ATOMS_MAX;
static_assert(ATOMS_MAX <= MAX_S, "ddpg_dist_critic_kernel keeps the tile's m in the LDS buffer of the states");

// The support, all of it f32: z_k = fmaf((float)k, delta, vmin), delta = (vmax - vmin) / (float)(n - 1) divided once on the host.
struct Support {
  int n;
  float vmin, vmax, delta;
};
__device__ __forceinline__ float atom(const Support& z, int k) { return fmaf((float)k, z.delta, z.vmin); }

// What a distributional step writes beside Work's rows: [B,n] each, ce [B].
struct DistRows { float *pt, *m, *p, *dz, *ce; };

// lg [n][16] <- c2 W_o + b_o on bufB = c2.  dense_fwd's statement (thread k owns atom k and adds in j order from the bias on) with
// the weights of 15 steps requested at once: the pass is one wave waiting on 300 strided loads, not on its arithmetic.
__device__ __forceinline__ void dist_logits(const Layout& L, const float* __restrict__ th, const float* bufB, int n, float* lg) {
  const float* __restrict__ wo = th + L.off[C_WO];
  for (int k = threadIdx.x; k < n; k += THREADS) {
    float acc[TILE];
    const float b = th[L.off[C_BO] + k];
#pragma unroll
    for (int r = 0; r < TILE; ++r) acc[r] = b;
#pragma unroll 15
    for (int j = 0; j < H2; ++j) tile_fma(acc, bufB + j * TILE, wo[(size_t)j * n + k]);
#pragma unroll
    for (int r = 0; r < TILE; ++r) lg[k * TILE + r] = acc[r];
  }
  __syncthreads();
}

// Row r's softmax by the one thread that calls it: the row maximum, the sum of exp(l - max) in k order, p_k = exp(l_k - max) / sum;
// lg[k][r] <- each(k, p_k, log p_k) with log p_k = (l_k - max) - log(sum), which stays finite where p_k rounds to zero.
// -> sum_k z_k p_k in k order.
template <class F>
__device__ __forceinline__ float dist_softmax(float* lg, int r, const Support& z, F each) {
  float mx = lg[r];
  for (int k = 1; k < z.n; ++k) mx = fmaxf(mx, lg[k * TILE + r]);
  float s = 0.f;
  for (int k = 0; k < z.n; ++k) s += expf(lg[k * TILE + r] - mx);
  const float ls = logf(s);
  float q = 0.f;
  for (int k = 0; k < z.n; ++k) {
    const float t = lg[k * TILE + r] - mx;
    const float p = expf(t) / s;
    q = fmaf(atom(z, k), p, q);
    lg[k * TILE + r] = each(k, p, t - ls);
  }
  return q;
}

// bufB [300][16] <- relu'(t_j) sum_k lg[k][r] W_o[j][k]: dense_bwd's statement (thread j owns row j of W_o and adds in k order),
// 16 of the row's weights requested at once; dt (may be null): the same to HBM
__device__ __forceinline__ void dist_head_bwd(const Layout& L, const float* __restrict__ th, const float* lg, int n, float* bufB,
                                              float* dt, int row0, int nrows) {
  for (int j = threadIdx.x; j < H2; j += THREADS) {
    float acc[TILE];
#pragma unroll
    for (int r = 0; r < TILE; ++r) acc[r] = 0.f;
    const float* __restrict__ wr = th + L.off[C_WO] + (size_t)j * n;
#pragma unroll 16
    for (int k = 0; k < n; ++k) tile_fma(acc, lg + k * TILE, wr[k]);
#pragma unroll
    for (int r = 0; r < TILE; ++r) {
      const float d = bufB[j * TILE + r] > 0.f ? acc[r] : 0.f;
      bufB[j * TILE + r] = d;
      if (dt && r < nrows) dt[(size_t)(row0 + r) * H2 + j] = d;
    }
  }
  __syncthreads();
}

// Steps 1-2 of a distributional step.  p' = softmax of the target critic's head at (s2, actor_target(s2)); per row g = 0 on a
// done row or without `future`, else the row's discount (row_discount); Tz_j = clip(fmaf(g, z_j, r), vmin, vmax),
// b_j = (Tz_j - vmin) / delta; m_k = sum_j p'_j max(0, 1 - |b_j - k|), j ascending, by the thread of (row, k); y = sum_k z_k m_k,
// q' = sum_k z_k p'_k.  Without `future` no net is evaluated: p' and q' are zero and m_k = max(0, 1 - |b - k|), b from r alone.
// b and m lie over bufA, which the trunk is done with.
__global__ __launch_bounds__(THREADS) void ddpg_dist_target_kernel(Layout L, const float* __restrict__ thT, Rows src, int B,
                                                                   float gamma, int future, Support z, float* __restrict__ y,
                                                                   float* __restrict__ qt, DistRows d,
                                                                   const float* __restrict__ disc, float* __restrict__ used) {
  __shared__ __attribute__((aligned(16))) float xin[MAX_S * TILE];
  __shared__ __attribute__((aligned(16))) float bufA[H1 * TILE];
  __shared__ __attribute__((aligned(16))) float bufB[H2 * TILE];
  __shared__ __attribute__((aligned(16))) float act[MAX_A * TILE];
  __shared__ __attribute__((aligned(16))) float lg[ATOMS_MAX * TILE];
  __shared__ float qv[TILE];
  const int S = L.S, A = L.A, n = z.n;
  const int row0 = blockIdx.x * TILE, nrows = min(TILE, B - row0);
  if (future) {
    load_rows(src, S + A + 2, S, xin, row0, nrows, nullptr);
    __syncthreads();
    actor_fwd(L, thT, xin, bufA, bufB, act, nullptr, ActorKeep{nullptr, nullptr, nullptr, nullptr, nullptr}, row0, nrows);
    critic_trunk(L, thT, xin, act, bufA, bufB, CriticKeep{nullptr, nullptr, nullptr}, row0, nrows);
    dist_logits(L, thT, bufB, n, lg);
    if (threadIdx.x < TILE) qv[threadIdx.x] = dist_softmax(lg, threadIdx.x, z, [](int, float p, float) { return p; });
  } else {
    for (int e = threadIdx.x; e < n * TILE; e += THREADS) lg[e] = 0.f;
    if (threadIdx.x < TILE) qv[threadIdx.x] = 0.f;
  }
  __syncthreads();
  float* bb = bufA;
  float* mm = bufA + ATOMS_MAX * TILE;
  for (int e = threadIdx.x; e < n * TILE; e += THREADS) {
    const int j = e / TILE, r = e % TILE;
    float b = 0.f;
    if (r < nrows) {
      const int64_t slot = src.idx ? src.idx[row0 + r] : row0 + r;
      const float rew = src.base[slot * src.rowf + S + A], done = src.base[slot * src.rowf + S + A + 1];
      const float disc_r = row_discount(disc, j == 0 ? used : nullptr, slot, row0 + r, gamma);
      const float g = future && done == 0.f ? disc_r : 0.f;
      const float tz = fminf(fmaxf(fmaf(g, atom(z, j), rew), z.vmin), z.vmax);
      b = (tz - z.vmin) / z.delta;
      d.pt[(size_t)(row0 + r) * n + j] = lg[e];
    }
    bb[e] = b;
  }
  __syncthreads();
  for (int e = threadIdx.x; e < n * TILE; e += THREADS) {
    const int k = e / TILE, r = e % TILE;
    float m = 0.f;
    if (future) {
      for (int j = 0; j < n; ++j) m = fmaf(lg[j * TILE + r], fmaxf(0.f, 1.0f - fabsf(bb[j * TILE + r] - (float)k)), m);
    } else {
      m = fmaxf(0.f, 1.0f - fabsf(bb[r] - (float)k));
    }
    mm[e] = m;
    if (r < nrows) d.m[(size_t)(row0 + r) * n + k] = m;
  }
  __syncthreads();
  if (threadIdx.x < nrows) {
    const int r = threadIdx.x;
    float s = 0.f;
    for (int k = 0; k < n; ++k) s = fmaf(atom(z, k), mm[k * TILE + r], s);
    y[row0 + r] = s;
    qt[row0 + r] = qv[r];
  }
}

// Step 3's forward and backward of a distributional step: p = softmax(logits), q = sum_k z_k p_k, the row's cross-entropy
// ce = -sum_k m_k log p_k, dz_k = (w / B)(p_k - m_k) (w: per_w's weight, 1 without), the delta at t from dz through W_o, and below
// that the scalar critic's backward.  "dq" is not written.
__global__ __launch_bounds__(THREADS) void ddpg_dist_critic_kernel(Layout L, const float* __restrict__ th, Rows src, int B,
                                                                   const float* __restrict__ per_w, Support z, Work w, DistRows d) {
  __shared__ __attribute__((aligned(16))) float xin[MAX_S * TILE];
  __shared__ __attribute__((aligned(16))) float bufA[H1 * TILE];
  __shared__ __attribute__((aligned(16))) float bufB[H2 * TILE];
  __shared__ __attribute__((aligned(16))) float act[MAX_A * TILE];
  __shared__ __attribute__((aligned(16))) float lg[ATOMS_MAX * TILE];
  const int S = L.S, A = L.A, n = z.n;
  const int row0 = blockIdx.x * TILE, nrows = min(TILE, B - row0);
  const CriticRows& cr = w.c[0];
  load_rows(src, 0, S, xin, row0, nrows, w.c_x);
  load_rows(src, S, A, act, row0, nrows, w.c_a);
  __syncthreads();
  critic_trunk(L, th, xin, act, bufA, bufB, CriticKeep{cr.xh1, cr.c1, cr.c2}, row0, nrows);
  float* mm = xin;                     // the trunk is done with the states: the tile's m [n][16], read once and coalesced
  for (int e = threadIdx.x; e < n * TILE; e += THREADS) {
    const int r = e / n, k = e % n;
    mm[k * TILE + r] = r < nrows ? d.m[(size_t)(row0 + r) * n + k] : 0.f;
  }
  dist_logits(L, th, bufB, n, lg);     // ends in a barrier
  if (threadIdx.x < TILE) {
    const int r = threadIdx.x;
    const bool live = r < nrows;
    const size_t at = (size_t)(row0 + r) * n;
    float c = 0.f;
    if (live) {
      c = 1.0f / (float)B;
      if (per_w) c *= per_w[row0 + r];
    }
    float ce = 0.f;
    const float q = dist_softmax(lg, r, z, [&](int k, float p, float logp) {
      const float m = mm[k * TILE + r];
      const float dz = c * (p - m);
      ce = fmaf(-m, logp, ce);
      if (live) {
        d.p[at + k] = p;
        d.dz[at + k] = dz;
      }
      return dz;
    });
    if (live) {
      cr.q[row0 + r] = q;
      d.ce[row0 + r] = ce;
    }
  }
  __syncthreads();
  dist_head_bwd(L, th, lg, n, bufB, cr.dt, row0, nrows);
  critic_bwd1(L, th, bufA, bufB, cr, row0, nrows);
}

// Steps 4-5's rows.  DIST: the critic's head is the atom head and dQ/dlogit_k = p_k (z_k - Q) stands where the scalar head has
// its weight: bufB[j] = relu'(t_j) sum_k p_k (z_k - Q) W_o[j][k].  lg: [n][16] in LDS, DIST only.  (static: its LDS arrays stay
// internal to each kernel, so the scalar kernel drops the head's q, which it does not read, as it did.)
template <bool DIST>
static __device__ __forceinline__ void actor_rows(const Layout& L, const float* __restrict__ th, const Rows& src, int B, const Noise& nz,
                                           const Work& w, const Support& z, float* lg) {
  __shared__ __attribute__((aligned(16))) float xin[MAX_S * TILE];
  __shared__ __attribute__((aligned(16))) float bufA[H1 * TILE];
  __shared__ __attribute__((aligned(16))) float bufB[H2 * TILE];
  __shared__ __attribute__((aligned(16))) float act[MAX_A * TILE];      // tanh output
  __shared__ __attribute__((aligned(16))) float noisy[MAX_A * TILE];    // + noise; later the delta at the output's pre-activation
  __shared__ __attribute__((aligned(16))) float dact[MAX_A * TILE];     // 1 - tanh^2
  __shared__ float qv[TILE];
  const int S = L.S, A = L.A;
  const int row0 = blockIdx.x * TILE, nrows = min(TILE, B - row0);
  load_rows(src, 0, S, xin, row0, nrows, nullptr);
  __syncthreads();
  actor_fwd(L, th, xin, bufA, bufB, act, dact, ActorKeep{w.a_xh1, w.a_a1, w.a_xh2, w.a_a2, w.a_out}, row0, nrows);
  for (int e = threadIdx.x; e < A * TILE; e += THREADS) {
    const int i = e / TILE, r = e % TILE;
    const float v = wrap_action(act[e] + nz.v[i], nz.wrap);
    noisy[e] = v;
    if (r < nrows) w.a_noisy[(size_t)(row0 + r) * A + i] = v;
  }
  __syncthreads();
  // the updated critic at (s, a_out); only the relu mask of t is needed for dq/da
  if constexpr (DIST) {
    critic_trunk(L, th, xin, noisy, bufA, bufB, CriticKeep{nullptr, nullptr, nullptr}, row0, nrows);
    dist_logits(L, th, bufB, z.n, lg);
    if (threadIdx.x < TILE) {
      const int r = threadIdx.x;
      const float q = dist_softmax(lg, r, z, [](int, float p, float) { return p; });
      for (int k = 0; k < z.n; ++k) lg[k * TILE + r] *= atom(z, k) - q;
    }
    __syncthreads();
    dist_head_bwd(L, th, lg, z.n, bufB, nullptr, row0, nrows);
  } else {
    critic_fwd(L, th, xin, noisy, bufA, bufB, qv, CriticKeep{nullptr, nullptr, nullptr}, row0, nrows);
    const float* __restrict__ wo = th + L.off[C_WO];
    for (int e = threadIdx.x; e < H2 * TILE; e += THREADS) bufB[e] = bufB[e] > 0.f ? wo[e / TILE] : 0.f;
    __syncthreads();
  }
  // g = dq/da (per row, no 1/B); the delta at actor_output's pre-activation is -g (1 - out^2)
  dense_bwd(th + L.off[C_WN], A, H2, bufB, [&](int i, int r, float g) {
    const float d = -g * dact[i * TILE + r];
    noisy[i * TILE + r] = r < nrows ? d : 0.f;
    if (r < nrows) {
      w.g[(size_t)(row0 + r) * A + i] = g;
      w.dout[(size_t)(row0 + r) * A + i] = d;
    }
  });
  // back through actor_norm2 / actor_fc2: the relu masks come from the rows this block stored above
  dense_bwd(th + L.off[A_WO], H2, A, noisy, [&](int k, int r, float s) {
    float d = 0.f;
    if (r < nrows) {
      d = w.a_a2[(size_t)(row0 + r) * H2 + k] > 0.f ? s : 0.f;
      w.a_dn2[(size_t)(row0 + r) * H2 + k] = d;
    }
    const float dh = d * bn_scale(th, L, A_MV2, A_GA2, k);
    bufB[k * TILE + r] = dh;
    if (r < nrows) w.a_dh2[(size_t)(row0 + r) * H2 + k] = dh;
  });
  dense_bwd(th + L.off[A_W2], H1, H2, bufB, [&](int k, int r, float s) {
    if (r < nrows) {
      const float d = w.a_a1[(size_t)(row0 + r) * H1 + k] > 0.f ? s : 0.f;
      w.a_dn1[(size_t)(row0 + r) * H1 + k] = d;
      w.a_dh1[(size_t)(row0 + r) * H1 + k] = d * bn_scale(th, L, A_MV1, A_GA1, k);
    }
  });
}

__global__ __launch_bounds__(THREADS) void ddpg_actor_kernel(Layout L, const float* __restrict__ th, Rows src, int B, Noise nz,
                                                             Work w) {
  actor_rows<false>(L, th, src, B, nz, w, Support{1, 0.f, 0.f, 0.f}, nullptr);
}

__global__ __launch_bounds__(THREADS) void ddpg_dist_actor_kernel(Layout L, const float* __restrict__ th, Rows src, int B, Noise nz,
                                                                  Work w, Support z) {
  __shared__ __attribute__((aligned(16))) float lg[ATOMS_MAX * TILE];
  actor_rows<true>(L, th, src, B, nz, w, z, lg);
}

// A prediction's rows up to the epilogue: the online actor on the tile's inputs -> its tanh output [A][16] in LDS, complete for
// every thread.  (static: its LDS arrays stay internal to each kernel.)
static __device__ __forceinline__ const float* predict_rows(const Layout& L, const float* __restrict__ th, const Input& in,
                                                            int row0, int nrows) {
  __shared__ __attribute__((aligned(16))) float xin[MAX_S * TILE];
  __shared__ __attribute__((aligned(16))) float bufA[H1 * TILE];
  __shared__ __attribute__((aligned(16))) float bufB[H2 * TILE];
  __shared__ __attribute__((aligned(16))) float act[MAX_A * TILE];
  load_input_tile<THREADS, false>(in, L.S, row0, nrows, xin, nullptr);
  __syncthreads();
  actor_fwd(L, th, xin, bufA, bufB, act, nullptr, ActorKeep{nullptr, nullptr, nullptr, nullptr, nullptr}, row0, nrows);
  return act;
}

__global__ __launch_bounds__(THREADS) void ddpg_predict_kernel(Layout L, const float* __restrict__ th, Input in, int B, Noise nz,
                                                               float* __restrict__ a_out) {
  const int A = L.A;
  const int row0 = blockIdx.x * TILE, nrows = min(TILE, B - row0);
  const float* act = predict_rows(L, th, in, row0, nrows);
  for (int e = threadIdx.x; e < A * TILE; e += THREADS) {
    const int i = e / TILE, r = e % TILE;
    const float v = wrap_action(act[e] + nz.v[i], nz.wrap);
    if (r < nrows) a_out[(size_t)(row0 + r) * A + i] = v;
  }
}

// Per-environment exploration noise of a handle's device actors (ga3c_ddpg_envnoise_create): row i is
// environment i, x and n are [N][A].  Everything but the two buffers and `done` is a launch argument the host knows.
struct EnvNoise {
  float* x;                  // the environments' OU states
  float* n;                  // their last normal draws
  const int* done;           // the last step's done, read when `reset` is set
  uint64_t seed, count;      // the draw of action j at prediction `count` is number k = count A + j of stream i
  double sigma, theta, dt, sqrt_dt;      // the handle's config as ga3c_ddpg_noise_step reads it: f32 values, sqrt in f64
  int reset;                 // x restarts at 0 after an episode's end
};

// ddpg_predict_kernel with 8r's epilogue in the shared process's place: the thread that owns (action j, environment i) steps
// x_i[j] by ga3c_ddpg_noise_step's expression on 8n's Box-Muller draw and adds it, unwrapped.  Rows >= B touch nothing.
__global__ __launch_bounds__(THREADS) void ddpg_predict_envnoise_kernel(Layout L, const float* __restrict__ th, Input in, int B,
                                                                        EnvNoise z, float* __restrict__ a_out) {
#pragma clang fp contract(off)
  const int A = L.A;
  const int row0 = blockIdx.x * TILE, nrows = min(TILE, B - row0);
  const float* act = predict_rows(L, th, in, row0, nrows);
  for (int e = threadIdx.x; e < A * TILE; e += THREADS) {
    const int j = e / TILE, r = e % TILE;
    if (r >= nrows) continue;
    const uint64_t i = (uint64_t)(row0 + r);
    const size_t at = (size_t)i * A + j;
    const uint64_t k = z.count * (uint64_t)A + (uint64_t)j;
    const double u1 = 1.0 - ga3c_uniform::actor_uniform(z.seed, i, 2 * k);
    const double u2 = ga3c_uniform::actor_uniform(z.seed, i, 2 * k + 1);
    const float nn = (float)(sqrt(-2.0 * log(u1)) * cos(6.283185307179586 * u2));
    const double xp = z.reset && z.done[i] ? 0.0 : (double)z.x[at];
    const float xn = (float)(xp + z.theta * (0.0 - xp) * z.dt + z.sigma * z.sqrt_dt * (double)nn);
    z.x[at] = xn;
    z.n[at] = nn;
    a_out[at] = act[e] + xn;
  }
}

// The gradient of variable v's element: sum over rows of in[r][k] d[r][j] (in null: of d[r][j]; mul: times mul[r][j]).
struct GradSrc {
  const float* in[NTRAIN];
  const float* d[NTRAIN];
  const float* mul[NTRAIN];
  int ld_in[NTRAIN], ld_d[NTRAIN];
};

__device__ __forceinline__ void opt_step(const Opt& o, int64_t i, float g) {
  if (o.adam) {
    float m = o.sa[i], v = o.sb[i];
    m += (g - m) * ADAM_OMB1;
    v += (g * g - v) * ADAM_OMB2;
    o.sa[i] = m;
    o.sb[i] = v;
    o.theta[i] -= o.lr * m / (sqrtf(v) + ADAM_EPS);
  } else {
    float m = o.sa[i];
    m += (g * g - m) * o.omr;
    o.sa[i] = m;
    const float step = o.sb[i] * o.mu + (g * o.lr) / sqrtf(o.eps + m);
    o.sb[i] = step;
    o.theta[i] -= step;
  }
}

__device__ __forceinline__ void soft_step(const Opt& o, int64_t i) {
  o.target[i] = o.tau * o.theta[i] + (1.0f - o.tau) * o.target[i];
}

// The thread's element of variables v0 .. v1-1 (one net's trainable ones, read through L).  FUSED: + the optimizer step
// (o.apply) and the soft update (o.soft).
template <bool FUSED>
__device__ __forceinline__ void wgrad_element(const Layout& L, const GradSrc& src, int v0, int v1, int B, const Opt& o) {
  const int64_t e = L.off[v0] + (int64_t)blockIdx.x * THREADS + threadIdx.x;
  if (e < L.off[v1]) {
    int v = v1 - 1;
    while (e < L.off[v]) --v;
    if (v != C_B2DEAD) {
      const int64_t loc = e - L.off[v];
      const int N = L.cols[v];
      const int k = (int)(loc / N), j = (int)(loc % N);
      const float* __restrict__ d = src.d[v];
      const float* __restrict__ x = src.in[v];
      const float* __restrict__ mul = src.mul[v];
      const int ld = src.ld_d[v], li = src.ld_in[v];
      float g = 0.f;
      if (x) {
        for (int r = 0; r < B; ++r) g = fmaf(x[(size_t)r * li + k], d[(size_t)r * ld + j], g);
      } else if (mul) {
        for (int r = 0; r < B; ++r) g = fmaf(mul[(size_t)r * ld + j], d[(size_t)r * ld + j], g);
      } else {
        for (int r = 0; r < B; ++r) g += d[(size_t)r * ld + j];
      }
      o.grad[e] = g;
      if (FUSED && o.apply) opt_step(o, e, g);
    }
    if (FUSED && o.soft) soft_step(o, e);
  }
}

// {max q, mean q}, summed in row order by the thread that calls it
__device__ __forceinline__ void q_stats(const Work& w, int B) {
  float mx = w.c[0].q[0], s = 0.f;
  for (int r = 0; r < B; ++r) {
    const float q = w.c[0].q[r];
    mx = fmaxf(mx, q);
    s += q;
  }
  w.qstat[0] = mx;
  w.qstat[1] = s / (float)B;
}

// The elements of variables v0 .. v1-1 of critic blockIdx.y (NC = 1: of the one net; the actor's too).  The arenas are the same
// for every critic, so one Opt serves them all.  The launch for the critics' variables also leaves critic 1's {max q, mean q}.
template <int NC, bool FUSED>
__global__ __launch_bounds__(THREADS) void ddpg_wgrad_kernel(PerCritic<Layout, NC> L, PerCritic<GradSrc, NC> src, int v0, int v1,
                                                             int B, Opt o, Work w) {
  const int c = NC == 1 ? 0 : blockIdx.y;
  wgrad_element<FUSED>(L.v[c], src.v[c], v0, v1, B, o);
  if (v0 == NACTOR && c == 0 && blockIdx.x == 0 && threadIdx.x == 0) q_stats(w, B);
}

// The block's variable v: tf.clip_by_norm (g clip / max(||g||, clip)), the step, the soft update.
__device__ __forceinline__ void update_variable(const Layout& L, int v, const Opt& o) {
  __shared__ float sh[RED];
  const int64_t lo = L.off[v], hi = L.off[v + 1];
  const bool dead = v == C_B2DEAD;
  float s = 0.f;
  for (int64_t i = lo + threadIdx.x; i < hi; i += THREADS) s += o.grad[i] * o.grad[i];
  const float scale = o.clip / fmaxf(sqrtf(block_sum<THREADS>(s, sh)), o.clip);
  for (int64_t i = lo + threadIdx.x; i < hi; i += THREADS) {
    if (!dead && o.apply) opt_step(o, i, o.grad[i] * scale);
    if (o.soft) soft_step(o, i);
  }
}

// One block per critic variable: blocks 0..9 critic 1's, with NC = 2 blocks 10..19 critic 2's.
template <int NC>
__global__ __launch_bounds__(THREADS) void ddpg_update_kernel(PerCritic<Layout, NC> L, Opt o) {
  update_variable(L.v[NC == 1 ? 0 : blockIdx.x / NCRITIC], NACTOR + blockIdx.x % NCRITIC, o);
}

// Ring slot (first + i) mod cap <- s | a | r | done | s2, from row `s[S] | s2[S] | done` of the transport and the staged r, a.
// disc (null without n-step returns): the slot's discount <- gamma, a one-step row's.
__global__ void ddpg_ring_gather_kernel(const char* __restrict__ seg, const int64_t* __restrict__ off, const float* __restrict__ r,
                                        const float* __restrict__ a, int n, float* __restrict__ ring, int64_t first, int64_t cap,
                                        int S, int A, float* __restrict__ disc, float gamma) {
  const int rowf = 2 * S + A + 2;
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (int64_t)n * rowf) return;
  const int i = (int)(e / rowf), c = (int)(e % rowf);
  const float* __restrict__ row = reinterpret_cast<const float*>(seg + off[i]);
  float v;
  if (c < S) v = row[c];
  else if (c < S + A) v = a[(size_t)i * A + c - S];
  else if (c == S + A) v = r[i];
  else if (c == S + A + 1) v = row[2 * S];
  else v = row[S + c - (S + A + 2)];
  ring[((first + i) % cap) * rowf + c] = v;
  if (disc && c == 0) disc[(first + i) % cap] = gamma;
}

// disc of the n slots from `first` on (mod cap) <- gamma: rows added by hand are one-step rows.  n <= cap.
__global__ void nstep_fill_kernel(float* __restrict__ disc, float gamma, int64_t first, int n, int64_t cap) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) disc[(first + i) % cap] = gamma;
}

// ------------------------------------------------------------------ prioritised replay
constexpr int PER_CHUNK = 1024;              // slots of one chunk sum
constexpr int PER_SUM_THREADS = 256;
constexpr int PER_THREADS = 1024;            // the one-workgroup kernels; also the most chunks a ring may have
constexpr int PER_WALK = 32;                 // slots a walk loads ahead of its additions (pa holds whole chunks)

using ga3c_uniform::actor_uniform;

// pa of the n slots from `first` on (mod cap) <- max_pa: a row nobody has trained on yet is as urgent as any seen.  n <= cap.
__global__ void per_fill_kernel(float* __restrict__ pa, const float* __restrict__ max_pa, int64_t first, int n, int64_t cap) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) pa[(first + i) % cap] = *max_pa;
}

// csum[c] = the f64 sum of chunk c's slots below `size`: thread t adds slots t, t + 256, t + 512, t + 768 in that order, the
// 256 partials fold by the halving tree.
__global__ __launch_bounds__(PER_SUM_THREADS) void per_chunk_sum_kernel(const float* __restrict__ pa, int size,
                                                                        double* __restrict__ csum) {
  __shared__ double red[PER_SUM_THREADS];
  const int t = threadIdx.x, base = blockIdx.x * PER_CHUNK;
  double s = 0.0;
  for (int k = 0; k < PER_CHUNK / PER_SUM_THREADS; ++k) {
    const int j = base + t + k * PER_SUM_THREADS;
    s += j < size ? (double)pa[j] : 0.0;
  }
  red[t] = s;
  __syncthreads();
  for (int h = PER_SUM_THREADS / 2; h > 0; h >>= 1) {
    if (t < h) red[t] += red[t + h];
    __syncthreads();
  }
  if (t == 0) csum[blockIdx.x] = red[0];
}

// w of row k before the batch's largest divides it: (size pa / total)^-beta
__device__ __forceinline__ double per_weight(float pa, int size, double total, double beta) {
  return pow((double)size * (double)pa / total, -beta);
}

// One workgroup.  The inclusive Hillis-Steele scan of the chunk sums (actors_compact_kernel's pattern, in f64), then row k
// of the batch: target = (k + u(seed, number, k)) total / B, the first chunk whose scanned sum exceeds it (the last if none
// does), and within it the first slot at which the running sum, started from the chunk before, exceeds it (the chunk's last
// slot below `size` if none does: the tree and the walk associate differently).  Every addition is tests/per_oracle.py's.
__global__ __launch_bounds__(PER_THREADS) void per_sample_kernel(const float* __restrict__ pa, const double* __restrict__ csum,
                                                                 int size, int B, uint64_t seed, uint64_t number, double beta,
                                                                 int32_t* __restrict__ slots, float* __restrict__ w) {
#pragma clang fp contract(off)
  __shared__ double x[PER_THREADS];
  __shared__ double wm[PER_THREADS];
  const int t = threadIdx.x;
  const int nchunks = (size + PER_CHUNK - 1) / PER_CHUNK;
  x[t] = t < nchunks ? csum[t] : 0.0;
  __syncthreads();
  for (int d = 1; d < PER_THREADS; d <<= 1) {
    const double v = t >= d ? x[t - d] : 0.0;
    __syncthreads();
    if (t >= d) x[t] += v;
    __syncthreads();
  }
  const double total = x[nchunks - 1], seg = total / (double)B;
  double mx = 0.0;
  for (int k = t; k < B; k += PER_THREADS) {
    const double target = ((double)k + actor_uniform(seed, number, (uint64_t)k)) * seg;
    int c = nchunks - 1;
    for (int i = 0; i < nchunks; ++i)
      if (target < x[i]) {
        c = i;
        break;
      }
    const int lo = c * PER_CHUNK, hi = min(size, lo + PER_CHUNK);
    double acc = c ? x[c - 1] : 0.0;
    int slot = hi - 1;
    bool hit = false;
    for (int j0 = lo; j0 < hi && !hit; j0 += PER_WALK) {
      f32x4 v[PER_WALK / 4];                 // the walk waits on memory, not on its additions: one wait per 32 slots
#pragma unroll
      for (int i = 0; i < PER_WALK / 4; ++i) v[i] = reinterpret_cast<const f32x4*>(pa + j0)[i];
#pragma unroll
      for (int i = 0; i < PER_WALK; ++i)
        if (!hit && j0 + i < hi) {
          acc += (double)v[i / 4][i % 4];
          if (target < acc) {
            slot = j0 + i;
            hit = true;
          }
        }
    }
    slots[k] = slot;
    mx = fmax(mx, per_weight(pa[slot], size, total, beta));
  }
  wm[t] = mx;
  __syncthreads();
  for (int h = PER_THREADS / 2; h > 0; h >>= 1) {
    if (t < h) wm[t] = fmax(wm[t], wm[t + h]);
    __syncthreads();
  }
  const double largest = wm[0];
  for (int k = t; k < B; k += PER_THREADS) w[k] = (float)(per_weight(pa[slots[k]], size, total, beta) / largest);
}

// One workgroup, after ddpg_critic_kernel: td_i = |y_i - q_i|, pa[slot_i] = (td_i + eps)^alpha, max_pa = max(max_pa, every
// new priority).  The batch's slots lie in LDS and row i stores only if no later row names its slot: the last row in batch
// order wins and no two rows store to one slot.  B <= MAX_B.
__global__ __launch_bounds__(PER_THREADS) void per_update_kernel(const int32_t* __restrict__ slots, const float* __restrict__ q,
                                                                 const float* __restrict__ y, int B, float eps, float alpha,
                                                                 float* __restrict__ pa, float* __restrict__ max_pa,
                                                                 float* __restrict__ td) {
  __shared__ int32_t sl[MAX_B];
  __shared__ float red[PER_THREADS];
  const int t = threadIdx.x;
  for (int i = t; i < B; i += PER_THREADS) sl[i] = slots[i];
  __syncthreads();
  float mx = 0.f;
  for (int i = t; i < B; i += PER_THREADS) {
    const float d = fabsf(y[i] - q[i]);
    td[i] = d;
    const float p = powf(d + eps, alpha);
    mx = fmaxf(mx, p);
    bool last = true;
    for (int j = i + 1; j < B; ++j)
      if (sl[j] == sl[i]) {
        last = false;
        break;
      }
    if (last) pa[sl[i]] = p;
  }
  red[t] = mx;
  __syncthreads();
  for (int h = PER_THREADS / 2; h > 0; h >>= 1) {
    if (t < h) red[t] = fmaxf(red[t], red[t + h]);
    __syncthreads();
  }
  if (t == 0) *max_pa = fmaxf(*max_pa, red[0]);
}

// ------------------------------------------------------------------ device actors
constexpr int ACT_THREADS = 256;             // the step kernel: one thread per environment
constexpr int ACT_MAX_UPDATES = 16;

// Everything the actor kernels touch besides the replay ring, by device address; per environment unless said otherwise.
struct ActState {
  int N;
  uint64_t seed;
  double* phys;              // [N][P] f64 physics
  int* elapsed;
  uint64_t* draws;           // uniforms drawn so far
  float* obs;                // [N][S] what the actor reads
  float* action;             // [N][A] the last prediction, actor(obs) + noise, as the ring keeps it
  double* reward;            // the last step's reward and done
  int* done;
  double* total_reward;      // of the running episode: the rewards in step order
  long long* total_length;   // its transitions
  ga3c_actors::Episodes ep;  // this step's finished episodes and the episode ring
};

using ga3c_actors::PendulumTask;

// One step of environment i = the thread's index, the one statement of it for the kernels below.  first: the handle's first
// ever step, the host's step(None): the zero action, nothing kept of the transition, its done not looked at.  Otherwise the
// action is a.action's row and keep(i, obs, a, reward, ended, terminal, obs') puts the transition where the kernel wants it,
// before the episode's totals move.  The f64 physics must not contract; neither may a `keep` that does arithmetic.
// task: the handle's, the fork's values until it is given one.  `ended` is the time limit reached: a.done, the
// episode record, the reset and its draws follow it; `terminal` is what a ring row calls done, `ended` unless the task
// truncates.  obs' is the observation before any reset; under reset_observation a.obs then becomes the observation of the
// reset physics.
template <class Env, class Keep>
__device__ __forceinline__ void actor_step(const ActState& a, int first, const PendulumTask& task, Keep keep) {
#pragma clang fp contract(off)
  const int i = blockIdx.x * ACT_THREADS + threadIdx.x;
  if (i >= a.N) return;
  constexpr int S = Env::S, P = Env::P, A = Env::A;
  double s[P];
  int elapsed;
  ga3c_actors::load_physics<P>(a.phys, a.elapsed, i, s, elapsed);
  float av[A];
  for (int j = 0; j < A; ++j) av[j] = first ? 0.f : a.action[(size_t)i * A + j];
  float* obs = a.obs + (size_t)i * S;
  float before[S], after[S];
  for (int k = 0; k < S; ++k) before[k] = obs[k];
  double reward;
  int done;
  Env::step(s, av, task, &elapsed, &reward, &done);
  Env::observe(s, after);
  for (int k = 0; k < S; ++k) obs[k] = after[k];
  a.reward[i] = reward;
  a.done[i] = done;
  a.ep.ep_flag[i] = 0;
  if (first) {
    for (int j = 0; j < A; ++j) a.action[(size_t)i * A + j] = 0.f;
    ga3c_actors::store_physics<P>(a.phys, a.elapsed, i, s, elapsed);
    return;
  }
  keep(i, before, av, reward, done, (done && !task.truncate) ? 1 : 0, after);
  double total = a.total_reward[i] + reward;
  long long length = a.total_length[i] + 1;
  if (done) {                           // ProcessAgent.run's record of an episode shipped as one rollout: len(experiences) + 1
    uint64_t draws = a.draws[i];
    length += 1;
    ga3c_actors::finish_episode<Env>(a.ep, i, a.seed, total, length, draws, s, elapsed);
    a.draws[i] = draws;
    if (task.reset_observation) {       // the next transition starts at the reset state
      float fresh[S];
      Env::observe(s, fresh);
      for (int k = 0; k < S; ++k) obs[k] = fresh[k];
    }
  }
  a.total_reward[i] = total;
  a.total_length[i] = length;
  ga3c_actors::store_physics<P>(a.phys, a.elapsed, i, s, elapsed);
}

// actor_step with the transition obs | a | (f32) reward | done | obs' into ring slot (slot0 + i) mod cap (n <= cap: no two
// threads share a slot).  With priorities that slot gets max_pa, which only per_update_kernel writes, earlier on this stream:
// per_fill_kernel's value.
// Fork: the task is known to be the fork's and `given` is not read, so the compiler folds the task's branches away; launched
// for a handle without a task, because at N = 4096 the step under the run-time task measured 0.1 us above the mark.
template <class Env, bool Fork>
__global__ __launch_bounds__(ACT_THREADS) void ddpg_actors_step_kernel(ActState a, PendulumTask given, int first,
                                                                       float* __restrict__ ring, int64_t slot0, int64_t cap,
                                                                       float* __restrict__ pa, const float* __restrict__ max_pa) {
#pragma clang fp contract(off)
  constexpr int S = Env::S, A = Env::A;
  constexpr int rowf = 2 * S + A + 2;
  const PendulumTask task = Fork ? PendulumTask::fork() : given;
  actor_step<Env>(a, first, task,
                  [&](int i, const float* before, const float* av, double reward, int, int terminal, const float* after) {
#pragma clang fp contract(off)
    const int64_t slot = (slot0 + i) % cap;
    float* row = ring + slot * rowf;
    for (int k = 0; k < S; ++k) row[k] = before[k];
    for (int j = 0; j < A; ++j) row[S + j] = av[j];
    row[S + A] = (float)reward;
    row[S + A + 1] = terminal ? 1.f : 0.f;
    for (int k = 0; k < S; ++k) row[S + A + 2 + k] = after[k];
    if (pa) pa[slot] = *max_pa;
  });
}

// The environments' windows of a handle with n-step returns: the last n transitions of each, entry-major and
// environment-minor, so that a wave's loads and stores of one field of one entry are contiguous.
struct NWindow {
  int n;                     // entries: transition c lies in entry c mod n
  float* f;                  // [n][2 S + A + 1][N]: s | a as predicted | done | s2
  double* r;                 // [n][N] the f64 rewards
};

// actor_step with the ring write delayed by n - 1 transitions.  entry = c mod n for the handle's transition count c (the
// host's: every environment steps on every step); emit = c >= n - 1.  The transition goes to window entry `entry`.
// On an emitting step the row of the transition that began at u = c - n + 1, which lies in entry (entry + 1) mod n, goes to ring
// slot (slot0 + i) mod cap: m = the first k in 1..n whose transition u + k - 1 is done, n if none; R = sum_{k<m} g_k r_{u+k} in
// f64, ascending k, g_0 = 1 and g_{k+1} = g_k gamma64; the row is s_u | a_u | (f32) R | done_{u+m-1} | s2_{u+m-1} and
// disc[slot] = (f32) g_m.  Nothing is summed across an episode's end; at n = 1 the row and gamma are ddpg_actors_step_kernel's.
// Under a task the window's done is `ended`, where the sum is cut; Pendulum ends at its time limit alone, so the
// last summed transition's `terminal` is that flag, or 0 for every row when the task truncates.
template <class Env>
__global__ __launch_bounds__(ACT_THREADS) void ddpg_actors_nstep_kernel(ActState a, PendulumTask task, NWindow w, int first,
                                                                        int entry, int emit, double gamma64, float* __restrict__ ring,
                                                                        int64_t slot0, int64_t cap, float* __restrict__ disc,
                                                                        float* __restrict__ pa, const float* __restrict__ max_pa) {
#pragma clang fp contract(off)
  constexpr int S = Env::S, A = Env::A;
  constexpr int rowf = 2 * S + A + 2, W = 2 * S + A + 1;
  const size_t N = (size_t)a.N;
  actor_step<Env>(a, first, task,
                  [&](int i, const float* before, const float* av, double reward, int ended, int, const float* after) {
#pragma clang fp contract(off)
    const int n = w.n;
    {
      float* e = w.f + (size_t)entry * W * N + i;
      for (int k = 0; k < S; ++k) e[k * N] = before[k];
      for (int j = 0; j < A; ++j) e[(S + j) * N] = av[j];
      e[(S + A) * N] = ended ? 1.f : 0.f;
      for (int k = 0; k < S; ++k) e[(S + A + 1 + k) * N] = after[k];
      w.r[(size_t)entry * N + i] = reward;
    }
    if (emit) {
      const int oldest = entry + 1 == n ? 0 : entry + 1;
      int j = oldest, last = oldest;
      double R = 0.0, g = 1.0;
      float d = 0.f;
      for (int k = 0; k < n; ++k) {
        R = R + g * w.r[(size_t)j * N + i];
        g = g * gamma64;
        d = w.f[((size_t)j * W + S + A) * N + i];
        last = j;
        if (d != 0.f) break;
        j = j + 1 == n ? 0 : j + 1;
      }
      const int64_t slot = (slot0 + i) % cap;
      float* row = ring + slot * rowf;
      const float* eo = w.f + (size_t)oldest * W * N + i;
      const float* el = w.f + (size_t)last * W * N + i;
      for (int k = 0; k < S + A; ++k) row[k] = eo[k * N];
      row[S + A] = (float)R;
      row[S + A + 1] = task.truncate ? 0.f : d;
      for (int k = 0; k < S; ++k) row[S + A + 2 + k] = el[(S + A + 1 + k) * N];
      disc[slot] = (float)g;
      if (pa) pa[slot] = *max_pa;
    }
  });
}

// One workgroup: the step's finished episodes go to the episode ring in environment order (ga3c_actors.hpp).
__global__ __launch_bounds__(ga3c_actors::SCAN_THREADS) void ddpg_actors_episodes_kernel(ActState a) {
  __shared__ int sep[ga3c_actors::SCAN_THREADS];
  ga3c_actors::scan_append_episodes(a.ep, a.N, sep);
}

// Row k of a step's B rows from a ring that holds size > B of them: stratum [k size / B, (k + 1) size / B) in integers, and in
// it the slot lo + min(w - 1, (int64)(u w)), u = u(seed, sample number, k).  The strata are disjoint and none is empty, so the
// slots are distinct, as random.sample's are.
__global__ void ddpg_uniform_slots_kernel(int64_t size, int B, uint64_t seed, uint64_t number, int32_t* __restrict__ slots) {
#pragma clang fp contract(off)
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= B) return;
  const int64_t lo = (int64_t)k * size / B, hi = ((int64_t)k + 1) * size / B, w = hi - lo;
  const double u = ga3c_uniform::actor_uniform(seed, number, (uint64_t)k);
  const int64_t j = (int64_t)(u * (double)w);
  slots[k] = (int32_t)(lo + (j < w - 1 ? j : w - 1));
}

// ------------------------------------------------------------------ evaluation episodes
constexpr int EVAL_MAX_ENVS = GA3C_DDPG_EVAL_MAX_ENVS;
constexpr int EVAL_MAX_STEPS = GA3C_DDPG_EVAL_MAX_STEPS;       // a Pendulum-v0 episode under its TimeLimit; the trace's row stride

// What a traced evaluation keeps of every step, [n][EVAL_MAX_STEPS][width]; all null: nothing is stored.
struct EvalTrace {
  double* phys;              // [..][P] the physics before the step
  float* obs;                // [..][S] what the actor read
  float* action;             // [..][A] what it answered
  double* reward;            // [..]
};

// The deterministic actor as an evaluation's policy: its forward, which ends in a barrier, and how thread r reads action j from
// the head's LDS buffer afterwards.  SoftPolicy (8u, below) is the soft actor's.
struct DetPolicy {
  __device__ static void fwd(const Layout& L, const float* th, const float* xin, float* bufA, float* bufB, float* head, int row0,
                             int nrows) {
    actor_fwd(L, th, xin, bufA, bufB, head, nullptr, ActorKeep{nullptr, nullptr, nullptr, nullptr, nullptr}, row0, nrows);
  }
  __device__ static float action(const float* head, int j, int r) { return head[j * TILE + r]; }
};

// A whole noise-free episode of `steps` steps for environments row0 .. row0 + 15, one workgroup: thread r < nrows keeps
// environment row0 + r's physics, step count and reward sum in registers; every step is the policy's forward on the tile's
// observations (th: the value arena or the target arena), then Env::step under the handle's task and Env::observe by those
// threads, as actor_step states them, and the reward added in step order in f64.  Every episode starts from start[i] with
// elapsed = 0.  Of the task only the reward matters here: no bound is reached after tanh (Env::step's wrap branch is the
// training actors' statement, kept whole), and there is no ring and no reset; `done` is Env::step's out-argument, and the loop
// is bounded by `steps` alone.
// Reads th and start; writes total_out, phys_out and the trace: no ActState, no ring, no priorities, no windows.
template <class Env, class Policy>
__global__ __launch_bounds__(THREADS) void ddpg_eval_kernel(Layout L, const float* __restrict__ th, int n, int steps,
                                                            PendulumTask task, const double* __restrict__ start,
                                                            double* __restrict__ total_out, double* __restrict__ phys_out,
                                                            EvalTrace tr) {
#pragma clang fp contract(off)
  __shared__ __attribute__((aligned(16))) float xin[MAX_S * TILE];
  __shared__ __attribute__((aligned(16))) float bufA[H1 * TILE];
  __shared__ __attribute__((aligned(16))) float bufB[H2 * TILE];
  __shared__ __attribute__((aligned(16))) float head[MAX_A * TILE];
  constexpr int S = Env::S, P = Env::P, A = Env::A;
  const int row0 = blockIdx.x * TILE, nrows = min(TILE, n - row0);
  const int r = threadIdx.x;
  const size_t i = (size_t)row0 + r;                 // the thread's environment, r < nrows
  double s[P];
  double total = 0.0;
  int elapsed = 0;
  float obs[S];
  if (r < TILE) {
    for (int k = 0; k < S; ++k) obs[k] = 0.f;
    if (r < nrows) {
      for (int k = 0; k < P; ++k) s[k] = start[i * P + k];
      Env::observe(s, obs);
    }
    for (int k = 0; k < S; ++k) xin[k * TILE + r] = obs[k];
  }
  __syncthreads();
  for (int t = 0; t < steps; ++t) {
    // ends in a barrier: head is whole, and no thread reads xin any more
    Policy::fwd(L, th, xin, bufA, bufB, head, row0, nrows);
    if (r < nrows) {
      float av[A];
      for (int j = 0; j < A; ++j) av[j] = Policy::action(head, j, r);
      const size_t at = i * EVAL_MAX_STEPS + t;
      if (tr.phys) {
        for (int k = 0; k < P; ++k) tr.phys[at * P + k] = s[k];
        for (int k = 0; k < S; ++k) tr.obs[at * S + k] = obs[k];
        for (int j = 0; j < A; ++j) tr.action[at * A + j] = av[j];
      }
      double reward;
      int done;
      Env::step(s, av, task, &elapsed, &reward, &done);
      total = total + reward;
      Env::observe(s, obs);
      for (int k = 0; k < S; ++k) xin[k * TILE + r] = obs[k];
      if (tr.phys) tr.reward[at] = reward;
    }
    __syncthreads();                                 // the next step's actor reads these observations
  }
  if (r < nrows) {
    total_out[i] = total;
    for (int k = 0; k < P; ++k) phys_out[i * P + k] = s[k];
  }
}

// ------------------------------------------------------------------ soft actor-critic
constexpr int SOFT_MAX_A = MAX_A / 2;        // the head's LDS arrays hold MAX_A rows and the head has 2 A
constexpr float SOFT_LN2 = 0.6931471805599453f, SOFT_HALF_LN_2PI = 0.9189385332046727f;

// What every soft kernel reads of the handle's state, by value.
struct SoftCfg {
  float ls_min, ls_max;
  int64_t la;                // where log_alpha lies in every arena
  uint64_t seed;
};

// The rows a soft step writes beside Work's: eps2, a2, mu, ls, eps, u [B,A]; logp2, vt, logp, q1, q2 [B]; stat: {mean logp}.
struct SoftRows {
  float *eps2, *a2, *logp2, *vt;
  float *mu, *ls, *eps, *u, *logp, *q1, *q2;
  float* stat;
};

// 8n's Box-Muller draw j of `stream`, unclipped: n = sqrt(-2 ln u1) cos(2 pi u2) in f64 on uniforms 2j and 2j + 1, then f32
__device__ __forceinline__ float soft_normal(uint64_t seed, uint64_t stream, uint64_t j) {
  const double u1 = 1.0 - ga3c_uniform::actor_uniform(seed, stream, 2 * j);
  const double u2 = ga3c_uniform::actor_uniform(seed, stream, 2 * j + 1);
  return (float)(sqrt(-2.0 * log(u1)) * cos(6.283185307179586 * u2));
}

// actor_fwd with the raw head of a soft handle: raw [2A][16] <- a2 W_o + b_o, W_o [300, 2A]; no tanh, nothing of the head kept.
__device__ void soft_actor_fwd(const Layout& L, const float* __restrict__ th, const float* xin, float* bufA, float* bufB, float* raw,
                               ActorKeep kp, int row0, int nrows) {
  dense_fwd<THREADS>(th + L.off[A_W1], th + L.off[A_B1], L.S, H1, xin, nullptr, 0, nullptr, [&](int j, int r, float h) {
    float n;
    const float xh = bn_apply(th, L, A_MM1, A_MV1, A_BE1, A_GA1, j, h, &n);
    const float a = fmaxf(n, 0.f);
    bufA[j * TILE + r] = a;
    if (kp.a1 && r < nrows) {
      kp.xh1[(size_t)(row0 + r) * H1 + j] = xh;
      kp.a1[(size_t)(row0 + r) * H1 + j] = a;
    }
  });
  dense_fwd<THREADS>(th + L.off[A_W2], th + L.off[A_B2], H1, H2, bufA, nullptr, 0, nullptr, [&](int j, int r, float h) {
    float n;
    const float xh = bn_apply(th, L, A_MM2, A_MV2, A_BE2, A_GA2, j, h, &n);
    const float a = fmaxf(n, 0.f);
    bufB[j * TILE + r] = a;
    if (kp.a2 && r < nrows) {
      kp.xh2[(size_t)(row0 + r) * H2 + j] = xh;
      kp.a2[(size_t)(row0 + r) * H2 + j] = a;
    }
  });
  dense_fwd<THREADS>(th + L.off[A_WO], th + L.off[A_BO], H2, L.cols[A_WO], bufB, nullptr, 0, nullptr,
                     [&](int j, int r, float h) { raw[j * TILE + r] = h; });
}

// The sample of the tile from raw [2A][16] and eps [A][16]: ls = clamp(raw[A + i]), sigma = exp(ls), u = fmaf(sigma, eps, mu),
// act[i][r] = tanh(u); sg (may be null) <- sigma, ub <- u; then, by the thread of row r, in i order,
// logp = sum_i (((-0.5 eps^2 - ls) - ln sqrt(2 pi)) - 2 ((ln 2 - |u|) - log1p(exp(-2 |u|)))): ln(1 - tanh^2 u) from u itself, which
// stays finite where tanhf rounds to 1.  Ends in a barrier.
__device__ __forceinline__ void soft_sample(int A, const SoftCfg& c, float* raw, const float* eps, float* act, float* ub, float* sg,
                                            float* lp) {
  for (int e = threadIdx.x; e < A * TILE; e += THREADS) {
    const float ls = fminf(fmaxf(raw[A * TILE + e], c.ls_min), c.ls_max);
    const float sigma = expf(ls);
    const float u = fmaf(sigma, eps[e], raw[e]);
    if (sg) sg[e] = sigma;
    ub[e] = u;
    act[e] = tanhf(u);
  }
  __syncthreads();
  if (threadIdx.x < TILE) {
    const int r = threadIdx.x;
    float s = 0.f;
    for (int i = 0; i < A; ++i) {
      const float n = eps[i * TILE + r], au = fabsf(ub[i * TILE + r]);
      const float ls = fminf(fmaxf(raw[(A + i) * TILE + r], c.ls_min), c.ls_max);
      const float l1 = 2.0f * ((SOFT_LN2 - au) - log1pf(expf(-2.0f * au)));
      s += ((-0.5f * n * n - ls) - SOFT_HALF_LN_2PI) - l1;
    }
    lp[r] = s;
  }
  __syncthreads();
}

struct SoftTarget {
  float *y, *qt, *qt1, *qt2;
  uint64_t number;           // the draws' stream: 2 t
};

// Steps 1-2 of a soft step.  The ONLINE actor (th) samples a2, logp2 at s2 on stream `number`; both target critics (thT) read a2,
// one after the other in the same buffers; q' = min, v' = q' - alpha logp2 with alpha = exp(log_alpha) as it stands, and
// y = r on a done row or without `future`, else fmaf(g, v', r).  "qt" stays min q'.
__global__ __launch_bounds__(THREADS) void ddpg_soft_target_kernel(PerCritic<Layout, 2> L, const float* __restrict__ th,
                                                                   const float* __restrict__ thT, Rows src, int B, float gamma,
                                                                   int future, SoftCfg cfg, SoftTarget t, SoftRows sr,
                                                                   const float* __restrict__ disc, float* __restrict__ used) {
  __shared__ __attribute__((aligned(16))) float xin[MAX_S * TILE];
  __shared__ __attribute__((aligned(16))) float bufA[H1 * TILE];
  __shared__ __attribute__((aligned(16))) float bufB[H2 * TILE];
  __shared__ __attribute__((aligned(16))) float raw[MAX_A * TILE];
  __shared__ __attribute__((aligned(16))) float act[SOFT_MAX_A * TILE];
  __shared__ __attribute__((aligned(16))) float eps[SOFT_MAX_A * TILE];
  __shared__ __attribute__((aligned(16))) float ub[SOFT_MAX_A * TILE];
  __shared__ float lp[TILE];
  __shared__ float qv[2][TILE];
  const int S = L.v[0].S, A = L.v[0].A;
  const int row0 = blockIdx.x * TILE, nrows = min(TILE, B - row0);
  if (future) {
    load_rows(src, S + A + 2, S, xin, row0, nrows, nullptr);
    for (int e = threadIdx.x; e < A * TILE; e += THREADS) {
      const int i = e / TILE, r = e % TILE;
      eps[e] = soft_normal(cfg.seed, t.number, (uint64_t)(row0 + r) * (uint64_t)A + (uint64_t)i);
    }
    __syncthreads();
    soft_actor_fwd(L.v[0], th, xin, bufA, bufB, raw, ActorKeep{nullptr, nullptr, nullptr, nullptr, nullptr}, row0, nrows);
    soft_sample(A, cfg, raw, eps, act, ub, nullptr, lp);
    for (int e = threadIdx.x; e < A * TILE; e += THREADS) {
      const int i = e / TILE, r = e % TILE;
      if (r < nrows) {
        sr.eps2[(size_t)(row0 + r) * A + i] = eps[e];
        sr.a2[(size_t)(row0 + r) * A + i] = act[e];
      }
    }
#pragma unroll
    for (int c = 0; c < 2; ++c) critic_fwd(L.v[c], thT, xin, act, bufA, bufB, qv[c], CriticKeep{nullptr, nullptr, nullptr}, row0, nrows);
  }
  if (threadIdx.x < nrows) {
    const int r = threadIdx.x;
    const int64_t slot = src.idx ? src.idx[row0 + r] : row0 + r;
    const float rew = src.base[slot * src.rowf + S + A], done = src.base[slot * src.rowf + S + A + 1];
    const float g = row_discount(disc, used, slot, row0 + r, gamma);
    const float q1 = future ? qv[0][r] : 0.f, q2 = future ? qv[1][r] : 0.f;
    const float qt = fminf(q1, q2);
    float y = rew;
    if (future) {
      const float alpha = expf(th[cfg.la]);
      const float vt = qt - alpha * lp[r];
      if (done == 0.f) y = fmaf(g, vt, rew);
      sr.logp2[row0 + r] = lp[r];
      sr.vt[row0 + r] = vt;
    }
    t.y[row0 + r] = y;
    t.qt[row0 + r] = qt;
    t.qt1[row0 + r] = q1;
    t.qt2[row0 + r] = q2;
  }
}

// Steps 4-5 of a soft step, on policy steps.  The actor samples a, logp at s on stream `number` (2 t + 1); the two UPDATED critics
// are evaluated one after the other in the same buffers, each leaving its q and its dq/da [A][16]; per row the smaller q selects
// its critic, critic 1 on a tie, and with g its dq/da, c = 1 / B:
//   du_i = c (2 alpha a_i - g_i (1 - a_i^2)), 1 - a^2 from u as actor_fwd's dact;  dmu_i = du_i;
//   dls_i = du_i sigma_i eps_i - c alpha where the raw ls lies inside (ls_min, ls_max), else 0.
// "do" = dmu | dls [B, 2A] goes back through the head and the trunk as actor_rows does it.
__global__ __launch_bounds__(THREADS) void ddpg_soft_actor_kernel(PerCritic<Layout, 2> L, const float* __restrict__ th, Rows src, int B,
                                                                  SoftCfg cfg, uint64_t number, Work w, SoftRows sr) {
  __shared__ __attribute__((aligned(16))) float xin[MAX_S * TILE];
  __shared__ __attribute__((aligned(16))) float bufA[H1 * TILE];
  __shared__ __attribute__((aligned(16))) float bufB[H2 * TILE];
  __shared__ __attribute__((aligned(16))) float raw[MAX_A * TILE];          // the raw head; later the delta at it
  __shared__ __attribute__((aligned(16))) float act[SOFT_MAX_A * TILE];
  __shared__ __attribute__((aligned(16))) float eps[SOFT_MAX_A * TILE];
  __shared__ __attribute__((aligned(16))) float ub[SOFT_MAX_A * TILE];
  __shared__ __attribute__((aligned(16))) float sg[SOFT_MAX_A * TILE];
  __shared__ __attribute__((aligned(16))) float gq[2][SOFT_MAX_A * TILE];   // each critic's dq/da
  __shared__ float lp[TILE];
  __shared__ float qv[2][TILE];
  const Layout& LA = L.v[0];
  const int S = LA.S, A = LA.A;
  const int row0 = blockIdx.x * TILE, nrows = min(TILE, B - row0);
  load_rows(src, 0, S, xin, row0, nrows, nullptr);
  for (int e = threadIdx.x; e < A * TILE; e += THREADS) {
    const int i = e / TILE, r = e % TILE;
    eps[e] = soft_normal(cfg.seed, number, (uint64_t)(row0 + r) * (uint64_t)A + (uint64_t)i);
  }
  __syncthreads();
  soft_actor_fwd(LA, th, xin, bufA, bufB, raw, ActorKeep{w.a_xh1, w.a_a1, w.a_xh2, w.a_a2, nullptr}, row0, nrows);
  // which raw ls lie inside the clamp, before soft_sample reads them: bit i of row r's mask
  __shared__ unsigned inside[TILE];
  if (threadIdx.x < TILE) {
    unsigned mask = 0;
    for (int i = 0; i < A; ++i) {
      const float o = raw[(A + i) * TILE + threadIdx.x];
      if (o > cfg.ls_min && o < cfg.ls_max) mask |= 1u << i;
    }
    inside[threadIdx.x] = mask;
  }
  soft_sample(A, cfg, raw, eps, act, ub, sg, lp);
  for (int e = threadIdx.x; e < A * TILE; e += THREADS) {
    const int i = e / TILE, r = e % TILE;
    if (r < nrows) {
      const size_t at = (size_t)(row0 + r) * A + i;
      sr.mu[at] = raw[e];
      sr.ls[at] = fminf(fmaxf(raw[A * TILE + e], cfg.ls_min), cfg.ls_max);
      sr.eps[at] = eps[e];
      sr.u[at] = ub[e];
      w.a_noisy[at] = act[e];
    }
  }
  if (threadIdx.x < nrows) sr.logp[row0 + threadIdx.x] = lp[threadIdx.x];
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    const Layout& LC = L.v[c];
    critic_fwd(LC, th, xin, act, bufA, bufB, qv[c], CriticKeep{nullptr, nullptr, nullptr}, row0, nrows);
    const float* __restrict__ wo = th + LC.off[C_WO];
    for (int e = threadIdx.x; e < H2 * TILE; e += THREADS) bufB[e] = bufB[e] > 0.f ? wo[e / TILE] : 0.f;
    __syncthreads();
    float* gc = gq[c];
    dense_bwd(th + LC.off[C_WN], A, H2, bufB, [&](int i, int r, float g) { gc[i * TILE + r] = g; });
  }
  const float alpha = expf(th[cfg.la]), cB = 1.0f / (float)B;
  if (threadIdx.x < nrows) {
    sr.q1[row0 + threadIdx.x] = qv[0][threadIdx.x];
    sr.q2[row0 + threadIdx.x] = qv[1][threadIdx.x];
  }
  for (int e = threadIdx.x; e < A * TILE; e += THREADS) {
    const int i = e / TILE, r = e % TILE;
    const float g = qv[1][r] < qv[0][r] ? gq[1][e] : gq[0][e];
    const float ex = expf(-2.0f * fabsf(ub[e]));
    const float dact = 4.0f * ex / ((1.0f + ex) * (1.0f + ex));
    float du = 0.f, dl = 0.f;
    if (r < nrows) {
      du = cB * (2.0f * alpha * act[e] - g * dact);
      if ((inside[r] >> i) & 1u) dl = du * sg[e] * eps[e] - cB * alpha;
      const size_t at = (size_t)(row0 + r) * (2 * A);
      w.g[(size_t)(row0 + r) * A + i] = g;
      w.dout[at + i] = du;
      w.dout[at + A + i] = dl;
    }
    raw[e] = du;
    raw[A * TILE + e] = dl;
  }
  __syncthreads();
  dense_bwd(th + LA.off[A_WO], H2, 2 * A, raw, [&](int k, int r, float s) {
    float d = 0.f;
    if (r < nrows) {
      d = w.a_a2[(size_t)(row0 + r) * H2 + k] > 0.f ? s : 0.f;
      w.a_dn2[(size_t)(row0 + r) * H2 + k] = d;
    }
    const float dh = d * bn_scale(th, LA, A_MV2, A_GA2, k);
    bufB[k * TILE + r] = dh;
    if (r < nrows) w.a_dh2[(size_t)(row0 + r) * H2 + k] = dh;
  });
  dense_bwd(th + LA.off[A_W2], H1, H2, bufB, [&](int k, int r, float s) {
    if (r < nrows) {
      const float d = w.a_a1[(size_t)(row0 + r) * H1 + k] > 0.f ? s : 0.f;
      w.a_dn1[(size_t)(row0 + r) * H1 + k] = d;
      w.a_dh1[(size_t)(row0 + r) * H1 + k] = d * bn_scale(th, LA, A_MV1, A_GA1, k);
    }
  });
}

// The temperature's step, by the one thread that calls it: mean logp over the rows in row order, the gradient of
// -log_alpha (mean logp + target_entropy), and ApplyAdam on the arenas' element `la` at `lr` (the annealed rate x alpha_lr, bias
// corrected at the actor's count).
struct SoftAlpha {
  const float* logp;
  float* stat;
  int64_t la;
  float target_entropy, lr;
};

// The actor's ddpg_wgrad_kernel<1, true> of a soft policy step, the temperature's step riding in it as q_stats rides in the
// critics': nothing later in the step reads alpha, and the next step's target kernel is a later launch.
__global__ __launch_bounds__(THREADS) void ddpg_soft_wgrad_kernel(Layout L, GradSrc src, int B, Opt o, SoftAlpha sa) {
  wgrad_element<true>(L, src, 0, NACTOR, B, o);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    float s = 0.f;
    for (int r = 0; r < B; ++r) s += sa.logp[r];
    const float mean = s / (float)B;
    const float g = -(mean + sa.target_entropy);
    sa.stat[0] = mean;
    o.grad[sa.la] = g;
    if (o.apply) {
      float m = o.sa[sa.la], v = o.sb[sa.la];
      m += (g - m) * ADAM_OMB1;
      v += (g * g - v) * ADAM_OMB2;
      o.sa[sa.la] = m;
      o.sb[sa.la] = v;
      o.theta[sa.la] -= sa.lr * m / (sqrtf(v) + ADAM_EPS);
    }
  }
}

// ddpg_predict_kernel for a soft handle.  mode GA3C_DDPG_NOISE_NONE: a = tanh(mu), no wrap.  GIVEN: eps = nz.v for every row.
// OWN: row r's eps[i] is draw count A + i of stream r under `seed` (the handle's seed + 1).  a = tanh(fmaf(sigma, eps, mu)).
// eps_out (may be null): the draws, [B][A].
__global__ __launch_bounds__(THREADS) void ddpg_soft_predict_kernel(Layout L, const float* __restrict__ th, Input in, int B,
                                                                    SoftCfg cfg, int mode, Noise nz, uint64_t seed, uint64_t count,
                                                                    float* __restrict__ a_out, float* __restrict__ eps_out) {
  __shared__ __attribute__((aligned(16))) float xin[MAX_S * TILE];
  __shared__ __attribute__((aligned(16))) float bufA[H1 * TILE];
  __shared__ __attribute__((aligned(16))) float bufB[H2 * TILE];
  __shared__ __attribute__((aligned(16))) float raw[MAX_A * TILE];
  const int A = L.A;
  const int row0 = blockIdx.x * TILE, nrows = min(TILE, B - row0);
  load_input_tile<THREADS, false>(in, L.S, row0, nrows, xin, nullptr);
  __syncthreads();
  soft_actor_fwd(L, th, xin, bufA, bufB, raw, ActorKeep{nullptr, nullptr, nullptr, nullptr, nullptr}, row0, nrows);
  for (int e = threadIdx.x; e < A * TILE; e += THREADS) {
    const int i = e / TILE, r = e % TILE;
    if (r >= nrows) continue;
    const size_t at = (size_t)(row0 + r) * A + i;
    float u = raw[e];
    if (mode != GA3C_DDPG_NOISE_NONE) {
      const float n = mode == GA3C_DDPG_NOISE_GIVEN ? nz.v[i] : soft_normal(seed, (uint64_t)(row0 + r), count * (uint64_t)A + (uint64_t)i);
      const float ls = fminf(fmaxf(raw[A * TILE + e], cfg.ls_min), cfg.ls_max);
      u = fmaf(expf(ls), n, u);
      if (eps_out) eps_out[at] = n;
    }
    a_out[at] = tanhf(u);
  }
}

// ddpg_eval_kernel's policy on a soft handle: the same episode under a = tanh(mu), mu the first A rows of the raw head.
struct SoftPolicy {
  __device__ static void fwd(const Layout& L, const float* th, const float* xin, float* bufA, float* bufB, float* head, int row0,
                             int nrows) {
    soft_actor_fwd(L, th, xin, bufA, bufB, head, ActorKeep{nullptr, nullptr, nullptr, nullptr, nullptr}, row0, nrows);
  }
  __device__ static float action(const float* head, int j, int r) { return tanhf(head[j * TILE + r]); }
};

// ------------------------------------------------------------------ host side
// The handle is a ga3c_vecnet::Core (ga3c_vecnet.hpp): stream, lanes, arenas, variables by name, checkpoint and registered
// segment are the shared ones.  Its own: the train step, the replay ring, the noise.

// The handle's normal generator: xoshiro256** seeded through splitmix64, Box-Muller on two uniforms per draw.
struct NormalGen {
  uint64_t s[4];
  void seed(uint64_t x) {
    for (int i = 0; i < 4; ++i) {
      x += 0x9E3779B97F4A7C15ull;
      uint64_t z = x;
      z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
      z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
      s[i] = z ^ (z >> 31);
    }
  }
  static uint64_t rotl(uint64_t x, int k) { return (x << k) | (x >> (64 - k)); }
  uint64_t next() {
    const uint64_t r = rotl(s[1] * 5, 7) * 9, t = s[1] << 17;
    s[2] ^= s[0]; s[3] ^= s[1]; s[1] ^= s[2]; s[0] ^= s[3]; s[2] ^= t; s[3] = rotl(s[3], 45);
    return r;
  }
  double uniform() { return ((double)(next() >> 11) + 0.5) * (1.0 / 9007199254740992.0); }   // (0, 1)
  double normal() {
    const double u1 = uniform(), u2 = uniform();
    return std::sqrt(-2.0 * std::log(u1)) * std::cos(6.283185307179586 * u2);
  }
};

}  // namespace ga3c_dd

using namespace ga3c_dd;
namespace vn = ga3c_vecnet;
using vn::fail;                   // HIPCHK's

// Prioritised replay of a handle (ga3c_ddpg_priorities_create).  pa holds a whole number of chunks, zero beyond the rows written.
struct Per {
  float alpha = 0.f, eps = 0.f;
  uint64_t seed = 0, samples = 0;       // the draw of sample number n is u(seed, n, row)
  float* pa = nullptr;                  // [capacity] priority ^ alpha by slot
  float* max_pa = nullptr;              // device f32: starts at 1, never decreases
  double* csum = nullptr;               // [PER_THREADS] chunk sums
  int32_t* slots = nullptr; float* w = nullptr; float* td = nullptr;     // [max_batch]: the last draw, its weights, the last |y - q|
  int32_t* h_slots = nullptr; float* h_w = nullptr;                      // pinned
  int w_rows = 0, td_rows = 0;          // rows of the last draw / prioritised step (fetch)
};

// Device actors of a handle (ga3c_ddpg_actors_create).  Everything below is read and written under train_mu.
struct DActors : ga3c_actors::ActorsCore {     // block: every device buffer of `d`, and `slots`; h_counts: d.ep.counts' two
  ActState d{};
  int32_t* slots = nullptr;             // [max_batch] the last draw without priorities
  int slots_rows = 0;                   // rows of the last draw, either way
  int updates = 1;                      // train steps after an actor step
  int batch = 0;                        // rows of a train step ("batch" of actors_set; starts at max_batch)
  uint64_t draw_seed = 0, samples = 0;  // the draw of sample number n without priorities is u(draw_seed, n, row)
  bool started = false;                 // the first actor step is the environments' step(None): one flag for all of them
  NWindow win{};                        // of a handle with n-step returns (in `block`); win.n = 0: none
  int64_t count = 0;                    // transitions every environment has made: the c of the next step
  EnvNoise noise{};                     // per-environment noise (ga3c_ddpg_envnoise_create): x, n in a block of their own at
                                        // noise.x; noise.x = null: none, the handle's shared process serves the predictions
  ~DActors() {
    (void)hipFree(noise.x);
    (void)hipGetLastError();
  }
};

// Twin critics of a handle (ga3c_ddpg_twin_create).  The arenas hold view.off[NVARS] floats while it lives.
struct Twin {
  int delay = 1;                        // a policy step when (step + 1) % delay == 0
  float sigma = 0.f, clip = 0.f;        // the target smoothing
  uint64_t seed = 0;                    // its draw at step + 1 = t is stream t of this seed
  Layout view{};                        // twin_view(L), set with the handle's table (set_table)
  float* work_base = nullptr;           // the twin-only rows of the handle's Work
};

// n-step returns of a handle (ga3c_ddpg_nstep_create).  The environments' windows are the actors'.
struct NStep {
  int n = 1;
  float* disc = nullptr;                // [capacity] the discount of the row in a slot: gamma^m, gamma for a row added by hand
  float* used = nullptr;                // [max_batch] the discounts the last step's target took
};

// A distributional critic of a handle (ga3c_ddpg_dist_create).  The handle's Layout has z.n columns in the critic's head.
struct Dist {
  Support z{1, 0.f, 0.f, 0.f};
  float* work_base = nullptr;           // the rows of the handle's DistRows
};

// PopArt of a handle (ga3c_ddpg_popart_create).  The arenas hold two floats behind the 26 variables while it lives: mu, nu.
struct Pop {
  float beta = 0.f, smin = 0.f, smax = 0.f;
  int64_t stat = 0;                     // where mu lies in every arena, nu behind it
  float* work_base = nullptr;           // the row "yn" of the handle's work table
};

// The soft actor-critic of a handle (ga3c_ddpg_soft_create).  The handle's Layout has 2 A columns in the actor's head and the
// arenas hold log_alpha behind the twin's 38 variables while it lives.
struct Soft {
  SoftCfg cfg{};                        // ls_min, ls_max, log_alpha's place, the seed
  float alpha_lr = 0.f, target_entropy = 0.f;
  std::atomic<int64_t> predictions{0};  // GA3C_DDPG_NOISE_OWN predictions served: the c of the next one's draws
  float* work_base = nullptr;           // the rows of the handle's SoftRows and its "do" [B, 2A]
  float* core_dout = nullptr;           // the handle's own "do" [B, A], back in place at destroy
  float* act_eps = nullptr;             // [max_batch, A] the device actors' last draws
};

// Evaluation episodes of a handle (ga3c_ddpg_eval_create).  block: the device buffers below; h_counts: the n f64 totals of the
// last run, pinned.  Read and written under train_mu.
struct Eval : ga3c_actors::ActorsCore {
  int n = 0;
  bool trace = false;
  double* start = nullptr;              // [n][2] where every run begins
  double* phys = nullptr;               // [n][2] where the last run ended
  double* total = nullptr;              // [n] its reward sums
  EvalTrace tr{};                       // null without a trace
  bool timed = false;                   // t0 / t1 hold the last run's kernel
  double* h_total() const { return reinterpret_cast<double*>(h_counts); }
};

struct ga3c_ddpg : vn::Core {     // arenas: value, target, slot a, slot b, gradient; a lane's one output is a[A]
  ga3c_ddpg_config cfg;
  Options opt;                    // what fixes the variables: vars, tnames, n, L and the twin's view are make_table(opt)'s
  Layout L;
  int rowf = 0;
  std::mutex add_mu;              // one replay_add at a time (its own staging); mu also orders the ring's bookkeeping
  std::mutex noise_mu;
  Work w{};
  float* work_base = nullptr;
  float* ring = nullptr;
  int64_t ring_total = 0;         // rows ever added; row t lies in slot t mod capacity
  float* h_stage = nullptr; float* d_stage = nullptr;     // train(): B rows in ring layout
  int32_t* h_idx = nullptr; int32_t* d_idx = nullptr;
  float* h_q = nullptr;
  float* h_add = nullptr;                                  // replay_add: rows in ring layout
  int64_t* h_aoff = nullptr; int64_t* d_aoff = nullptr; float* h_ar = nullptr; float* d_ar = nullptr;
  float* h_aa = nullptr; float* d_aa = nullptr;
  hipEvent_t aev = nullptr;
  NormalGen gen;
  std::vector<float> ou_x;
  Per* per = nullptr;             // null: no priorities, and every path is the one it was without them
  DActors* actors = nullptr;      // null: no device actors
  Twin* twin = nullptr;           // null: one critic
  NStep* nstep = nullptr;         // null: one-step rows, the scalar gamma everywhere
  Dist* dist = nullptr;           // null: the scalar critic
  Eval* eval = nullptr;           // null: no evaluation episodes
  Pop* pop = nullptr;             // null: the critic's output is the return itself
  float* yn = nullptr;            // [B] its normalised targets, null without
  bool has_task = false;          // ga3c_ddpg_task_create has been called: what the task's ABI answers by, and selects no kernel
  PendulumTask task = PendulumTask::fork();      // by value to the actors' and the evaluator's kernels; the fork's until created
  DistRows dw{};                  // the distributional critic's rows, null without
  Soft* soft = nullptr;           // null: the deterministic actor
  SoftRows sw{};                  // its rows, null without
  std::vector<std::string> tnames;      // the target copies' names, by variable
};

namespace {

int tiles(int B) { return (B + TILE - 1) / TILE; }

// The rows of the train workspace by the name ga3c_ddpg_fetch knows them under.  tag: W_TWIN rows exist while the handle has twin
// critics, W_DIST rows while it has a distributional critic, W_POP rows while it has PopArt, each kind in a block of its own
// (Twin::work_base, Dist::work_base, Pop::work_base), W_SOFT rows while it has the soft actor-critic (Soft::work_base), where
// "do" is one of them, [B, 2A];
// the others live as long as the handle (work_base).
enum WorkTag { W_CORE, W_TWIN, W_DIST, W_POP, W_SOFT };
struct WorkRow {
  const char* name;
  float** ptr;
  size_t width;
  WorkTag tag;
};

std::vector<WorkRow> work_table(ga3c_ddpg* m) {
  const size_t S = m->L.S, A = m->L.A;
  Work& w = m->w;
  CriticRows &c = w.c[0], &d = w.c[1];
  DistRows& z = m->dw;
  const size_t N = m->dist ? (size_t)m->dist->z.n : 0;
  SoftRows& sr = m->sw;
  const WorkRow dout = m->soft ? WorkRow{"do", &w.dout, 2 * A, W_SOFT} : WorkRow{"do", &w.dout, A, W_CORE};
  return {{"y", &w.y, 1, W_CORE},           {"qt", &w.qt, 1, W_CORE},         {"q", &c.q, 1, W_CORE},           {"dq", &c.dq, 1, W_CORE},
          {"c_x", &w.c_x, S, W_CORE},       {"c_a", &w.c_a, A, W_CORE},       {"c_xh1", &c.xh1, H1, W_CORE},    {"c_c1", &c.c1, H1, W_CORE},
          {"c_dn1", &c.dn1, H1, W_CORE},    {"c_dh1", &c.dh1, H1, W_CORE},    {"c_c2", &c.c2, H2, W_CORE},      {"c_dt", &c.dt, H2, W_CORE},
          {"a_xh1", &w.a_xh1, H1, W_CORE},  {"a_a1", &w.a_a1, H1, W_CORE},    {"a_dn1", &w.a_dn1, H1, W_CORE},  {"a_dh1", &w.a_dh1, H1, W_CORE},
          {"a_xh2", &w.a_xh2, H2, W_CORE},  {"a_a2", &w.a_a2, H2, W_CORE},    {"a_dn2", &w.a_dn2, H2, W_CORE},  {"a_dh2", &w.a_dh2, H2, W_CORE},
          {"a_out", &w.a_out, A, W_CORE},   {"a_noisy", &w.a_noisy, A, W_CORE}, {"g", &w.g, A, W_CORE},         dout,
          {"qt1", &w.qt1, 1, W_TWIN},        {"qt2", &w.qt2, 1, W_TWIN},        {"q2", &d.q, 1, W_TWIN},           {"dq2", &d.dq, 1, W_TWIN},
          {"t_eps", &w.t_eps, A, W_TWIN},    {"t_a", &w.t_a, A, W_TWIN},        {"c2_xh1", &d.xh1, H1, W_TWIN},    {"c2_c1", &d.c1, H1, W_TWIN},
          {"c2_dn1", &d.dn1, H1, W_TWIN},    {"c2_dh1", &d.dh1, H1, W_TWIN},    {"c2_c2", &d.c2, H2, W_TWIN},      {"c2_dt", &d.dt, H2, W_TWIN},
          {"d_pt", &z.pt, N, W_DIST},      {"d_m", &z.m, N, W_DIST},        {"d_p", &z.p, N, W_DIST},        {"d_dz", &z.dz, N, W_DIST},
          {"d_ce", &z.ce, 1, W_DIST},      {"yn", &m->yn, 1, W_POP},
          {"s_eps2", &sr.eps2, A, W_SOFT}, {"s_a2", &sr.a2, A, W_SOFT},     {"s_logp2", &sr.logp2, 1, W_SOFT}, {"s_vt", &sr.vt, 1, W_SOFT},
          {"s_mu", &sr.mu, A, W_SOFT},     {"s_ls", &sr.ls, A, W_SOFT},     {"s_eps", &sr.eps, A, W_SOFT},   {"s_u", &sr.u, A, W_SOFT},
          {"s_logp", &sr.logp, 1, W_SOFT}, {"s_q1", &sr.q1, 1, W_SOFT},     {"s_q2", &sr.q2, 1, W_SOFT}};
}

// One zeroed block for the table's rows of one tag; *end: the four floats behind them.
int carve_work(ga3c_ddpg* m, WorkTag tag, float** base, float** end) {
  std::vector<float**> ptrs;
  std::vector<size_t> widths;
  for (const WorkRow& r : work_table(m))
    if (r.tag == tag) {
      ptrs.push_back(r.ptr);
      widths.push_back(r.width);
    }
  return vn::carve_rows((size_t)m->cfg.max_batch, widths, ptrs, base, end);
}

// The actor's entries and critic c's.
GradSrc grad_src(ga3c_ddpg* m, int c) {
  GradSrc g;
  const Work& w = m->w;
  const CriticRows& cr = w.c[c];
  const int S = m->L.S, A = m->L.A;
  for (int v = 0; v < NTRAIN; ++v) {
    g.in[v] = g.d[v] = g.mul[v] = nullptr;
    g.ld_in[v] = g.ld_d[v] = 0;
  }
  auto set = [&](int v, const float* in, int li, const float* d, int ld, const float* mul) {
    g.in[v] = in; g.ld_in[v] = li; g.d[v] = d; g.ld_d[v] = ld; g.mul[v] = mul;
  };
  set(A_W1, w.c_x, S, w.a_dh1, H1, nullptr);       // the actor step reads the same states the critic step stored
  set(A_B1, nullptr, 0, w.a_dh1, H1, nullptr);
  set(A_BE1, nullptr, 0, w.a_dn1, H1, nullptr);
  set(A_GA1, nullptr, 0, w.a_dn1, H1, w.a_xh1);
  set(A_W2, w.a_a1, H1, w.a_dh2, H2, nullptr);
  set(A_B2, nullptr, 0, w.a_dh2, H2, nullptr);
  set(A_BE2, nullptr, 0, w.a_dn2, H2, nullptr);
  set(A_GA2, nullptr, 0, w.a_dn2, H2, w.a_xh2);
  set(A_WO, w.a_a2, H2, w.dout, m->L.cols[A_WO], nullptr);      // (2 A on a soft handle)
  set(A_BO, nullptr, 0, w.dout, m->L.cols[A_WO], nullptr);
  set(C_W1, w.c_x, S, cr.dh1, H1, nullptr);
  set(C_B1, nullptr, 0, cr.dh1, H1, nullptr);
  set(C_BE1, nullptr, 0, cr.dn1, H1, nullptr);
  set(C_GA1, nullptr, 0, cr.dn1, H1, cr.xh1);
  set(C_W2, cr.c1, H1, cr.dt, H2, nullptr);
  set(C_WN, w.c_a, A, cr.dt, H2, nullptr);
  set(C_BN, nullptr, 0, cr.dt, H2, nullptr);
  set(C_WO, cr.c2, H2, cr.dq, 1, nullptr);
  set(C_BO, nullptr, 0, cr.dq, 1, nullptr);
  if (m->dist) {                                   // the head's delta is dz [B,n] (no twin then: c = 0)
    set(C_WO, cr.c2, H2, m->dw.dz, m->dist->z.n, nullptr);
    set(C_BO, nullptr, 0, m->dw.dz, m->dist->z.n, nullptr);
  }
  return g;
}

Opt make_opt(ga3c_ddpg* m, bool actor, float lr, int64_t t, bool apply, bool soft) {
  Opt o;
  o.theta = m->arena[0]; o.target = m->arena[1]; o.sa = m->arena[2]; o.sb = m->arena[3]; o.grad = m->arena[4];
  const ga3c_ddpg_config& c = m->cfg;
  o.adam = actor || (c.flags & GA3C_DDPG_CRITIC_ADAM) ? 1 : 0;
  const double rate = (double)(actor ? c.actor_lr : c.critic_lr) * (double)lr;
  if (o.adam) o.lr = (float)(rate * std::sqrt(1.0 - std::pow(ADAM_B2, (double)t)) / (1.0 - std::pow(ADAM_B1, (double)t)));
  else o.lr = (float)rate;
  o.omr = 1.0f - c.rmsprop_decay;
  o.mu = c.rmsprop_momentum;
  o.eps = c.rmsprop_epsilon;
  o.clip = c.grad_clip_norm;
  o.tau = c.tau;
  o.apply = apply ? 1 : 0;
  o.soft = soft ? 1 : 0;
  return o;
}

// The noise a predict / step 4 adds: the handle's own OU step, the caller's vector, or none.
int make_noise(ga3c_ddpg* m, int mode, const float* given, Noise* nz) {
  const int A = m->L.A;
  memset(nz, 0, sizeof *nz);
  if (mode == GA3C_DDPG_NOISE_GIVEN) {
    if (!given) return fail(GA3C_EINVAL, "GA3C_DDPG_NOISE_GIVEN without a noise vector");
    memcpy(nz->v, given, sizeof(float) * A);
  } else if (mode == GA3C_DDPG_NOISE_OWN) {
    if (m->cfg.flags & GA3C_DDPG_OU_NOISE) CHK(ga3c_ddpg_noise_step(m, nz->v, nullptr));
    else nz->wrap = 1;
  } else if (mode == GA3C_DDPG_NOISE_NONE) {
    nz->wrap = 1;
  } else {
    return fail(GA3C_EINVAL, "noise_mode %d not in [0,2]", mode);
  }
  return GA3C_OK;
}

// The discounts by slot for a step on `rows`: only ring rows have a slot; train, compute and the staged rows keep the scalar.
const float* row_discounts(const ga3c_ddpg* m, const Rows& rows) {
  return m->nstep && rows.base == m->ring ? m->nstep->disc : nullptr;
}

// Steps 1 .. stop_after of train_DDPG on `rows` for a handle with NC critics (caller holds train_mu and mu).  stop_after 6: the
// whole step.  Twin critics: smoothed targets from the smaller of two target critics, both critics stepped on
// them in the paired form, and only when t is a multiple of the delay the actor's step, at its own Adam count, and the soft
// update of all three nets.  One critic is that rule at delay 1, with the loss form the handle's flag names.  The soft
// actor-critic is the twin's rule with the soft target kernel in the target kernel's place and, on a policy step,
// the soft actor kernel and the actor's weight-gradient launch that carries the temperature's step; its draws at step t are
// streams 2 t (target) and 2 t + 1 (policy) of the soft seed, and no noise argument is read.
template <int NC>
int enqueue_step_nc(ga3c_ddpg* m, const Rows& rows, int B, float lr, const Noise& nz, int stop_after, const float* per_w) {
  const ga3c_ddpg_config& c = m->cfg;
  const Work& w = m->w;
  const int64_t t = m->step.load() + 1;
  const int delay = NC == 2 ? m->twin->delay : 1;
  const bool policy = t % delay == 0, full = stop_after >= 6, clip = (c.flags & GA3C_DDPG_GRAD_CLIP) != 0;
  const int paired = NC == 2 || (c.flags & GA3C_DDPG_LOSS_PAIRED) ? 1 : 0;
  PerCritic<Layout, NC> L;
  PerCritic<GradSrc, NC> gs;
  Target<NC> tg;
  L.v[0] = m->L;
  gs.v[0] = grad_src(m, 0);
  tg.y = w.y;
  tg.qt = w.qt;
  if constexpr (NC == 2) {
    const Twin& tw = *m->twin;
    L.v[1] = tw.view;
    gs.v[1] = grad_src(m, 1);
    tg.qt1 = w.qt1; tg.qt2 = w.qt2; tg.t_eps = w.t_eps; tg.t_a = w.t_a;
    tg.sigma = tw.sigma; tg.clip = tw.clip; tg.seed = tw.seed; tg.number = (uint64_t)t;
  }
  const dim3 grid(tiles(B)), gridc(tiles(B), NC), block(THREADS);
  const Dist* ds = NC == 1 ? m->dist : nullptr;    // a distributional critic: its three kernels in the scalar ones' places
  const Soft* so = NC == 2 ? m->soft : nullptr;
  const int future = (c.flags & GA3C_DDPG_FUTURE_REWARD) ? 1 : 0;
  float* used = m->nstep ? m->nstep->used : nullptr;
  if (ds) {
    hipLaunchKernelGGL(ddpg_dist_target_kernel, grid, block, 0, m->st, m->L, (const float*)m->arena[1], rows, B, c.gamma, future,
                       ds->z, w.y, w.qt, m->dw, row_discounts(m, rows), used);
    hipLaunchKernelGGL(ddpg_dist_critic_kernel, grid, block, 0, m->st, m->L, (const float*)m->arena[0], rows, B, per_w, ds->z, w,
                       m->dw);
  } else {
    // PopArt: the targets are de-normalised with the statistics as they stand, the one-workgroup kernel moves
    // them, rescales both output layers and leaves yn, and the critic step runs on yn where y was
    const Pop* pp = NC == 1 ? m->pop : nullptr;
    float* stat = pp ? m->arena[0] + pp->stat : nullptr;
    if (so) {
      if constexpr (NC == 2)
        hipLaunchKernelGGL(ddpg_soft_target_kernel, grid, block, 0, m->st, L, (const float*)m->arena[0], (const float*)m->arena[1],
                           rows, B, c.gamma, future, so->cfg, SoftTarget{w.y, w.qt, w.qt1, w.qt2, (uint64_t)(2 * t)}, m->sw,
                           row_discounts(m, rows), used);
    } else {
      hipLaunchKernelGGL(ddpg_target_kernel<NC>, grid, block, 0, m->st, L, (const float*)m->arena[1], rows, B, c.gamma, future, tg,
                         row_discounts(m, rows), used, PopStats{stat, pp ? (double)pp->smin : 0.0, pp ? (double)pp->smax : 0.0});
    }
    Work wc = w;
    if (pp) {
      float *a0 = m->arena[0], *a1 = m->arena[1];
      const Layout& K = m->L;
      hipLaunchKernelGGL(ddpg_popart_kernel, dim3(1), block, 0, m->st,
                         PopArt{stat, a1 + pp->stat, a0 + K.off[C_WO], a0 + K.off[C_BO], a1 + K.off[C_WO], a1 + K.off[C_BO],
                                (const float*)w.y, m->yn, w.qstat + 2, (double)pp->beta, (double)pp->smin, (double)pp->smax},
                         B);
      wc.y = m->yn;
    }
    hipLaunchKernelGGL(ddpg_critic_kernel<NC>, gridc, block, 0, m->st, L, (const float*)m->arena[0], rows, B, paired, per_w, wc);
  }
  const int cblocks = (int)((m->L.off[NTRAIN] - m->L.off[NACTOR] + THREADS - 1) / THREADS);
  const int ablocks = (int)((m->L.off[NACTOR] + THREADS - 1) / THREADS);
  const Opt oc = make_opt(m, false, lr, t, true, full && policy);
  if (clip) {
    hipLaunchKernelGGL((ddpg_wgrad_kernel<NC, false>), dim3(cblocks, NC), block, 0, m->st, L, gs, NACTOR, NTRAIN, B, oc, w);
    hipLaunchKernelGGL(ddpg_update_kernel<NC>, dim3(NC * NCRITIC), block, 0, m->st, L, oc);
  } else {
    hipLaunchKernelGGL((ddpg_wgrad_kernel<NC, true>), dim3(cblocks, NC), block, 0, m->st, L, gs, NACTOR, NTRAIN, B, oc, w);
  }
  if (stop_after >= 4 && policy) {
    const Opt oa = make_opt(m, true, lr, t / delay, full, full);
    if (so) {
      if constexpr (NC == 2) {
        hipLaunchKernelGGL(ddpg_soft_actor_kernel, grid, block, 0, m->st, L, (const float*)m->arena[0], rows, B, so->cfg,
                           (uint64_t)(2 * t + 1), w, m->sw);
        // the temperature's Adam: the actor's bias correction on alpha_lr x the rate (oa.lr is that correction on actor_lr x the rate)
        const double tt = (double)(t / delay);
        const float lra = (float)((double)so->alpha_lr * (double)lr * std::sqrt(1.0 - std::pow(ADAM_B2, tt)) / (1.0 - std::pow(ADAM_B1, tt)));
        hipLaunchKernelGGL(ddpg_soft_wgrad_kernel, dim3(ablocks), block, 0, m->st, m->L, gs.v[0], B, oa,
                           SoftAlpha{(const float*)m->sw.logp, m->sw.stat, so->cfg.la, so->target_entropy, lra});
      }
    } else {
      if (ds) hipLaunchKernelGGL(ddpg_dist_actor_kernel, grid, block, 0, m->st, m->L, (const float*)m->arena[0], rows, B, nz, w, ds->z);
      else hipLaunchKernelGGL(ddpg_actor_kernel, grid, block, 0, m->st, m->L, (const float*)m->arena[0], rows, B, nz, w);
      hipLaunchKernelGGL((ddpg_wgrad_kernel<1, true>), dim3(ablocks), block, 0, m->st, PerCritic<Layout, 1>{{m->L}},
                         PerCritic<GradSrc, 1>{{gs.v[0]}}, 0, NACTOR, B, oa, w);
    }
  }
  HIPCHK(hipGetLastError());
  return GA3C_OK;
}

int enqueue_step(ga3c_ddpg* m, const Rows& rows, int B, float lr, const Noise& nz, int stop_after, const float* per_w = nullptr) {
  return m->twin ? enqueue_step_nc<2>(m, rows, B, lr, nz, stop_after, per_w) : enqueue_step_nc<1>(m, rows, B, lr, nz, stop_after, per_w);
}

// {max q, mean q} of the last step enqueued, on their way to the host; with PopArt {mu', sigma'} come behind them in the same copy.
int copy_qstats(ga3c_ddpg* m) {
  HIPCHK(hipMemcpyAsync(m->h_q, m->w.qstat, (m->pop ? 4 : 2) * sizeof(float), hipMemcpyDeviceToHost, m->st));
  return GA3C_OK;
}

int finish_step(ga3c_ddpg* m) {
  CHK(copy_qstats(m));
  HIPCHK(hipEventRecord(m->tev, m->st));
  return GA3C_OK;
}

// ... and, after the wait, to the caller (caller holds train_mu).  With PopArt the critic's output is normalised and the stats
// go out in return units: sigma' max(n) + mu' and sigma' mean(n) + mu'.
void give_qstats(const ga3c_ddpg* m, float* q_stats) {
  if (!q_stats) return;
  memcpy(q_stats, m->h_q, 2 * sizeof(float));
  if (m->pop)
    for (int i = 0; i < 2; ++i) q_stats[i] = fmaf(m->h_q[3], m->h_q[i], m->h_q[2]);
}

// n rows in ring layout, s | a | r | done | s2, into `dst` (the one place)
void pack_rows(const ga3c_ddpg* m, float* dst, const float* s, const float* a, const float* r, const float* done, const float* s2,
               int n) {
  const int S = m->L.S, A = m->L.A, rowf = m->rowf;
  for (int i = 0; i < n; ++i) {
    float* row = dst + (size_t)i * rowf;
    memcpy(row, s + (size_t)i * S, sizeof(float) * S);
    memcpy(row + S, a + (size_t)i * A, sizeof(float) * A);
    row[S + A] = r[i];
    row[S + A + 1] = done[i] != 0.f ? 1.f : 0.f;
    memcpy(row + S + A + 2, s2 + (size_t)i * S, sizeof(float) * S);
  }
}

// train / compute on host rows: staged in ring layout, then the same kernels as train_replay.  stop_after is 6 from train and
// what ga3c_ddpg_compute checked from there.
int step_host(ga3c_ddpg* m, const float* s, const float* a, const float* r, const float* done, const float* s2, int B, float lr,
              int mode, const float* noise, int stop_after, float* q_stats) {
  if (!m || !s || !a || !r || !done || !s2) return fail(GA3C_EINVAL, "null argument");
  CHK(vn::check_batch(m, B));
  HIPCHK(hipSetDevice(m->device));
  std::lock_guard<std::mutex> tl(m->train_mu);
  Noise nz;
  CHK(make_noise(m, mode, noise, &nz));
  pack_rows(m, m->h_stage, s, a, r, done, s2, B);
  {
    std::lock_guard<std::mutex> lk(m->mu);
    HIPCHK(hipMemcpyAsync(m->d_stage, m->h_stage, sizeof(float) * B * m->rowf, hipMemcpyHostToDevice, m->st));
    CHK(enqueue_step(m, Rows{m->d_stage, nullptr, m->rowf}, B, lr, nz, stop_after));
    CHK(finish_step(m));
    m->last_B = B;
  }
  HIPCHK(hipEventSynchronize(m->tev));
  give_qstats(m, q_stats);
  if (stop_after >= 6) m->step.fetch_add(1);
  return GA3C_OK;
}

// The launch arguments of a soft handle's prediction in `mode`: the caller's eps for GA3C_DDPG_NOISE_GIVEN, and for
// GA3C_DDPG_NOISE_OWN the handle's prediction count, which this call advances by one.
int soft_predict_args(ga3c_ddpg* m, int mode, const float* given, Noise* nz, uint64_t* count) {
  memset(nz, 0, sizeof *nz);
  *count = 0;
  if (mode == GA3C_DDPG_NOISE_GIVEN) {
    if (!given) return fail(GA3C_EINVAL, "GA3C_DDPG_NOISE_GIVEN without a noise vector");
    memcpy(nz->v, given, sizeof(float) * m->L.A);
  } else if (mode == GA3C_DDPG_NOISE_OWN) {
    *count = (uint64_t)m->soft->predictions.fetch_add(1);
  } else if (mode != GA3C_DDPG_NOISE_NONE) {
    return fail(GA3C_EINVAL, "noise_mode %d not in [0,2]", mode);
  }
  return GA3C_OK;
}

void launch_soft_predict(ga3c_ddpg* m, const Input& in, int B, int mode, const Noise& nz, uint64_t count, float* a_out, float* eps_out) {
  hipLaunchKernelGGL(ddpg_soft_predict_kernel, dim3(tiles(B)), dim3(THREADS), 0, m->st, m->L, (const float*)m->arena[0], in, B,
                     m->soft->cfg, mode, nz, m->soft->cfg.seed + 1, count, a_out, eps_out);
}

int predict_begin(ga3c_ddpg* m, const float* x, const int64_t* off, int B, int mode, const float* noise, int* ticket) {
  CHK(vn::predict_check(m, off, B));
  Noise nz;
  if (m->soft) {
    uint64_t count;
    CHK(soft_predict_args(m, mode, noise, &nz, &count));
    return vn::predict_begin(m, x, off, B, ticket, [&](const Input& in, vn::PLane& P) {
      launch_soft_predict(m, in, B, mode, nz, count, P.out[0].d, nullptr);
    });
  }
  CHK(make_noise(m, mode, noise, &nz));        // before a lane is taken: one step of the process per call, whatever the batch
  return vn::predict_begin(m, x, off, B, ticket, [&](const Input& in, vn::PLane& P) {
    hipLaunchKernelGGL(ddpg_predict_kernel, dim3(tiles(B)), dim3(THREADS), 0, m->st, m->L, (const float*)m->arena[0], in, B, nz,
                       P.out[0].d);
  });
}

// v, which only the gather entries ask for, is the first action column.
int predict_end(ga3c_ddpg* m, int ticket, int B, float* a, float* v) {
  vn::PLane* P;
  CHK(vn::predict_end(m, ticket, B, &P));
  const int A = m->L.A;
  const float* h_a = P->out[0].h;
  if (a) memcpy(a, h_a, sizeof(float) * B * A);
  if (v)
    for (int i = 0; i < B; ++i) v[i] = h_a[(size_t)i * A];
  vn::give_lane(m, P);
  return GA3C_OK;
}

// The handle's variables become those of `opt` (ga3c_ddpg_vars.hpp's table, the one statement of them); the arenas are the
// caller's business.  Caller holds train_mu and mu, or owns the handle alone.
void set_table(ga3c_ddpg* m, const Options& opt) {
  Table t = make_table(opt);
  m->opt = opt;
  m->L = t.L;
  if (m->twin) m->twin->view = t.view;
  m->vars = std::move(t.vars);
  m->tnames = std::move(t.tnames);
  m->n = t.n;
}

// where the variable called `name` lies in every arena (a name of the table)
int64_t var_offset(const ga3c_ddpg* m, const char* name) { return m->vars[(size_t)ga3c_ckpt::find_var(m->vars, name)].off; }

// The five arenas re-laid for the variables of `to` (relay, on the host: a variable keeps its value, target copy, slots and
// gradient where the handle has one of that name and shape, and starts as ga3c_ddpg_create would leave it otherwise), then the
// handle's table set to it.  The old arenas are freed only after the last new one is allocated and written: on any failure the
// handle is as it was.  Caller holds train_mu and mu.
int relay_arenas(ga3c_ddpg* m, const Options& to, float log_alpha = 0.f) {
  const Table from = make_table(m->opt), next = make_table(to);
  float* laid[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  auto build = [&]() -> int {
    HIPCHK(hipStreamSynchronize(m->st));           // a prediction in flight has finished before its arena is freed
    std::vector<float> old((size_t)from.n);
    for (int a = 0; a < m->narena; ++a) {
      HIPCHK(hipMemcpy(old.data(), m->arena[a], sizeof(float) * from.n, hipMemcpyDeviceToHost));
      const std::vector<float> image = relay(from, old, next, a, log_alpha);
      CHK(vn::dalloc(&laid[a], (size_t)next.n));
      HIPCHK(hipMemcpy(laid[a], image.data(), sizeof(float) * next.n, hipMemcpyHostToDevice));
    }
    return GA3C_OK;
  };
  const int rc = build();
  if (rc != GA3C_OK) {
    for (float* g : laid) (void)hipFree(g);
    (void)hipGetLastError();
    return rc;
  }
  for (int a = 0; a < m->narena; ++a) {
    (void)hipFree(m->arena[a]);
    m->arena[a] = laid[a];
  }
  set_table(m, to);
  return GA3C_OK;
}

// The block of an option's work rows freed, and every row of that tag null again.
void free_work(ga3c_ddpg* m, WorkTag tag, float* base) {
  (void)hipFree(base);
  (void)hipGetLastError();
  for (const WorkRow& r : work_table(m))
    if (r.tag == tag) *r.ptr = nullptr;
}

// The state, its rows and its variables' names; the arenas keep their size, and nothing names what lies behind the table's end.
void pop_free(ga3c_ddpg* m) {
  Pop* p = m->pop;
  if (!p) return;
  free_work(m, W_POP, p->work_base);
  delete p;
  m->pop = nullptr;
  Options opt = m->opt;
  opt.pop = false;
  set_table(m, opt);
}

void twin_free(ga3c_ddpg* m) {
  Twin* t = m->twin;
  if (!t) return;
  free_work(m, W_TWIN, t->work_base);
  delete t;
  m->twin = nullptr;
  Options opt = m->opt;
  opt.twin = false;
  set_table(m, opt);
}

void per_free(ga3c_ddpg* m) {
  Per* p = m->per;
  if (!p) return;
  (void)hipFree(p->pa); (void)hipFree(p->max_pa); (void)hipFree(p->csum); (void)hipFree(p->slots); (void)hipFree(p->w);
  (void)hipFree(p->td); (void)hipHostFree(p->h_slots); (void)hipHostFree(p->h_w);
  (void)hipGetLastError();
  delete p;
  m->per = nullptr;
}

void nstep_free(ga3c_ddpg* m) {
  NStep* ns = m->nstep;
  if (!ns) return;
  (void)hipFree(ns->disc); (void)hipFree(ns->used);
  (void)hipGetLastError();
  delete ns;
  m->nstep = nullptr;
}

// The state and its rows; the arenas stay as they are laid (dist_destroy re-lays them first, ga3c_ddpg_destroy frees them).
void dist_free(ga3c_ddpg* m) {
  Dist* d = m->dist;
  if (!d) return;
  free_work(m, W_DIST, d->work_base);
  delete d;
  m->dist = nullptr;
}

// The state and its rows; the arenas stay as they are laid (soft_destroy re-lays them first, ga3c_ddpg_destroy frees them).
void soft_free(ga3c_ddpg* m) {
  Soft* s = m->soft;
  if (!s) return;
  (void)hipFree(s->act_eps);
  free_work(m, W_SOFT, s->work_base);              // "do" among them: the handle's own is back in place below
  m->sw.stat = nullptr;                            // (the floats behind the rows)
  if (s->core_dout) m->w.dout = s->core_dout;
  delete s;
  m->soft = nullptr;
}

void dactors_free(ga3c_ddpg* m) {
  ga3c_actors::actors_free(m->actors);
  m->actors = nullptr;
}

void eval_free(ga3c_ddpg* m) {
  ga3c_actors::actors_free(m->eval);
  m->eval = nullptr;
}

void free_all(ga3c_ddpg* m) {
  if (m->actors && m->st) {       // live actors: what they enqueued may still run
    (void)hipStreamSynchronize(m->st);
    (void)hipGetLastError();
  }
  dactors_free(m);
  eval_free(m);
  per_free(m);
  soft_free(m);
  twin_free(m);
  pop_free(m);
  nstep_free(m);
  dist_free(m);
  vn::free_core(m);
  (void)hipFree(m->work_base);
  (void)hipFree(m->ring);
  (void)hipHostFree(m->h_stage); (void)hipFree(m->d_stage); (void)hipHostFree(m->h_idx); (void)hipFree(m->d_idx);
  (void)hipHostFree(m->h_q); (void)hipHostFree(m->h_add);
  (void)hipHostFree(m->h_aoff); (void)hipFree(m->d_aoff); (void)hipHostFree(m->h_ar); (void)hipFree(m->d_ar);
  (void)hipHostFree(m->h_aa); (void)hipFree(m->d_aa);
  if (m->aev) (void)hipEventDestroy(m->aev);
  (void)hipGetLastError();
}

int alloc_all(ga3c_ddpg* m) {
  const ga3c_ddpg_config& c = m->cfg;
  const size_t B = (size_t)c.max_batch, A = c.num_actions, rowf = (size_t)m->rowf;
  CHK(vn::alloc_core(m, c.predict_lanes));
  // every variable at its initial value (initial_value: moving_variance = 1 in both copies, the RMSProp ms slot of the critic 1);
  // alloc_core left the slot b and gradient arenas zero, which is theirs
  const Table table = make_table(m->opt);
  for (int a = 0; a <= 2; ++a)
    HIPCHK(hipMemcpy(m->arena[a], relay(Table{}, {}, table, a, 0.f).data(), sizeof(float) * m->n, hipMemcpyHostToDevice));
  CHK(carve_work(m, W_CORE, &m->work_base, &m->w.qstat));
  CHK(vn::dalloc(&m->ring, (size_t)c.replay_capacity * rowf));
  HIPCHK(hipMemset(m->ring, 0, sizeof(float) * (size_t)c.replay_capacity * rowf));
  CHK(vn::halloc(&m->h_stage, B * rowf)); CHK(vn::dalloc(&m->d_stage, B * rowf));
  CHK(vn::halloc(&m->h_idx, B)); CHK(vn::dalloc(&m->d_idx, B));
  CHK(vn::halloc(&m->h_q, 4));
  CHK(vn::halloc(&m->h_add, B * rowf));
  CHK(vn::halloc(&m->h_aoff, B)); CHK(vn::dalloc(&m->d_aoff, B)); CHK(vn::halloc(&m->h_ar, B)); CHK(vn::dalloc(&m->d_ar, B));
  CHK(vn::halloc(&m->h_aa, B * A)); CHK(vn::dalloc(&m->d_aa, B * A));
  HIPCHK(hipEventCreateWithFlags(&m->aev, hipEventDisableTiming));
  return GA3C_OK;
}

int64_t ring_size(const ga3c_ddpg* m) { return std::min<int64_t>(m->ring_total, m->cfg.replay_capacity); }

// the row count of a replay_add / replay_add_gather
int check_add_rows(const ga3c_ddpg* m, int n) {
  if (n < 1 || n > m->cfg.max_batch || n > m->cfg.replay_capacity)
    return fail(GA3C_EINVAL, "%d rows outside [1, min(max_batch %d, replay_capacity %d)]", n, m->cfg.max_batch, m->cfg.replay_capacity);
  return GA3C_OK;
}

// n rows into the ring at its write position, from `src` (device or pinned host) in ring layout; caller holds mu.
int ring_copy_in(ga3c_ddpg* m, const float* src, int n, hipMemcpyKind kind) {
  const int64_t cap = m->cfg.replay_capacity, first = m->ring_total % cap;
  const int64_t n1 = std::min<int64_t>(n, cap - first);
  const size_t rowb = sizeof(float) * (size_t)m->rowf;
  HIPCHK(hipMemcpyAsync(m->ring + first * m->rowf, src, rowb * n1, kind, m->st));
  if (n1 < n) HIPCHK(hipMemcpyAsync(m->ring, src + n1 * m->rowf, rowb * (n - n1), kind, m->st));
  return GA3C_OK;
}

// The n rows just written from slot `first` on get max_pa (caller holds mu; right after the ring write, on its stream).
void per_fill(ga3c_ddpg* m, int64_t first, int64_t n) {
  if (!m->per || n < 1) return;
  hipLaunchKernelGGL(per_fill_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, m->st, m->per->pa,
                     (const float*)m->per->max_pa, first, (int)n, (int64_t)m->cfg.replay_capacity);
}

// ... and, on a handle with n-step returns, the discount of a one-step row: gamma.
void nstep_fill(ga3c_ddpg* m, int64_t first, int64_t n) {
  if (!m->nstep || n < 1) return;
  hipLaunchKernelGGL(nstep_fill_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, m->st, m->nstep->disc, m->cfg.gamma, first,
                     (int)n, (int64_t)m->cfg.replay_capacity);
}

// Sample number per->samples: B slots and their weights into per->slots / per->w (caller holds mu; the ring holds a row).
void per_enqueue_sample(ga3c_ddpg* m, int B, float beta) {
  Per* p = m->per;
  const int size = (int)ring_size(m);
  hipLaunchKernelGGL(per_chunk_sum_kernel, dim3((size + PER_CHUNK - 1) / PER_CHUNK), dim3(PER_SUM_THREADS), 0, m->st,
                     (const float*)p->pa, size, p->csum);
  hipLaunchKernelGGL(per_sample_kernel, dim3(1), dim3(PER_THREADS), 0, m->st, (const float*)p->pa, (const double*)p->csum, size, B,
                     p->seed, p->samples, (double)beta, p->slots, p->w);
  ++p->samples;
  p->w_rows = B;
}

// One prioritised step: the draw, train_DDPG on its slots with its weights, the new priorities (caller holds train_mu and mu).
int per_enqueue_step(ga3c_ddpg* m, int B, float beta, float lr, const Noise& nz) {
  Per* p = m->per;
  per_enqueue_sample(m, B, beta);
  CHK(enqueue_step(m, Rows{m->ring, p->slots, m->rowf}, B, lr, nz, 6, p->w));
  // (with PopArt the critic's q is normalised and so is the target it met: |yn - n|, a TD error free of the returns' scale)
  hipLaunchKernelGGL(per_update_kernel, dim3(1), dim3(PER_THREADS), 0, m->st, (const int32_t*)p->slots, (const float*)m->w.c[0].q,
                     (const float*)(m->pop ? m->yn : m->w.y), B, p->eps, p->alpha, p->pa, p->max_pa, p->td);
  HIPCHK(hipGetLastError());
  p->td_rows = B;
  return GA3C_OK;
}

int per_check(const ga3c_ddpg* m, const char* what) {
  if (!m->per) return fail(GA3C_ESTATE, "%s: the handle has no priorities (ga3c_ddpg_priorities_create)", what);
  return GA3C_OK;
}

int per_check_beta(float beta) {
  if (!(beta >= 0.f) || std::isinf(beta)) return fail(GA3C_EINVAL, "beta_is %g: a finite exponent >= 0", beta);
  return GA3C_OK;
}

void ring_report(ga3c_ddpg* m, int64_t* size, int64_t* total) {
  if (size) *size = ring_size(m);
  if (total) *total = m->ring_total;
}

// The timed loop of ga3c_ddpg_time_*: `iters` calls of `enqueue` between the events t0 and t1 (caller holds train_mu and mu) ...
template <class F>
int timed_loop(ga3c_ddpg* m, int batch, int iters, F enqueue) {
  HIPCHK(hipEventRecord(m->t0, m->st));
  for (int i = 0; i < iters; ++i) CHK(enqueue());
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(m->t1, m->st));
  m->last_B = batch;
  return GA3C_OK;
}

// ... and, with mu released, the wait for it and the time between the two.
int timed_wait(ga3c_ddpg* m, float* elapsed_ms) {
  HIPCHK(hipEventSynchronize(m->t1));
  HIPCHK(hipEventElapsedTime(elapsed_ms, m->t0, m->t1));
  return GA3C_OK;
}

}  // namespace

extern "C" {

int ga3c_ddpg_create(const ga3c_ddpg_config* cfg, ga3c_ddpg** out) {
  if (!cfg || !out) return fail(GA3C_EINVAL, "null argument");
  *out = nullptr;
  CHK(vn::check_dims(*cfg, MAX_S, MAX_A, MAX_B));
  if (cfg->replay_capacity < 1 || cfg->replay_capacity > (1 << 26))
    return fail(GA3C_EINVAL, "replay_capacity %d outside [1,%d]", cfg->replay_capacity, 1 << 26);
  if (cfg->flags & ~(uint32_t)(GA3C_DDPG_FUTURE_REWARD | GA3C_DDPG_LOSS_PAIRED | GA3C_DDPG_GRAD_CLIP | GA3C_DDPG_CRITIC_ADAM |
                               GA3C_DDPG_OU_NOISE))
    return fail(GA3C_EINVAL, "flags 0x%x: not GA3C_DDPG_* flags", cfg->flags);
  if (!(cfg->tau >= 0.f && cfg->tau <= 1.f)) return fail(GA3C_EINVAL, "tau %g outside [0,1]", cfg->tau);
  CHK(vn::check_device(*cfg));
  ga3c_ddpg* m = new (std::nothrow) ga3c_ddpg();
  if (!m) return fail(GA3C_EINVAL, "out of host memory");
  m->cfg = *cfg;
  m->kind = "DDPG network";
  m->device = cfg->device;
  m->S = cfg->state_dim;
  m->max_batch = cfg->max_batch;
  m->out_widths = {cfg->num_actions};
  m->narena = 5;
  m->writable = {0, 1, 2, 3};
  Options opt;
  opt.S = cfg->state_dim;
  opt.A = cfg->num_actions;
  opt.critic_adam = (cfg->flags & GA3C_DDPG_CRITIC_ADAM) != 0;
  set_table(m, opt);
  m->rowf = 2 * cfg->state_dim + cfg->num_actions + 2;
  m->gen.seed((uint64_t)cfg->seed);
  m->ou_x.assign((size_t)cfg->num_actions, 0.f);
  const int rc = alloc_all(m);
  if (rc != GA3C_OK) {
    free_all(m);
    delete m;
    return rc;
  }
  *out = m;
  return GA3C_OK;
}

int ga3c_ddpg_destroy(ga3c_ddpg* m) {
  if (!m) return fail(GA3C_EINVAL, "null argument");
  (void)hipSetDevice(m->device);
  free_all(m);
  delete m;
  return GA3C_OK;
}

int32_t ga3c_ddpg_num_params(ga3c_ddpg* m) { return vn::num_params(m); }

const char* ga3c_ddpg_param_name(ga3c_ddpg* m, int32_t index) { return vn::param_name(m, index); }

const char* ga3c_ddpg_target_name(ga3c_ddpg* m, int32_t index) {
  return (m && index >= 0 && index < (int32_t)m->tnames.size()) ? m->tnames[index].c_str() : nullptr;
}

int ga3c_ddpg_param_info(ga3c_ddpg* m, const char* name, int64_t* count, int32_t* ndim, int64_t shape[4], int32_t* trainable) {
  CHK(vn::param_info(m, name, nullptr, count, ndim, shape));
  if (trainable) *trainable = ga3c_dd::trainable(m->vars[(size_t)ga3c_ckpt::find_var(m->vars, name)]) ? 1 : 0;
  return GA3C_OK;
}

int ga3c_ddpg_get_param(ga3c_ddpg* m, const char* name, int32_t which, float* out, int64_t count) {
  if (!out) return fail(GA3C_EINVAL, "null argument");
  return vn::param_copy(m, name, which, out, nullptr, count);
}

int ga3c_ddpg_set_param(ga3c_ddpg* m, const char* name, int32_t which, const float* in, int64_t count) {
  if (!in) return fail(GA3C_EINVAL, "null argument");
  return vn::param_copy(m, name, which, nullptr, in, count);
}

int ga3c_ddpg_get_step(ga3c_ddpg* m, int64_t* step) { return vn::get_step(m, step); }

int ga3c_ddpg_set_step(ga3c_ddpg* m, int64_t step) {      // Adam's t: never below zero
  if (!m || step < 0) return fail(GA3C_EINVAL, "bad argument");
  return vn::set_step(m, step);
}

// A distributional handle's file also holds "dist_support", f32 [2]: vmin, vmax (the atoms are critic_output/W's columns); a soft
// handle's "soft_config", f32 [3]: target_entropy, ls_min, ls_max.
int ga3c_ddpg_save(ga3c_ddpg* m, const char* path) {
  if (!m || !path) return fail(GA3C_EINVAL, "null argument");
  if (!m->dist && !m->soft) return vn::save(m, path);
  ga3c_ckpt::Arenas arena;
  CHK(vn::read_arenas(m, &arena));
  std::vector<ga3c_ckpt::Member> members = ga3c_ckpt::pack_members(m->vars, m->step.load(), arena);
  float extra[3];
  ga3c_ckpt::Member mb;
  if (m->dist) {
    extra[0] = m->dist->z.vmin; extra[1] = m->dist->z.vmax;
    mb.name = "dist_support";
    mb.shape = {2};
  } else {
    extra[0] = m->soft->target_entropy; extra[1] = m->soft->cfg.ls_min; extra[2] = m->soft->cfg.ls_max;
    mb.name = "soft_config";
    mb.shape = {3};
  }
  mb.descr = "<f4";
  mb.bytes.assign(reinterpret_cast<const uint8_t*>(extra), reinterpret_cast<const uint8_t*>(extra) + sizeof(float) * (m->dist ? 2 : 3));
  members.insert(members.begin() + 1, std::move(mb));        // beside "step"
  std::string err;
  if (!ga3c_ckpt::write_npz(path, members, &err)) return fail(GA3C_ESTATE, "%s", err.c_str());
  return GA3C_OK;
}

int ga3c_ddpg_load(ga3c_ddpg* m, const char* path) {
  if (!m || !path) return fail(GA3C_EINVAL, "null argument");
  std::map<std::string, ga3c_ckpt::Member> members;
  CHK(vn::read_checkpoint(path, &members));
  int64_t step = 0;
  CHK(vn::checkpoint_step(path, members, &step));
  if (step < 0) return fail(GA3C_ESTATE, "%s: step %lld", path, (long long)step);      // before anything is written
  if (!m->twin && members.count(std::string(TWIN_VAR_NAMES[0]) + ":0"))
    return fail(GA3C_ESTATE, "%s holds %s: the checkpoint of a handle with twin critics, which this one has not", path, TWIN_VAR_NAMES[0]);
  if (!m->pop && members.count(std::string(POP_VAR_NAMES[0]) + ":0"))
    return fail(GA3C_ESTATE, "%s holds %s: the checkpoint of a handle with PopArt, which this one has not", path, POP_VAR_NAMES[0]);
  const auto sup = members.find("dist_support");
  if (!m->dist && sup != members.end())
    return fail(GA3C_ESTATE, "%s holds dist_support: the checkpoint of a handle with a distributional critic, which this one has not", path);
  if (m->dist) {
    float v[2];
    if (sup == members.end() || sup->second.descr != "<f4" || sup->second.bytes.size() != sizeof v)
      return fail(GA3C_ESTATE, "%s holds no f32 dist_support [2]: not the checkpoint of a handle with a distributional critic", path);
    memcpy(v, sup->second.bytes.data(), sizeof v);
    if (v[0] != m->dist->z.vmin || v[1] != m->dist->z.vmax)
      return fail(GA3C_ESTATE, "%s: support [%g, %g], this handle's is [%g, %g]", path, v[0], v[1], m->dist->z.vmin, m->dist->z.vmax);
  }
  const auto scf = members.find("soft_config");
  if (!m->soft && (scf != members.end() || members.count(std::string(SOFT_VAR_NAME) + ":0")))
    return fail(GA3C_ESTATE, "%s holds soft_config: the checkpoint of a handle with the soft actor-critic, which this one has not", path);
  if (m->soft) {
    float v[3];
    if (scf == members.end() || scf->second.descr != "<f4" || scf->second.bytes.size() != sizeof v)
      return fail(GA3C_ESTATE, "%s holds no f32 soft_config [3]: not the checkpoint of a handle with the soft actor-critic", path);
    memcpy(v, scf->second.bytes.data(), sizeof v);
    if (v[0] != m->soft->target_entropy || v[1] != m->soft->cfg.ls_min || v[2] != m->soft->cfg.ls_max)
      return fail(GA3C_ESTATE, "%s: soft_config (%g, %g, %g), this handle's is (%g, %g, %g)", path, v[0], v[1], v[2],
                  m->soft->target_entropy, m->soft->cfg.ls_min, m->soft->cfg.ls_max);
  }
  return vn::load(m, path, members);                          // another atom count is another shape of critic_output/W
}

int ga3c_ddpg_noise_step(ga3c_ddpg* m, float* x, float* n) {
  if (!m) return fail(GA3C_EINVAL, "null argument");
  std::lock_guard<std::mutex> lk(m->noise_mu);
  const ga3c_ddpg_config& c = m->cfg;
  for (int i = 0; i < m->L.A; ++i) {
    // x' = x + theta (mu - x) dt + sigma sqrt(dt) n with mu = 0 (OrnsteinUhlenbeckActionNoise.__call__, :470-476)
    const float nn = (float)m->gen.normal();
    const double xp = m->ou_x[i];
    m->ou_x[i] = (float)(xp + (double)c.ou_theta * (0.0 - xp) * (double)c.ou_dt +
                         (double)c.ou_sigma * std::sqrt((double)c.ou_dt) * (double)nn);
    if (x) x[i] = m->ou_x[i];
    if (n) n[i] = nn;
  }
  return GA3C_OK;
}

int ga3c_ddpg_predict(ga3c_ddpg* m, const float* x, int32_t batch, int32_t noise_mode, const float* noise, float* a) {
  if (!m || !x || !a) return fail(GA3C_EINVAL, "null argument");
  int ticket;
  CHK(predict_begin(m, x, nullptr, batch, noise_mode, noise, &ticket));
  return predict_end(m, ticket, batch, a, nullptr);
}

// The segment must not change under a replay_add_gather either, so add_mu is held round the shared call, which takes
// train_mu, then mu.  Every other path takes add_mu -> mu (replay_add*) or train_mu -> mu and never add_mu while it holds
// train_mu or mu, so the order add_mu -> train_mu -> mu has no cycle.
int ga3c_ddpg_register_host(ga3c_ddpg* m, void* base, int64_t bytes) {
  if (!m) return fail(GA3C_EINVAL, "bad argument");
  std::lock_guard<std::mutex> al(m->add_mu);
  return vn::register_host(m, base, bytes);
}

int ga3c_ddpg_unregister_host(ga3c_ddpg* m) {
  if (!m) return fail(GA3C_EINVAL, "null argument");
  std::lock_guard<std::mutex> al(m->add_mu);
  return vn::unregister_host(m);
}

int ga3c_ddpg_predict_gather(void* net, const int64_t* offsets, int32_t batch, int32_t u8, float* p, float* v, float* z) {
  ga3c_ddpg* m = static_cast<ga3c_ddpg*>(net);
  (void)z;
  int ticket;
  CHK(ga3c_ddpg_predict_gather_begin(net, offsets, batch, u8, &ticket));
  return predict_end(m, ticket, batch, p, v);
}

int ga3c_ddpg_predict_gather_begin(void* net, const int64_t* offsets, int32_t batch, int32_t u8, int32_t* ticket) {
  ga3c_ddpg* m = static_cast<ga3c_ddpg*>(net);
  if (!m || !offsets || !ticket) return fail(GA3C_EINVAL, "null argument");
  if (u8) return fail(GA3C_EINVAL, "the DDPG networks read f32 rows (u8 = 0)");
  return predict_begin(m, nullptr, offsets, batch, GA3C_DDPG_NOISE_OWN, nullptr, ticket);
}

int ga3c_ddpg_predict_gather_end(void* net, int32_t ticket, int32_t batch, float* p, float* v) {
  ga3c_ddpg* m = static_cast<ga3c_ddpg*>(net);
  if (!m || !p || !v) return fail(GA3C_EINVAL, "null argument");
  return predict_end(m, ticket, batch, p, v);
}

int ga3c_ddpg_replay_add(ga3c_ddpg* m, const float* s, const float* a, const float* r, const float* done, const float* s2,
                         int32_t n, int64_t* size, int64_t* total) {
  if (!m || !s || !a || !r || !done || !s2) return fail(GA3C_EINVAL, "null argument");
  CHK(check_add_rows(m, n));
  HIPCHK(hipSetDevice(m->device));
  std::lock_guard<std::mutex> al(m->add_mu);
  pack_rows(m, m->h_add, s, a, r, done, s2, n);
  {
    std::lock_guard<std::mutex> lk(m->mu);
    CHK(ring_copy_in(m, m->h_add, n, hipMemcpyHostToDevice));
    per_fill(m, m->ring_total % m->cfg.replay_capacity, n);
    nstep_fill(m, m->ring_total % m->cfg.replay_capacity, n);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(m->aev, m->st));
    m->ring_total += n;
    ring_report(m, size, total);
  }
  HIPCHK(hipEventSynchronize(m->aev));
  return GA3C_OK;
}

int ga3c_ddpg_replay_add_gather(ga3c_ddpg* m, const int64_t* offsets, const float* r, const float* a, int32_t n, int64_t* size,
                                int64_t* total) {
  if (!m || !offsets || !r || !a) return fail(GA3C_EINVAL, "null argument");
  CHK(check_add_rows(m, n));
  HIPCHK(hipSetDevice(m->device));
  std::lock_guard<std::mutex> al(m->add_mu);
  const int S = m->L.S, A = m->L.A;
  {
    std::lock_guard<std::mutex> lk(m->mu);
    CHK(vn::check_offsets(m, offsets, n, 2 * S + 1));
    memcpy(m->h_aoff, offsets, sizeof(int64_t) * n);
    memcpy(m->h_ar, r, sizeof(float) * n);
    memcpy(m->h_aa, a, sizeof(float) * n * A);
    HIPCHK(hipMemcpyAsync(m->d_aoff, m->h_aoff, sizeof(int64_t) * n, hipMemcpyHostToDevice, m->st));
    HIPCHK(hipMemcpyAsync(m->d_ar, m->h_ar, sizeof(float) * n, hipMemcpyHostToDevice, m->st));
    HIPCHK(hipMemcpyAsync(m->d_aa, m->h_aa, sizeof(float) * n * A, hipMemcpyHostToDevice, m->st));
    const int64_t cap = m->cfg.replay_capacity, elems = (int64_t)n * m->rowf;
    hipLaunchKernelGGL(ddpg_ring_gather_kernel, dim3((unsigned)((elems + 255) / 256)), dim3(256), 0, m->st, m->reg_dev,
                       (const int64_t*)m->d_aoff, (const float*)m->d_ar, (const float*)m->d_aa, n, m->ring, m->ring_total % cap, cap,
                       S, A, m->nstep ? m->nstep->disc : nullptr, m->cfg.gamma);
    per_fill(m, m->ring_total % cap, n);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(m->aev, m->st));
    m->ring_total += n;
    ring_report(m, size, total);
  }
  HIPCHK(hipEventSynchronize(m->aev));
  return GA3C_OK;
}

int ga3c_ddpg_replay_get(ga3c_ddpg* m, int64_t slot, float* s, float* a, float* r, float* done, float* s2) {
  if (!m) return fail(GA3C_EINVAL, "null argument");
  HIPCHK(hipSetDevice(m->device));
  std::vector<float> row((size_t)m->rowf);
  {
    std::lock_guard<std::mutex> lk(m->mu);
    const int64_t size = ring_size(m);
    if (slot < 0 || slot >= size) return fail(GA3C_EINVAL, "slot %lld outside the ring's %lld rows", (long long)slot, (long long)size);
    HIPCHK(hipStreamSynchronize(m->st));
    HIPCHK(hipMemcpy(row.data(), m->ring + slot * m->rowf, sizeof(float) * m->rowf, hipMemcpyDeviceToHost));
  }
  const int S = m->L.S, A = m->L.A;
  if (s) memcpy(s, row.data(), sizeof(float) * S);
  if (a) memcpy(a, row.data() + S, sizeof(float) * A);
  if (r) *r = row[S + A];
  if (done) *done = row[S + A + 1];
  if (s2) memcpy(s2, row.data() + S + A + 2, sizeof(float) * S);
  return GA3C_OK;
}

int ga3c_ddpg_replay_size(ga3c_ddpg* m, int64_t* size, int64_t* total) {
  if (!m) return fail(GA3C_EINVAL, "null argument");
  std::lock_guard<std::mutex> lk(m->mu);
  ring_report(m, size, total);
  return GA3C_OK;
}

int ga3c_ddpg_train(ga3c_ddpg* m, const float* s, const float* a, const float* r, const float* done, const float* s2,
                    int32_t batch, float learning_rate, int32_t noise_mode, const float* noise, float* q_stats) {
  return step_host(m, s, a, r, done, s2, batch, learning_rate, noise_mode, noise, 6, q_stats);
}

int ga3c_ddpg_compute(ga3c_ddpg* m, const float* s, const float* a, const float* r, const float* done, const float* s2,
                      int32_t batch, float learning_rate, int32_t noise_mode, const float* noise, int32_t stop_after,
                      float* q_stats) {
  if (stop_after != 3 && stop_after != 4) return fail(GA3C_EINVAL, "stop_after %d not in {3, 4}", stop_after);
  return step_host(m, s, a, r, done, s2, batch, learning_rate, noise_mode, noise, stop_after, q_stats);
}

int ga3c_ddpg_train_replay(ga3c_ddpg* m, const int32_t* slots, int32_t batch, int64_t stamp, float learning_rate,
                           int32_t noise_mode, const float* noise, float* q_stats) {
  if (!m || !slots) return fail(GA3C_EINVAL, "null argument");
  CHK(vn::check_batch(m, batch));
  HIPCHK(hipSetDevice(m->device));
  std::lock_guard<std::mutex> tl(m->train_mu);
  {
    std::lock_guard<std::mutex> lk(m->mu);
    // Validated under the lock that orders ring writes: a slot is refused if a row was written into it after `stamp`.
    const int64_t cap = m->cfg.replay_capacity, total = m->ring_total, size = ring_size(m);
    for (int i = 0; i < batch; ++i) {
      const int64_t sl = slots[i];
      if (sl < 0 || sl >= size) return fail(GA3C_EINVAL, "slot %lld of row %d outside the ring's %lld rows", (long long)sl, i, (long long)size);
      if (stamp >= 0) {
        const int64_t last = (total - 1) - ((total - 1 - sl) % cap);     // number of the row that lies in the slot now
        if (last >= stamp)
          return fail(GA3C_ELOST, "slot %lld was overwritten by row %lld after the batch was sampled at %lld", (long long)sl,
                      (long long)last, (long long)stamp);
      }
    }
    Noise nz;
    CHK(make_noise(m, noise_mode, noise, &nz));
    memcpy(m->h_idx, slots, sizeof(int32_t) * batch);
    HIPCHK(hipMemcpyAsync(m->d_idx, m->h_idx, sizeof(int32_t) * batch, hipMemcpyHostToDevice, m->st));
    CHK(enqueue_step(m, Rows{m->ring, m->d_idx, m->rowf}, batch, learning_rate, nz, 6));
    CHK(finish_step(m));
    m->last_B = batch;
  }
  HIPCHK(hipEventSynchronize(m->tev));
  give_qstats(m, q_stats);
  m->step.fetch_add(1);
  return GA3C_OK;
}

int ga3c_ddpg_fetch(ga3c_ddpg* m, const char* name, float* out, int64_t count) {
  if (!m || !name || !out) return fail(GA3C_EINVAL, "null argument");
  const bool per_w = strcmp(name, "per_w") == 0;
  if (per_w || strcmp(name, "per_td") == 0) {       // of the last draw / the last prioritised step, whatever ran since
    HIPCHK(hipSetDevice(m->device));
    std::lock_guard<std::mutex> tl(m->train_mu);
    std::lock_guard<std::mutex> lk(m->mu);
    CHK(per_check(m, name));
    const int rows = per_w ? m->per->w_rows : m->per->td_rows;
    if (count != rows) return fail(GA3C_EINVAL, "%s holds %d floats, not %lld", name, rows, (long long)count);
    HIPCHK(hipStreamSynchronize(m->st));
    HIPCHK(hipMemcpy(out, per_w ? m->per->w : m->per->td, sizeof(float) * count, hipMemcpyDeviceToHost));
    return GA3C_OK;
  }
  if (strcmp(name, "disc") == 0) {                  // the discounts the last step's target took, by row
    HIPCHK(hipSetDevice(m->device));
    std::lock_guard<std::mutex> tl(m->train_mu);
    std::lock_guard<std::mutex> lk(m->mu);
    if (!m->nstep) return fail(GA3C_ESTATE, "%s: the handle has no n-step returns (ga3c_ddpg_nstep_create)", name);
    if (count != m->last_B) return fail(GA3C_EINVAL, "%s of the last step is %d floats, not %lld", name, m->last_B, (long long)count);
    HIPCHK(hipStreamSynchronize(m->st));
    HIPCHK(hipMemcpy(out, m->nstep->used, sizeof(float) * count, hipMemcpyDeviceToHost));
    return GA3C_OK;
  }
  for (const WorkRow& r : work_table(m)) {
    if (strcmp(name, r.name) != 0) continue;
    if (r.tag == W_CORE) return vn::fetch(m, name, *r.ptr, (int64_t)r.width, out, count);
    HIPCHK(hipSetDevice(m->device));                // under both locks throughout: twin_destroy / dist_destroy free these rows
    std::lock_guard<std::mutex> tl(m->train_mu);
    std::lock_guard<std::mutex> lk(m->mu);
    if (r.tag == W_TWIN && !m->twin) return fail(GA3C_ESTATE, "%s: the handle has no twin critics (ga3c_ddpg_twin_create)", name);
    if (r.tag == W_DIST && !m->dist)
      return fail(GA3C_ESTATE, "%s: the handle has no distributional critic (ga3c_ddpg_dist_create)", name);
    if (r.tag == W_POP && !m->pop) return fail(GA3C_ESTATE, "%s: the handle has no PopArt (ga3c_ddpg_popart_create)", name);
    if (r.tag == W_SOFT && !m->soft) return fail(GA3C_ESTATE, "%s: the handle has no soft actor-critic (ga3c_ddpg_soft_create)", name);
    const int64_t want = (int64_t)r.width * m->last_B;
    if (count != want) return fail(GA3C_EINVAL, "%s of the last step is %lld floats, not %lld", name, (long long)want, (long long)count);
    HIPCHK(hipStreamSynchronize(m->st));
    HIPCHK(hipMemcpy(out, *r.ptr, sizeof(float) * count, hipMemcpyDeviceToHost));
    return GA3C_OK;
  }
  return fail(GA3C_EINVAL, "no buffer named %s", name);
}

// Unlike the actor-critic nets' it advances `step` with every iteration: Adam's t must move.
int ga3c_ddpg_time_resident(ga3c_ddpg* m, int32_t mode, int32_t batch, int32_t iters, float learning_rate, float* elapsed_ms) {
  if (!m || !elapsed_ms || iters < 1 || (mode != 0 && mode != 1)) return fail(GA3C_EINVAL, "bad argument");
  CHK(vn::check_batch(m, batch));
  HIPCHK(hipSetDevice(m->device));
  std::lock_guard<std::mutex> tl(m->train_mu);
  {
    std::lock_guard<std::mutex> lk(m->mu);
    if (batch > ring_size(m)) return fail(GA3C_ESTATE, "batch %d: the ring holds %lld rows", batch, (long long)ring_size(m));
    for (int i = 0; i < batch; ++i) m->h_idx[i] = i;
    HIPCHK(hipMemcpyAsync(m->d_idx, m->h_idx, sizeof(int32_t) * batch, hipMemcpyHostToDevice, m->st));
    Noise nz;
    memset(&nz, 0, sizeof nz);
    const Rows rows{m->ring, m->d_idx, m->rowf};
    const Input in{reinterpret_cast<const char*>(m->ring), nullptr, 4 * (int64_t)m->rowf};
    CHK(timed_loop(m, batch, iters, [&]() -> int {
      if (mode == 0) {
        if (m->soft) launch_soft_predict(m, in, batch, GA3C_DDPG_NOISE_NONE, nz, 0, m->w.a_out, nullptr);
        else
          hipLaunchKernelGGL(ddpg_predict_kernel, dim3(tiles(batch)), dim3(THREADS), 0, m->st, m->L, (const float*)m->arena[0], in,
                             batch, nz, m->w.a_out);
        return GA3C_OK;
      }
      CHK(enqueue_step(m, rows, batch, learning_rate, nz, 6));
      m->step.fetch_add(1);
      return GA3C_OK;
    }));
  }
  return timed_wait(m, elapsed_ms);
}

// ---- prioritised replay

int ga3c_ddpg_priorities_create(ga3c_ddpg* m, float alpha, float eps, int64_t seed) {
  if (!m) return fail(GA3C_EINVAL, "null argument");
  if (!(alpha >= 0.f && alpha <= 1.f)) return fail(GA3C_EINVAL, "alpha %g outside [0,1]", alpha);
  if (!(eps > 0.f) || std::isinf(eps)) return fail(GA3C_EINVAL, "eps %g: a finite number > 0", eps);
  if (m->cfg.replay_capacity > PER_THREADS * PER_CHUNK)
    return fail(GA3C_EINVAL, "replay_capacity %d: priorities cover at most %d slots (%d chunks of %d)", m->cfg.replay_capacity,
                PER_THREADS * PER_CHUNK, PER_THREADS, PER_CHUNK);
  if (!(m->cfg.flags & GA3C_DDPG_LOSS_PAIRED))
    return fail(GA3C_ESTATE, "priorities need GA3C_DDPG_LOSS_PAIRED: under the fork's loss the critic regresses on mean(y) "
                             "and a row has no TD error of its own");
  HIPCHK(hipSetDevice(m->device));
  std::lock_guard<std::mutex> tl(m->train_mu);
  std::lock_guard<std::mutex> lk(m->mu);
  if (m->per) return fail(GA3C_ESTATE, "the handle has priorities already");
  Per* p = new (std::nothrow) Per();
  if (!p) return fail(GA3C_EINVAL, "out of host memory");
  m->per = p;
  p->alpha = alpha;
  p->eps = eps;
  p->seed = (uint64_t)seed;
  const size_t cap = (size_t)m->cfg.replay_capacity, B = (size_t)m->cfg.max_batch;
  const size_t padded = (cap + PER_CHUNK - 1) / PER_CHUNK * PER_CHUNK;
  const float one = 1.0f;
  auto build = [&]() -> int {
    CHK(vn::dalloc(&p->pa, padded)); CHK(vn::dalloc(&p->max_pa, 1)); CHK(vn::dalloc(&p->csum, PER_THREADS));
    CHK(vn::dalloc(&p->slots, B)); CHK(vn::dalloc(&p->w, B)); CHK(vn::dalloc(&p->td, B));
    CHK(vn::halloc(&p->h_slots, B)); CHK(vn::halloc(&p->h_w, B));
    HIPCHK(hipMemsetAsync(p->pa, 0, sizeof(float) * padded, m->st));
    HIPCHK(hipMemsetAsync(p->csum, 0, sizeof(double) * PER_THREADS, m->st));
    HIPCHK(hipMemsetAsync(p->w, 0, sizeof(float) * B, m->st));
    HIPCHK(hipMemsetAsync(p->td, 0, sizeof(float) * B, m->st));
    HIPCHK(hipMemsetAsync(p->slots, 0, sizeof(int32_t) * B, m->st));
    HIPCHK(hipMemcpyAsync(p->max_pa, &one, sizeof(float), hipMemcpyHostToDevice, m->st));
    per_fill(m, 0, ring_size(m));                  // rows the ring holds already: max_pa = 1
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(m->st));
    return GA3C_OK;
  };
  const int rc = build();
  if (rc != GA3C_OK) per_free(m);
  return rc;
}

int ga3c_ddpg_priorities_destroy(ga3c_ddpg* m) {
  if (!m) return fail(GA3C_EINVAL, "null argument");
  HIPCHK(hipSetDevice(m->device));
  std::lock_guard<std::mutex> tl(m->train_mu);
  std::lock_guard<std::mutex> lk(m->mu);
  CHK(per_check(m, "priorities_destroy"));
  HIPCHK(hipStreamSynchronize(m->st));
  per_free(m);
  return GA3C_OK;
}

int ga3c_ddpg_priorities_get(ga3c_ddpg* m, float* pa, float* max_pa) {
  if (!m || !pa || !max_pa) return fail(GA3C_EINVAL, "null argument");
  HIPCHK(hipSetDevice(m->device));
  std::lock_guard<std::mutex> tl(m->train_mu);
  std::lock_guard<std::mutex> lk(m->mu);
  CHK(per_check(m, "priorities_get"));
  HIPCHK(hipStreamSynchronize(m->st));
  HIPCHK(hipMemcpy(pa, m->per->pa, sizeof(float) * (size_t)m->cfg.replay_capacity, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(max_pa, m->per->max_pa, sizeof(float), hipMemcpyDeviceToHost));
  return GA3C_OK;
}

int ga3c_ddpg_priorities_set(ga3c_ddpg* m, const float* pa, float max_pa) {
  if (!m || !pa) return fail(GA3C_EINVAL, "null argument");
  if (!(max_pa > 0.f) || std::isinf(max_pa)) return fail(GA3C_EINVAL, "max_pa %g: a finite number > 0", max_pa);
  HIPCHK(hipSetDevice(m->device));
  std::lock_guard<std::mutex> tl(m->train_mu);
  std::lock_guard<std::mutex> lk(m->mu);
  CHK(per_check(m, "priorities_set"));
  const int64_t cap = m->cfg.replay_capacity, size = ring_size(m);
  for (int64_t i = 0; i < cap; ++i) {
    if (!(pa[i] >= 0.f) || std::isinf(pa[i])) return fail(GA3C_EINVAL, "pa[%lld] = %g: negative or not a number", (long long)i, pa[i]);
    if (i < size && pa[i] == 0.f) return fail(GA3C_EINVAL, "pa[%lld] = 0 in a slot that holds a row: it could never be drawn", (long long)i);
  }
  HIPCHK(hipStreamSynchronize(m->st));
  HIPCHK(hipMemcpy(m->per->pa, pa, sizeof(float) * (size_t)cap, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(m->per->max_pa, &max_pa, sizeof(float), hipMemcpyHostToDevice));
  return GA3C_OK;
}

int ga3c_ddpg_sample_prioritized(ga3c_ddpg* m, int32_t batch, float beta_is, int32_t* slots, float* weights) {
  if (!m || !slots || !weights) return fail(GA3C_EINVAL, "null argument");
  HIPCHK(hipSetDevice(m->device));
  std::lock_guard<std::mutex> tl(m->train_mu);
  {
    std::lock_guard<std::mutex> lk(m->mu);
    CHK(per_check(m, "sample_prioritized"));
    CHK(vn::check_batch(m, batch));
    CHK(per_check_beta(beta_is));
    if (ring_size(m) < 1) return fail(GA3C_ESTATE, "the ring holds no row");
    per_enqueue_sample(m, batch, beta_is);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(m->per->h_slots, m->per->slots, sizeof(int32_t) * batch, hipMemcpyDeviceToHost, m->st));
    HIPCHK(hipMemcpyAsync(m->per->h_w, m->per->w, sizeof(float) * batch, hipMemcpyDeviceToHost, m->st));
    HIPCHK(hipEventRecord(m->tev, m->st));
  }
  HIPCHK(hipEventSynchronize(m->tev));
  memcpy(slots, m->per->h_slots, sizeof(int32_t) * batch);      // (train_mu is held: priorities_destroy waits)
  memcpy(weights, m->per->h_w, sizeof(float) * batch);
  return GA3C_OK;
}

int ga3c_ddpg_train_prioritized(ga3c_ddpg* m, int32_t batch, float beta_is, float learning_rate, int32_t noise_mode,
                                const float* noise, float* q_stats, int32_t* out_slots) {
  if (!m) return fail(GA3C_EINVAL, "null argument");
  HIPCHK(hipSetDevice(m->device));
  std::lock_guard<std::mutex> tl(m->train_mu);
  {
    std::lock_guard<std::mutex> lk(m->mu);
    CHK(per_check(m, "train_prioritized"));
    CHK(vn::check_batch(m, batch));
    CHK(per_check_beta(beta_is));
    if (!(ring_size(m) > batch))                  // ThreadReplay.sample's rule: a batch is drawn from MORE rows than it holds
      return fail(GA3C_ESTATE, "batch %d: the ring holds %lld rows, not more than a batch", batch, (long long)ring_size(m));
    Noise nz;
    CHK(make_noise(m, noise_mode, noise, &nz));
    CHK(per_enqueue_step(m, batch, beta_is, learning_rate, nz));
    if (out_slots) HIPCHK(hipMemcpyAsync(m->per->h_slots, m->per->slots, sizeof(int32_t) * batch, hipMemcpyDeviceToHost, m->st));
    CHK(finish_step(m));
    m->last_B = batch;
  }
  HIPCHK(hipEventSynchronize(m->tev));
  give_qstats(m, q_stats);
  if (out_slots) memcpy(out_slots, m->per->h_slots, sizeof(int32_t) * batch);
  m->step.fetch_add(1);
  return GA3C_OK;
}

// As ga3c_ddpg_time_resident's mode 1, with every step drawing its own rows.
int ga3c_ddpg_time_prioritized(ga3c_ddpg* m, int32_t batch, int32_t iters, float beta_is, float learning_rate, float* elapsed_ms) {
  if (!m || !elapsed_ms || iters < 1) return fail(GA3C_EINVAL, "bad argument");
  HIPCHK(hipSetDevice(m->device));
  std::lock_guard<std::mutex> tl(m->train_mu);
  {
    std::lock_guard<std::mutex> lk(m->mu);
    CHK(per_check(m, "time_prioritized"));
    CHK(vn::check_batch(m, batch));
    CHK(per_check_beta(beta_is));
    if (!(ring_size(m) > batch))
      return fail(GA3C_ESTATE, "batch %d: the ring holds %lld rows, not more than a batch", batch, (long long)ring_size(m));
    Noise nz;
    memset(&nz, 0, sizeof nz);
    CHK(timed_loop(m, batch, iters, [&]() -> int {
      CHK(per_enqueue_step(m, batch, beta_is, learning_rate, nz));
      m->step.fetch_add(1);
      return GA3C_OK;
    }));
  }
  return timed_wait(m, elapsed_ms);
}

// ---- twin critics

int ga3c_ddpg_twin_create(ga3c_ddpg* m, int32_t policy_delay, float target_sigma, float target_clip, int64_t seed) {
  if (!m) return fail(GA3C_EINVAL, "null argument");
  if (policy_delay < 1 || policy_delay > 16) return fail(GA3C_EINVAL, "policy_delay %d outside [1,16]", policy_delay);
  if (!(target_sigma >= 0.f) || std::isinf(target_sigma)) return fail(GA3C_EINVAL, "target_sigma %g: a finite number >= 0", target_sigma);
  if (!(target_clip >= 0.f) || std::isinf(target_clip)) return fail(GA3C_EINVAL, "target_clip %g: a finite number >= 0", target_clip);
  if (!(m->cfg.flags & GA3C_DDPG_LOSS_PAIRED))
    return fail(GA3C_ESTATE, "twin critics need GA3C_DDPG_LOSS_PAIRED: under the fork's loss the critics regress on mean(y) and a "
                             "row has no target of its own");
  HIPCHK(hipSetDevice(m->device));
  std::lock_guard<std::mutex> tl(m->train_mu);
  std::lock_guard<std::mutex> lk(m->mu);
  if (m->twin) return fail(GA3C_ESTATE, "the handle has twin critics already");
  if (m->dist) return fail(GA3C_ESTATE, "the handle has a distributional critic: two distributions have no smaller one");
  if (m->pop) return fail(GA3C_ESTATE, "the handle has PopArt, which normalises one scalar critic (ga3c_ddpg_popart_destroy first)");
  Twin* t = new (std::nothrow) Twin();
  if (!t) return fail(GA3C_EINVAL, "out of host memory");
  t->delay = policy_delay;
  t->sigma = target_sigma;
  t->clip = target_clip;
  t->seed = (uint64_t)seed;
  // Every arena grows by critic 2's variables, which start as ga3c_ddpg_create leaves the others; the 26 keep their values.
  Options to = m->opt;
  to.twin = true;
  m->twin = t;
  float* end = nullptr;
  int rc = carve_work(m, W_TWIN, &t->work_base, &end);
  if (rc == GA3C_OK) rc = relay_arenas(m, to);
  if (rc != GA3C_OK) twin_free(m);
  return rc;
}

int ga3c_ddpg_twin_destroy(ga3c_ddpg* m) {
  if (!m) return fail(GA3C_EINVAL, "null argument");
  HIPCHK(hipSetDevice(m->device));
  std::lock_guard<std::mutex> tl(m->train_mu);
  std::lock_guard<std::mutex> lk(m->mu);
  if (!m->twin) return fail(GA3C_ESTATE, "the handle has no twin critics (ga3c_ddpg_twin_create)");
  if (m->soft) return fail(GA3C_ESTATE, "twin_destroy: the handle's soft actor-critic trains both critics (ga3c_ddpg_soft_destroy first)");
  HIPCHK(hipStreamSynchronize(m->st));
  twin_free(m);
  return GA3C_OK;
}

// ---- soft actor-critic

int ga3c_ddpg_soft_create(ga3c_ddpg* m, float log_alpha, float alpha_lr, float target_entropy, float ls_min, float ls_max, int64_t seed) {
  if (!m) return fail(GA3C_EINVAL, "null argument");
  if (2 * m->L.A > MAX_A) return fail(GA3C_EINVAL, "%d actions: the Gaussian head has 2 A columns and the head holds %d", m->L.A, MAX_A);
  if (!std::isfinite(log_alpha) || !std::isfinite(alpha_lr) || !std::isfinite(target_entropy) || !std::isfinite(ls_min) ||
      !std::isfinite(ls_max))
    return fail(GA3C_EINVAL, "log_alpha %g, alpha_lr %g, target_entropy %g, log-std bounds [%g, %g]: finite numbers", log_alpha,
                alpha_lr, target_entropy, ls_min, ls_max);
  if (!(ls_min < ls_max)) return fail(GA3C_EINVAL, "log-std bounds [%g, %g]: the first the smaller", ls_min, ls_max);
  if (!(alpha_lr >= 0.f)) return fail(GA3C_EINVAL, "alpha_lr %g: a factor >= 0", alpha_lr);
  HIPCHK(hipSetDevice(m->device));
  std::lock_guard<std::mutex> tl(m->train_mu);
  std::lock_guard<std::mutex> lk(m->mu);
  if (m->soft) return fail(GA3C_ESTATE, "the handle has the soft actor-critic already");
  if (!m->twin) return fail(GA3C_ESTATE, "the soft actor-critic trains twin critics (ga3c_ddpg_twin_create first)");
  if (m->actors || m->eval)
    return fail(GA3C_ESTATE, "the handle has device actors or evaluation episodes: the order is twin, soft, then those");
  Soft* s = new (std::nothrow) Soft();
  if (!s) return fail(GA3C_EINVAL, "out of host memory");
  s->cfg.ls_min = ls_min;
  s->cfg.ls_max = ls_max;
  s->cfg.seed = (uint64_t)seed;
  s->alpha_lr = alpha_lr;
  s->target_entropy = target_entropy;
  s->core_dout = m->w.dout;
  m->soft = s;                                     // work_table sizes "do" by it
  int rc = carve_work(m, W_SOFT, &s->work_base, &m->sw.stat);
  if (rc == GA3C_OK) rc = vn::dalloc(&s->act_eps, (size_t)m->cfg.max_batch * m->L.A);
  if (rc == GA3C_OK && hipMemset(s->act_eps, 0, sizeof(float) * (size_t)m->cfg.max_batch * m->L.A) != hipSuccess)
    rc = fail(GA3C_EHIP, "hipMemset failed");
  // the Gaussian head's 2 A columns start as ga3c_ddpg_create leaves variables, log_alpha lies behind critic 2's twelve
  Options to = m->opt;
  to.soft = true;
  to.head = 2 * m->L.A;
  if (rc == GA3C_OK) rc = relay_arenas(m, to, log_alpha);
  if (rc != GA3C_OK) {
    soft_free(m);
    return rc;
  }
  s->cfg.la = var_offset(m, SOFT_VAR_NAME);
  return GA3C_OK;
}

int ga3c_ddpg_soft_destroy(ga3c_ddpg* m) {
  if (!m) return fail(GA3C_EINVAL, "null argument");
  HIPCHK(hipSetDevice(m->device));
  std::lock_guard<std::mutex> tl(m->train_mu);
  std::lock_guard<std::mutex> lk(m->mu);
  if (!m->soft) return fail(GA3C_ESTATE, "the handle has no soft actor-critic (ga3c_ddpg_soft_create)");
  if (m->actors || m->eval)
    return fail(GA3C_ESTATE, "soft_destroy: the handle's device actors or evaluation episodes step under its policy (destroy them first)");
  Options to = m->opt;
  to.soft = false;
  to.head = 0;
  CHK(relay_arenas(m, to));
  soft_free(m);
  return GA3C_OK;
}

int ga3c_ddpg_soft_info(ga3c_ddpg* m, float* log_alpha, float* target_entropy, float* mean_logp, int64_t* predictions) {
  if (!m) return fail(GA3C_EINVAL, "null argument");
  HIPCHK(hipSetDevice(m->device));
  std::lock_guard<std::mutex> tl(m->train_mu);
  std::lock_guard<std::mutex> lk(m->mu);
  if (!m->soft) return fail(GA3C_ESTATE, "the handle has no soft actor-critic (ga3c_ddpg_soft_create)");
  HIPCHK(hipStreamSynchronize(m->st));
  if (log_alpha) HIPCHK(hipMemcpy(log_alpha, m->arena[0] + m->soft->cfg.la, sizeof(float), hipMemcpyDeviceToHost));
  if (mean_logp) HIPCHK(hipMemcpy(mean_logp, m->sw.stat, sizeof(float), hipMemcpyDeviceToHost));
  if (target_entropy) *target_entropy = m->soft->target_entropy;
  if (predictions) *predictions = m->soft->predictions.load();
  return GA3C_OK;
}

// ---- distributional critic

int ga3c_ddpg_dist_create(ga3c_ddpg* m, int32_t atoms, float vmin, float vmax) {
  if (!m) return fail(GA3C_EINVAL, "null argument");
  if (atoms < 2 || atoms > GA3C_DDPG_ATOMS_MAX) return fail(GA3C_EINVAL, "atoms %d outside [2,%d]", atoms, GA3C_DDPG_ATOMS_MAX);
  if (!std::isfinite(vmin) || !std::isfinite(vmax) || !(vmin < vmax))
    return fail(GA3C_EINVAL, "support [%g, %g]: two finite numbers, the first the smaller", vmin, vmax);
  const float delta = (vmax - vmin) / (float)(atoms - 1);
  if (!std::isfinite(delta) || !(delta > 0.f)) return fail(GA3C_EINVAL, "support [%g, %g]: its width is not an f32", vmin, vmax);
  if (!(m->cfg.flags & GA3C_DDPG_LOSS_PAIRED))
    return fail(GA3C_ESTATE, "a distributional critic needs GA3C_DDPG_LOSS_PAIRED: under the fork's loss a row has no target of "
                             "its own");
  HIPCHK(hipSetDevice(m->device));
  std::lock_guard<std::mutex> tl(m->train_mu);
  std::lock_guard<std::mutex> lk(m->mu);
  if (m->dist) return fail(GA3C_ESTATE, "the handle has a distributional critic already");
  if (m->twin) return fail(GA3C_ESTATE, "the handle has twin critics: two distributions have no smaller one");
  if (m->pop) return fail(GA3C_ESTATE, "the handle has PopArt, which normalises one scalar critic (ga3c_ddpg_popart_destroy first)");
  Dist* d = new (std::nothrow) Dist();
  if (!d) return fail(GA3C_EINVAL, "out of host memory");
  d->z = Support{atoms, vmin, vmax, delta};
  m->dist = d;                                     // work_table sizes the rows by it
  float* end = nullptr;
  int rc = carve_work(m, W_DIST, &d->work_base, &end);
  Options to = m->opt;                             // critic_output/W and /b, reshaped, start as ga3c_ddpg_create leaves variables
  to.atoms = atoms;
  if (rc == GA3C_OK) rc = relay_arenas(m, to);
  if (rc != GA3C_OK) dist_free(m);
  return rc;
}

int ga3c_ddpg_dist_destroy(ga3c_ddpg* m) {
  if (!m) return fail(GA3C_EINVAL, "null argument");
  HIPCHK(hipSetDevice(m->device));
  std::lock_guard<std::mutex> tl(m->train_mu);
  std::lock_guard<std::mutex> lk(m->mu);
  if (!m->dist) return fail(GA3C_ESTATE, "the handle has no distributional critic (ga3c_ddpg_dist_create)");
  Options to = m->opt;
  to.atoms = 1;
  CHK(relay_arenas(m, to));
  dist_free(m);
  return GA3C_OK;
}

int ga3c_ddpg_dist_info(ga3c_ddpg* m, int32_t* atoms, float* vmin, float* vmax) {
  if (!m) return fail(GA3C_EINVAL, "null argument");
  std::lock_guard<std::mutex> lk(m->mu);
  if (atoms) *atoms = m->dist ? m->dist->z.n : 1;
  if (vmin) *vmin = m->dist ? m->dist->z.vmin : 0.f;
  if (vmax) *vmax = m->dist ? m->dist->z.vmax : 0.f;
  return GA3C_OK;
}

// ---- PopArt

int ga3c_ddpg_popart_create(ga3c_ddpg* m, float beta, float sigma_min, float sigma_max) {
  if (!m) return fail(GA3C_EINVAL, "null argument");
  if (!(beta >= 0.f && beta <= 1.f)) return fail(GA3C_EINVAL, "beta %g outside [0,1]", beta);
  if (!std::isfinite(sigma_min) || !std::isfinite(sigma_max) || !(sigma_min > 0.f) || !(sigma_min < sigma_max))
    return fail(GA3C_EINVAL, "sigma bounds [%g, %g]: two finite numbers, 0 < the first < the second", sigma_min, sigma_max);
  if (!(m->cfg.flags & GA3C_DDPG_LOSS_PAIRED))
    return fail(GA3C_ESTATE, "PopArt needs GA3C_DDPG_LOSS_PAIRED: under the fork's loss the critic regresses on mean(y) and a row "
                             "has no target of its own to normalise");
  HIPCHK(hipSetDevice(m->device));
  std::lock_guard<std::mutex> tl(m->train_mu);
  std::lock_guard<std::mutex> lk(m->mu);
  if (m->pop) return fail(GA3C_ESTATE, "the handle has PopArt already");
  if (m->twin) return fail(GA3C_ESTATE, "the handle has twin critics: PopArt normalises one scalar critic");
  if (m->dist) return fail(GA3C_ESTATE, "the handle has a distributional critic: its support fixes the returns' scale");
  Pop* p = new (std::nothrow) Pop();
  if (!p) return fail(GA3C_EINVAL, "out of host memory");
  p->beta = beta;
  p->smin = sigma_min;
  p->smax = sigma_max;
  // Every arena grows by the two statistics: mu = 0, nu = 1 in the value and the target arena, zero elsewhere.  The 26 keep
  // their values.
  Options to = m->opt;
  to.pop = true;
  m->pop = p;
  float* end = nullptr;
  int rc = carve_work(m, W_POP, &p->work_base, &end);
  if (rc == GA3C_OK) rc = relay_arenas(m, to);
  if (rc != GA3C_OK) {
    pop_free(m);
    return rc;
  }
  p->stat = var_offset(m, POP_VAR_NAMES[0]);
  return GA3C_OK;
}

int ga3c_ddpg_popart_destroy(ga3c_ddpg* m) {
  if (!m) return fail(GA3C_EINVAL, "null argument");
  HIPCHK(hipSetDevice(m->device));
  std::lock_guard<std::mutex> tl(m->train_mu);
  std::lock_guard<std::mutex> lk(m->mu);
  if (!m->pop) return fail(GA3C_ESTATE, "the handle has no PopArt (ga3c_ddpg_popart_create)");
  HIPCHK(hipStreamSynchronize(m->st));
  pop_free(m);
  return GA3C_OK;
}

int ga3c_ddpg_popart_info(ga3c_ddpg* m, float* beta, float* mu, float* nu, float* sigma) {
  if (!m) return fail(GA3C_EINVAL, "null argument");
  HIPCHK(hipSetDevice(m->device));
  std::lock_guard<std::mutex> tl(m->train_mu);
  std::lock_guard<std::mutex> lk(m->mu);
  if (!m->pop) return fail(GA3C_ESTATE, "the handle has no PopArt (ga3c_ddpg_popart_create)");
  float stat[2];
  HIPCHK(hipStreamSynchronize(m->st));
  HIPCHK(hipMemcpy(stat, m->arena[0] + m->pop->stat, sizeof stat, hipMemcpyDeviceToHost));
  if (beta) *beta = m->pop->beta;
  if (mu) *mu = stat[0];
  if (nu) *nu = stat[1];
  if (sigma) {     // the kernels' expression, on the host
    const double v = std::sqrt(std::fmax((double)stat[1] - (double)stat[0] * (double)stat[0], 0.0));
    *sigma = (float)std::fmin(std::fmax(v, (double)m->pop->smin), (double)m->pop->smax);
  }
  return GA3C_OK;
}

// ---- n-step returns

namespace {
int nstep_check(const ga3c_ddpg* m, const char* what) {
  if (!m->nstep) return fail(GA3C_ESTATE, "%s: the handle has no n-step returns (ga3c_ddpg_nstep_create)", what);
  return GA3C_OK;
}
}  // namespace

int ga3c_ddpg_nstep_create(ga3c_ddpg* m, int32_t n) {
  if (!m) return fail(GA3C_EINVAL, "null argument");
  if (n < 1 || n > GA3C_DDPG_NSTEP_MAX) return fail(GA3C_EINVAL, "n %d outside [1,%d]", n, GA3C_DDPG_NSTEP_MAX);
  if (!(m->cfg.flags & GA3C_DDPG_FUTURE_REWARD))
    return fail(GA3C_ESTATE, "n-step returns need GA3C_DDPG_FUTURE_REWARD: without it y = r and no discount is read");
  HIPCHK(hipSetDevice(m->device));
  std::lock_guard<std::mutex> tl(m->train_mu);
  std::lock_guard<std::mutex> lk(m->mu);
  if (m->nstep) return fail(GA3C_ESTATE, "the handle has n-step returns already");
  if (m->actors) return fail(GA3C_ESTATE, "the handle has device actors: their windows are sized at actors_create, so n-step comes first");
  NStep* ns = new (std::nothrow) NStep();
  if (!ns) return fail(GA3C_EINVAL, "out of host memory");
  m->nstep = ns;
  ns->n = n;
  const size_t cap = (size_t)m->cfg.replay_capacity, B = (size_t)m->cfg.max_batch;
  auto build = [&]() -> int {
    CHK(vn::dalloc(&ns->disc, cap)); CHK(vn::dalloc(&ns->used, B));
    HIPCHK(hipMemsetAsync(ns->used, 0, sizeof(float) * B, m->st));
    nstep_fill(m, 0, (int64_t)cap);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(m->st));
    return GA3C_OK;
  };
  const int rc = build();
  if (rc != GA3C_OK) nstep_free(m);
  return rc;
}

int ga3c_ddpg_nstep_destroy(ga3c_ddpg* m) {
  if (!m) return fail(GA3C_EINVAL, "null argument");
  HIPCHK(hipSetDevice(m->device));
  std::lock_guard<std::mutex> tl(m->train_mu);
  std::lock_guard<std::mutex> lk(m->mu);
  CHK(nstep_check(m, "nstep_destroy"));
  if (m->actors) return fail(GA3C_ESTATE, "nstep_destroy: the handle's device actors hold its windows (ga3c_ddpg_actors_destroy first)");
  HIPCHK(hipStreamSynchronize(m->st));
  nstep_free(m);
  return GA3C_OK;
}

int ga3c_ddpg_nstep_get(ga3c_ddpg* m, float* disc, int64_t count) {
  if (!m || !disc) return fail(GA3C_EINVAL, "null argument");
  HIPCHK(hipSetDevice(m->device));
  std::lock_guard<std::mutex> tl(m->train_mu);
  std::lock_guard<std::mutex> lk(m->mu);
  CHK(nstep_check(m, "nstep_get"));
  if (count != m->cfg.replay_capacity) return fail(GA3C_EINVAL, "disc holds %d floats, not %lld", m->cfg.replay_capacity, (long long)count);
  HIPCHK(hipStreamSynchronize(m->st));
  HIPCHK(hipMemcpy(disc, m->nstep->disc, sizeof(float) * (size_t)count, hipMemcpyDeviceToHost));
  return GA3C_OK;
}

int ga3c_ddpg_nstep_set(ga3c_ddpg* m, const float* disc, int64_t count) {
  if (!m || !disc) return fail(GA3C_EINVAL, "null argument");
  HIPCHK(hipSetDevice(m->device));
  std::lock_guard<std::mutex> tl(m->train_mu);
  std::lock_guard<std::mutex> lk(m->mu);
  CHK(nstep_check(m, "nstep_set"));
  if (count != m->cfg.replay_capacity) return fail(GA3C_EINVAL, "disc holds %d floats, not %lld", m->cfg.replay_capacity, (long long)count);
  for (int64_t i = 0; i < count; ++i)
    if (!(disc[i] >= 0.f && disc[i] <= 1.f)) return fail(GA3C_EINVAL, "disc[%lld] = %g outside [0,1]", (long long)i, disc[i]);
  HIPCHK(hipStreamSynchronize(m->st));
  HIPCHK(hipMemcpy(m->nstep->disc, disc, sizeof(float) * (size_t)count, hipMemcpyHostToDevice));
  return GA3C_OK;
}

// ---- the task of the device actors and the evaluator

namespace {
int task_check(const ga3c_ddpg* m, const char* what, bool idle) {
  if (!m->has_task) return fail(GA3C_ESTATE, "%s: the handle has no task (ga3c_ddpg_task_create)", what);
  if (idle && (m->actors || m->eval))
    return fail(GA3C_ESTATE, "%s: the handle's device actors or evaluation episodes step under its task (destroy them first)", what);
  return GA3C_OK;
}
}  // namespace

int ga3c_ddpg_task_create(ga3c_ddpg* m, int32_t bound, int32_t time_limit, int32_t reset_observation, double reward_scale,
                          double reward_offset) {
  if (!m) return fail(GA3C_EINVAL, "null argument");
  if (bound != GA3C_DDPG_TASK_WRAP && bound != GA3C_DDPG_TASK_CLIP)
    return fail(GA3C_EINVAL, "bound %d is neither GA3C_DDPG_TASK_WRAP nor GA3C_DDPG_TASK_CLIP", bound);
  if (time_limit != GA3C_DDPG_TASK_TERMINAL && time_limit != GA3C_DDPG_TASK_TRUNCATE)
    return fail(GA3C_EINVAL, "time_limit %d is neither GA3C_DDPG_TASK_TERMINAL nor GA3C_DDPG_TASK_TRUNCATE", time_limit);
  if (reset_observation != 0 && reset_observation != 1)
    return fail(GA3C_EINVAL, "reset_observation %d is neither 0 nor 1", reset_observation);
  if (!std::isfinite(reward_scale) || !(reward_scale > 0.0)) return fail(GA3C_EINVAL, "reward_scale %g is not a finite number above 0", reward_scale);
  if (!std::isfinite(reward_offset)) return fail(GA3C_EINVAL, "reward_offset %g is not finite", reward_offset);
  std::lock_guard<std::mutex> tl(m->train_mu);
  if (m->has_task) return fail(GA3C_ESTATE, "the handle has a task already");
  if (m->actors || m->eval)
    return fail(GA3C_ESTATE, "the handle has device actors or evaluation episodes: they step under the task they were made with, so the task comes first");
  m->task = PendulumTask{bound == GA3C_DDPG_TASK_CLIP, time_limit == GA3C_DDPG_TASK_TRUNCATE, reset_observation, reward_scale,
                         reward_offset};
  m->has_task = true;
  return GA3C_OK;
}

int ga3c_ddpg_task_destroy(ga3c_ddpg* m) {
  if (!m) return fail(GA3C_EINVAL, "null argument");
  std::lock_guard<std::mutex> tl(m->train_mu);
  CHK(task_check(m, "task_destroy", true));
  m->has_task = false;
  m->task = PendulumTask::fork();
  return GA3C_OK;
}

int ga3c_ddpg_task_info(ga3c_ddpg* m, int32_t* bound, int32_t* time_limit, int32_t* reset_observation, double* reward_scale,
                        double* reward_offset) {
  if (!m) return fail(GA3C_EINVAL, "null argument");
  std::lock_guard<std::mutex> tl(m->train_mu);
  CHK(task_check(m, "task_info", false));
  const PendulumTask& t = m->task;
  if (bound) *bound = t.clip ? GA3C_DDPG_TASK_CLIP : GA3C_DDPG_TASK_WRAP;
  if (time_limit) *time_limit = t.truncate ? GA3C_DDPG_TASK_TRUNCATE : GA3C_DDPG_TASK_TERMINAL;
  if (reset_observation) *reset_observation = t.reset_observation;
  if (reward_scale) *reward_scale = t.reward_scale;
  if (reward_offset) *reward_offset = t.reward_offset;
  return GA3C_OK;
}

// ---- device actors

using DEnv = ga3c_actors::PendulumBounded;

int ga3c_ddpg_actors_create(ga3c_ddpg* m, int32_t n, int32_t updates, int64_t seed) {
  if (!m) return fail(GA3C_EINVAL, "null argument");
  const int most = std::min(m->cfg.max_batch, m->cfg.replay_capacity);
  if (n < 1 || n > most)
    return fail(GA3C_EINVAL, "%d actors outside [1, min(max_batch %d, replay_capacity %d)]", n, m->cfg.max_batch, m->cfg.replay_capacity);
  if (updates < 1 || updates > ACT_MAX_UPDATES) return fail(GA3C_EINVAL, "updates %d outside [1,%d]", updates, ACT_MAX_UPDATES);
  if (m->L.S != DEnv::S || m->L.A != DEnv::A)
    return fail(GA3C_EINVAL, "the environment has %d state floats and %d actions, the network %d and %d", DEnv::S, DEnv::A, m->L.S, m->L.A);
  HIPCHK(hipSetDevice(m->device));
  std::lock_guard<std::mutex> tl(m->train_mu);
  if (m->actors) return fail(GA3C_ESTATE, "this network has device actors already");
  DActors* a = new (std::nothrow) DActors();
  if (!a) return fail(GA3C_EINVAL, "out of host memory");
  ActState& d = a->d;
  ga3c_actors::Episodes& e = d.ep;
  d.N = n;
  e.ep_cap = n * GA3C_ACTORS_MAX_STEPS;
  d.seed = (uint64_t)seed;
  a->updates = updates;
  a->batch = m->cfg.max_batch;
  a->draw_seed = (uint64_t)seed;
  const size_t Nn = (size_t)n, S = DEnv::S, P = DEnv::P, A = DEnv::A;
  const size_t wn = m->nstep ? (size_t)m->nstep->n : 0;      // n-step returns: every environment's window of n transitions
  a->win.n = (int)wn;
  size_t total = 0;
  m->actors = a;
  if (!ga3c_actors::carve_block(a, 2, &total, [&](auto carve) {
        carve(&d.phys, Nn * P); carve(&d.elapsed, Nn); carve(&d.draws, Nn); carve(&d.obs, Nn * S); carve(&d.action, Nn * A);
        carve(&d.reward, Nn); carve(&d.done, Nn); carve(&d.total_reward, Nn); carve(&d.total_length, Nn); carve(&e.ep_flag, Nn);
        carve(&e.ep_reward, Nn); carve(&e.ep_length, Nn); carve(&e.counts, 2);
        carve(&e.ring_ep_reward, (size_t)e.ep_cap); carve(&e.ring_ep_length, (size_t)e.ep_cap);
        carve(&a->slots, (size_t)m->cfg.max_batch);
        carve(&a->win.f, wn * (2 * S + A + 1) * Nn); carve(&a->win.r, wn * Nn);
      }) ||
      !ga3c_actors::initial_physics<DEnv>(d.seed, Nn, d.phys, d.draws)) {
    (void)hipGetLastError();
    dactors_free(m);
    return fail(GA3C_EHIP, "no memory for %d device actors (%zu bytes)", n, total);
  }
  a->fields = {
      {"phys", d.phys, 8, P, true},    {"elapsed", d.elapsed, 4, 1, true, 1 << 30}, {"draws", d.draws, 8, 1, true},
      {"obs", d.obs, 4, S, true},      {"action", d.action, 4, A, false},           {"reward", d.reward, 8, 1, false},
      {"done", d.done, 4, 1, false},
  };
  return GA3C_OK;
}

int ga3c_ddpg_actors_destroy(ga3c_ddpg* m) { return ga3c_actors::actors_destroy(m); }

namespace {
// The environments' step under the handle's task, one thread each: with a window of n the n-step kernel, from which a row
// leaves when `emit` is set; without one the step kernel, compiled on the fork's task for a handle that has none (8w: the one
// place has_task chooses code, kept for 0.1 us at N = 4096).
void launch_actor_step(ga3c_ddpg* m, DActors* a, int first, bool emit) {
  const ActState& d = a->d;
  const dim3 grid((d.N + ACT_THREADS - 1) / ACT_THREADS), block(ACT_THREADS);
  const int64_t cap = m->cfg.replay_capacity;
  float* pa = m->per ? m->per->pa : nullptr;
  const float* max_pa = m->per ? m->per->max_pa : nullptr;
  if (const int wn = a->win.n)
    hipLaunchKernelGGL(ddpg_actors_nstep_kernel<DEnv>, grid, block, 0, m->st, d, m->task, a->win, first, (int)(a->count % wn),
                       emit ? 1 : 0, (double)m->cfg.gamma, m->ring, m->ring_total % cap, cap, m->nstep->disc, pa, max_pa);
  else {
    const auto kernel = m->has_task ? ddpg_actors_step_kernel<DEnv, false> : ddpg_actors_step_kernel<DEnv, true>;
    hipLaunchKernelGGL(kernel, grid, block, 0, m->st, d, m->task, first, m->ring, m->ring_total % cap, cap, pa, max_pa);
  }
}
}  // namespace

// `steps` actor steps, each followed, when `train` is set and the ring holds MORE than a batch, by `updates` train steps.
// Everything is enqueued without a wait in between: the host knows every launch argument (N transitions per actor step, B rows
// per train step).  One wait at the end, a second only when episodes finished and their records are fetched.
int ga3c_ddpg_actors_run(ga3c_ddpg* m, int32_t steps, float learning_rate, float beta_is, int32_t train, int32_t noise_mode,
                         const float* noise, int64_t* out_stats, float* q_stats) {
  if (!m) return fail(GA3C_EINVAL, "null argument");
  HIPCHK(hipSetDevice(m->device));
  std::lock_guard<std::mutex> tl(m->train_mu);
  DActors* a = m->actors;
  if (!a) return fail(GA3C_ESTATE, "this network has no device actors");
  if (steps < 1 || steps > GA3C_ACTORS_MAX_STEPS) return fail(GA3C_EINVAL, "steps %d outside [1,%d]", steps, GA3C_ACTORS_MAX_STEPS);
  if (noise_mode < 0 || noise_mode > 2) return fail(GA3C_EINVAL, "noise_mode %d not in [0,2]", noise_mode);
  if (noise_mode == GA3C_DDPG_NOISE_GIVEN && !noise) return fail(GA3C_EINVAL, "GA3C_DDPG_NOISE_GIVEN without a noise vector");
  if (train && m->per) CHK(per_check_beta(beta_is));
  const ActState& d = a->d;
  const int N = d.N, B = a->batch;
  int64_t calls = 0;
  {
    std::lock_guard<std::mutex> lk(m->mu);
    HIPCHK(hipMemsetAsync(d.ep.counts, 0, 2 * sizeof(int), m->st));     // the episode ring starts empty
  }
  for (int s = 0; s < steps; ++s) {
    std::lock_guard<std::mutex> lk(m->mu);
    const int first = a->started ? 0 : 1;
    Noise nz;
    if (!first) {                       // step(None) asks for no prediction: no step of the noise process either
      const Input in{reinterpret_cast<const char*>(d.obs), nullptr, 4 * (int64_t)DEnv::S};
      if (m->soft) {                    // 8u: the policy's own sample, row = environment; the last draws stay readable
        uint64_t count;
        CHK(soft_predict_args(m, noise_mode, noise, &nz, &count));
        launch_soft_predict(m, in, N, noise_mode, nz, count, d.action, m->soft->act_eps);
      } else if (a->noise.x && noise_mode == GA3C_DDPG_NOISE_OWN) {      // 8r: every environment's own process, stepped by the kernel
        hipLaunchKernelGGL(ddpg_predict_envnoise_kernel, dim3(tiles(N)), dim3(THREADS), 0, m->st, m->L, (const float*)m->arena[0],
                           in, N, a->noise, d.action);
        ++a->noise.count;
      } else {
        CHK(make_noise(m, noise_mode, noise, &nz));
        hipLaunchKernelGGL(ddpg_predict_kernel, dim3(tiles(N)), dim3(THREADS), 0, m->st, m->L, (const float*)m->arena[0], in, N, nz,
                           d.action);
      }
    }
    const bool emit = !first && a->count >= a->win.n - 1;      // n-step returns: a row leaves the window from transition n - 1 on
    launch_actor_step(m, a, first, emit);
    hipLaunchKernelGGL(ddpg_actors_episodes_kernel, dim3(1), dim3(ga3c_actors::SCAN_THREADS), 0, m->st, d);
    HIPCHK(hipGetLastError());
    a->started = true;
    if (!first) ++a->count;
    if (emit) m->ring_total += N;
    if (train && ring_size(m) > B) {    // ThreadReplay.sample's rule: a batch is drawn from MORE rows than it holds
      for (int k = 0; k < a->updates; ++k) {
        CHK(make_noise(m, noise_mode, noise, &nz));
        if (m->per) {
          CHK(per_enqueue_step(m, B, beta_is, learning_rate, nz));
        } else {
          hipLaunchKernelGGL(ddpg_uniform_slots_kernel, dim3((B + 255) / 256), dim3(256), 0, m->st, ring_size(m), B, a->draw_seed,
                             a->samples, a->slots);
          ++a->samples;
          CHK(enqueue_step(m, Rows{m->ring, a->slots, m->rowf}, B, learning_rate, nz, 6));
        }
        a->slots_rows = B;
        m->last_B = B;
        m->step.fetch_add(1);           // Adam's t is computed per enqueue
        ++calls;
      }
    }
  }
  {
    std::lock_guard<std::mutex> lk(m->mu);
    if (calls) CHK(copy_qstats(m));
    HIPCHK(hipMemcpyAsync(a->h_counts, d.ep.counts, 2 * sizeof(int), hipMemcpyDeviceToHost, m->st));
    HIPCHK(hipEventRecord(m->tev, m->st));
  }
  HIPCHK(hipEventSynchronize(m->tev));
  if (calls) give_qstats(m, q_stats);
  int64_t ne = 0;
  {
    std::lock_guard<std::mutex> lk(m->mu);
    CHK(ga3c_actors::fetch_episodes(a, d.ep, a->h_counts[0], &ne));      // the wait on tev above was the wait for the ring
  }
  if (out_stats) {
    out_stats[0] = (int64_t)N * steps;
    out_stats[1] = calls;
    out_stats[2] = calls * B;
    out_stats[3] = ne;
  }
  return GA3C_OK;
}

int ga3c_ddpg_actors_episodes(ga3c_ddpg* m, double* total_reward, int64_t* total_length, int32_t max, int32_t* count) {
  return ga3c_actors::actors_episodes(m, total_reward, total_length, max, count);
}

namespace {

// get (out) / set (in) of an actor buffer by name; `bytes` must be its size.
int dactors_access(ga3c_ddpg* m, const char* name, void* out, const void* in, int64_t bytes) {
  if (!m || !name || (!out && !in)) return fail(GA3C_EINVAL, "null argument");
  HIPCHK(hipSetDevice(m->device));
  std::lock_guard<std::mutex> tl(m->train_mu);
  DActors* a = m->actors;
  if (!a) return fail(GA3C_ESTATE, "this network has no device actors");
  std::lock_guard<std::mutex> lk(m->mu);
  HIPCHK(hipStreamSynchronize(m->st));
  const ActState& d = a->d;
  const std::string nm(name);
  auto sized = [&](int64_t want) {
    return bytes == want ? GA3C_OK : fail(GA3C_EINVAL, "%s is %lld bytes, not %lld", name, (long long)want, (long long)bytes);
  };
  if (nm == "batch") {                  // of the handle, not per environment: the rows of a train step
    CHK(sized(4));
    if (out) { *static_cast<int32_t*>(out) = a->batch; return GA3C_OK; }
    const int32_t v = *static_cast<const int32_t*>(in);
    if (v < 1 || v > m->cfg.max_batch) return fail(GA3C_EINVAL, "batch %d outside [1, max_batch %d]", v, m->cfg.max_batch);
    a->batch = v;
    return GA3C_OK;
  }
  if (nm == "draw_seed") {              // ... and the seed of its draws without priorities
    CHK(sized(8));
    if (out) *static_cast<int64_t*>(out) = (int64_t)a->draw_seed;
    else a->draw_seed = (uint64_t)*static_cast<const int64_t*>(in);
    return GA3C_OK;
  }
  if (nm == "nstep" || nm == "nstep_count") {       // the window's entries (1 without n-step returns) and the c of the next step
    if (!out) return fail(GA3C_EINVAL, "%s is read only", name);
    if (nm == "nstep") { CHK(sized(4)); *static_cast<int32_t*>(out) = a->win.n ? a->win.n : 1; }
    else { CHK(sized(8)); *static_cast<int64_t*>(out) = a->count; }
    return GA3C_OK;
  }
  if (nm == "slots") {                  // the last draw
    if (!out) return fail(GA3C_EINVAL, "%s is read only", name);
    CHK(sized(4 * (int64_t)a->slots_rows));
    if (a->slots_rows) HIPCHK(hipMemcpy(out, m->per ? m->per->slots : a->slots, (size_t)bytes, hipMemcpyDeviceToHost));
    return GA3C_OK;
  }
  if (nm == "soft_eps") {               // the last GA3C_DDPG_NOISE_OWN / _GIVEN prediction's draws, [N][A]
    if (!m->soft) return fail(GA3C_ESTATE, "%s: the handle has no soft actor-critic (ga3c_ddpg_soft_create)", name);
    if (!out) return fail(GA3C_EINVAL, "%s is read only", name);
    CHK(sized(4 * (int64_t)d.N * m->L.A));
    HIPCHK(hipMemcpy(out, m->soft->act_eps, (size_t)bytes, hipMemcpyDeviceToHost));
    return GA3C_OK;
  }
  if (nm == "noise_x" || nm == "noise_n" || nm == "noise_count") {      // per-environment noise
    EnvNoise& z = a->noise;
    if (!z.x) return fail(GA3C_ESTATE, "%s: the device actors have no per-environment noise (ga3c_ddpg_envnoise_create)", name);
    if (nm == "noise_count") {          // the c of the next prediction
      CHK(sized(8));
      if (out) { *static_cast<int64_t*>(out) = (int64_t)z.count; return GA3C_OK; }
      const int64_t v = *static_cast<const int64_t*>(in);
      if (v < 0) return fail(GA3C_EINVAL, "noise_count %lld is negative", (long long)v);
      z.count = (uint64_t)v;
      return GA3C_OK;
    }
    const size_t cells = (size_t)d.N * m->L.A;
    CHK(sized(4 * (int64_t)cells));
    if (out) {
      HIPCHK(hipMemcpy(out, nm == "noise_x" ? z.x : z.n, (size_t)bytes, hipMemcpyDeviceToHost));
      return GA3C_OK;
    }
    if (nm == "noise_n") return fail(GA3C_EINVAL, "%s is read only", name);
    const float* v = static_cast<const float*>(in);
    for (size_t i = 0; i < cells; ++i)
      if (!std::isfinite(v[i])) return fail(GA3C_EINVAL, "noise_x[%zu] = %g is not finite", i, v[i]);
    HIPCHK(hipMemcpy(z.x, in, (size_t)bytes, hipMemcpyHostToDevice));
    return GA3C_OK;
  }
  return ga3c_actors::field_access(a, d.N, name, out, in, bytes);
}

}  // namespace

// ---- per-environment exploration noise

int ga3c_ddpg_envnoise_create(ga3c_ddpg* m, int64_t seed, int32_t reset_on_done) {
  if (!m) return fail(GA3C_EINVAL, "null argument");
  if (reset_on_done != 0 && reset_on_done != 1) return fail(GA3C_EINVAL, "reset_on_done %d is neither 0 nor 1", reset_on_done);
  HIPCHK(hipSetDevice(m->device));
  std::lock_guard<std::mutex> tl(m->train_mu);
  DActors* a = m->actors;
  if (!a) return fail(GA3C_ESTATE, "envnoise_create: this network has no device actors, whose number sizes the noise state");
  if (a->noise.x) return fail(GA3C_ESTATE, "the device actors have per-environment noise already");
  if (m->soft) return fail(GA3C_ESTATE, "envnoise_create: the soft actor-critic samples its own action for every environment");
  const ga3c_ddpg_config& c = m->cfg;
  if (!(c.flags & GA3C_DDPG_OU_NOISE))
    return fail(GA3C_ESTATE, "envnoise_create: the handle has no noise process to give each environment (GA3C_DDPG_OU_NOISE)");
  const size_t cells = (size_t)a->d.N * m->L.A;
  float* block = nullptr;
  if (hipMalloc((void**)&block, 2 * cells * sizeof(float)) != hipSuccess || hipMemset(block, 0, 2 * cells * sizeof(float)) != hipSuccess) {
    (void)hipFree(block);
    (void)hipGetLastError();
    return fail(GA3C_EHIP, "no memory for the noise of %d environments (%zu bytes)", a->d.N, 2 * cells * sizeof(float));
  }
  EnvNoise& z = a->noise;
  z.x = block;
  z.n = block + cells;
  z.done = a->d.done;
  z.seed = (uint64_t)seed;
  z.count = 0;
  z.sigma = (double)c.ou_sigma;
  z.theta = (double)c.ou_theta;
  z.dt = (double)c.ou_dt;
  z.sqrt_dt = std::sqrt((double)c.ou_dt);
  z.reset = reset_on_done;
  return GA3C_OK;
}

int ga3c_ddpg_envnoise_destroy(ga3c_ddpg* m) {
  if (!m) return fail(GA3C_EINVAL, "null argument");
  HIPCHK(hipSetDevice(m->device));
  std::lock_guard<std::mutex> tl(m->train_mu);
  DActors* a = m->actors;
  if (!a || !a->noise.x) return fail(GA3C_ESTATE, "the device actors have no per-environment noise");
  {
    std::lock_guard<std::mutex> lk(m->mu);
    HIPCHK(hipStreamSynchronize(m->st));
  }
  (void)hipFree(a->noise.x);
  (void)hipGetLastError();
  a->noise = EnvNoise{};
  return GA3C_OK;
}

int ga3c_ddpg_actors_get(ga3c_ddpg* m, const char* name, void* out, int64_t bytes) {
  if (!out) return fail(GA3C_EINVAL, "null argument");
  return dactors_access(m, name, out, nullptr, bytes);
}

int ga3c_ddpg_actors_set(ga3c_ddpg* m, const char* name, const void* in, int64_t bytes) {
  if (!in) return fail(GA3C_EINVAL, "null argument");
  return dactors_access(m, name, nullptr, in, bytes);
}

// ---- evaluation episodes

int ga3c_ddpg_eval_create(ga3c_ddpg* m, int32_t n, int64_t seed, int32_t trace) {
  if (!m) return fail(GA3C_EINVAL, "null argument");
  if (n < 1 || n > EVAL_MAX_ENVS) return fail(GA3C_EINVAL, "%d evaluation environments outside [1,%d]", n, EVAL_MAX_ENVS);
  if (trace != 0 && trace != 1) return fail(GA3C_EINVAL, "trace %d is neither 0 nor 1", trace);
  if (m->L.S != DEnv::S || m->L.A != DEnv::A)
    return fail(GA3C_EINVAL, "the environment has %d state floats and %d actions, the network %d and %d", DEnv::S, DEnv::A, m->L.S, m->L.A);
  HIPCHK(hipSetDevice(m->device));
  std::lock_guard<std::mutex> tl(m->train_mu);
  if (m->eval) return fail(GA3C_ESTATE, "this network has evaluation episodes already");
  Eval* e = new (std::nothrow) Eval();
  if (!e) return fail(GA3C_EINVAL, "out of host memory");
  e->n = n;
  e->trace = trace != 0;
  const size_t Nn = (size_t)n, S = DEnv::S, P = DEnv::P, A = DEnv::A, T = e->trace ? Nn * EVAL_MAX_STEPS : 0;
  // the start states, drawn once: Pendulum::reset on the first two uniforms of environment i's stream under this seed
  std::vector<double> start(Nn * P);
  for (size_t i = 0; i < Nn; ++i) {
    double ru[DEnv::RESET_DRAWS];
    int elapsed = 0;
    for (int k = 0; k < DEnv::RESET_DRAWS; ++k) ru[k] = ga3c_uniform::actor_uniform((uint64_t)seed, i, (uint64_t)k);
    DEnv::reset(&start[i * P], &elapsed, ru);
  }
  size_t total = 0;
  m->eval = e;
  if (!ga3c_actors::carve_block(e, (int)(Nn * sizeof(double) / sizeof(int)), &total, [&](auto carve) {
        carve(&e->start, Nn * P); carve(&e->phys, Nn * P); carve(&e->total, Nn);
        carve(&e->tr.phys, T * P); carve(&e->tr.obs, T * S); carve(&e->tr.action, T * A); carve(&e->tr.reward, T);
      }) ||
      hipMemcpy(e->start, start.data(), start.size() * sizeof(double), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(e->phys, start.data(), start.size() * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) {
    (void)hipGetLastError();
    eval_free(m);
    return fail(GA3C_EHIP, "no memory for %d evaluation environments (%zu bytes)", n, total);
  }
  if (!e->trace) e->tr = EvalTrace{nullptr, nullptr, nullptr, nullptr};      // (carved with no elements: not to be stored to)
  e->fields = {{"start", e->start, 8, P, true}, {"phys", e->phys, 8, P, false}};
  if (e->trace) {
    e->fields.push_back({"trace_phys", e->tr.phys, 8, EVAL_MAX_STEPS * P, false});
    e->fields.push_back({"trace_obs", e->tr.obs, 4, EVAL_MAX_STEPS * S, false});
    e->fields.push_back({"trace_action", e->tr.action, 4, EVAL_MAX_STEPS * A, false});
    e->fields.push_back({"trace_reward", e->tr.reward, 8, EVAL_MAX_STEPS, false});
  }
  return GA3C_OK;
}

int ga3c_ddpg_eval_destroy(ga3c_ddpg* m) {
  if (!m) return fail(GA3C_EINVAL, "null argument");
  HIPCHK(hipSetDevice(m->device));
  std::lock_guard<std::mutex> tl(m->train_mu);
  if (!m->eval) return fail(GA3C_ESTATE, "this network has no evaluation episodes");
  {
    std::lock_guard<std::mutex> lk(m->mu);
    HIPCHK(hipStreamSynchronize(m->st));
  }
  eval_free(m);
  return GA3C_OK;
}

namespace {
// An episode of `steps` steps under the handle's task for every evaluation environment, by the handle's policy on the value
// arena or the target arena.
void launch_eval(ga3c_ddpg* m, Eval* e, int steps, bool target) {
  const auto kernel = m->soft ? ddpg_eval_kernel<DEnv, SoftPolicy> : ddpg_eval_kernel<DEnv, DetPolicy>;
  hipLaunchKernelGGL(kernel, dim3(tiles(e->n)), dim3(THREADS), 0, m->st, m->L, (const float*)m->arena[target ? 1 : 0], e->n, steps,
                     m->task, (const double*)e->start, e->total, e->phys, e->tr);
}
}  // namespace

// One launch, one copy back, one wait.  The kernel stands on the handle's stream between whole train steps, so the arena it
// reads is that of exactly one of them.
int ga3c_ddpg_eval_run(ga3c_ddpg* m, int32_t steps, int32_t target, double* total_reward) {
  if (!m || !total_reward) return fail(GA3C_EINVAL, "null argument");
  HIPCHK(hipSetDevice(m->device));
  std::lock_guard<std::mutex> tl(m->train_mu);
  Eval* e = m->eval;
  if (!e) return fail(GA3C_ESTATE, "this network has no evaluation episodes");
  if (steps < 1 || steps > EVAL_MAX_STEPS) return fail(GA3C_EINVAL, "steps %d outside [1,%d]", steps, EVAL_MAX_STEPS);
  if (target != 0 && target != 1) return fail(GA3C_EINVAL, "target %d is neither 0 nor 1", target);
  {
    std::lock_guard<std::mutex> lk(m->mu);
    HIPCHK(hipEventRecord(m->t0, m->st));
    launch_eval(m, e, (int)steps, target != 0);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(m->t1, m->st));
    HIPCHK(hipMemcpyAsync(e->h_total(), e->total, sizeof(double) * e->n, hipMemcpyDeviceToHost, m->st));
    HIPCHK(hipEventRecord(m->tev, m->st));
  }
  HIPCHK(hipEventSynchronize(m->tev));
  e->timed = true;
  memcpy(total_reward, e->h_total(), sizeof(double) * e->n);
  return GA3C_OK;
}

namespace {

int eval_access(ga3c_ddpg* m, const char* name, void* out, const void* in, int64_t bytes) {
  if (!m || !name || (!out && !in)) return fail(GA3C_EINVAL, "null argument");
  HIPCHK(hipSetDevice(m->device));
  std::lock_guard<std::mutex> tl(m->train_mu);
  Eval* e = m->eval;
  if (!e) return fail(GA3C_ESTATE, "this network has no evaluation episodes");
  if (!e->trace && strncmp(name, "trace_", 6) == 0) return fail(GA3C_ESTATE, "%s: the evaluation episodes keep no trace (trace = 1 at create)", name);
  std::lock_guard<std::mutex> lk(m->mu);
  HIPCHK(hipStreamSynchronize(m->st));
  if (strcmp(name, "elapsed_ms") == 0) {             // the last run's kernel between two events on the handle's stream
    if (!out) return fail(GA3C_EINVAL, "%s is read only", name);
    if (bytes != 4) return fail(GA3C_EINVAL, "%s is 4 bytes, not %lld", name, (long long)bytes);
    if (!e->timed) return fail(GA3C_ESTATE, "%s: no evaluation has run", name);
    HIPCHK(hipEventElapsedTime(static_cast<float*>(out), m->t0, m->t1));
    return GA3C_OK;
  }
  return ga3c_actors::field_access(e, e->n, name, out, in, bytes);
}

}  // namespace

int ga3c_ddpg_eval_get(ga3c_ddpg* m, const char* name, void* out, int64_t bytes) {
  if (!out) return fail(GA3C_EINVAL, "null argument");
  return eval_access(m, name, out, nullptr, bytes);
}

int ga3c_ddpg_eval_set(ga3c_ddpg* m, const char* name, const void* in, int64_t bytes) {
  if (!in) return fail(GA3C_EINVAL, "null argument");
  return eval_access(m, name, nullptr, in, bytes);
}

}  // extern "C"
