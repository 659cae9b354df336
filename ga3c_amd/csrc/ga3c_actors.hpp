// ga3c_actors.hpp -- actors that live on the device (Config.DEVICE_AGENTS): N environments, their rollouts and
// their training rows stay in HBM, and a vector-state network's handle steps them with the kernels below between its own
// predict and train kernels, which it reaches through the Net hooks of ga3c_vecnet.hpp (rows, enqueue_train).  Nothing here
// asks which network it serves; the one game-specific piece is the Env parameter (CartPole and Pendulum below).
//
// One actor step of the handle, all on its one stream:
//   rows(PREDICT) on the observation buffer             the network's own kernel, untouched
//   actors_step_kernel<Env>   one thread per environment: draw the action (action 0 on an environment's first ever step;
//                             Env::CONTINUOUS: no draw, the action is the prediction row, the zero vector on the first
//                             step), f64 physics, reward, done, append to the rollout ring, cut the rollout (done, or
//                             time_count == TIME_MAX), its returns, the episode record and the reset
//   actors_compact_kernel<Env>  one workgroup: an exclusive scan over the environments' cut rollouts and finished episodes
//                             lays the rows out as one batch in environment order (offsets into the rings, y_r, one-hot
//                             actions or the action vectors) and appends the episode records to the episode ring in
//                             environment order
//   enqueue_train on the batch, when the step cut any rollout
// The host reads the batch's row count between the two halves (one 12-byte copy and an event wait per step): the train
// kernels take their row count as an argument.  No kernel is persistent, none waits for another workgroup, none launches
// from the device, and every loop is bounded by an argument.  No float atomics: the same seed gives the same bits.
//
// What the step restates is ProcessAgent.run_episode / run over EnvironmentCart.Environment (EnvironmentPend.Environment for
// Pendulum) with ga3c_returns_fork and ga3c_select_action (ga3c_host.cpp); tests/device_agents_oracle.py and
// tests/device_pendulum_oracle.py are the same statement in numpy.  The f64 arithmetic is
// compiled with contraction off, as the host library's is.  The uniforms are the one deviation: a stateless function of
// (seed, environment, draw number), actor_uniform (ga3c_uniform.hpp).
//
// The DDPG handle's actors (ga3c_ddpg.hip) write transitions into a replay ring where these cut rollouts, in
// kernels of their own, and share what does not ask which of the two a step produces: Episodes, load_physics /
// store_physics, finish_episode and the episode scan on the device; ActorsCore and the functions over it on the host.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <deque>
#include <new>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "ga3c_uniform.hpp"
#include "ga3c_vecnet.hpp"

namespace ga3c_actors {

using namespace ga3c_vecnet;

constexpr int STEP_THREADS = 256;
constexpr int SCAN_THREADS = 1024;
constexpr int MAX_STEPS = GA3C_ACTORS_MAX_STEPS;     // actor steps of one actors_run call: bounds the episode ring

using ga3c_uniform::actor_uniform;          // u(seed, environment, draw number), shared with prioritised replay
using ga3c_uniform::mix64;

// ga3c_select_action (ga3c_host.cpp): sequential f64 cumulative sum of the f32 policy, the first index with
// u < cdf[i] / cdf[n - 1], clamped to n - 1.  The sum is run twice instead of being kept: the same additions, the same bits.
__device__ inline int select_action(const float* p, int n, double u) {
#pragma clang fp contract(off)
  double last = 0.0;
  for (int i = 0; i < n; ++i) last += (double)p[i];
  double acc = 0.0;
  for (int i = 0; i < n; ++i) {
    acc += (double)p[i];
    if (u < acc / last) return i;
  }
  return n - 1;
}

// An Env states: S observation floats, P f64 physics values, A actions (CONTINUOUS: the width of the action vector),
// RESET_DRAWS uniforms per reset, step (an action index, or CONTINUOUS the f32 action vector), observe (physics -> what the
// network reads) and reset.

// gym's CartPole-v0 under its TimeLimit, as EnvironmentCart.py restates it, with the reference's wrapper: reward r * 0.005 - 1.
struct CartPole {
  static constexpr int S = 4;          // observation = f32 of the physics
  static constexpr int P = 4;
  static constexpr int A = 2;
  static constexpr int RESET_DRAWS = 4;
  static constexpr bool CONTINUOUS = false;

  __device__ static void step(double* s, int action, int* elapsed, double* reward, int* done) {
#pragma clang fp contract(off)
    const double gravity = 9.8, masscart = 1.0, masspole = 0.1, length = 0.5, force_mag = 10.0, tau = 0.02;
    const double total_mass = masspole + masscart, polemass_length = masspole * length;
    const double theta_limit = 12 * 2 * 3.141592653589793 / 360, x_limit = 2.4;
    double x = s[0], x_dot = s[1], theta = s[2], theta_dot = s[3];
    const double force = action == 1 ? force_mag : -force_mag;
    const double costheta = cos(theta), sintheta = sin(theta);
    const double temp = (force + polemass_length * (theta_dot * theta_dot) * sintheta) / total_mass;
    const double thetaacc = (gravity * sintheta - costheta * temp) /
                            (length * (4.0 / 3.0 - masspole * (costheta * costheta) / total_mass));
    const double xacc = temp - polemass_length * thetaacc * costheta / total_mass;
    x = x + tau * x_dot;
    x_dot = x_dot + tau * xacc;
    theta = theta + tau * theta_dot;
    theta_dot = theta_dot + tau * thetaacc;
    s[0] = x; s[1] = x_dot; s[2] = theta; s[3] = theta_dot;
    *elapsed += 1;
    const bool fell = x < -x_limit || x > x_limit || theta < -theta_limit || theta > theta_limit;
    *done = (fell || *elapsed >= 200) ? 1 : 0;
    *reward = 1.0 * 0.005 - 1.0;
  }

  __device__ static void observe(const double* s, float* obs) {
    for (int k = 0; k < S; ++k) obs[k] = (float)s[k];
  }

  // U(-0.05, 0.05)^4 as numpy draws it, low + (high - low) u; the observation is left alone
  __host__ __device__ static void reset(double* s, int* elapsed, const double* u) {
#pragma clang fp contract(off)
    const double low = -0.05, high = 0.05;
    for (int k = 0; k < 4; ++k) s[k] = low + (high - low) * u[k];
    *elapsed = 0;
  }
};

// gym's Pendulum-v0 under its TimeLimit, as EnvironmentPend.py restates it (Pendulum.step / reset), with the reference's
// wrapper (Environment.step): torque 2 a, reward -cost * 0.005 - 1.  Physics (th, thdot); observation [cos th, sin th, thdot].
// Two branches of the host's statement are absent because the device cannot reach them: the action is the
// network's atan2f(Y, X) / PI_F, which lies in [-1, 1] (the zero vector on the first step), so check_bounds(a, 1, -1,
// turnaround) returns it as it is, and 2 a lies in [-2, 2], so clip(u, -2, 2) does too.
struct Pendulum {
  static constexpr int S = 3;
  static constexpr int P = 2;
  static constexpr int A = 1;
  static constexpr int RESET_DRAWS = 2;
  static constexpr bool CONTINUOUS = true;

  // numpy's float remainder: ((x + pi) % (2 pi)) - pi
  __device__ static double angle_normalize(double x) {
#pragma clang fp contract(off)
    const double pi = 3.141592653589793;
    double m = fmod(x + pi, 2 * pi);
    if (m < 0) m += 2 * pi;
    return m - pi;
  }

  // gym's step without its wrapper: the physics move, `elapsed` counts, -> the cost.
  // T: float, the action vector itself; double (PendulumBounded below), the action as check_bounds hands it on
  template <class T>
  __device__ static double advance(double* s, const T* a, int* elapsed) {
#pragma clang fp contract(off)
    const double pi = 3.141592653589793, dt = 0.05, max_speed = 8.0;
    const double th = s[0], thdot = s[1];
    const double u = (double)a[0] * 2.0;
    const double an = angle_normalize(th);
    const double cost = an * an + 0.1 * (thdot * thdot) + 0.001 * (u * u);
    double newthdot = thdot + (-15.0 * sin(th + pi) + 3.0 * u) * dt;      // -3 g / (2 l) = -15, 3 / (m l^2) = 3
    const double newth = th + newthdot * dt;
    newthdot = newthdot < -max_speed ? -max_speed : (newthdot > max_speed ? max_speed : newthdot);   // after th' has used it
    s[0] = newth; s[1] = newthdot;
    *elapsed += 1;
    return cost;
  }

  template <class T>
  __device__ static void step(double* s, const T* a, int* elapsed, double* reward, int* done) {
#pragma clang fp contract(off)
    const double cost = advance(s, a, elapsed);
    *done = *elapsed >= 200 ? 1 : 0;
    *reward = -cost * 0.005 - 1.0;
  }

  __device__ static void observe(const double* s, float* obs) {
    obs[0] = (float)cos(s[0]);
    obs[1] = (float)sin(s[0]);
    obs[2] = (float)s[1];
  }

  // th ~ U(-pi, pi), thdot ~ U(-1, 1) as numpy draws them, low + (high - low) u; the observation is left alone
  __host__ __device__ static void reset(double* s, int* elapsed, const double* u) {
#pragma clang fp contract(off)
    const double pi = 3.141592653589793;
    s[0] = -pi + (pi - -pi) * u[0];
    s[1] = -1.0 + (1.0 - -1.0) * u[1];
    *elapsed = 0;
  }
};

// What "Pendulum-v0" means to the DDPG handle's device actors and evaluator (ga3c_ddpg_task_create, DESIGN.md 8t, 8w;
// tests/ddpg_task_oracle.py is the same statement), by value in the arguments of their kernels.
struct PendulumTask {
  int clip;                  // the action is clipped to [-1, 1], not wrapped
  int truncate;              // the time limit ends the episode and is no terminal state: the row's done stays 0
  int reset_observation;     // a reset rewrites the observation from the reset physics
  double reward_scale, reward_offset;      // reward = -cost scale + offset

  // The fork's task, EnvironmentPend.Environment's: what a handle steps under until ga3c_ddpg_task_create says otherwise.
  static constexpr PendulumTask fork() { return {0, 0, 0, 0.005, -1.0}; }
};

// Pendulum under an action that can leave [-1, 1]: the DDPG actor's tanh output plus Ornstein-Uhlenbeck noise (Config.DEVICE_DDPG,
// DESIGN.md 8l).  check_bounds(a, 1, -1, turnaround) is reachable there and is applied as EnvironmentPend.check_bounds applies
// it, in f64 to the f32 action; its operands are positive, so fmod is Python's %.  What it returns lies in [-1, 1], so
// clip(u, -2, 2) stays an identity and stays absent.  The arithmetic after it is Pendulum's.
struct PendulumBounded : Pendulum {
  __device__ static double check_bounds(float a) {
#pragma clang fp contract(off)
    double v = (double)a;
    if (v < -1.0) v = 1.0 - fmod(-1.0 - v, 2.0);
    if (v > 1.0) v = fmod(v - 1.0, 2.0) - 1.0;
    return v;
  }

  // check_bounds(a, 1, -1, turnaround=False): 2 clip(a) is gym's clip(2 a, -2, 2) exactly, which stays absent here too
  __device__ static double clip_bounds(float a) {
    const double v = (double)a;
    return v < -1.0 ? -1.0 : (v > 1.0 ? 1.0 : v);
  }

  // The step under a task (PendulumTask above): its bound, then Pendulum's physics and cost, its reward.  *ended:
  // the time limit has been reached, whatever the task makes of that.
  __device__ static void step(double* s, const float* a, const PendulumTask& task, int* elapsed, double* reward, int* ended) {
#pragma clang fp contract(off)
    const double bounded = task.clip ? clip_bounds(a[0]) : check_bounds(a[0]);
    const double cost = Pendulum::advance(s, &bounded, elapsed);
    *ended = *elapsed >= 200 ? 1 : 0;
    *reward = -cost * task.reward_scale + task.reward_offset;
  }
};

// The episodes a step finishes and the ring that keeps their records for the host: the part of the device state that the
// rollout actors (State below) and the DDPG actors (ActState, ga3c_ddpg.hip) both hold.
struct Episodes {
  int ep_cap;
  int* ep_flag;              // per environment: this step finished an episode, and its record
  double* ep_reward;
  long long* ep_length;
  int* counts;               // [2]: records in the episode ring, episodes this step finished
  double* ring_ep_reward;    // [ep_cap] the episode ring, in the order the episodes finished
  long long* ring_ep_length;
};

// Everything the kernels touch, by device address.  Per environment unless said otherwise; T1 = TIME_MAX + 1.
struct State {
  int N, T1, S, P, A, time_max;
  double gamma;
  uint64_t seed;
  double* phys;              // [N][P] f64 physics
  int* elapsed;
  int* time_count;
  int* started;              // 0 until the first ever step: no observation yet (the host's current_state is None)
  uint64_t* draws;           // uniforms drawn so far
  float* obs;                // [N][S] what the network reads
  float* ring_x;             // [N][T1][S] the rollout: states, ...
  int* ring_a;               // [N][T1]    actions (Env::CONTINUOUS: none, ring_av [N][T1][A] f32 action vectors), ...
  float* ring_av;
  double* ring_r;            // [N][T1]    rewards; row t of the rollout is slot (head + t) % T1
  int* head;
  int* rlen;
  double* reward_sum;        // since the last cut
  double* total_reward;      // of the running episode, as ProcessAgent.run counts them
  long long* total_length;
  float* p; float* v; float* z;   // [N][A], [N], [N][ZW]: the last prediction
  double* u;                 // the last step's uniform (-1: none drawn), action, reward, done
  int* action;               // (Env::CONTINUOUS: none, action_v [N][A] f32)
  float* action_v;
  double* reward;
  int* done;
  int* cut;                  // rows of the rollout this step cut (0: none), where it starts in the ring, its returns [N][T1]
  int* cut_head;
  float* cut_y;
  int64_t* off;              // [N T1] the batch: byte offsets of its rows from ring_x, environment order
  float* by;                 // [N T1] y_r     (the handle's train staging)
  float* ba;                 // [N T1][A] one-hot (Env::CONTINUOUS: the action vectors)
  int* counts;               // [3]: rows of the batch, then ep.counts' two: what the host copies after a step
  Episodes ep;               // ep.counts = counts + 1
};

// The P physics values and `elapsed` of environment i, into and out of a step kernel's registers.
template <int P>
__device__ __forceinline__ void load_physics(const double* phys, const int* elapsed, int i, double* s, int& el) {
  for (int k = 0; k < P; ++k) s[k] = phys[(size_t)i * P + k];
  el = elapsed[i];
}

template <int P>
__device__ __forceinline__ void store_physics(double* phys, int* elapsed, int i, const double* s, int el) {
  for (int k = 0; k < P; ++k) phys[(size_t)i * P + k] = s[k];
  elapsed[i] = el;
}

// The end of environment i's episode: its record for this step's scan, the running totals back to zero, and the reset on the
// next RESET_DRAWS uniforms of the environment in draw order.  The observation is left alone.
template <class Env>
__device__ __forceinline__ void finish_episode(const Episodes& e, int i, uint64_t seed, double& total, long long& length,
                                               uint64_t& draws, double* s, int& elapsed) {
#pragma clang fp contract(off)
  e.ep_flag[i] = 1;
  e.ep_reward[i] = total;
  e.ep_length[i] = length;
  total = 0.0;
  length = 0;
  double ru[Env::RESET_DRAWS];
  for (int k = 0; k < Env::RESET_DRAWS; ++k) ru[k] = actor_uniform(seed, (uint64_t)i, draws++);
  Env::reset(s, &elapsed, ru);
}

template <class Env>
__global__ __launch_bounds__(STEP_THREADS) void actors_step_kernel(State a) {
#pragma clang fp contract(off)
  const int i = blockIdx.x * STEP_THREADS + threadIdx.x;
  if (i >= a.N) return;
  constexpr int S = Env::S, P = Env::P, A = Env::A;
  const int T1 = a.T1;
  double s[P];
  int elapsed;
  load_physics<P>(a.phys, a.elapsed, i, s, elapsed);
  uint64_t draws = a.draws[i];
  const bool started = a.started[i] != 0;
  a.cut[i] = 0;
  a.ep.ep_flag[i] = 0;

  [[maybe_unused]] int action = 0;
  [[maybe_unused]] float av[A];                          // CONTINUOUS: the action is the prediction row, no draw; step(None) is the zero vector
  double u = -1.0;
  double reward;
  int done;
  if constexpr (Env::CONTINUOUS) {
    for (int j = 0; j < A; ++j) {
      av[j] = started ? a.p[(size_t)i * A + j] : 0.f;
      a.action_v[(size_t)i * A + j] = av[j];
    }
    Env::step(s, av, &elapsed, &reward, &done);
  } else {
    if (started) {
      u = actor_uniform(a.seed, (uint64_t)i, draws++);
      action = select_action(a.p + (size_t)i * a.A, a.A, u);
    }
    Env::step(s, action, &elapsed, &reward, &done);
    a.action[i] = action;
  }
  a.u[i] = u;
  a.reward[i] = reward;
  a.done[i] = done;
  float* obs = a.obs + (size_t)i * S;
  if (!started) {                       // the host's step(None): no experience, and its `done` is not looked at
    store_physics<P>(a.phys, a.elapsed, i, s, elapsed);
    Env::observe(s, obs);
    a.started[i] = 1;
    return;
  }

  int head = a.head[i], rlen = a.rlen[i], tc = a.time_count[i];
  if (rlen < T1) {                      // (always: a rollout is cut at T1 rows at the latest)
    const int slot = (head + rlen) % T1;
    float* row = a.ring_x + ((size_t)i * T1 + slot) * S;
    for (int k = 0; k < S; ++k) row[k] = obs[k];
    if constexpr (Env::CONTINUOUS) {
      for (int j = 0; j < A; ++j) a.ring_av[((size_t)i * T1 + slot) * A + j] = av[j];
    } else {
      a.ring_a[(size_t)i * T1 + slot] = action;
    }
    a.ring_r[(size_t)i * T1 + slot] = reward;
    ++rlen;
  }
  Env::observe(s, obs);
  double rsum = a.reward_sum[i] + reward;

  if (done || tc == a.time_max || rlen == T1) {
    // ga3c_returns_fork, DISCOUNTING without intermediate rewards: the last row keeps its reward, the others get
    // gamma^(T-1-t) terminal_reward by sequential products, terminal_reward being the last reward
    const int T = rlen;
    float* y = a.cut_y + (size_t)i * T1;
    y[T - 1] = (float)a.ring_r[(size_t)i * T1 + (head + T - 1) % T1];
    double acc = reward;
    for (int t = T - 2; t >= 0; --t) {
      acc = a.gamma * acc;
      y[t] = (float)acc;
    }
    a.cut[i] = T;
    a.cut_head[i] = head;
    double total = a.total_reward[i] + rsum;
    long long length = a.total_length[i] + (T + 1);
    rsum = 0.0;
    tc = 0;
    if (done) {
      finish_episode<Env>(a.ep, i, a.seed, total, length, draws, s, elapsed);
      head = 0;
      rlen = 0;
    } else {                            // the last experience is row 0 of the next rollout
      head = (head + T - 1) % T1;
      rlen = 1;
    }
    a.total_reward[i] = total;
    a.total_length[i] = length;
  }
  if (!done) tc += 1;                   // (a new episode starts at time_count 0)
  store_physics<P>(a.phys, a.elapsed, i, s, elapsed);
  a.draws[i] = draws;
  a.head[i] = head;
  a.rlen[i] = rlen;
  a.time_count[i] = tc;
  a.reward_sum[i] = rsum;
}

// Inclusive Hillis-Steele scan over the threads of a workgroup of SCAN_THREADS, of K int[SCAN_THREADS] arrays in LDS at once:
// thread t has stored its element of each.  Ten rounds, each ending in a barrier.
template <int K>
__device__ __forceinline__ void scan_threads(int* const (&s)[K], int t) {
  __syncthreads();
  for (int d = 1; d < SCAN_THREADS; d <<= 1) {
    int add[K];
    for (int k = 0; k < K; ++k) add[k] = t >= d ? s[k][t - d] : 0;
    __syncthreads();
    for (int k = 0; k < K; ++k) s[k][t] += add[k];
    __syncthreads();
  }
}

// A step's finished episodes go to the episode ring in environment order in three parts: count_episodes, a scan_threads
// that has `sep` among its arrays, append_episodes.  EpisodeScan is what thread t carries from the first to the last: the
// environments it owns, [lo, hi) = [t c, (t + 1) c) clipped to N, c = ceil(N / SCAN_THREADS) (the last owning thread may have
// fewer than c and the threads after it none), the records in the ring before this step and the episodes its own finished.
struct EpisodeScan {
  int lo, hi, ep0, eps;
};

__device__ __forceinline__ EpisodeScan count_episodes(const Episodes& e, int N, int t, int* sep) {
  const int chunk = (N + SCAN_THREADS - 1) / SCAN_THREADS, lo = min(N, t * chunk);
  EpisodeScan c{lo, min(N, lo + chunk), e.counts[0], 0};
  for (int i = c.lo; i < c.hi; ++i) c.eps += e.ep_flag[i];
  sep[t] = c.eps;
  return c;
}

// Every thread read counts[0] before the scan, in count_episodes; the last thread writes it here, after the scan.  Each of
// the scan's barriers is a workgroup fence as well, so every read has returned before any thread is past the first of them:
// no barrier between the append and the write, in either kernel.
__device__ __forceinline__ void append_episodes(const Episodes& e, const EpisodeScan& c, int t, const int* sep) {
  int ep = c.ep0 + sep[t] - c.eps;
  for (int i = c.lo; i < c.hi; ++i)
    if (e.ep_flag[i]) {
      if (ep < e.ep_cap) {
        e.ring_ep_reward[ep] = e.ep_reward[i];
        e.ring_ep_length[ep] = e.ep_length[i];
      }
      ++ep;
    }
  if (t == SCAN_THREADS - 1) {
    e.counts[0] = min(c.ep0 + sep[t], e.ep_cap);
    e.counts[1] = sep[t];
  }
}

// The three in a row, for a kernel of one workgroup of SCAN_THREADS that scans nothing else; sep: its int[SCAN_THREADS] in LDS.
__device__ __forceinline__ void scan_append_episodes(const Episodes& e, int N, int* sep) {
  const int t = threadIdx.x;
  const EpisodeScan c = count_episodes(e, N, t, sep);
  int* const arrays[1] = {sep};
  scan_threads(arrays, t);
  append_episodes(e, c, t, sep);
}

// One workgroup.  The scan over the threads' sums gives each its first batch row and, with it, its first episode record.
template <class Env>
__global__ __launch_bounds__(SCAN_THREADS) void actors_compact_kernel(State a) {
  __shared__ int srow[SCAN_THREADS];
  __shared__ int sep[SCAN_THREADS];
  const int t = threadIdx.x;
  const EpisodeScan c = count_episodes(a.ep, a.N, t, sep);
  int rows = 0;
  for (int i = c.lo; i < c.hi; ++i) rows += a.cut[i];
  srow[t] = rows;
  int* const arrays[2] = {srow, sep};
  scan_threads(arrays, t);
  int row = srow[t] - rows;
  const int T1 = a.T1, A = a.A, cap = a.N * T1;
  for (int i = c.lo; i < c.hi; ++i) {
    const int T = min(a.cut[i], T1), h = a.cut_head[i];
    for (int k = 0; k < T && row < cap; ++k, ++row) {
      const int slot = (h + k) % T1;
      a.off[row] = ((int64_t)i * T1 + slot) * a.S * (int64_t)sizeof(float);
      a.by[row] = a.cut_y[(size_t)i * T1 + k];
      if constexpr (Env::CONTINUOUS) {
        for (int j = 0; j < A; ++j) a.ba[(size_t)row * A + j] = a.ring_av[((size_t)i * T1 + slot) * A + j];
      } else {
        const int act = a.ring_a[(size_t)i * T1 + slot];
        for (int j = 0; j < A; ++j) a.ba[(size_t)row * A + j] = j == act ? 1.0f : 0.0f;
      }
    }
  }
  if (t == SCAN_THREADS - 1) a.counts[0] = srow[t];
  append_episodes(a.ep, c, t, sep);
}

// ------------------------------------------------------------------ host side

constexpr int32_t NO_BOUND = -1;

struct Field {               // a buffer actors_get / actors_set reach by name
  const char* name;
  void* dev;
  size_t elem;               // bytes of an element
  size_t per_env;            // elements per environment
  bool settable;
  int32_t hi = NO_BOUND;     // a settable int32 field: its values lie in [0, hi]; NO_BOUND: no check
};

// What a handle's actors keep on the host whichever kernels step them: Actors below, DActors of ga3c_ddpg.hip.
struct ActorsCore {
  char* block = nullptr;     // every device buffer the derived struct carved
  int* h_counts = nullptr;   // pinned: the counts the host copies after a step
  std::vector<Field> fields;
  std::deque<std::pair<double, long long>> finished;   // episode records not yet drained
};

struct Actors : ActorsCore {
  State d{};                 // by / ba are the handle's, everything else lies in `block`
  int batch_rows = 0;        // rows of the last step's batch
};

template <class T>           // T: Actors or DActors
void actors_free(T* a) {
  if (!a) return;
  (void)hipFree(a->block);
  (void)hipHostFree(a->h_counts);
  (void)hipGetLastError();
  delete a;
}

// One zeroed device block for every buffer that `list` names, and `counts` pinned ints.  list(carve) calls carve(&pointer,
// elements) once per buffer and is run twice: for the sizes, then for the addresses (each buffer 16-byte aligned).
// -> false: no memory; *total is the block's size either way.
template <class List>
bool carve_block(ActorsCore* a, int counts, size_t* total, List list) {
  for (int pass = 0; pass < 2; ++pass) {
    size_t at = 0;
    list([&](auto** p, size_t count) {
      using T = std::remove_pointer_t<std::remove_pointer_t<decltype(p)>>;
      if (pass) *p = reinterpret_cast<T*>(a->block + at);
      at += (count * sizeof(T) + 15) / 16 * 16;
    });
    if (pass) break;
    *total = at;
    if (hipMalloc((void**)&a->block, at) != hipSuccess || hipMemset(a->block, 0, at) != hipSuccess ||
        hipHostMalloc((void**)&a->h_counts, counts * sizeof(int), hipHostMallocDefault) != hipSuccess)
      return false;
  }
  return true;
}

// An environment starts as the host's does: reset() when it is made (draws 0..RESET_DRAWS-1) and again when its first
// episode begins (the next RESET_DRAWS), no observation.  -> false: a copy to the device failed.
template <class Env>
bool initial_physics(uint64_t seed, size_t n, double* d_phys, uint64_t* d_draws) {
  std::vector<double> phys(n * Env::P);
  std::vector<uint64_t> draws(n, 2 * Env::RESET_DRAWS);
  for (size_t i = 0; i < n; ++i) {
    double ru[Env::RESET_DRAWS];
    int elapsed = 0;
    for (int k = 0; k < Env::RESET_DRAWS; ++k) ru[k] = actor_uniform(seed, i, (uint64_t)(Env::RESET_DRAWS + k));
    Env::reset(&phys[i * Env::P], &elapsed, ru);
  }
  return hipMemcpy(d_phys, phys.data(), phys.size() * sizeof(double), hipMemcpyHostToDevice) == hipSuccess &&
         hipMemcpy(d_draws, draws.data(), draws.size() * sizeof(uint64_t), hipMemcpyHostToDevice) == hipSuccess;
}

// m: a Net-derived handle with cfg and an `Actors* actors` member.  Its train staging d_y / d_a holds the batch's y_r and a.
template <class Env, class N>
int actors_create(N* m, int n, int time_max, double discount, int64_t seed) {
  if (!m) return fail(GA3C_EINVAL, "null argument");
  std::lock_guard<std::mutex> tl(m->train_mu);
  if (m->actors) return fail(GA3C_ESTATE, "this network has device actors already");
  if (m->S != Env::S || m->A != Env::A)
    return fail(GA3C_EINVAL, "the environment has %d state floats and %d actions, the network %d and %d", Env::S, Env::A, m->S, m->A);
  if (n < 1 || time_max < 1) return fail(GA3C_EINVAL, "n %d and time_max %d must be at least 1", n, time_max);
  const int64_t T1 = (int64_t)time_max + 1;
  if ((int64_t)n * T1 > m->max_batch)
    return fail(GA3C_EINVAL, "%d actors x (time_max + 1 = %lld) rows exceed the network's max_batch %d", n, (long long)T1, m->max_batch);
  HIPCHK(hipSetDevice(m->device));
  Actors* a = new (std::nothrow) Actors();
  if (!a) return fail(GA3C_EINVAL, "out of host memory");
  State& d = a->d;
  Episodes& e = d.ep;
  d.N = n; d.T1 = (int)T1; d.S = m->S; d.P = Env::P; d.A = m->A; d.time_max = time_max; e.ep_cap = n * MAX_STEPS;
  d.gamma = discount;
  d.seed = (uint64_t)seed;
  const size_t Nn = (size_t)n, S = (size_t)m->S, P = (size_t)Env::P, A = (size_t)m->A, R = Nn * (size_t)T1, ZW = (size_t)m->ZW;
  const size_t AI = Env::CONTINUOUS ? 0 : 1, AV = Env::CONTINUOUS ? A : 0;      // per row: an action index or an action vector
  size_t total = 0;
  if (!carve_block(a, 3, &total, [&](auto carve) {
        carve(&d.phys, Nn * P); carve(&d.elapsed, Nn); carve(&d.time_count, Nn); carve(&d.started, Nn); carve(&d.draws, Nn);
        carve(&d.obs, Nn * S); carve(&d.ring_x, R * S); carve(&d.ring_a, R * AI); carve(&d.ring_av, R * AV); carve(&d.ring_r, R); carve(&d.head, Nn);
        carve(&d.rlen, Nn); carve(&d.reward_sum, Nn); carve(&d.total_reward, Nn); carve(&d.total_length, Nn);
        carve(&d.p, Nn * A); carve(&d.v, Nn); carve(&d.z, Nn * ZW); carve(&d.u, Nn); carve(&d.action, Nn * AI); carve(&d.action_v, Nn * AV); carve(&d.reward, Nn);
        carve(&d.done, Nn); carve(&d.cut, Nn); carve(&d.cut_head, Nn); carve(&d.cut_y, R); carve(&e.ep_flag, Nn);
        carve(&e.ep_reward, Nn); carve(&e.ep_length, Nn); carve(&d.off, R); carve(&d.counts, 3);
        carve(&e.ring_ep_reward, (size_t)e.ep_cap); carve(&e.ring_ep_length, (size_t)e.ep_cap);
      })) {
    (void)hipGetLastError();
    actors_free(a);
    return fail(GA3C_EHIP, "no memory for %d device actors (%zu bytes)", n, total);
  }
  e.counts = d.counts + 1;
  d.by = m->d_y;
  d.ba = m->d_a;
  if (!initial_physics<Env>(d.seed, Nn, d.phys, d.draws)) {
    (void)hipGetLastError();
    actors_free(a);
    return fail(GA3C_EHIP, "copy to the device actors failed");
  }
  a->fields = {
      {"phys", d.phys, 8, P, true},          {"elapsed", d.elapsed, 4, 1, true, 1 << 30}, {"time_count", d.time_count, 4, 1, true, time_max},
      {"started", d.started, 4, 1, true, 1}, {"draws", d.draws, 8, 1, true},         {"obs", d.obs, 4, S, true},
      {"rollout_len", d.rlen, 4, 1, false},  {"p", d.p, 4, A, false},                {"v", d.v, 4, 1, false},
      {"u", d.u, 8, 1, false},               {"reward", d.reward, 8, 1, false},
      {"done", d.done, 4, 1, false},         {"cut", d.cut, 4, 1, false},
  };
  if (Env::CONTINUOUS) a->fields.push_back({"action", d.action_v, 4, A, false});
  else a->fields.push_back({"action", d.action, 4, 1, false});
  m->actors = a;
  return GA3C_OK;
}

// Frees the handle's actors, if any, whatever state the stream is in (the handle's own destroy).
template <class N>
void actors_drop(N* m) {
  std::lock_guard<std::mutex> tl(m->train_mu);
  {
    std::lock_guard<std::mutex> lk(m->mu);
    (void)hipStreamSynchronize(m->st);
    (void)hipGetLastError();
  }
  actors_free(m->actors);
  m->actors = nullptr;
}

// From here on m is any handle with device, train_mu, mu, st and an `actors` pointer to a struct derived from ActorsCore.
template <class N>
int actors_destroy(N* m) {
  if (!m) return fail(GA3C_EINVAL, "null argument");
  HIPCHK(hipSetDevice(m->device));
  std::lock_guard<std::mutex> tl(m->train_mu);
  if (!m->actors) return fail(GA3C_ESTATE, "this network has no device actors");
  {
    std::lock_guard<std::mutex> lk(m->mu);
    HIPCHK(hipStreamSynchronize(m->st));
  }
  actors_free(m->actors);
  m->actors = nullptr;
  return GA3C_OK;
}

// The episode ring's records, `records` of them as the host copied the count, appended to a->finished.  The stream has
// finished the steps that wrote them: the caller has waited, in its own way.
inline int fetch_episodes(ActorsCore* a, const Episodes& e, int records, int64_t* fetched) {
  const int ne = std::min(std::max(records, 0), e.ep_cap);
  *fetched = ne;
  if (ne == 0) return GA3C_OK;
  std::vector<double> er((size_t)ne);
  std::vector<long long> el((size_t)ne);
  HIPCHK(hipMemcpy(er.data(), e.ring_ep_reward, sizeof(double) * ne, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(el.data(), e.ring_ep_length, sizeof(long long) * ne, hipMemcpyDeviceToHost));
  for (int i = 0; i < ne; ++i) a->finished.emplace_back(er[i], el[i]);
  return GA3C_OK;
}

// `steps` actor steps, each followed by a train step on the rollouts it cut when `train` is set.  stats (may be null):
// agent steps, train calls, rows trained, episodes finished.
template <class Env, class N>
int actors_run(N* m, int steps, float lr, float beta, int train, int64_t* stats) {
  if (!m) return fail(GA3C_EINVAL, "null argument");
  HIPCHK(hipSetDevice(m->device));
  std::lock_guard<std::mutex> tl(m->train_mu);
  Actors* a = m->actors;
  if (!a) return fail(GA3C_ESTATE, "this network has no device actors");
  if (steps < 1 || steps > MAX_STEPS) return fail(GA3C_EINVAL, "steps %d outside [1,%d]", steps, MAX_STEPS);
  const State& d = a->d;
  int64_t calls = 0, rows_trained = 0, episodes = 0;
  {
    std::lock_guard<std::mutex> lk(m->mu);
    HIPCHK(hipMemsetAsync(d.counts, 0, 3 * sizeof(int), m->st));     // the episode ring starts empty
  }
  int rc = GA3C_OK;
  for (int s = 0; s < steps; ++s) {
    {
      std::lock_guard<std::mutex> lk(m->mu);
      m->rows(PREDICT, Input{reinterpret_cast<const char*>(d.obs), nullptr, 4 * (int64_t)d.S}, d.N, 0.f, d.p, d.v, d.z);
      hipLaunchKernelGGL(actors_step_kernel<Env>, dim3((d.N + STEP_THREADS - 1) / STEP_THREADS), dim3(STEP_THREADS), 0, m->st, d);
      hipLaunchKernelGGL(actors_compact_kernel<Env>, dim3(1), dim3(SCAN_THREADS), 0, m->st, d);
      HIPCHK(hipGetLastError());
      HIPCHK(hipMemcpyAsync(a->h_counts, d.counts, 3 * sizeof(int), hipMemcpyDeviceToHost, m->st));
      HIPCHK(hipEventRecord(m->tev, m->st));
    }
    HIPCHK(hipEventSynchronize(m->tev));
    const int B = a->h_counts[0];
    if (B < 0 || B > m->max_batch) {      // (cannot happen: the compaction stops at N T1 rows) -- the episodes are still handed on
      a->batch_rows = 0;
      rc = fail(GA3C_ESTATE, "the actors laid out %d rows, max_batch is %d", B, m->max_batch);
      break;
    }
    a->batch_rows = B;
    if (train && B > 0) {
      std::lock_guard<std::mutex> lk(m->mu);
      CHK(enqueue_train(m, Input{reinterpret_cast<const char*>(d.ring_x), d.off, 0}, B, beta, true, lr));
      m->last_B = B;
      m->step.fetch_add(1);
      ++calls;
      rows_trained += B;
    }
  }
  if (a->h_counts[1] > 0) {               // the last step's train step may still run
    std::lock_guard<std::mutex> lk(m->mu);
    HIPCHK(hipStreamSynchronize(m->st));
    CHK(fetch_episodes(a, d.ep, a->h_counts[1], &episodes));
  }
  if (stats) {
    stats[0] = (int64_t)d.N * steps;
    stats[1] = calls;
    stats[2] = rows_trained;
    stats[3] = episodes;
  }
  return rc;
}

// Drains up to `max` finished episodes, oldest first.
template <class N>
int actors_episodes(N* m, double* total_reward, int64_t* total_length, int max, int32_t* count) {
  if (!m || !count || max < 0 || (max > 0 && (!total_reward || !total_length))) return fail(GA3C_EINVAL, "bad argument");
  std::lock_guard<std::mutex> tl(m->train_mu);
  ActorsCore* a = m->actors;
  if (!a) return fail(GA3C_ESTATE, "this network has no device actors");
  int n = 0;
  for (; n < max && !a->finished.empty(); ++n) {
    total_reward[n] = a->finished.front().first;
    total_length[n] = a->finished.front().second;
    a->finished.pop_front();
  }
  *count = n;
  return GA3C_OK;
}

// get (out) / set (in) of one of a->fields' buffers of n environments by name; `bytes` must be the buffer's size.  The
// stream is idle.
inline int field_access(const ActorsCore* a, int n, const char* name, void* out, const void* in, int64_t bytes) {
  for (const Field& f : a->fields) {
    if (strcmp(name, f.name) != 0) continue;
    const int64_t want = (int64_t)(f.elem * f.per_env * (size_t)n);
    if (bytes != want) return fail(GA3C_EINVAL, "%s is %lld bytes, not %lld", name, (long long)want, (long long)bytes);
    if (out) {
      HIPCHK(hipMemcpy(out, f.dev, (size_t)want, hipMemcpyDeviceToHost));
      return GA3C_OK;
    }
    if (!f.settable) return fail(GA3C_EINVAL, "%s is read only", name);
    if (f.hi != NO_BOUND) {
      const int32_t* v = static_cast<const int32_t*>(in);
      for (int i = 0; i < n; ++i)
        if (v[i] < 0 || v[i] > f.hi) return fail(GA3C_EINVAL, "%s[%d] = %d outside [0,%d]", name, i, v[i], f.hi);
    }
    HIPCHK(hipMemcpy(f.dev, in, (size_t)want, hipMemcpyHostToDevice));
    return GA3C_OK;
  }
  return fail(GA3C_EINVAL, "the device actors have nothing named %s", name);
}

// get (out) / set (in) of a buffer by name; `bytes` must be the buffer's size.
template <class N>
int actors_access(N* m, const char* name, void* out, const void* in, int64_t bytes) {
  if (!m || !name || (!out && !in)) return fail(GA3C_EINVAL, "null argument");
  HIPCHK(hipSetDevice(m->device));
  std::lock_guard<std::mutex> tl(m->train_mu);
  Actors* a = m->actors;
  if (!a) return fail(GA3C_ESTATE, "this network has no device actors");
  std::lock_guard<std::mutex> lk(m->mu);
  HIPCHK(hipStreamSynchronize(m->st));
  const State& d = a->d;
  const std::string nm(name);
  const int B = a->batch_rows;
  if (out && nm.compare(0, 6, "batch_") == 0) {       // the last step's batch: its row count, x gathered as the train kernel reads it
    const size_t S = (size_t)d.S, A = (size_t)d.A;
    const int64_t want = nm == "batch_rows" ? 4 : nm == "batch_x" ? (int64_t)(4 * S * B) : nm == "batch_y_r" ? 4 * (int64_t)B
                       : nm == "batch_a" ? (int64_t)(4 * A * B) : -1;
    if (want < 0) return fail(GA3C_EINVAL, "the device actors have nothing named %s", name);
    if (bytes != want) return fail(GA3C_EINVAL, "%s is %lld bytes, not %lld", name, (long long)want, (long long)bytes);
    if (nm == "batch_rows") { *static_cast<int32_t*>(out) = B; return GA3C_OK; }
    if (B == 0) return GA3C_OK;
    if (nm == "batch_y_r") { HIPCHK(hipMemcpy(out, d.by, (size_t)want, hipMemcpyDeviceToHost)); return GA3C_OK; }
    if (nm == "batch_a") { HIPCHK(hipMemcpy(out, d.ba, (size_t)want, hipMemcpyDeviceToHost)); return GA3C_OK; }
    std::vector<int64_t> off((size_t)B);
    std::vector<float> ring((size_t)d.N * d.T1 * S);
    HIPCHK(hipMemcpy(off.data(), d.off, sizeof(int64_t) * B, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(ring.data(), d.ring_x, sizeof(float) * ring.size(), hipMemcpyDeviceToHost));
    for (int r = 0; r < B; ++r)
      memcpy(static_cast<float*>(out) + (size_t)r * S, reinterpret_cast<const char*>(ring.data()) + off[r], 4 * S);
    return GA3C_OK;
  }
  return field_access(a, d.N, name, out, in, bytes);
}

}  // namespace ga3c_actors
