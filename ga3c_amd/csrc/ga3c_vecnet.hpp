// ga3c_vecnet.hpp -- the host half that the vector-state handles share, in two layers.
//
// Core: what all three handles have (ga3c_mlp.hip, ga3c_dmlp.hip, ga3c_ddpg.hip) -- return codes, one stream, a lane per
// prediction in flight, train-type calls serialised, the registered host segment, the arenas, the variables by name and the
// .npz checkpoint.  A handle fills, before alloc_core,
//   kind, device, S, max_batch                 what it calls itself in an error text; S: the floats of a prediction row
//   out_widths                                 the outputs of a lane, floats per row each: p[A], v[1], z[ZW], or DDPG's a[A]
//   narena, writable                           arenas, and which of them set_* and a checkpoint reach: 4 / {0,1,2}, DDPG's
//                                              5 / {0,1,2,3}, or 7 / {0,1,2,4,5} with two optimizers (Net::dual)
//   vars                                       the variable table, each variable with its (checkpoint member, arena) pairs
// and passes predict_begin the launch of its own row kernel.
//
// Net: the actor-critic layer of ga3c_mlp and ga3c_dmlp on top of Core -- TF-1 RMSProp on arenas 0/1/2/3, the train staging
// and the train-type calls.  With `dual` set before create() (ga3c_mlp only) it also allocates arenas 4/5/6, the
// value optimizer's ms / mom / last gradient; the network's own hooks below then step both optimizers.  A network's handle N
// derives from Net, fills the variable table (add_dense) before create() and supplies
//   cfg                                        its ABI config: device, state_dim, num_actions, max_batch, flags,
//                                              rmsprop_decay / _momentum / _epsilon, grad_clip_norm, predict_lanes
//   w                                          its Work: the rows p, v, z the train-type calls write and losses[3]
//   alloc_work(B), free_work()                 w's device memory for B rows (carve_rows)
//   rows(mode, in, B, beta, p, v, z)           enqueue the row kernel on `in`, outputs to p, v, z
//   wgrad(B, opt, fused)                       enqueue the weight gradients and the loss sums; fused: + RMSProp
//   update(opt, clip)                          enqueue the optimizer step on arena 3
//   loss(B)                                    enqueue the loss sums alone
// struct ga3c_ddpg derives from Core alone: its train step, its replay ring and its noise are its own.
// Everything else the handles differ in is data of Core or Net.  Nothing here asks which network it serves.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <map>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "../../include/ga3c_abi.h"
#include "ga3c_vartable.hpp"

void ga3c_set_last_error(const char* msg);   // ga3c_engine.hip: the thread's ga3c_last_error() message

namespace ga3c_vecnet {

struct Input {         // row r of the batch: S floats at base + (off ? off[r] : r * stride) bytes
  const char* base;
  const int64_t* off;
  int64_t stride;
};

struct Opt {           // TF-1 ApplyRMSProp: ms += (g*g - ms)(1-rho); mom = mom*mu + g*lr/sqrt(eps+ms); theta -= mom
  float* theta; float* ms; float* mom; float* grad;
  float lr, omr, mu, eps, clip;
};

enum { PREDICT = 0, EVAL = 1, TRAIN = 2 };

inline int fail(int code, const char* fmt, ...) {
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

// ------------------------------------------------------------------ Core: every vector-state handle

struct Out {                      // one output of a lane: B x width floats, pinned host and device
  float* h; float* d;
  int width;
};

struct PLane {                    // one prediction in flight: pinned staging + device outputs + completion event
  int64_t* h_off = nullptr; float* h_x = nullptr;
  int64_t* d_off = nullptr; float* d_x = nullptr;
  std::vector<Out> out;           // in the order of Core::out_widths
  hipEvent_t ev = nullptr;
  bool busy = false;
  int B = 0;
};

using ga3c_ckpt::Var;             // the variable table and its checkpoint members: ga3c_vartable.hpp

struct Core {
  const char* kind = "";          // what the network calls itself in an error text
  int S = 0;                      // floats of a prediction row
  int max_batch = 0, device = 0;
  std::vector<int> out_widths;    // a lane's outputs, floats per row each
  std::vector<Var> vars;          // arena order
  int64_t n = 0;                  // arena size
  int narena = 0;
  std::vector<int> writable;      // the arenas that set_* and a checkpoint reach; the others are read only
  float* arena[7] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  hipStream_t st = nullptr;       // every kernel and copy of the network: a prediction sees the weights before or after a
                                  // train step, never a mix, and needs no second buffer
  std::mutex mu;                  // enqueue order on `st` and the lanes' bookkeeping
  std::condition_variable lane_cv;
  std::mutex train_mu;            // one train / evaluate / arena call at a time (they share the network's train staging)
  std::vector<PLane> lanes;
  hipEvent_t tev = nullptr, t0 = nullptr, t1 = nullptr;
  int last_B = 0;                 // rows of the last train / evaluate / resident step (fetch)
  std::atomic<int64_t> step{0};
  const char* reg_host = nullptr;
  const char* reg_dev = nullptr;
  int64_t reg_bytes = 0;
};

inline int check_batch(const Core* m, int B) {
  if (B < 1 || B > m->max_batch) return fail(GA3C_EINVAL, "batch %d outside [1,%d]", B, m->max_batch);
  return GA3C_OK;
}

// offsets of rows in the registered segment: each must hold `floats` whole floats inside it
inline int check_offsets(const Core* m, const int64_t* off, int B, int floats) {
  if (!m->reg_dev) return fail(GA3C_ESTATE, "no host segment registered");
  const int64_t row = 4 * (int64_t)floats;
  for (int i = 0; i < B; ++i)
    if (off[i] < 0 || off[i] % 4 != 0 || off[i] > m->reg_bytes - row)
      return fail(GA3C_EINVAL, "offset %lld of row %d is not a 4-byte aligned row of %lld bytes inside the %lld-byte segment",
                  (long long)off[i], i, (long long)row, (long long)m->reg_bytes);
  return GA3C_OK;
}

inline PLane* take_lane(Core* m, std::unique_lock<std::mutex>& lk, int* ticket) {
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

inline void give_lane(Core* m, PLane* P) {
  {
    std::lock_guard<std::mutex> lk(m->mu);
    P->busy = false;
  }
  m->lane_cv.notify_one();
}

// What a prediction is refused for, before the network draws or takes anything for it; leaves its device current.
inline int predict_check(const Core* m, const int64_t* off, int B) {
  CHK(check_batch(m, B));
  HIPCHK(hipSetDevice(m->device));
  if (off) CHK(check_offsets(m, off, B, m->S));
  return GA3C_OK;
}

// Enqueues one prediction that passed predict_check on a lane of its own (x: host rows; off: rows of the registered
// segment): the input copy, launch(in, lane) -- the network's row kernel from `in` into the lane's out[].d -- and one copy to
// the host per output, in their order.
template <class Launch>
int predict_begin(Core* m, const float* x, const int64_t* off, int B, int* ticket, Launch launch) {
  std::unique_lock<std::mutex> lk(m->mu);
  PLane* P = take_lane(m, lk, ticket);
  const int S = m->S;
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
    launch(in, *P);
    e = hipGetLastError();
  }
  for (const Out& o : P->out)
    if (e == hipSuccess) e = hipMemcpyAsync(o.h, o.d, sizeof(float) * B * o.width, hipMemcpyDeviceToHost, m->st);
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

// Waits for the prediction begun under `ticket`.  GA3C_OK: *lane holds its B rows in out[].h and stays the caller's until
// give_lane; otherwise the lane is free again.
inline int predict_end(Core* m, int ticket, int B, PLane** lane) {
  if (ticket < 0 || ticket >= (int)m->lanes.size()) return fail(GA3C_ESTATE, "no prediction begun under ticket %d", ticket);
  PLane* P = &m->lanes[ticket];
  {
    std::lock_guard<std::mutex> lk(m->mu);
    if (!P->busy) return fail(GA3C_ESTATE, "no prediction begun under ticket %d", ticket);
  }
  const hipError_t e = hipEventSynchronize(P->ev);     // the lane's staging is free for the next begin only after this
  if (e != hipSuccess) {
    give_lane(m, P);
    (void)hipGetLastError();
    return fail(GA3C_EHIP, "prediction failed: %s", hipGetErrorString(e));
  }
  if (B != P->B) {
    give_lane(m, P);
    return fail(GA3C_EINVAL, "batch %d, begun with %d", B, P->B);
  }
  *lane = P;
  return GA3C_OK;
}

inline int arena_copy(Core* m, int which, int64_t off, int64_t count, float* out, const float* in) {
  if (which < 0 || which >= m->narena) return fail(GA3C_EINVAL, "arena selector %d not in [0,%d]", which, m->narena - 1);
  if (in && std::find(m->writable.begin(), m->writable.end(), which) == m->writable.end())
    return fail(GA3C_EINVAL, "arena %d is read only", which);
  HIPCHK(hipSetDevice(m->device));
  std::lock_guard<std::mutex> tl(m->train_mu);
  std::lock_guard<std::mutex> lk(m->mu);
  HIPCHK(hipStreamSynchronize(m->st));
  if (out) HIPCHK(hipMemcpy(out, m->arena[which] + off, sizeof(float) * count, hipMemcpyDeviceToHost));
  else HIPCHK(hipMemcpy(m->arena[which] + off, in, sizeof(float) * count, hipMemcpyHostToDevice));
  return GA3C_OK;
}

inline int param_count(Core* m, int64_t* count) {
  if (!m || !count) return fail(GA3C_EINVAL, "null argument");
  *count = m->n;
  return GA3C_OK;
}

inline int get_arena(Core* m, int32_t which, float* out, int64_t count) {
  if (!m || !out) return fail(GA3C_EINVAL, "null argument");
  if (count != m->n) return fail(GA3C_EINVAL, "count %lld != arena size %lld", (long long)count, (long long)m->n);
  return arena_copy(m, which, 0, count, out, nullptr);
}

inline int set_arena(Core* m, int32_t which, const float* in, int64_t count) {
  if (!m || !in) return fail(GA3C_EINVAL, "null argument");
  if (count != m->n) return fail(GA3C_EINVAL, "count %lld != arena size %lld", (long long)count, (long long)m->n);
  return arena_copy(m, which, 0, count, nullptr, in);
}

inline int get_step(Core* m, int64_t* step) {
  if (!m || !step) return fail(GA3C_EINVAL, "null argument");
  *step = m->step.load();
  return GA3C_OK;
}

inline int set_step(Core* m, int64_t step) {
  if (!m) return fail(GA3C_EINVAL, "null argument");
  m->step.store(step);
  return GA3C_OK;
}

inline int32_t num_params(Core* m) { return m ? (int32_t)m->vars.size() : 0; }

inline const char* param_name(Core* m, int32_t index) {
  return (m && index >= 0 && index < (int32_t)m->vars.size()) ? m->vars[index].name.c_str() : nullptr;
}

inline int param_info(Core* m, const char* name, int64_t* offset, int64_t* count, int32_t* ndim, int64_t shape[4]) {
  if (!m || !name) return fail(GA3C_EINVAL, "null argument");
  const int i = ga3c_ckpt::find_var(m->vars, name);
  if (i < 0) return fail(GA3C_EINVAL, "no variable named %s", name);
  const Var& var = m->vars[i];
  if (offset) *offset = var.off;
  if (count) *count = var.count;
  if (ndim) *ndim = var.ndim;
  if (shape) memcpy(shape, var.shape, sizeof var.shape);
  return GA3C_OK;
}

// get_param (out) / set_param (in)
inline int param_copy(Core* m, const char* name, int32_t which, float* out, const float* in, int64_t count) {
  if (!m || !name || (!out && !in)) return fail(GA3C_EINVAL, "null argument");
  const int i = ga3c_ckpt::find_var(m->vars, name);
  if (i < 0) return fail(GA3C_EINVAL, "no variable named %s", name);
  const Var& var = m->vars[i];
  if (count != var.count) return fail(GA3C_EINVAL, "%s has %lld elements, not %lld", name, (long long)var.count, (long long)count);
  return arena_copy(m, which, var.off, count, out, in);
}

// The writable arenas on the host, by arena number, as save writes and load starts from them.
inline int read_arenas(Core* m, ga3c_ckpt::Arenas* arena) {
  arena->assign((size_t)m->narena, std::vector<float>());
  for (int w : m->writable) {
    (*arena)[w].resize((size_t)m->n);
    CHK(get_arena(m, w, (*arena)[w].data(), m->n));
  }
  return GA3C_OK;
}

inline int save(Core* m, const char* path) {
  if (!m || !path) return fail(GA3C_EINVAL, "null argument");
  ga3c_ckpt::Arenas arena;
  CHK(read_arenas(m, &arena));
  std::string err;
  if (!ga3c_ckpt::write_npz(path, ga3c_ckpt::pack_members(m->vars, m->step.load(), arena), &err))
    return fail(GA3C_ESTATE, "%s", err.c_str());
  return GA3C_OK;
}

inline int read_checkpoint(const char* path, std::map<std::string, ga3c_ckpt::Member>* members) {
  std::string err;
  if (!ga3c_ckpt::read_npz(path, members, &err)) return fail(GA3C_ESTATE, "%s", err.c_str());
  return GA3C_OK;
}

inline int checkpoint_step(const char* path, const std::map<std::string, ga3c_ckpt::Member>& members, int64_t* step) {
  std::string err;
  if (!ga3c_ckpt::checkpoint_step(path, members, step, &err)) return fail(GA3C_ESTATE, "%s", err.c_str());
  return GA3C_OK;
}

// `members`: the file, read already.  What unpack_members refuses is refused before anything is written; an arena element
// that no member names keeps its value.
inline int load(Core* m, const char* path, const std::map<std::string, ga3c_ckpt::Member>& members) {
  ga3c_ckpt::Arenas arena;
  CHK(read_arenas(m, &arena));
  int64_t step = 0;
  std::string err;
  if (!ga3c_ckpt::unpack_members(path, m->kind, m->vars, members, &arena, &step, &err)) return fail(GA3C_ESTATE, "%s", err.c_str());
  for (int w : m->writable) CHK(set_arena(m, w, arena[w].data(), m->n));
  m->step.store(step);
  return GA3C_OK;
}

inline int load(Core* m, const char* path) {
  if (!m || !path) return fail(GA3C_EINVAL, "null argument");
  std::map<std::string, ga3c_ckpt::Member> members;
  CHK(read_checkpoint(path, &members));
  return load(m, path, members);
}

inline int register_host(Core* m, void* base, int64_t bytes) {
  if (!m || !base || bytes < 16) return fail(GA3C_EINVAL, "bad argument");
  if (m->reg_host) return fail(GA3C_ESTATE, "a host segment is already registered");
  HIPCHK(hipSetDevice(m->device));
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

inline int unregister_host(Core* m) {
  if (!m) return fail(GA3C_EINVAL, "null argument");
  if (!m->reg_host) return GA3C_OK;
  HIPCHK(hipSetDevice(m->device));
  std::lock_guard<std::mutex> tl(m->train_mu);
  std::lock_guard<std::mutex> lk(m->mu);
  HIPCHK(hipStreamSynchronize(m->st));
  HIPCHK(hipHostUnregister((void*)m->reg_host));
  m->reg_host = m->reg_dev = nullptr;
  m->reg_bytes = 0;
  return GA3C_OK;
}

// `src`: `name`'s rows of the workspace, `wd` floats each, as the network's own table found them
inline int fetch(Core* m, const char* name, const float* src, int64_t wd, float* out, int64_t count) {
  if (count != wd * m->last_B)
    return fail(GA3C_EINVAL, "%s of the last step is %lld floats, not %lld", name, (long long)(wd * m->last_B), (long long)count);
  HIPCHK(hipSetDevice(m->device));
  std::lock_guard<std::mutex> tl(m->train_mu);
  std::lock_guard<std::mutex> lk(m->mu);
  HIPCHK(hipStreamSynchronize(m->st));
  HIPCHK(hipMemcpy(out, src, sizeof(float) * count, hipMemcpyDeviceToHost));
  return GA3C_OK;
}

// One zeroed device block cut into row buffers: *dst[i] gets B x widths[i] floats, rounded up to whole float4s; *end is the
// four floats behind the last of them.
inline int carve_rows(size_t B, const std::vector<size_t>& widths, const std::vector<float**>& dst, float** base, float** end) {
  size_t total = 0;
  for (size_t wd : widths) total += (B * wd + 3) / 4 * 4;
  CHK(dalloc(base, total + 4));
  HIPCHK(hipMemset(*base, 0, sizeof(float) * (total + 4)));
  float* q = *base;
  for (size_t i = 0; i < widths.size(); ++i) {
    *dst[i] = q;
    q += (B * widths[i] + 3) / 4 * 4;
  }
  *end = q;
  return GA3C_OK;
}

// The stream, the zeroed arenas, the events and `lanes` lanes (0: four) of a Core whose sizes and outputs are filled.
inline int alloc_core(Core* m, int lanes) {
  const size_t B = (size_t)m->max_batch, S = m->S;
  HIPCHK(hipStreamCreateWithFlags(&m->st, hipStreamNonBlocking));
  for (int i = 0; i < m->narena; ++i) {
    CHK(dalloc(&m->arena[i], (size_t)m->n));
    HIPCHK(hipMemset(m->arena[i], 0, sizeof(float) * m->n));
  }
  HIPCHK(hipEventCreateWithFlags(&m->tev, hipEventDisableTiming));
  HIPCHK(hipEventCreate(&m->t0));
  HIPCHK(hipEventCreate(&m->t1));
  m->lanes.resize((size_t)(lanes > 0 ? lanes : 4));
  for (PLane& P : m->lanes) {
    CHK(halloc(&P.h_off, B)); CHK(halloc(&P.h_x, B * S));
    CHK(dalloc(&P.d_off, B)); CHK(dalloc(&P.d_x, B * S));
    for (int wd : m->out_widths) {
      P.out.push_back(Out{nullptr, nullptr, wd});
      CHK(halloc(&P.out.back().h, B * wd));
      CHK(dalloc(&P.out.back().d, B * wd));
    }
    HIPCHK(hipEventCreateWithFlags(&P.ev, hipEventDisableTiming));
  }
  return GA3C_OK;
}

// Waits for the stream, then frees what alloc_core made, however far it came.  The network's own buffers go after it.
inline void free_core(Core* m) {
  if (m->st) (void)hipStreamSynchronize(m->st);
  for (PLane& P : m->lanes) {
    (void)hipHostFree(P.h_off); (void)hipHostFree(P.h_x);
    (void)hipFree(P.d_off); (void)hipFree(P.d_x);
    for (Out& o : P.out) {
      (void)hipHostFree(o.h);
      (void)hipFree(o.d);
    }
    if (P.ev) (void)hipEventDestroy(P.ev);
  }
  for (float*& a : m->arena) (void)hipFree(a);
  for (hipEvent_t e : {m->tev, m->t0, m->t1})
    if (e) (void)hipEventDestroy(e);
  if (m->reg_host) (void)hipHostUnregister((void*)m->reg_host);
  if (m->st) (void)hipStreamDestroy(m->st);
  (void)hipGetLastError();
}

// The checks of a config that come before the network's own: the sizes every layer table is built from.
template <class C>
int check_dims(const C& c, int max_s, int max_a, int max_b) {
  if (c.state_dim < 1 || c.state_dim > max_s) return fail(GA3C_EINVAL, "state_dim %d outside [1,%d]", c.state_dim, max_s);
  if (c.num_actions < 1 || c.num_actions > max_a) return fail(GA3C_EINVAL, "num_actions %d outside [1,%d]", c.num_actions, max_a);
  if (c.max_batch < 1 || c.max_batch > max_b) return fail(GA3C_EINVAL, "max_batch %d outside [1,%d]", c.max_batch, max_b);
  return GA3C_OK;
}

// ... and those that come after them; leaves the config's device current.
template <class C>
int check_device(const C& c) {
  if (c.predict_lanes < 0 || c.predict_lanes > 64) return fail(GA3C_EINVAL, "predict_lanes %d outside [0,64]", c.predict_lanes);
  int ndev = 0;
  HIPCHK(hipGetDeviceCount(&ndev));
  if (c.device < 0 || c.device >= ndev) return fail(GA3C_EINVAL, "device %d not in [0,%d)", c.device, ndev);
  HIPCHK(hipSetDevice(c.device));
  hipDeviceProp_t prop;
  HIPCHK(hipGetDeviceProperties(&prop, c.device));
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return fail(GA3C_ESTATE, "device %d is %s; this library is built for gfx950 only", c.device, prop.gcnArchName);
  return GA3C_OK;
}

// ------------------------------------------------------------------ Net: the actor-critic layer (ga3c_mlp, ga3c_dmlp)

struct Net : Core {               // arenas: theta, ms, mom, grad; dual: + the value optimizer's ms, mom, grad
  int A = 0;
  bool dual = false;              // two optimizers, one per cost: arenas 1/2/3 are cost_p's, 4/5/6 cost_v's
  int ZW = 0;                     // logits per row
  bool clip = false;
  Opt opt{};                      // the arenas and the optimizer's constants; lr is the call's
  // train staging: pinned host + device
  float* h_x = nullptr; float* h_y = nullptr; float* h_a = nullptr; int64_t* h_off = nullptr; float* h_loss = nullptr;
  float* d_x = nullptr; float* d_y = nullptr; float* d_a = nullptr; int64_t* d_off = nullptr;
  int res_B = 0;                  // rows uploaded for the resident path

  // the w [in, out] at arena element `off` and the b [out] behind it: one dense layer's variables, TF creation order
  void add_dense(const std::string& w_name, const std::string& b_name, int64_t off, int in, int out) {
    vars.push_back(Var{w_name, off, (int64_t)in * out, 2, {in, out}, {}});
    vars.push_back(Var{b_name, off + (int64_t)in * out, out, 1, {out, 0}, {}});
    for (Var* var : {&vars[vars.size() - 2], &vars.back()}) ga3c_ckpt::single_members(var);
    n = off + (int64_t)in * out + out;
  }
};

inline Opt make_opt(const Net* m, float lr) {
  Opt o = m->opt;
  o.lr = lr;
  return o;
}

// Stages y_r / a and the states (x: host rows, or offsets into the registered segment) of a train-type call; caller holds
// train_mu.  Returns the Input the row kernel reads.
inline int stage_train(Net* m, const float* x, const int64_t* off, const float* y, const float* a, int B, Input* in) {
  const int S = m->S, A = m->A;
  if (off) CHK(check_offsets(m, off, B, S));
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

template <class N>
int finish_train(N* m) {
  HIPCHK(hipMemcpyAsync(m->h_loss, m->w.losses, 3 * sizeof(float), hipMemcpyDeviceToHost, m->st));
  HIPCHK(hipEventRecord(m->tev, m->st));
  return GA3C_OK;
}

inline int wait_train(Net* m, float* losses) {
  HIPCHK(hipEventSynchronize(m->tev));
  if (losses) memcpy(losses, m->h_loss, 3 * sizeof(float));
  return GA3C_OK;
}

// Enqueue a train step on `in` (caller holds mu): the row kernel, the weight gradients and, apply != 0, the update.
template <class N>
int enqueue_train(N* m, const Input& in, int B, float beta, bool apply, float lr) {
  m->rows(TRAIN, in, B, beta, m->w.p, m->w.v, m->w.z);
  const Opt o = make_opt(m, lr);
  m->wgrad(B, o, apply && !m->clip);
  if (apply && m->clip) m->update(o, true);
  HIPCHK(hipGetLastError());
  return GA3C_OK;
}

// train / compute_grads on host rows or on offsets
template <class N>
int train_common(N* m, const float* x, const int64_t* off, const float* y, const float* a, int B, bool apply, float lr,
                 float beta, float* losses) {
  if (!m || (!x && !off) || !y || !a) return fail(GA3C_EINVAL, "null argument");
  CHK(check_batch(m, B));
  HIPCHK(hipSetDevice(m->device));
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

template <class N>
int train_gather(N* m, const int64_t* offsets, int32_t u8, const float* y, const float* a, int B, float lr, float beta,
                 float* losses) {
  if (u8) return fail(GA3C_EINVAL, "the vector-state network reads f32 rows (u8 = 0)");
  if (!offsets) return fail(GA3C_EINVAL, "null argument");
  return train_common(m, nullptr, offsets, y, a, B, true, lr, beta, losses);
}

template <class N>
int apply_grads(N* m, float lr) {
  if (!m) return fail(GA3C_EINVAL, "null argument");
  HIPCHK(hipSetDevice(m->device));
  std::lock_guard<std::mutex> tl(m->train_mu);
  {
    std::lock_guard<std::mutex> lk(m->mu);
    m->update(make_opt(m, lr), m->clip);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(m->tev, m->st));
  }
  HIPCHK(hipEventSynchronize(m->tev));
  m->step.fetch_add(1);
  return GA3C_OK;
}

struct RowsOut {                  // B x width floats of the workspace, copied to `host` unless it is null
  float* host;
  const float* dev;
  size_t width;
};

// Forward + loss of the batch on the current weights, no update; `acts`: the activations the network's entry returns.
template <class N>
int evaluate(N* m, const float* x, const int64_t* offsets, const float* y, const float* a, int B, float beta, float* losses,
             std::initializer_list<RowsOut> acts, float* v, float* p) {
  if (!m || (!x && !offsets) || (x && offsets) || !y || !a) return fail(GA3C_EINVAL, "bad argument");
  CHK(check_batch(m, B));
  HIPCHK(hipSetDevice(m->device));
  std::lock_guard<std::mutex> tl(m->train_mu);
  {
    std::lock_guard<std::mutex> lk(m->mu);
    Input in;
    CHK(stage_train(m, x, offsets, y, a, B, &in));
    m->rows(EVAL, in, B, beta, m->w.p, m->w.v, m->w.z);
    m->loss(B);
    HIPCHK(hipGetLastError());
    CHK(finish_train(m));
    m->last_B = B;
  }
  CHK(wait_train(m, losses));
  for (const RowsOut& o : acts)
    if (o.host) HIPCHK(hipMemcpy(o.host, o.dev, (size_t)B * o.width * sizeof(float), hipMemcpyDeviceToHost));
  if (v) HIPCHK(hipMemcpy(v, m->w.v, (size_t)B * sizeof(float), hipMemcpyDeviceToHost));
  if (p) HIPCHK(hipMemcpy(p, m->w.p, (size_t)B * m->A * sizeof(float), hipMemcpyDeviceToHost));
  return GA3C_OK;
}

// A lane's outputs are p, v, z.
template <class N>
int predict_begin(N* m, const float* x, const int64_t* off, int B, int* ticket) {
  CHK(predict_check(m, off, B));
  return predict_begin(m, x, off, B, ticket,
                       [m, B](const Input& in, PLane& P) { m->rows(PREDICT, in, B, 0.f, P.out[0].d, P.out[1].d, P.out[2].d); });
}

inline int predict_end(Net* m, int ticket, int B, float* p, float* v, float* z) {
  PLane* P;
  CHK(predict_end(m, ticket, B, &P));
  float* const dst[3] = {p, v, z};
  for (int i = 0; i < 3; ++i)
    if (dst[i]) memcpy(dst[i], P->out[i].h, sizeof(float) * B * P->out[i].width);
  give_lane(m, P);
  return GA3C_OK;
}

template <class N>
int predict(N* m, const float* x, int B, float* p, float* v, float* z) {
  if (!m || !x || !p || !v) return fail(GA3C_EINVAL, "null argument");
  int ticket;
  CHK(predict_begin(m, x, nullptr, B, &ticket));
  return predict_end(m, ticket, B, p, v, z);
}

template <class N>
int predict_gather_begin(N* m, const int64_t* offsets, int B, int32_t u8, int32_t* ticket) {
  if (!m || !offsets || !ticket) return fail(GA3C_EINVAL, "null argument");
  if (u8) return fail(GA3C_EINVAL, "the vector-state network reads f32 rows (u8 = 0)");
  return predict_begin(m, nullptr, offsets, B, ticket);
}

template <class N>
int predict_gather(N* m, const int64_t* offsets, int B, int32_t u8, float* p, float* v, float* z) {
  int ticket;
  CHK(predict_gather_begin(m, offsets, B, u8, &ticket));
  return predict_end(m, ticket, B, p, v, z);
}

inline int predict_gather_end(Net* m, int ticket, int B, float* p, float* v) {
  if (!m || !p || !v) return fail(GA3C_EINVAL, "null argument");
  return predict_end(m, ticket, B, p, v, nullptr);
}

inline int upload(Net* m, const float* x, const float* y, const float* a, int B) {
  if (!m || !x || !y || !a) return fail(GA3C_EINVAL, "null argument");
  CHK(check_batch(m, B));
  HIPCHK(hipSetDevice(m->device));
  std::lock_guard<std::mutex> tl(m->train_mu);
  std::lock_guard<std::mutex> lk(m->mu);
  Input in;
  CHK(stage_train(m, x, nullptr, y, a, B, &in));
  HIPCHK(hipStreamSynchronize(m->st));
  m->res_B = B;
  return GA3C_OK;
}

template <class N>
int time_resident(N* m, int32_t mode, int B, int iters, float lr, float beta, float* elapsed_ms) {
  if (!m || !elapsed_ms || iters < 1 || (mode != 0 && mode != 1)) return fail(GA3C_EINVAL, "bad argument");
  if (B < 1 || B > m->res_B) return fail(GA3C_ESTATE, "batch %d: %d rows uploaded", B, m->res_B);
  HIPCHK(hipSetDevice(m->device));
  std::lock_guard<std::mutex> tl(m->train_mu);
  {
    std::lock_guard<std::mutex> lk(m->mu);
    const Input in{reinterpret_cast<const char*>(m->d_x), nullptr, 4 * (int64_t)m->S};
    HIPCHK(hipEventRecord(m->t0, m->st));
    for (int i = 0; i < iters; ++i) {
      if (mode == 0) m->rows(PREDICT, in, B, 0.f, m->w.p, m->w.v, m->w.z);
      else CHK(enqueue_train(m, in, B, beta, true, lr));
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(m->t1, m->st));
    m->last_B = B;
  }
  HIPCHK(hipEventSynchronize(m->t1));
  HIPCHK(hipEventElapsedTime(elapsed_ms, m->t0, m->t1));
  if (mode == 1) m->step.fetch_add(iters);
  return GA3C_OK;
}

template <class N>
void free_all(N* m) {
  free_core(m);
  m->free_work();
  (void)hipHostFree(m->h_x); (void)hipHostFree(m->h_y); (void)hipHostFree(m->h_a); (void)hipHostFree(m->h_off);
  (void)hipHostFree(m->h_loss);
  (void)hipFree(m->d_x); (void)hipFree(m->d_y); (void)hipFree(m->d_a); (void)hipFree(m->d_off);
  (void)hipGetLastError();
}

template <class N>
int alloc_all(N* m) {
  const size_t B = (size_t)m->max_batch, S = m->S, A = m->A;
  CHK(alloc_core(m, m->cfg.predict_lanes));
  std::vector<float> ones((size_t)m->n, 1.0f);     // the RMSProp ms slot starts at 1 (TF-1 RMSPropOptimizer)
  HIPCHK(hipMemcpy(m->arena[1], ones.data(), sizeof(float) * m->n, hipMemcpyHostToDevice));
  if (m->dual) HIPCHK(hipMemcpy(m->arena[4], ones.data(), sizeof(float) * m->n, hipMemcpyHostToDevice));
  m->opt.theta = m->arena[0]; m->opt.ms = m->arena[1]; m->opt.mom = m->arena[2]; m->opt.grad = m->arena[3];
  CHK(m->alloc_work(B));
  CHK(halloc(&m->h_x, B * S)); CHK(halloc(&m->h_y, B)); CHK(halloc(&m->h_a, B * A)); CHK(halloc(&m->h_off, B));
  CHK(halloc(&m->h_loss, 4));
  CHK(dalloc(&m->d_x, B * S)); CHK(dalloc(&m->d_y, B)); CHK(dalloc(&m->d_a, B * A)); CHK(dalloc(&m->d_off, B));
  return GA3C_OK;
}

// m: a new handle with cfg, kind, ZW and the variable table filled.  On failure m is freed.
template <class N>
int create(N* m, N** out) {
  const auto& c = m->cfg;
  m->S = c.state_dim;
  m->A = c.num_actions;
  m->max_batch = c.max_batch;
  m->device = c.device;
  m->out_widths = {m->A, 1, m->ZW};
  m->narena = m->dual ? 7 : 4;
  m->writable = {0, 1, 2};
  if (m->dual) m->writable.insert(m->writable.end(), {4, 5});
  m->clip = (c.flags & GA3C_FLAG_GRAD_CLIP) != 0;
  m->opt.omr = 1.0f - c.rmsprop_decay;
  m->opt.mu = c.rmsprop_momentum;
  m->opt.eps = c.rmsprop_epsilon;
  m->opt.clip = c.grad_clip_norm;
  const int rc = alloc_all(m);
  if (rc != GA3C_OK) {
    free_all(m);
    delete m;
    return rc;
  }
  *out = m;
  return GA3C_OK;
}

template <class N>
int destroy(N* m) {
  if (!m) return fail(GA3C_EINVAL, "null argument");
  (void)hipSetDevice(m->device);
  free_all(m);
  delete m;
  return GA3C_OK;
}

}  // namespace ga3c_vecnet
