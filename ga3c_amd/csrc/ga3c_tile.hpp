// ga3c_tile.hpp -- the device half of the vector-state networks (ga3c_mlp.hip, ga3c_dmlp.hip, ga3c_ddpg.hip), beside
// ga3c_vecnet.hpp's host half.  DESIGN.md 8e-1.
//
// A workgroup of THREADS threads (256 for mlp and dmlp, 448 for ddpg) owns one tile of 16 batch rows; a layer's activations
// lie in LDS as [width][16], so a column of the tile is 16 consecutive floats that every thread reads as four broadcast
// 16-byte LDS reads.  Every block here fixes which thread owns which sum and the order of its additions: no atomics, and
// the same call gives the same bits.  From the host half it takes Input and Opt alone.
#pragma once

#include <hip/hip_runtime.h>

#include "ga3c_vecnet.hpp"

namespace ga3c_tile {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int TILE = 16;                  // rows per workgroup

__device__ __forceinline__ float sigm(float h) { return 1.0f / (1.0f + expf(-h)); }

// acc[r] += column[r] w for the 16 rows of the tile: one step of a thread's own sum, in the order the caller walks k (or j).
__device__ __forceinline__ void tile_fma(float (&acc)[TILE], const float* column, float w) {
  const f32x4* col = reinterpret_cast<const f32x4*>(column);
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const f32x4 c = col[q];
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[4 * q + i] = fmaf(c[i], w, acc[4 * q + i]);
  }
}

// xin[s][r] = row row0 + r of the batch (zeros beyond nrows); KEEP: the same rows to `keep`, row-major [B][S] (else `keep`
// is not read).  No barrier: the caller's.
template <int THREADS, bool KEEP>
__device__ __forceinline__ void load_input_tile(const ga3c_vecnet::Input& in, int S, int row0, int nrows, float* xin,
                                                float* __restrict__ keep) {
  for (int e = threadIdx.x; e < S * TILE; e += THREADS) {
    const int r = e / S, s = e % S;
    float xv = 0.f;
    if (r < nrows) {
      const int64_t ob = in.off ? in.off[row0 + r] : (int64_t)(row0 + r) * in.stride;
      xv = reinterpret_cast<const float*>(in.base + ob)[s];
      if (KEEP) keep[(size_t)(row0 + r) * S + s] = xv;
    }
    xin[s * TILE + r] = xv;
  }
}

// ep(j, r, bias[j] + sum_k in[k][r] W[k][j] + sum_k in2[k][r] W2[k][j]) for the tile; thread j owns column j (coalesced
// weight reads) and adds in k order, the second operand (K2 = 0: none) after the first.  Ends in a barrier.
template <int THREADS, class EP>
__device__ __forceinline__ void dense_fwd(const float* __restrict__ W, const float* __restrict__ bias, int K, int N, const float* in,
                                          const float* __restrict__ W2, int K2, const float* in2, EP ep) {
  for (int j = threadIdx.x; j < N; j += THREADS) {
    float acc[TILE];
    const float b = bias[j];
#pragma unroll
    for (int r = 0; r < TILE; ++r) acc[r] = b;
    for (int k = 0; k < K; ++k) tile_fma(acc, in + k * TILE, W[(size_t)k * N + j]);
    for (int k = 0; k < K2; ++k) tile_fma(acc, in2 + k * TILE, W2[(size_t)k * N + j]);
#pragma unroll
    for (int r = 0; r < TILE; ++r) ep(j, r, acc[r]);
  }
  __syncthreads();
}

// finish(k, r, sum_j W(k, j) gout[j][r]) for k < K <= THREADS.  P threads share a k (the largest power of two with
// P K <= THREADS), each summing the strided slice j = p, p + P, ... in that order; the P partials meet in `scratch`
// (P K 16 floats; unused when P = 1) and are added in p order.  Ends in a barrier.
template <int THREADS, class WF, class FIN>
__device__ __forceinline__ void dense_bwd_split(WF W, int K, int N, const float* gout, float* scratch, FIN finish) {
  int P = 1;
  while (P * 2 * K <= THREADS) P *= 2;
  const int t = threadIdx.x;
  if (t < P * K) {
    const int k = t / P, p = t % P;
    float acc[TILE];
#pragma unroll
    for (int r = 0; r < TILE; ++r) acc[r] = 0.f;
    for (int j = p; j < N; j += P) tile_fma(acc, gout + j * TILE, W(k, j));
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

// TF-1 ApplyRMSProp on element i with gradient g (Opt, ga3c_vecnet.hpp) -> the step taken.
__device__ __forceinline__ float rms_step(const ga3c_vecnet::Opt& o, int64_t i, float g) {
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

// The sum of every thread's v in a fixed order: the halving tree over the next power of two above THREADS leaves (256 for
// 256 threads, 512 for 448, the leaves beyond THREADS zero).  A thread's v is its own strided partial, i = t, t + THREADS,
// ... in that order.  sh: that many floats; a second sum takes another sh, or a barrier first.
template <int THREADS>
__device__ __forceinline__ float block_sum(float v, float* sh) {
  constexpr int RED = THREADS & (THREADS - 1) ? 1 << (32 - __builtin_clz(THREADS)) : THREADS;
  sh[threadIdx.x] = v;
  if (RED > THREADS && threadIdx.x + THREADS < RED) sh[threadIdx.x + THREADS] = 0.f;
  __syncthreads();
  for (int h = RED / 2; h > 0; h >>= 1) {
    if (threadIdx.x < h) sh[threadIdx.x] += sh[threadIdx.x + h];
    __syncthreads();
  }
  return sh[0];
}

// Sums over the batch rows, in row order.  The loads of ROWS_AHEAD rows are issued together and the additions stay one chain:
// the order of the plain loop at the latency of B / ROWS_AHEAD round trips to L2 instead of B.
constexpr int ROWS_AHEAD = 16;

// The chains are in double and rounded once.  A gradient or a loss column is a sum over up to 65536 rows, often of one sign:
// where the terms are nearly equal a float chain rounds the same way at every addition (a loss of 2225.49 for 2226.92 at 65536
// rows), and RMSProp's ms takes the square of the sum (the value head's bias sums v - y_r; with float chains two steps of 65536
// rows left ms 1.1 to 1.3 times 1e-5 x max(ms) from the oracle).  tests/test_gpu_vector_batch.py holds both.
__device__ __forceinline__ float sum_rows(const float* __restrict__ d, int ld, int B) {
  double g = 0.0;
  int r = 0;
  for (; r + ROWS_AHEAD <= B; r += ROWS_AHEAD) {
    float t[ROWS_AHEAD];
#pragma unroll
    for (int i = 0; i < ROWS_AHEAD; ++i) t[i] = d[(size_t)(r + i) * ld];
#pragma unroll
    for (int i = 0; i < ROWS_AHEAD; ++i) g += (double)t[i];
  }
  for (; r < B; ++r) g += (double)d[(size_t)r * ld];
  return (float)g;
}

__device__ __forceinline__ float dot_rows(const float* __restrict__ x, int ldx, const float* __restrict__ d, int ldd, int B) {
  double g = 0.0;
  int r = 0;
  for (; r + ROWS_AHEAD <= B; r += ROWS_AHEAD) {
    float tx[ROWS_AHEAD], td[ROWS_AHEAD];
#pragma unroll
    for (int i = 0; i < ROWS_AHEAD; ++i) {
      tx[i] = x[(size_t)(r + i) * ldx];
      td[i] = d[(size_t)(r + i) * ldd];
    }
#pragma unroll
    for (int i = 0; i < ROWS_AHEAD; ++i) g = fma((double)tx[i], (double)td[i], g);
  }
  for (; r < B; ++r) g = fma((double)x[(size_t)r * ldx], (double)d[(size_t)r * ldd], g);
  return (float)g;
}

// losses[c] = sum over the rows of lossrow[r][c], c < 3: threads 0..2 of the one block that says `mine`, each by sum_rows.
__device__ __forceinline__ void loss_sums(const float* __restrict__ lossrow, float* __restrict__ losses, int B, bool mine = true) {
  if (mine && threadIdx.x < 3) losses[threadIdx.x] = sum_rows(lossrow + threadIdx.x, 3, B);
}

// One block on elements lo .. hi-1 of one variable.  CLIP: tf.clip_by_average_norm, g *= clip / max(||g||_2 / (hi - lo), clip),
// the sum of squares by block_sum.  Then the RMSProp step, thread t on i = lo + t, lo + t + THREADS, ...
template <int THREADS, bool CLIP>
__device__ __forceinline__ void clip_and_step(int64_t lo, int64_t hi, const ga3c_vecnet::Opt& o, float* sh) {
  float scale = 1.f;
  if (CLIP) {
    float s = 0.f;
    for (int64_t i = lo + threadIdx.x; i < hi; i += THREADS) s += o.grad[i] * o.grad[i];
    scale = o.clip / fmaxf(sqrtf(block_sum<THREADS>(s, sh)) / (float)(hi - lo), o.clip);
  }
  for (int64_t i = lo + threadIdx.x; i < hi; i += THREADS) {
    float g = o.grad[i];
    if (CLIP) g *= scale;
    rms_step(o, i, g);
  }
}

}  // namespace ga3c_tile
