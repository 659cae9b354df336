// ga3c_uniform.hpp -- the counter-based uniforms of the device code: a stateless function of
// (seed, stream, draw number), the same on host and device.  The device actors (ga3c_actors.hpp) number their streams by
// environment, prioritised replay (ga3c_ddpg.hip) by sample; tests/device_agents_oracle.py::uniform is the same
// statement in numpy.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace ga3c_uniform {

// splitmix64's finalizer
__host__ __device__ inline uint64_t mix64(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// Uniform number `draw` of environment `env` under `seed`: 53 bits to a double in [0, 1).  All sums wrap at 2^64.
__host__ __device__ inline double actor_uniform(uint64_t seed, uint64_t env, uint64_t draw) {
  const uint64_t golden = 0x9E3779B97F4A7C15ull;
  const uint64_t stream = mix64(seed + golden * (env + 1));
  const uint64_t bits = mix64(stream + golden * (draw + 1));
  return (double)(bits >> 11) * 0x1.0p-53;
}

}  // namespace ga3c_uniform
