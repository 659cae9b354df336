"""Per-environment exploration noise of the DDPG device actors (Config.DEVICE_DDPG_NOISE = 'per_env', ga3c_ddpg_envnoise_*,
DESIGN.md 8r) in numpy: the statement the kernel's epilogue is held to.

Environment i of N owns an Ornstein-Uhlenbeck state x_i[A] in f32, 0 at the start.  On prediction number c of the handle
(0 for the first; step(None) predicts nothing and does not count), for action j with k = c A + j:
    u1 = 1 - u(seed, i, 2k),  u2 = u(seed, i, 2k + 1)          device_agents_oracle.uniform: the environment is the stream
    n  = (f32)(sqrt(-2 ln u1) cos(2 pi u2))                    in f64
    x_prev = 0 if the handle resets on done and environment i's last step was done, else x_i[j]
    x' = (f32) ddpg_oracle.ou_step(x_prev, n)                  in f64, sigma, theta and dt the f32 values of the handle's config
    action = actor(obs_i)[j] + x'                              in f32, not wrapped
The seed is the noise's own: the environments' reset draws are another stream set."""
import numpy as np

import ddpg_oracle as o
import device_agents_oracle as ao

TWO_PI = 6.283185307179586


def f32_config(sigma=0.3, theta=0.15, dt=1e-2):
    """The process's constants as the handle's config holds them: f32 values, read in f64."""
    return dict(sigma=np.float64(np.float32(sigma)), theta=np.float64(np.float32(theta)), dt=np.float64(np.float32(dt)))


def uniforms(seed, n_envs, count, A):
    """-> (u1, u2) f64 [n_envs][A] of prediction `count`."""
    i = np.repeat(np.arange(n_envs, dtype=np.uint64)[:, None], A, axis=1)
    k = np.uint64(count) * np.uint64(A) + np.repeat(np.arange(A, dtype=np.uint64)[None, :], n_envs, axis=0)
    u1 = 1.0 - ao.uniform(seed, i, np.uint64(2) * k)
    u2 = ao.uniform(seed, i, np.uint64(2) * k + np.uint64(1))
    return u1, u2


def draws(seed, n_envs, count, A):
    """-> n f32 [n_envs][A]: the normal draws of prediction `count`."""
    u1, u2 = uniforms(seed, n_envs, count, A)
    return (np.sqrt(-2.0 * np.log(u1)) * np.cos(TWO_PI * u2)).astype(np.float32)


def x_prev(x, done, reset):
    """What the step starts from: f64 [N][A]."""
    x = np.asarray(x, np.float32).astype(np.float64)
    if not reset:
        return x
    return np.where(np.asarray(done).astype(bool)[:, None], 0.0, x)


def step(x, n, done=None, reset=False, **config):
    """x f32 [N][A], n f32 [N][A] -> x' f32 [N][A]."""
    prev = x_prev(x, np.zeros(len(x), bool) if done is None else done, reset)
    return o.ou_step(prev, np.asarray(n, np.float32).astype(np.float64), **f32_config(**config)).astype(np.float32)


class EnvNoise:
    """The state of a handle's per-environment noise: x, the last draws n and the count of predictions."""

    def __init__(self, n_envs, A, seed, reset=False, **config):
        self.N, self.A, self.seed, self.reset, self.config = int(n_envs), int(A), int(seed), bool(reset), config
        self.x = np.zeros((self.N, self.A), np.float32)
        self.n = np.zeros((self.N, self.A), np.float32)
        self.count = 0

    def predict(self, done=None):
        """One prediction's noise -> x' f32 [N][A], what is added to the actor's output."""
        self.n = draws(self.seed, self.N, self.count, self.A)
        self.x = step(self.x, self.n, done, self.reset, **self.config)
        self.count += 1
        return self.x
