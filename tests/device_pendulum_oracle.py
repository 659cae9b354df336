"""Oracle of the device actors for Pendulum-v0 (Config.DEVICE_AGENTS with DEVICE_PENDULUM; struct Pendulum and
the Env::CONTINUOUS path of csrc/ga3c_actors.hpp): one actor step restated in numpy f64.

The uniforms, the fork's returns and the way N environments make one batch are tests/device_agents_oracle.py's (uniform,
CounterRNG, returns_fork, Actors.step) and are used from there.  That file's Actor.step has CartPole written into it, so
the step is stated here once more with the environment passed in -- EnvActor -- and test_device_pendulum_cpu.py holds
EnvActor over CartPoleEnv to device_agents_oracle.Actor bit for bit: the bookkeeping (first ever step, rollout cut, re-use of
the last row, returns, episode records, reset) is the same statement, only the environment differs.

What PendulumEnv restates is EnvironmentPend.Pendulum.step / reset under EnvironmentPend.Environment.step:
  * u = 2 a, a the f32 action; cost = angle_normalize(th)^2 + 0.1 thdot^2 + 0.001 u^2 with the squares as products (the
    host's `**` is pow, which differs from the product in about 1 case in 1000: the reward is held to one ulp, 2^-52);
  * thdot' = thdot + (-3 g / (2 l) sin(th + pi) + 3 / (m l^2) u) dt;  th' = th + thdot' dt;  thdot' clipped to +-8 after that;
  * reward -cost * 0.005 - 1; done when elapsed >= 200; observation [cos th, sin th, thdot] in f64, cast to f32;
  * reset: th = -pi + 2 pi u0, thdot = -1 + 2 u1 (numpy's low + (high - low) u), two draws, the observation left alone;
  * angle_normalize is numpy's float remainder: m = fmod(x + pi, 2 pi), + 2 pi when m < 0, then - pi.
Absent, because the device's action cannot reach them: check_bounds(a, 1, -1, turnaround) and clip(u, -2, 2) are identities
on [-1, 1] and [-2, 2], and the action is atan2f(Y, X) / pi (or the zero vector of an environment's first ever step).
CONTINUOUS: the action is the prediction row itself; no draw, u = -1, and `draws` moves only at a reset.
"""
import numpy as np

import device_agents_oracle as o

G, M, L, DT, MAX_SPEED, ACTION_BOUND = 10.0, 1.0, 1.0, 0.05, 8.0, 2.0
TIME_LIMIT = 200


class ResetRNG(o.CounterRNG):
    """CounterRNG whose uniform takes array bounds, as Pendulum.reset gives them: one draw per element, in order."""

    def uniform(self, low=0.0, high=1.0, size=None):
        low, high = np.asarray(low, np.float64), np.asarray(high, np.float64)
        shape = np.broadcast(low, high).shape if size is None else tuple(np.atleast_1d(size))
        u = np.array([self.random() for _ in range(int(np.prod(shape)))], np.float64).reshape(shape)
        return low + (high - low) * u


def angle_normalize(x):
    m = np.fmod(np.float64(x) + np.pi, 2 * np.pi)
    if m < 0:
        m = m + 2 * np.pi
    return m - np.pi


class CartPoleEnv:
    """device_agents_oracle's CartPole as an environment of EnvActor."""
    STATE_DIM, NUM_ACTIONS, CONTINUOUS = o.STATE_DIM, o.NUM_ACTIONS, False

    @staticmethod
    def reset(rng):
        return rng.uniform(low=-0.05, high=0.05, size=(4,))

    @staticmethod
    def step(phys, action):
        return o.physics(phys, action), 1.0 * 0.005 - 1.0

    @staticmethod
    def over(phys):
        return o.fell(phys)

    @staticmethod
    def observe(phys):
        return np.asarray(phys, np.float64).astype(np.float32)

    @staticmethod
    def batch_actions(actions):
        return np.eye(o.NUM_ACTIONS, dtype=np.float32)[[int(k) for k in actions]]


class PendulumEnv:
    STATE_DIM, NUM_ACTIONS, CONTINUOUS = 3, 1, True

    @staticmethod
    def reset(rng):
        return rng.uniform(low=[-np.pi, -1.0], high=[np.pi, 1.0])

    @staticmethod
    def step(phys, action):
        """-> (new (th, thdot), reward) from the f32 action vector."""
        return PendulumEnv.physics(phys, np.float64(np.float32(np.asarray(action).reshape(-1)[0])))

    @staticmethod
    def physics(phys, a64):
        """-> (new (th, thdot), reward) from the action in f64: step's cast, or what check_bounds made of it
        (ddpg_actors_oracle.env_step)."""
        th, thdot = np.float64(phys[0]), np.float64(phys[1])
        u = np.float64(a64) * ACTION_BOUND
        an = angle_normalize(th)
        cost = an * an + 0.1 * (thdot * thdot) + 0.001 * (u * u)
        newthdot = thdot + (-3 * G / (2 * L) * np.sin(th + np.pi) + 3.0 / (M * L * L) * u) * DT
        newth = th + newthdot * DT
        newthdot = min(max(newthdot, -MAX_SPEED), MAX_SPEED)
        return np.array([newth, newthdot], np.float64), float(-cost * 0.005 - 1.0)

    @staticmethod
    def over(phys):
        return False

    @staticmethod
    def observe(phys):
        th, thdot = np.float64(phys[0]), np.float64(phys[1])
        return np.array([np.cos(th), np.sin(th), thdot], np.float64).astype(np.float32)

    @staticmethod
    def batch_actions(actions):
        return np.array(actions, np.float32).reshape(len(actions), 1)


class EnvActor(o.Actor):
    """device_agents_oracle.Actor with the environment passed in.  step() takes, besides `action` and `done`, a `reward`
    to use instead of the oracle's own, so that a host's or a device's trajectory can be followed."""

    def __init__(self, seed, env, time_max, gamma, game=PendulumEnv):
        self.game = game
        self.rng = ResetRNG(seed, env)
        self.time_max, self.gamma = int(time_max), float(gamma)
        self.phys = game.reset(self.rng)            # Environment.__init__ resets once, the first run_episode once more
        self.phys = game.reset(self.rng)
        self.elapsed = 0
        self.time_count = 0
        self.started = False
        self.obs = np.zeros(game.STATE_DIM, np.float32)
        self.rollout = []                           # [state f32[S], action, reward f64]
        self.reward_sum = 0.0
        self.total_reward = 0.0
        self.total_length = 0
        self.forced_reward = None                   # set by PendulumActors.step for the next step

    def step(self, p, action=None, done=None, reward=None):
        game = self.game
        out = dict(u=-1.0, cut=None, episode=None)
        if reward is None:
            reward, self.forced_reward = self.forced_reward, None
        if game.CONTINUOUS:                         # the action is the prediction row; step(None) is the zero vector
            own_action = np.array(p, np.float32).reshape(-1) if self.started else np.zeros(game.NUM_ACTIONS, np.float32)
            act = own_action if action is None else np.array(action, np.float32).reshape(-1)
        else:
            own_action = 0
            if self.started:
                out["u"] = self.rng.random()
                own_action = o.select(p, out["u"])
            act = own_action if action is None else int(action)
        state_before = self.obs.copy()
        self.phys, own_reward = game.step(self.phys, act)
        self.elapsed += 1
        own_done = game.over(self.phys) or self.elapsed >= TIME_LIMIT
        d = own_done if done is None else bool(done)
        reward = own_reward if reward is None else float(reward)
        out.update(action=act, own_action=own_action, reward=reward, own_reward=own_reward, done=d, own_done=own_done)
        self.obs = game.observe(self.phys)
        if not self.started:
            self.started = True
            return out
        self.reward_sum += reward
        self.rollout.append([state_before, act, reward])
        if d or self.time_count == self.time_max:
            y = o.returns_fork([r for _, _, r in self.rollout], self.gamma, reward)
            x = np.array([s for s, _, _ in self.rollout], np.float32)
            a = game.batch_actions([k for _, k, _ in self.rollout])
            out["cut"] = (x, a, y.astype(np.float32))
            self.total_reward += self.reward_sum
            self.total_length += len(self.rollout) + 1
            self.time_count = 0
            self.rollout = [self.rollout[-1]]
            self.reward_sum = 0.0
            if d:
                out["episode"] = (self.total_reward, self.total_length)
                self.total_reward, self.total_length = 0.0, 0
                self.phys = game.reset(self.rng)
                self.elapsed = 0
                self.rollout = []
        if not d:
            self.time_count += 1
        return out


class PendulumActors(o.Actors):
    """N Pendulum environments stepped together; the batch and the episode list are device_agents_oracle.Actors.step's."""

    def __init__(self, n, seed, time_max, gamma, game=PendulumEnv):
        self.env = [EnvActor(seed, i, time_max, gamma, game) for i in range(n)]

    def step(self, p, actions=None, dones=None, rewards=None):
        if rewards is not None:
            for e, r in zip(self.env, rewards):
                e.forced_reward = float(r)
        return super().step(p, actions, dones)
