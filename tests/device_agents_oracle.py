"""Oracle of the device actors (Config.DEVICE_AGENTS; csrc/ga3c_actors.hpp): one actor step and its
bookkeeping restated in numpy f64, with the counter-based uniforms the device draws.

What it restates is ProcessAgent.run_episode / run over EnvironmentCart.Environment with RETURN_MODE = 'fork':
  * an environment's first ever step is action 0 with no prediction, no draw and no experience, and its `done` is ignored;
  * reset() redraws the physics from four uniforms in (-0.05, 0.05), clears `elapsed` and leaves the observation alone;
  * reward r * 0.005 - 1; done on |x| > 2.4, |th| > THETA_LIMIT or elapsed >= 200;
  * a rollout is cut on done or when time_count == TIME_MAX, and within an episode its last row is row 0 of the next;
  * the fork's returns (DISCOUNTING, no intermediate rewards) in f64 by sequential products, terminal_reward = the last
    reward, cast to f32 where they become y_r;
  * total_reward / total_length count reward_sum and len(rollout) + 1 per rollout, as run() does;
  * the action is ga3c_select_action's: sequential f64 cumulative sum of the f32 policy, first i with u < cdf[i] / cdf[-1].
tests/test_device_agents_cpu.py holds this file to the real ProcessAgent bit for bit; tests/test_gpu_device_agents.py holds
the device to this file.

The uniforms -- the one thing that is the device's own, not the host agents':
    mix(z):  z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9;  z = (z ^ z >> 27) * 0x94D049BB133111EB;  z ^ z >> 31      (splitmix64)
    u(seed, env, draw) = (mix(mix(seed + G (env + 1)) + G (draw + 1)) >> 11) * 2^-53,   G = 0x9E3779B97F4A7C15,  mod 2^64
An action takes one draw, a reset four; an environment's draws are numbered in the order it takes them, an environment
starts with eight drawn: the reset that makes it took 0..3 and the one that begins its first episode 4..7.
"""
import numpy as np

GOLDEN = np.uint64(0x9E3779B97F4A7C15)
M1 = np.uint64(0xBF58476D1CE4E5B9)
M2 = np.uint64(0x94D049BB133111EB)

GRAVITY, MASSCART, MASSPOLE, LENGTH, FORCE_MAG, TAU = 9.8, 1.0, 0.1, 0.5, 10.0, 0.02
TOTAL_MASS = MASSPOLE + MASSCART
POLEMASS_LENGTH = MASSPOLE * LENGTH
THETA_LIMIT = 12 * 2 * np.pi / 360
X_LIMIT = 2.4
TIME_LIMIT = 200
STATE_DIM, NUM_ACTIONS = 4, 2


def mix64(z):
    z = np.atleast_1d(np.asarray(z, np.uint64))                # (arrays wrap silently; numpy warns about scalars)
    z = (z ^ (z >> np.uint64(30))) * M1
    z = (z ^ (z >> np.uint64(27))) * M2
    return z ^ (z >> np.uint64(31))


def uniform(seed, env, draw):
    """u(seed, env, draw) of the module text, elementwise over env and draw; seed as the 64 bits of an int64."""
    with np.errstate(over="ignore"):
        seed = np.atleast_1d(np.asarray(np.int64(seed))).astype(np.uint64)
        env, draw = np.asarray(env).astype(np.uint64), np.asarray(draw).astype(np.uint64)
        shape = np.broadcast(env, draw).shape
        stream = mix64((seed + GOLDEN * (np.atleast_1d(env) + np.uint64(1))).reshape(-1)).reshape(np.shape(env) or (1,))
        bits = mix64((stream + GOLDEN * (np.atleast_1d(draw) + np.uint64(1))).reshape(-1))
    return ((bits >> np.uint64(11)).astype(np.float64) * 2.0 ** -53).reshape(shape)


class CounterRNG:
    """The uniforms of one environment in the order it takes them.  random() is what an action draws; uniform(low, high,
    size) is numpy's Generator.uniform on this stream, low + (high - low) u, which is what CartPole.reset calls."""

    def __init__(self, seed, env, draws=0):
        self.seed, self.env, self.draws = int(seed), int(env), int(draws)

    def random(self):
        u = float(uniform(self.seed, self.env, self.draws))
        self.draws += 1
        return u

    def uniform(self, low=0.0, high=1.0, size=None):
        n = int(np.prod(size)) if size is not None else 1
        u = np.array([self.random() for _ in range(n)], np.float64)
        out = low + (high - low) * u
        return out.reshape(size) if size is not None else out[0]


def select(p, u):
    """ga3c_select_action."""
    p = np.asarray(p, np.float32)
    cdf, acc = [], np.float64(0.0)
    for t in p:
        acc = acc + np.float64(t)
        cdf.append(acc)
    for i, c in enumerate(cdf):
        if u < c / cdf[-1]:
            return i
    return len(cdf) - 1


def cdf_edges(p):
    """The normalised cdf select() compares u with."""
    cdf = np.cumsum(np.asarray(p, np.float32).astype(np.float64))
    return cdf / cdf[-1]


def physics(state, action):
    """One Euler step of gym's CartPole on np.float64 scalars -> the new (x, xdot, th, thdot)."""
    x, x_dot, theta, theta_dot = (np.float64(t) for t in state)
    force = FORCE_MAG if int(action) == 1 else -FORCE_MAG
    costheta, sintheta = np.cos(theta), np.sin(theta)
    temp = (force + POLEMASS_LENGTH * theta_dot ** 2 * sintheta) / TOTAL_MASS
    thetaacc = (GRAVITY * sintheta - costheta * temp) / (LENGTH * (4.0 / 3.0 - MASSPOLE * costheta ** 2 / TOTAL_MASS))
    xacc = temp - POLEMASS_LENGTH * thetaacc * costheta / TOTAL_MASS
    x = x + TAU * x_dot
    x_dot = x_dot + TAU * xacc
    theta = theta + TAU * theta_dot
    theta_dot = theta_dot + TAU * thetaacc
    return np.array([x, x_dot, theta, theta_dot], np.float64)


def fell(state):
    x, _, theta, _ = state
    return bool(x < -X_LIMIT or x > X_LIMIT or theta < -THETA_LIMIT or theta > THETA_LIMIT)


def returns_fork(rewards, gamma, terminal_reward):
    """ga3c_returns_fork with DISCOUNTING and without intermediate rewards, f64."""
    out = [float(r) for r in rewards]
    reward_sum = float(terminal_reward)
    for t in range(len(out) - 2, -1, -1):
        reward_sum = gamma * reward_sum
        out[t] = reward_sum
    return np.array(out, np.float64)


class Actor:
    """One environment and the agent bookkeeping around it."""

    def __init__(self, seed, env, time_max, gamma):
        self.rng = CounterRNG(seed, env)
        self.time_max, self.gamma = int(time_max), float(gamma)
        self.phys = self.rng.uniform(low=-0.05, high=0.05, size=(4,))       # Environment.__init__ resets once (draws 0..3),
        self.phys = self.rng.uniform(low=-0.05, high=0.05, size=(4,))       # the first run_episode once more (draws 4..7)
        self.elapsed = 0
        self.time_count = 0
        self.started = False                                                # current_state is None
        self.obs = np.zeros(STATE_DIM, np.float32)
        self.rollout = []                                                   # [state f32[S], action, reward f64]
        self.reward_sum = 0.0
        self.total_reward = 0.0
        self.total_length = 0

    def step(self, p, action=None, done=None):
        """One agent step on the policy row p (ignored on the first ever step).  `action` / `done` given: taken instead of
        the oracle's own (the draw is still counted), so that a device's trajectory can be followed.
        -> dict(u, action, reward, done, cut, episode): cut = (x f32[T,S], a f32[T,A] one-hot, y_r f32[T]) or None,
        episode = (total_reward, total_length) or None."""
        out = dict(u=-1.0, cut=None, episode=None)
        own_action = 0
        if self.started:
            out["u"] = self.rng.random()
            own_action = select(p, out["u"])
        act = own_action if action is None else int(action)
        state_before = self.obs.copy()
        self.phys = physics(self.phys, act)
        self.elapsed += 1
        own_done = fell(self.phys) or self.elapsed >= TIME_LIMIT
        d = own_done if done is None else bool(done)
        reward = 1.0 * 0.005 - 1.0
        out.update(action=act, own_action=own_action, reward=reward, done=d, own_done=own_done)
        self.obs = self.phys.astype(np.float32)
        if not self.started:
            self.started = True
            return out
        self.reward_sum += reward
        self.rollout.append([state_before, act, reward])
        if d or self.time_count == self.time_max:
            y = returns_fork([r for _, _, r in self.rollout], self.gamma, reward)
            x = np.array([s for s, _, _ in self.rollout], np.float32)
            a = np.eye(NUM_ACTIONS, dtype=np.float32)[[k for _, k, _ in self.rollout]]
            out["cut"] = (x, a, y.astype(np.float32))
            self.total_reward += self.reward_sum
            self.total_length += len(self.rollout) + 1
            self.time_count = 0
            self.rollout = [self.rollout[-1]]
            self.reward_sum = 0.0
            if d:
                out["episode"] = (self.total_reward, self.total_length)
                self.total_reward, self.total_length = 0.0, 0
                self.phys = self.rng.uniform(low=-0.05, high=0.05, size=(4,))
                self.elapsed = 0
                self.rollout = []
        if not d:
            self.time_count += 1
        return out


class Actors:
    """N environments stepped together, as the device steps them: the batch of a step is the cut rollouts in environment
    order, its episode records likewise."""

    def __init__(self, n, seed, time_max, gamma):
        self.env = [Actor(seed, i, time_max, gamma) for i in range(n)]

    def step(self, p, actions=None, dones=None):
        res = [e.step(p[i], None if actions is None else actions[i], None if dones is None else dones[i])
               for i, e in enumerate(self.env)]
        cuts = [r["cut"] for r in res if r["cut"] is not None]
        batch = tuple(np.concatenate([c[k] for c in cuts]) for k in range(3)) if cuts else None
        episodes = [r["episode"] for r in res if r["episode"] is not None]
        return res, batch, episodes
