"""Oracle of the DDPG device actors (Config.DEVICE_DDPG, ga3c_ddpg_actors_*; the kernels are
ddpg_actors_step_kernel<PendulumBounded>, ddpg_actors_episodes_kernel and ddpg_uniform_slots_kernel of csrc/ga3c_ddpg.hip): one
actor step, the ring it writes and the uniform draw of a train step's rows, restated in numpy.

What it restates is ProcessAgent.run_episode and _ship under USE_DDPG over EnvironmentPend.Environment:
  * the handle's first ever step is step(None) for every environment: the zero action, no transition, its done not looked at;
  * afterwards the action is the prediction row, f32 and unbounded (tanh output plus noise); the environment applies
    check_bounds(a, 1, -1, turnaround) to it in f64 -- below -1: 1 - (-1 - v) % 2, above 1: (v - 1) % 2 - 1 -- and steps
    device_pendulum_oracle.PendulumEnv's arithmetic on the result; clip(u, -2, 2) is an identity after the wrap;
  * the transition is obs | a as predicted | (f32) reward | done | obs'; reset() redraws the physics from two counter uniforms
    and leaves the observation alone, so a later episode's first transition starts from the last observation of the one before;
  * an episode's record is the f64 sum of its rewards in step order and its transitions + 1 (ProcessAgent.run for an episode
    shipped as one rollout, TIME_MAX >= 200; at a smaller TIME_MAX the host ships row 0 of a re-used rollout twice, the device
    writes every transition once);
  * transitions go to ring slot (rows ever added + i) mod capacity in environment order; with priorities the slot gets max_pa.
The uniforms are device_agents_oracle's: u(seed, environment, draw), two per reset, draws 0..1 passed over at create and 2..3
taken for the first physics.

The draw of a train step without priorities (the stated deviation from random.Random(seed).sample): row k of B from a ring of
size > B rows takes slot lo + min(hi - lo - 1, int(u (hi - lo))), lo = k size // B, hi = (k + 1) size // B,
u = u(draw_seed, sample number, k).  The strata are disjoint and none is empty: the slots are distinct.
"""
import numpy as np

import device_agents_oracle as o
import device_pendulum_oracle as po

S, A = 3, 1
ROWF = 2 * S + A + 2


def check_bounds(a):
    """EnvironmentPend.check_bounds(a, 1, -1, True) on one f32 action -> f64."""
    v = np.float64(np.float32(a))
    if v < -1.0:
        v = 1.0 - np.fmod(-1.0 - v, 2.0)
    if v > 1.0:
        v = np.fmod(v - 1.0, 2.0) - 1.0
    return np.float64(v)


def env_step(phys, action):
    """-> (new (th, thdot), reward): PendulumEnv's physics on the wrapped f64 action in the f32 action's place."""
    return po.PendulumEnv.physics(phys, check_bounds(np.asarray(action, np.float32).reshape(-1)[0]))


class Actor:
    """One environment.  step(None) is the first ever step; step(action) -> dict(row, episode, reward, done): row the
    transition (s, a, r f32, done f32, s2), episode None or (total_reward, total_length).  `reward`: use it instead of the
    oracle's own (to follow a host's rewards, whose `**` may differ from the product in the last bit)."""

    def __init__(self, seed, env):
        self.rng = po.ResetRNG(seed, env)
        self.phys = po.PendulumEnv.reset(self.rng)      # Environment.__init__ resets once, the first run_episode once more
        self.phys = po.PendulumEnv.reset(self.rng)
        self.elapsed = 0
        self.obs = np.zeros(S, np.float32)
        self.total_reward = 0.0
        self.total_length = 0

    def step(self, action, reward=None):
        first = action is None
        act = np.zeros(A, np.float32) if first else np.array(action, np.float32).reshape(A)
        before = self.obs.copy()
        self.phys, own_reward = env_step(self.phys, act)
        self.elapsed += 1
        done = self.elapsed >= po.TIME_LIMIT
        self.obs = po.PendulumEnv.observe(self.phys)
        reward = own_reward if reward is None else float(reward)
        out = dict(row=None, episode=None, reward=reward, own_reward=own_reward, done=done, action=act)
        if first:
            return out
        out["row"] = (before, act, np.float32(reward), np.float32(1.0 if done else 0.0), self.obs.copy())
        self.total_reward += reward
        self.total_length += 1
        if done:
            out["episode"] = (self.total_reward, self.total_length + 1)
            self.total_reward, self.total_length = 0.0, 0
            self.phys = po.PendulumEnv.reset(self.rng)
            self.elapsed = 0
        return out


def pack(row):
    s, a, r, d, s2 = row
    return np.concatenate([s, a, [r], [d], s2]).astype(np.float32)


class Ring:
    """The replay ring: rows [capacity, ROWF], rows ever added, and with priorities pa per slot and max_pa."""

    def __init__(self, capacity, prioritized=False):
        self.capacity, self.total = int(capacity), 0
        self.rows = np.zeros((self.capacity, ROWF), np.float32)
        self.pa = np.zeros(self.capacity, np.float32) if prioritized else None
        self.max_pa = np.float32(1.0)

    @property
    def size(self):
        return min(self.total, self.capacity)

    def add(self, rows):
        """-> the slots written, in the order of the rows."""
        slots = []
        for row in rows:
            slot = self.total % self.capacity
            self.rows[slot] = pack(row)
            if self.pa is not None:
                self.pa[slot] = self.max_pa
            self.total += 1
            slots.append(slot)
        return slots


class Actors:
    """N environments of one handle.  step(actions) with actions None on the first ever step, else [N, A] predictions
    -> (transitions in environment order, episode records in environment order)."""

    def __init__(self, n, seed):
        self.env = [Actor(seed, i) for i in range(n)]
        self.started = False

    def step(self, actions=None, rewards=None):
        assert (actions is None) == (not self.started)
        rows, episodes, outs = [], [], []
        for i, e in enumerate(self.env):
            r = e.step(None if actions is None else actions[i], None if rewards is None else rewards[i])
            outs.append(r)
            if r["row"] is not None:
                rows.append(r["row"])
            if r["episode"] is not None:
                episodes.append(r["episode"])
        self.started = True
        return rows, episodes, outs


def uniform_slots(seed, number, size, batch):
    """The draw of sample `number`: int32 [batch] distinct slots below `size` (size > batch)."""
    size, batch = int(size), int(batch)
    assert size > batch >= 1
    k = np.arange(batch, dtype=np.int64)
    lo, hi = k * size // batch, (k + 1) * size // batch
    w = hi - lo
    u = o.uniform(seed, int(number), k)
    j = (u * w.astype(np.float64)).astype(np.int64)
    return (lo + np.minimum(w - 1, j)).astype(np.int32)
