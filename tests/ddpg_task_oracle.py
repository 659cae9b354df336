"""Oracle of the task of the DDPG device actors and evaluation episodes (Config.DEVICE_DDPG_ACTION_BOUND, _TIME_LIMIT,
_RESET_OBSERVATION, _REWARD_SCALE, _REWARD_OFFSET, ga3c_ddpg_task_*; the kernels are ddpg_actors_step_kernel,
ddpg_actors_nstep_kernel and ddpg_eval_kernel of csrc/ga3c_ddpg.hip, which take the task from their arguments, 8w), restated in numpy on ddpg_actors_oracle and
device_pendulum_oracle.

A task is Task(bound, time_limit, reset_observation, reward_scale, reward_offset); FORK = ('wrap', 'terminal', False, 0.005,
-1.0) is EnvironmentPend.Environment's, what ddpg_actors_oracle states.  A non-first actor step of an environment, for the f32
action a as predicted (actor + noise):
  * bound: v = (f64) a.  'wrap': ddpg_actors_oracle.check_bounds.  'clip': v < -1 -> -1, v > 1 -> 1, which is
    EnvironmentPend.check_bounds(a, 1, -1, turnaround=False).  Then PendulumEnv's physics and cost on u = 2 v, unchanged;
    2 clip(a) is gym's clip(2 a, -2, 2) exactly, so gym's own clip stays an identity and stays absent;
  * reward = -cost * reward_scale + reward_offset in f64, in that operand order; at (0.005, -1.0) the bits of -cost * 0.005 - 1.0;
  * ended = elapsed' >= 200; terminal = ended and time_limit == 'terminal';
  * the transition is obs | a as predicted | (f32) reward | terminal ? 1 : 0 | obs', obs' the observation of the physics after
    the step and BEFORE any reset: under 'truncate' the state the bootstrap reads;
  * the actor's `done`, the episode record, the reset and its two draws follow `ended`; with reset_observation the environment's
    observation then becomes observe(reset physics) and the next transition starts there; without it the observation stays;
  * the first ever step(None) stays as it was.
n-step returns (nstep_oracle's delay line): the sum is cut at `ended`, and the row's done is the `terminal` of the last transition
summed, so a row cut by a truncating time limit is s_u | a_u | R | 0 | s2_{u+m-1} with disc = (f32) gamma^m.
Evaluation episodes (ddpg_eval_oracle): only the reward differs -- after tanh no bound is reached, there is no ring and no reset.
"""
from collections import namedtuple

import numpy as np

import ddpg_actors_oracle as do
import device_pendulum_oracle as po
import nstep_oracle as ns

Task = namedtuple("Task", "bound time_limit reset_observation reward_scale reward_offset")
FORK = Task('wrap', 'terminal', False, 0.005, -1.0)
GYM = Task('clip', 'truncate', True, 1.0, 0.0)
S, A = do.S, do.A


def clip_bounds(a):
    """EnvironmentPend.check_bounds(a, 1, -1, False) on one f32 action -> f64."""
    v = np.float64(np.float32(a))
    if v < -1.0:
        v = np.float64(-1.0)
    if v > 1.0:
        v = np.float64(1.0)
    return v


def bound(task, a):
    return clip_bounds(a) if task.bound == 'clip' else do.check_bounds(a)


def physics_cost(phys, v64):
    """-> (new (th, thdot), cost): PendulumEnv.physics's arithmetic with the cost handed on in the reward's place."""
    th, thdot = np.float64(phys[0]), np.float64(phys[1])
    u = np.float64(v64) * po.ACTION_BOUND
    an = po.angle_normalize(th)
    cost = an * an + 0.1 * (thdot * thdot) + 0.001 * (u * u)
    newthdot = thdot + (-3 * po.G / (2 * po.L) * np.sin(th + np.pi) + 3.0 / (po.M * po.L * po.L) * u) * po.DT
    newth = th + newthdot * po.DT
    newthdot = min(max(newthdot, -po.MAX_SPEED), po.MAX_SPEED)
    return np.array([newth, newthdot], np.float64), np.float64(cost)


def reward_of(task, cost):
    """-cost * scale + offset in f64, in that order; works on arrays."""
    return -np.asarray(cost, np.float64) * np.float64(task.reward_scale) + np.float64(task.reward_offset)


def env_step(task, phys, action):
    """-> (new (th, thdot), reward) from the f32 action vector under `task`."""
    stepped, cost = physics_cost(phys, bound(task, np.asarray(action, np.float32).reshape(-1)[0]))
    return stepped, float(reward_of(task, cost))


class Actor(do.Actor):
    """ddpg_actors_oracle.Actor under a task.  step's dict also has `terminal`; its `done` is `ended`, what the actor field and
    the episode follow; the row's done is `terminal`."""

    def __init__(self, seed, env, task=FORK):
        super().__init__(seed, env)
        self.task = task

    def step(self, action, reward=None):
        task = self.task
        first = action is None
        act = np.zeros(A, np.float32) if first else np.array(action, np.float32).reshape(A)
        before = self.obs.copy()
        self.phys, own_reward = env_step(task, self.phys, act)
        self.elapsed += 1
        ended = self.elapsed >= po.TIME_LIMIT
        terminal = ended and task.time_limit == 'terminal'
        self.obs = po.PendulumEnv.observe(self.phys)
        reward = own_reward if reward is None else float(reward)
        out = dict(row=None, episode=None, reward=reward, own_reward=own_reward, done=ended, terminal=terminal, action=act)
        if first:
            return out
        out["row"] = (before, act, np.float32(reward), np.float32(1.0 if terminal else 0.0), self.obs.copy())
        self.total_reward += reward
        self.total_length += 1
        if ended:
            out["episode"] = (self.total_reward, self.total_length + 1)
            self.total_reward, self.total_length = 0.0, 0
            self.phys = po.PendulumEnv.reset(self.rng)
            self.elapsed = 0
            if task.reset_observation:
                self.obs = po.PendulumEnv.observe(self.phys)
        return out


class Actors(do.Actors):
    """N environments of one handle under one task; step as ddpg_actors_oracle.Actors.step."""

    def __init__(self, n, seed, task=FORK):
        self.env = [Actor(seed, i, task) for i in range(n)]
        self.started = False


def nstep_row(entries, gamma):
    """entries: the transitions (s, a, r f64, ended, terminal, s2) from u on, oldest first, at most n of them -> (row, disc):
    nstep_oracle.nstep_row with the cut at `ended` and the row's done the `terminal` of the last transition summed."""
    g64 = ns.gamma64(gamma)
    R, g, last = 0.0, 1.0, None
    for t in entries:
        R = R + g * float(t[2])
        g = g * g64
        last = t
        if t[3]:
            break
    return (entries[0][0], entries[0][1], np.float32(R), np.float32(1.0 if last[4] else 0.0), last[5]), np.float32(g)


class NStepActors(Actors):
    """Actors whose transitions pass through nstep_oracle's delay line, cut as nstep_row above cuts them.  step(actions, s2=None)
    -> (emitted [(row, disc)] in environment order, empty on a silent step; episode records; the per-environment outputs)."""

    def __init__(self, n_env, seed, n, gamma, task=FORK):
        super().__init__(n_env, seed, task)
        self.n, self.gamma, self.count = int(n), gamma, 0
        self.win = [[None] * self.n for _ in range(n_env)]

    def step(self, actions=None, rewards=None, s2=None):
        rows, episodes, outs = super().step(actions, rewards)
        if not rows:
            return [], episodes, outs
        n, c = self.n, self.count
        for i, (w, row, out) in enumerate(zip(self.win, rows, outs)):
            w[c % n] = (row[0], row[1], np.float64(out["reward"]), bool(out["done"]), bool(out["terminal"]),
                        row[4] if s2 is None else np.array(s2[i], np.float32))
        self.count += 1
        if c < n - 1:
            return [], episodes, outs
        oldest = (c + 1) % n
        return [nstep_row([w[(oldest + k) % n] for k in range(n)], self.gamma) for w in self.win], episodes, outs


def step_many(task, phys, action):
    """ddpg_eval_oracle.step_many under a task -> (new physics f64 [n, 2], reward f64 [n], observation f32 [n, S])."""
    phys = np.asarray(phys, np.float64).reshape(-1, 2)
    th, thdot = phys[:, 0], phys[:, 1]
    v = np.asarray(action, np.float32).reshape(-1).astype(np.float64)
    if task.bound == 'clip':
        v = np.where(v < -1.0, -1.0, v)
        v = np.where(v > 1.0, 1.0, v)
    else:
        with np.errstate(invalid="ignore"):
            v = np.where(v < -1.0, 1.0 - np.fmod(-1.0 - v, 2.0), v)
            v = np.where(v > 1.0, np.fmod(v - 1.0, 2.0) - 1.0, v)
    u = v * po.ACTION_BOUND
    m = np.fmod(th + np.pi, 2 * np.pi)
    an = np.where(m < 0, m + 2 * np.pi, m) - np.pi
    cost = an * an + 0.1 * (thdot * thdot) + 0.001 * (u * u)
    newthdot = thdot + (-3 * po.G / (2 * po.L) * np.sin(th + np.pi) + 3.0 / (po.M * po.L * po.L) * u) * po.DT
    newth = th + newthdot * po.DT
    newthdot = np.minimum(np.maximum(newthdot, -po.MAX_SPEED), po.MAX_SPEED)
    obs = np.stack([np.cos(newth), np.sin(newth), newthdot], axis=1).astype(np.float32)
    return np.stack([newth, newthdot], axis=1), reward_of(task, cost), obs


def gym_return(task, mean_total, steps):
    """The mean return gym's Pendulum-v0 would report: undoes the task's scale and offset per step."""
    return (float(mean_total) - steps * task.reward_offset) / task.reward_scale
