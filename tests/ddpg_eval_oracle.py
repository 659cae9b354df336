"""Oracle of the DDPG handle's evaluation episodes (Config.DEVICE_DDPG_EVAL_ENVS, ga3c_ddpg_eval_*; the kernel is
ddpg_eval_kernel<PendulumBounded> of csrc/ga3c_ddpg.hip): a whole noise-free episode restated in numpy.

  * environment i of n starts at th = -pi + 2 pi u(seed, i, 0), thdot = -1 + 2 u(seed, i, 1), device_agents_oracle.uniform's
    draws 0 and 1 of stream i, through Pendulum.reset's low + (high - low) u; elapsed = 0; every run starts there again;
  * a step: the observation [cos th, sin th, thdot] cast to f32, ddpg_oracle.actor_forward on it in f64, its tanh output cast to
    f32 -- the action, with no noise -- and ddpg_actors_oracle.env_step on that action: check_bounds, which is an identity after
    tanh, then the physics and the reward -cost * 0.005 - 1;
  * total = the f64 sum of the rewards in step order; done when elapsed reaches 200.
Nothing else exists: no first zero-action step (the start state is observed directly), no reset, no ring, no episode record.

step_many is env_step and PendulumEnv.observe for n environments at once, the same operations on arrays;
tests/test_ddpg_eval_cpu.py holds it to the two bit for bit, and the rollout to the real EnvironmentPend.Environment.
"""
import numpy as np

import ddpg_actors_oracle as do
import ddpg_oracle as o
import device_agents_oracle as ao
import device_pendulum_oracle as po

S, A = do.S, do.A
MAX_STEPS = po.TIME_LIMIT


def start_states(seed, n):
    """-> f64 [n, 2]: where the n evaluation environments of `seed` start."""
    env = np.arange(int(n))
    u0, u1 = ao.uniform(seed, env, 0), ao.uniform(seed, env, 1)
    return np.stack([-np.pi + (np.pi - -np.pi) * u0, -1.0 + (1.0 - -1.0) * u1], axis=1)


def policy(P, obs):
    """The actor's f32 actions [n] on f32 observations [n, S], computed in the precision of P's arrays; no noise."""
    obs = np.asarray(obs, np.float32).reshape(-1, S)
    return np.asarray(o.actor_forward(P, obs)["out"][:, 0], np.float64).astype(np.float32)


def step_many(phys, action):
    """-> (new physics f64 [n, 2], reward f64 [n], observation f32 [n, S]): ddpg_actors_oracle.env_step and
    PendulumEnv.observe, elementwise over n environments and their f32 actions [n]."""
    phys = np.asarray(phys, np.float64).reshape(-1, 2)
    th, thdot = phys[:, 0], phys[:, 1]
    v = np.asarray(action, np.float32).reshape(-1).astype(np.float64)
    with np.errstate(invalid="ignore"):
        v = np.where(v < -1.0, 1.0 - np.fmod(-1.0 - v, 2.0), v)           # check_bounds(a, 1, -1, turnaround)
        v = np.where(v > 1.0, np.fmod(v - 1.0, 2.0) - 1.0, v)
    u = v * po.ACTION_BOUND
    m = np.fmod(th + np.pi, 2 * np.pi)
    an = np.where(m < 0, m + 2 * np.pi, m) - np.pi
    cost = an * an + 0.1 * (thdot * thdot) + 0.001 * (u * u)
    newthdot = thdot + (-3 * po.G / (2 * po.L) * np.sin(th + np.pi) + 3.0 / (po.M * po.L * po.L) * u) * po.DT
    newth = th + newthdot * po.DT
    newthdot = np.minimum(np.maximum(newthdot, -po.MAX_SPEED), po.MAX_SPEED)
    obs = np.stack([np.cos(newth), np.sin(newth), newthdot], axis=1).astype(np.float32)
    return np.stack([newth, newthdot], axis=1), -cost * 0.005 - 1.0, obs


def observe_many(phys):
    phys = np.asarray(phys, np.float64).reshape(-1, 2)
    return np.stack([np.cos(phys[:, 0]), np.sin(phys[:, 0]), phys[:, 1]], axis=1).astype(np.float32)


def rollout(P, start, steps, rewards=None):
    """One episode of `steps` steps from every row of start [n, 2] under the actor of P.  rewards [n, steps] (optional): added up
    in the oracle's own rewards' place, to follow an environment whose `**` differs from the product in the last bit.
    -> dict: total f64 [n], phys f64 [n, 2] (after the last step), done bool [steps], and the trace trace_phys [n, steps, 2]
    (before step t), trace_obs f32 [n, steps, S], trace_action f32 [n, steps], trace_reward f64 [n, steps] (the oracle's own)."""
    phys = np.array(start, np.float64).reshape(-1, 2)
    n, steps = len(phys), int(steps)
    assert 1 <= steps <= MAX_STEPS
    out = dict(done=np.zeros(steps, bool), trace_phys=np.zeros((n, steps, 2), np.float64),
               trace_obs=np.zeros((n, steps, S), np.float32), trace_action=np.zeros((n, steps), np.float32),
               trace_reward=np.zeros((n, steps), np.float64))
    total, elapsed = np.zeros(n, np.float64), 0
    obs = observe_many(phys)
    for t in range(steps):
        action = policy(P, obs)
        out["trace_phys"][:, t], out["trace_obs"][:, t], out["trace_action"][:, t] = phys, obs, action
        phys, reward, obs = step_many(phys, action)
        elapsed += 1
        out["trace_reward"][:, t], out["done"][t] = reward, elapsed >= po.TIME_LIMIT
        total = total + (reward if rewards is None else np.asarray(rewards, np.float64)[:, t])
    out["total"], out["phys"] = total, phys
    return out


def gym_return(mean_total, steps):
    """The mean return gym's Pendulum-v0 would report: undoes the wrapper's r * 0.005 - 1 per step."""
    return (float(mean_total) + int(steps)) / 0.005
