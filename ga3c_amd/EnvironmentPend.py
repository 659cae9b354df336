"""Vector-state environment of Config.GAME = 'Pendulum-v0' (reference ga3c/EnvironmentPend.py:44-99), with gym's
classic-control Pendulum-v0 restated in numpy: gym is not part of this image and nothing is downloaded.

Pendulum-v0 (gym/envs/classic_control/pendulum.py, TimeLimit 200):
    g = 10, m = l = 1, dt = 0.05, max_speed = 8, max_torque = 2
    u = clip(u, -2, 2);  cost = angle_normalize(th)^2 + 0.1 thdot^2 + 0.001 u^2;  reward = -cost
    thdot' = thdot + (-3 g / (2 l) sin(th + pi) + 3 / (m l^2) u) dt;  th' = th + thdot' dt;  thdot' = clip(thdot', -8, 8)
    observation [cos th, sin th, thdot];  reset: th ~ U(-pi, pi), thdot ~ U(-1, 1);  done after 200 steps

The reference's wrapper around it, kept as it is:
  * current_state is None only before the agent's first episode, which therefore begins with one zero-torque step
    (ProcessAgent.py:127-129 calls step(None) while it is None);
  * reset() resets the pendulum and the step limit but not current_state: the first action of every later episode is
    predicted from the previous episode's last observation (EnvironmentPend.py:76-79 discards reset's observation);
  * the action goes through check_bounds(a, 1, -1, turnaround=True) (PyperEnvironment.py:42-55) and is then multiplied
    by the action bound 2; the reward handed on is r * 0.005 - 1.
Deviation: gym's seeding stream cannot be reproduced without gym.  The draws come from PCG64(RANDOM_SEED + agent id), as
Environment.py's do; the reference seeds every agent's game with the same RANDOM_SEED.
"""
import numpy as np

from Config import Config

GAME = 'Pendulum-v0'
STATE_DIM = 3
NUM_ACTIONS = 1
ACTION_BOUND = 2.0          # action_space.high
MAX_SPEED = 8.0
MAX_TORQUE = 2.0
DT = 0.05
G = 10.0
M = 1.0
L = 1.0
TIME_LIMIT = 200


def angle_normalize(x):
    return ((x + np.pi) % (2 * np.pi)) - np.pi


def check_bounds(value, posbound, negbound=0, turnaround=True):
    """PyperEnvironment.check_bounds, element by element (the reference calls it on a 1-element array)."""
    out = np.array(value, dtype=np.float64).reshape(-1)
    for i, v in enumerate(out):
        if turnaround is False:
            v = min(max(v, negbound), posbound)
        else:
            size = posbound - negbound
            if v < negbound:
                v = posbound - ((negbound - v) % size)
            if v > posbound:
                v = ((v - posbound) % size) + negbound
        out[i] = v
    return out


class Pendulum:
    """gym's Pendulum-v0 with its TimeLimit wrapper."""

    def __init__(self, rng):
        self.rng = rng
        self.state = None
        self.elapsed = 0

    def reset(self):
        self.state = self.rng.uniform(low=[-np.pi, -1.0], high=[np.pi, 1.0])
        self.elapsed = 0
        return self._obs()

    def _obs(self):
        th, thdot = self.state
        return np.array([np.cos(th), np.sin(th), thdot])

    def step(self, u):
        th, thdot = self.state
        u = float(np.clip(u, -MAX_TORQUE, MAX_TORQUE)[0])
        cost = angle_normalize(th) ** 2 + 0.1 * thdot ** 2 + 0.001 * (u ** 2)
        newthdot = thdot + (-3 * G / (2 * L) * np.sin(th + np.pi) + 3.0 / (M * L ** 2) * u) * DT
        newth = th + newthdot * DT
        newthdot = np.clip(newthdot, -MAX_SPEED, MAX_SPEED)
        self.state = np.array([newth, newthdot])
        self.elapsed += 1
        return self._obs(), -cost, self.elapsed >= TIME_LIMIT


class Environment:
    vector_state = True
    on_device = False           # (the agent loop asks: no frame queue on the device)

    def __init__(self, agent_id=0):
        self.game = Pendulum(np.random.Generator(np.random.PCG64(Config.RANDOM_SEED + int(agent_id))))
        self.previous_state = None
        self.current_state = None
        self.total_reward = 0
        self.action_dim = NUM_ACTIONS
        self.action_bound = ACTION_BOUND
        self.state_dim = STATE_DIM
        self.reset()

    def get_num_actions(self):
        return self.action_dim

    @staticmethod
    def get_state_dim():
        return (STATE_DIM,)

    # the state as the transport ships it (ProcessAgent.run_episode reads .current_u8): f32 [S], whatever STATE_TRANSPORT
    @property
    def current_u8(self):
        return self.current_state

    @property
    def previous_u8(self):
        return self.previous_state

    def reset(self):
        self.game.reset()

    def step(self, action):
        if action is None:
            action = np.zeros(self.action_dim)
        action = check_bounds(action, 1.0, -1.0, True)
        env_action = action * self.action_bound
        self.previous_state = self.current_state
        obs, reward, done = self.game.step(env_action)
        self.current_state = np.asarray(obs, dtype=np.float32).reshape(-1)
        return reward * 0.005 - 1.0, done
