"""Vector-state environment of Config.GAME = 'CartPole-v0' (the reference runs it through the wrapper it uses for Pendulum,
ga3c/EnvironmentPend.py:43-99, with DISCRATE_INPUT set by Server.py:40-43), with gym's classic-control CartPole-v0 restated
in numpy: gym is not part of this image and nothing is downloaded.

CartPole-v0 (gym/envs/classic_control/cartpole.py, TimeLimit 200), state (x, xdot, th, thdot), two actions:
    gravity = 9.8, masscart = 1.0, masspole = 0.1, length = 0.5 (half the pole), force_mag = 10, tau = 0.02, Euler
    f = +force_mag for action 1, -force_mag for action 0
    temp  = (f + 0.05 thdot^2 sin th) / 1.1
    thacc = (g sin th - cos th temp) / (0.5 (4/3 - 0.1 cos^2 th / 1.1))
    xacc  = temp - 0.05 thacc cos th / 1.1
    x += tau xdot;  xdot += tau xacc;  th += tau thdot;  thdot += tau thacc            (in that order)
    done when |x| > 2.4 or |th| > 12 degrees, or after 200 steps;  reward 1 per step;  reset: U(-0.05, 0.05)^4

The reference's wrapper around it, kept as it is:
  * current_state is None only before the agent's first episode, which therefore begins with one step of action 0
    (ProcessAgent.py:127-129 calls step(None) while it is None; EnvironmentPend.py:90-91 makes that action 0);
  * reset() resets the game and the step limit but not current_state: the first action of every later episode is predicted
    from the previous episode's last observation;
  * the reward handed on is r * 0.005 - 1, i.e. -0.995 on every step.
Deviations:
  * the reference's wrapper cannot run this game: it hands gym a one-hot integer array (EnvironmentPend.py:89-92) where
    Discrete.contains wants an index.  Here the index itself is passed;
  * gym's seeding stream cannot be reproduced without gym.  The draws come from PCG64(RANDOM_SEED + agent id), as
    Environment.py's and EnvironmentPend.py's do; the reference seeds every agent's game with the same RANDOM_SEED.
Parity with gym itself is unpinned (gym is absent), as for Pendulum.
"""
import numpy as np

from Config import Config

GAME = 'CartPole-v0'
STATE_DIM = 4
NUM_ACTIONS = 2
GRAVITY = 9.8
MASSCART = 1.0
MASSPOLE = 0.1
TOTAL_MASS = MASSPOLE + MASSCART
LENGTH = 0.5                # half the pole's length
POLEMASS_LENGTH = MASSPOLE * LENGTH
FORCE_MAG = 10.0
TAU = 0.02
THETA_LIMIT = 12 * 2 * np.pi / 360
X_LIMIT = 2.4
TIME_LIMIT = 200


class CartPole:
    """gym's CartPole-v0 with its TimeLimit wrapper."""

    def __init__(self, rng):
        self.rng = rng
        self.state = None
        self.elapsed = 0

    def reset(self):
        self.state = self.rng.uniform(low=-0.05, high=0.05, size=(4,))
        self.elapsed = 0
        return np.array(self.state)

    def step(self, action):
        action = int(action)
        if action not in (0, 1):
            raise ValueError("action %r is not 0 or 1" % (action,))
        x, x_dot, theta, theta_dot = self.state
        force = FORCE_MAG if action == 1 else -FORCE_MAG
        costheta, sintheta = np.cos(theta), np.sin(theta)
        temp = (force + POLEMASS_LENGTH * theta_dot ** 2 * sintheta) / TOTAL_MASS
        thetaacc = (GRAVITY * sintheta - costheta * temp) / (LENGTH * (4.0 / 3.0 - MASSPOLE * costheta ** 2 / TOTAL_MASS))
        xacc = temp - POLEMASS_LENGTH * thetaacc * costheta / TOTAL_MASS
        x = x + TAU * x_dot
        x_dot = x_dot + TAU * xacc
        theta = theta + TAU * theta_dot
        theta_dot = theta_dot + TAU * thetaacc
        self.state = np.array([x, x_dot, theta, theta_dot])
        self.elapsed += 1
        fell = bool(x < -X_LIMIT or x > X_LIMIT or theta < -THETA_LIMIT or theta > THETA_LIMIT)
        return np.array(self.state), 1.0, fell or self.elapsed >= TIME_LIMIT


class Environment:
    vector_state = True
    on_device = False           # (the agent loop asks: no frame queue on the device)

    def __init__(self, agent_id=0):
        self.game = CartPole(np.random.Generator(np.random.PCG64(Config.RANDOM_SEED + int(agent_id))))
        self.previous_state = None
        self.current_state = None
        self.total_reward = 0
        self.action_dim = NUM_ACTIONS
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
            action = 0
        self.previous_state = self.current_state
        obs, reward, done = self.game.step(action)
        self.current_state = np.asarray(obs, dtype=np.float32).reshape(-1)
        return reward * 0.005 - 1.0, done
