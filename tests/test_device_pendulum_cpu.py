"""Device actors for Pendulum-v0 (Config.DEVICE_PENDULUM) on the CPU: tests/device_pendulum_oracle.py -- the
statement the device is held to -- against the real ProcessAgent.run_episode over EnvironmentPend.Environment; the oracle's
restated bookkeeping against device_agents_oracle.Actor; the branches the device leaves out; the Config gate; the six new
ABI entries; and a Server run that starts the device-agent thread and nothing else.

Exact against the agent: states, action vectors, physics, done, rollout boundaries, the length of every episode record.
Bounded: the reward.  EnvironmentPend squares with `**` (pow), the oracle and the device with a product; the two differ in
about 1 case in 1000, and a reward lies in [-1.09, -1], where one ulp is 2^-52: |r_oracle - r_env| <= 2^-52 on every step.
y_r and total_reward follow from the rewards, so they are compared bit for bit with the environment's own rewards fed to the
oracle."""
import os
import re

import numpy as np
import pytest

import device_agents_oracle as o
import device_pendulum_oracle as po

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED, GAMMA = 4242, 0.99
REWARD_BOUND = 2.0 ** -52


def swing(obs):
    """Stand-in policy of the observation: an f32 action vector in [-1, 1]."""
    t = np.float32(0.9) * np.float32(np.tanh(np.float32(2.0) * np.float32(obs[1]) + np.float32(0.3) * np.float32(obs[2])))
    return np.array([t + np.float32(0.05) * np.float32(obs[0])], np.float32)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _host_run(policy, time_max, episodes, env_id=0):
    """The real agent loop over EnvironmentPend.Environment with the oracle's counter uniforms behind the reset
    -> (rollouts, episode records, per-step log [(physics, reward, done)], last observation of every episode, index of every
    episode's first rollout)."""
    import ga3c_amd  # noqa: F401
    from Config import Config
    import EnvironmentPend
    from ProcessAgent import ProcessAgent

    saved = {k: getattr(Config, k) for k in ("TIME_MAX", "GAME", "RETURN_MODE", "DISCOUNTING", "USE_INTERMEDIATE_REWARD",
                                             "CONTINUOUS_INPUT", "PLAY_MODE", "STATE_TRANSPORT", "REWARD_CLIPPING")}
    Config.TIME_MAX, Config.GAME, Config.RETURN_MODE = time_max, 'Pendulum-v0', 'fork'
    Config.DISCOUNTING, Config.USE_INTERMEDIATE_REWARD, Config.CONTINUOUS_INPUT, Config.PLAY_MODE = True, False, True, False
    try:
        agent = ProcessAgent(env_id, "unused", None, config={"DISCOUNT": GAMMA})
        env = EnvironmentPend.Environment(env_id)
        env.game.rng = po.ResetRNG(SEED, env_id)
        env.reset()                                   # the reset that makes the environment: draws 0..1 (run_episode's: 2..3)
        agent.env, agent.num_actions, agent.actions = env, 1, np.arange(1)

        def predict_and_select(state, flags=0):
            p = policy(state)
            return p, np.float32(0.0), p.copy()       # CONTINUOUS_INPUT: the action is the prediction
        agent.predict_and_select = predict_and_select
        step, log = env.step, []

        def logged_step(action):
            reward, done = step(action)
            log.append((np.array(env.game.state, np.float64), float(reward), bool(done)))
            return reward, done
        env.step = logged_step
        rollouts, records, last_obs, firsts = [], [], [], []
        for _ in range(episodes):
            firsts.append(len(rollouts))
            total_reward, total_length = 0, 0
            for experiences, reward_sum in agent.run_episode():
                total_reward += reward_sum
                total_length += len(experiences) + 1
                x_, r_, a_, _, _ = agent.convert_data(experiences)
                rollouts.append((x_.astype(np.float32), a_, r_.astype(np.float32)))
            records.append((total_reward, total_length))
            last_obs.append(env.current_state.copy())
        return rollouts, records, log, last_obs, firsts
    finally:
        for k, v in saved.items():
            setattr(Config, k, v)


def _oracle_run(policy, time_max, steps, env_id=0, rewards=None):
    actor = po.EnvActor(SEED, env_id, time_max, GAMMA)
    rollouts, records, log = [], [], []
    for k in range(steps):
        r = actor.step(policy(actor.obs), reward=None if rewards is None else rewards[k])
        log.append((None if r["episode"] is not None else actor.phys.copy(), r["own_reward"], r["own_done"]))
        if r["cut"] is not None:
            rollouts.append(r["cut"])
        if r["episode"] is not None:
            records.append(r["episode"])
    assert actor.rng.draws == 4 + 2 * len(records)    # no draw for an action: two per reset
    return rollouts, records, log


@pytest.mark.parametrize("time_max", [1, 2, 5])
def test_oracle_is_process_agent(time_max):
    rollouts, records, log, last_obs, firsts = _host_run(swing, time_max, episodes=3)
    steps = len(log)
    assert steps == 3 * po.TIME_LIMIT                 # step(None) and 199 experiences, then 200 and 200
    own, own_records, own_log = _oracle_run(swing, time_max, steps)
    assert len(own) == len(rollouts) and len(own_records) == len(records) == 3
    # exact: states, action vectors, rollout boundaries, record lengths, physics, done; bounded: the reward
    for k, (h, w) in enumerate(zip(rollouts, own)):
        for name, hh, ww in zip(("states", "actions"), h[:2], w[:2]):
            assert hh.dtype == ww.dtype == np.float32 and hh.shape == ww.shape, (k, name, hh.shape, ww.shape)
            assert np.array_equal(_bits(hh), _bits(ww)), (k, name)
        assert h[2].shape == w[2].shape
    assert rollouts[0][1].shape[1:] == (1,) and rollouts[0][0].shape[1:] == (3,)
    assert [n for _, n in records] == [n for _, n in own_records]
    worst = 0.0
    for k, ((hp, hr, hd), (wp, wr, wd)) in enumerate(zip(log, own_log)):
        assert hd == wd, k
        if wp is not None:                            # (after a done the oracle holds the next episode's physics already)
            assert np.array_equal(_bits(hp), _bits(wp)), k
        worst = max(worst, abs(hr - wr))
        assert abs(hr - wr) <= REWARD_BOUND, (k, hr, wr)
    assert [k for k, entry in enumerate(log) if entry[2]] == [199, 399, 599]
    print("worst |r_oracle - r_env| = %.3e (bound %.3e)" % (worst, REWARD_BOUND))
    # fed the environment's own rewards, the returns and the episode totals are the agent's bit for bit
    fed, fed_records, _ = _oracle_run(swing, time_max, steps, rewards=[r for _, r, _ in log])
    for k, (h, w) in enumerate(zip(rollouts, fed)):
        assert h[2].dtype == w[2].dtype == np.float32 and np.array_equal(_bits(h[2]), _bits(w[2])), k
    for (hr_, hl), (or_, ol) in zip(records, fed_records):
        assert np.float64(hr_).view(np.uint64) == np.float64(or_).view(np.uint64) and int(hl) == int(ol)
    assert max(len(r[0]) for r in rollouts) == time_max + 1
    # the stale first observation: the first row of a later episode is the last observation of the one before, not the
    # observation of the physics the reset drew
    for ep in (1, 2):
        first = rollouts[firsts[ep]][0][0]
        assert np.array_equal(_bits(first), _bits(last_obs[ep - 1]))
        assert not np.array_equal(first, rollouts[firsts[ep] - 1][0][-1])     # (not a row carried over from the rollout before)


def test_restated_bookkeeping_is_device_agents_oracles():
    """EnvActor over CartPoleEnv against device_agents_oracle.Actor: the same uniforms, cuts, returns and records."""
    def topple(obs):
        w = np.float32(0.8) + np.float32(0.1) * np.float32(np.tanh(np.float32(obs[1])))
        return np.array([np.float32(1.0) - w, w], np.float32)
    for time_max in (1, 5):
        old, new = o.Actor(SEED, 3, time_max, GAMMA), po.EnvActor(SEED, 3, time_max, GAMMA, po.CartPoleEnv)
        cuts = episodes = 0
        for _ in range(150):
            a, b = old.step(topple(old.obs)), new.step(topple(new.obs))
            assert (a["u"], a["action"], a["reward"], a["done"]) == (b["u"], b["action"], b["reward"], b["done"])
            assert np.array_equal(_bits(old.phys), _bits(new.phys)) and np.array_equal(_bits(old.obs), _bits(new.obs))
            assert (old.elapsed, old.time_count, old.rng.draws, old.total_length) == \
                (new.elapsed, new.time_count, new.rng.draws, new.total_length)
            assert (a["cut"] is None) == (b["cut"] is None) and a["episode"] == b["episode"]
            if a["cut"] is not None:
                cuts += 1
                assert all(x.dtype == y.dtype and np.array_equal(_bits(x), _bits(y)) for x, y in zip(a["cut"], b["cut"]))
            episodes += a["episode"] is not None
        assert cuts > 20 and episodes >= 2


def test_angle_normalize_is_numpys_remainder():
    import ga3c_amd  # noqa: F401
    import EnvironmentPend
    rng = np.random.Generator(np.random.PCG64(1))
    xs = np.concatenate([rng.uniform(-90, 90, 20000), [0.0, np.pi, -np.pi, 3 * np.pi, -3 * np.pi, np.nextafter(np.pi, 4),
                                                        np.nextafter(-np.pi, -4), 2 * np.pi, -2 * np.pi]])
    for x in xs:
        assert np.float64(po.angle_normalize(x)).view(np.uint64) == np.float64(EnvironmentPend.angle_normalize(x)).view(np.uint64), x


def test_the_absent_branches_are_identities():
    """check_bounds(a, 1, -1, turnaround) and the torque clip on what the device's action can be: atan2f(Y, X) / pi lies in
    [-1, 1], the first step's action is 0."""
    import ga3c_amd  # noqa: F401
    import EnvironmentPend
    one = np.float32(1.0)
    for a in (-one, one, np.nextafter(one, np.float32(0)), np.nextafter(-one, np.float32(0)), np.float32(0.0)):
        action = np.array([a], np.float32)
        bounded = EnvironmentPend.check_bounds(action, 1.0, -1.0, True)
        assert bounded.dtype == np.float64 and np.array_equal(_bits(bounded), _bits(action.astype(np.float64)))
        torque = bounded * EnvironmentPend.ACTION_BOUND
        clipped = np.clip(torque, -EnvironmentPend.MAX_TORQUE, EnvironmentPend.MAX_TORQUE)
        assert np.array_equal(_bits(clipped), _bits(np.float64(a) * 2.0 * np.ones(1)))
    # ... and the largest quotient the head can give: atan2f(+-0, -1) / PI_F with the kernel's f32 constant
    pi_f = np.float32(3.14159265358979)
    for y in (np.float32(0.0), -np.float32(0.0)):
        assert abs(np.float32(np.arctan2(y, np.float32(-1.0))) / pi_f) <= one


BASE = dict(GAME='Pendulum-v0', DEVICE_AGENTS=64, DEVICE_PENDULUM=True, TIME_MAX=5, RETURN_MODE='fork', PLAY_MODE=False,
            DYNAMIC_SETTINGS=False, USE_DDPG=False, DISCOUNTING=True, USE_INTERMEDIATE_REWARD=False, DEVICE_AGENT_STEPS=32,
            DUAL_RMSPROP=False)
GATE = [
    (dict(DEVICE_PENDULUM=False), "CartPole-v0 only"),
    (dict(DEVICE_PENDULUM=False), "DEVICE_PENDULUM"),
    (dict(GAME='CartPole-v0'), "DEVICE_PENDULUM"),
    (dict(GAME='PongDeterministic-v4'), "DEVICE_PENDULUM"),
    (dict(USE_DDPG=True), "USE_DDPG"),
    (dict(USE_DDPG=True, DEVICE_PENDULUM=False), "USE_DDPG"),
    (dict(RETURN_MODE='nstep'), "RETURN_MODE"),
    (dict(PLAY_MODE=True), "PLAY_MODE"),
    (dict(DYNAMIC_SETTINGS=True), "DYNAMIC_SETTINGS"),
    (dict(DISCOUNTING=False), "DISCOUNTING"),
    (dict(USE_INTERMEDIATE_REWARD=True), "USE_INTERMEDIATE_REWARD"),
    (dict(DEVICE_AGENTS=65536 // 6 + 1), "max_batch"),
]


@pytest.mark.parametrize("case", GATE, ids=["%s_%d" % (sorted(c[0].items())[0][0], i) for i, c in enumerate(GATE)])
def test_the_gate(case, monkeypatch):
    import ga3c_amd  # noqa: F401
    import Config as cfg
    settings, message = case
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    assert cfg.Config.DEVICE_PENDULUM is False
    for k, v in BASE.items():
        monkeypatch.setattr(cfg.Config, k, v)
    cfg.resolve_device_agents()                       # Pendulum with the key passes
    monkeypatch.setattr(cfg.Config, "DUAL_RMSPROP", True)
    cfg.resolve_device_agents()                       # ... with two optimizers as well
    monkeypatch.setattr(cfg.Config, "DEVICE_AGENTS", 65536 // 6)
    cfg.resolve_device_agents()                       # ... up to max_batch rows
    monkeypatch.setattr(cfg.Config, "DEVICE_AGENTS", 64)
    for k, v in settings.items():
        monkeypatch.setattr(cfg.Config, k, v)
    with pytest.raises(ValueError, match=re.escape(message)):
        cfg.resolve_device_agents()
    monkeypatch.setattr(cfg.Config, "DEVICE_AGENTS", 0)         # off: nothing is checked
    cfg.resolve_device_agents()


def test_world_size_is_refused(monkeypatch):
    import ga3c_amd  # noqa: F401
    import Config as cfg
    for k, v in BASE.items():
        monkeypatch.setattr(cfg.Config, k, v)
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(ValueError, match="WORLD_SIZE"):
        cfg.resolve_device_agents()


def test_abi_entries_and_field_tables():
    import ga3c_amd  # noqa: F401
    import _native as nat
    import NetworkVP_discrate
    import NetworkVP_vecnet
    import NetworkVP_vector
    text = open(os.path.join(ROOT, "include", "ga3c_abi.h")).read()
    lib = nat.hip_lib()
    for entry in ("create", "destroy", "run", "episodes", "get", "set"):
        name = "ga3c_mlp_actors_" + entry
        assert re.search(r"\bint %s\s*\(ga3c_mlp\* net" % name, text), name
        assert nat.HIP_SIGNATURES[name] == nat.HIP_SIGNATURES["ga3c_dmlp_actors_" + entry], name
        assert hasattr(lib, name), name
    for module in (NetworkVP_discrate, NetworkVP_vector):
        assert issubclass(module.Network, NetworkVP_vecnet.DeviceActors)
        assert module.Network.ACTOR_FIELDS is module.ACTOR_FIELDS
        assert "actors_run" not in vars(module.Network)          # the methods are the mixin's
    assert NetworkVP_discrate.ACTOR_FIELDS["phys"] == (np.float64, "S") and NetworkVP_discrate.ACTOR_FIELDS["action"] == (np.int32, 1)
    assert NetworkVP_vector.ACTOR_FIELDS["phys"] == (np.float64, 2) and NetworkVP_vector.ACTOR_FIELDS["action"] == (np.float32, "A")
    assert set(NetworkVP_vector.ACTOR_FIELDS) == set(NetworkVP_discrate.ACTOR_FIELDS)


@pytest.mark.timeout(120)
def test_server_starts_the_device_agent_thread_and_nothing_else(tmp_path, monkeypatch):
    import ga3c_amd  # noqa: F401
    from Config import Config
    from test_device_agents_cpu import _StandInModel

    class StandIn(_StandInModel):
        """... with Pendulum environments behind actors_run, in lockstep as the device's are."""

        def actors_create(self, n, time_max, discount, seed):
            self.created = (n, time_max, discount, seed)
            self.actors = po.PendulumActors(n, seed, time_max, discount)
            self.batches = []

        def actors_run(self, steps, train=True):
            self.calls.append((steps, train))
            self.rates.append((self.learning_rate, self.beta))
            calls = rows = episodes = 0
            for _ in range(steps):
                _, batch, eps = self.actors.step(np.array([swing(e.obs) for e in self.actors.env]))
                if batch is not None:
                    calls, rows = calls + 1, rows + len(batch[2])
                    self.batches.append(len(batch[2]))
                self.pending += eps
                self.finished += eps
                episodes += len(eps)
            return len(self.actors.env) * steps, calls, rows, episodes

    monkeypatch.chdir(tmp_path)
    for k, v in dict(GAME='Pendulum-v0', DEVICE_AGENTS=6, DEVICE_PENDULUM=True, DEVICE_AGENT_STEPS=4, TIME_MAX=5,
                     DYNAMIC_SETTINGS=False, SAVE_MODELS=False, LEARNING_RATE_START=0.0007, LEARNING_RATE_END=0.0007,
                     USE_DDPG=False, RETURN_MODE='fork', PLAY_MODE=False, DISCOUNTING=True, USE_INTERMEDIATE_REWARD=False).items():
        monkeypatch.setattr(Config, k, v)
    for k in ("AGENTS", "PREDICTORS", "TRAINERS", "CONTINUOUS_INPUT", "DISCRATE_INPUT", "RANDOM_SEED"):
        monkeypatch.setattr(Config, k, getattr(Config, k))      # (Server resolves some of them: put back afterwards)
    import Server as server_module
    started = []
    for cls in ("ProcessAgent", "ThreadPredictor", "ThreadTrainer"):
        monkeypatch.setattr(server_module, cls, lambda *a, _c=cls, **k: started.append(_c))
    model = StandIn()
    srv = server_module.Server(model=model)
    srv.main(max_seconds=3)
    assert Config.CONTINUOUS_INPUT is True
    assert not started and not srv.agents and not srv.predictors and not srv.trainers
    assert srv.failure is None and not srv.dynamic_adjustment.is_alive() and srv.dynamic_adjustment.ident is None
    assert model.created == (6, 5, Config.DISCOUNT, Config.RANDOM_SEED) and model.destroyed
    assert model.calls and set(model.calls) == {(4, True)}
    agents = srv.device_agents
    assert agents is not None and not agents.is_alive()
    assert agents.agent_steps == 6 * 4 * len(model.calls) and srv.predictions_served == agents.agent_steps - 6
    assert srv.training_step == srv.stats.training_count.value == len(model.batches) > 0
    # lockstep: every train step takes every environment's rollout, 6 rows each (5 or 4 only where an episode ends)
    assert model.batches[0] == 6 * 6 and set(model.batches) <= {6 * 6, 6 * 5, 6 * 4}
    assert len(model.finished) % 6 == 0               # the environments finish their episodes on the same step
