"""Evaluation episodes of the DDPG handle (Config.DEVICE_DDPG_EVAL_ENVS) on the CPU: tests/ddpg_eval_oracle.py --
the statement the device is held to -- against the real EnvironmentPend.Environment driven by the same policy; the draw of the
start states; the Config rules; the five new ABI entries; ThreadDeviceAgents' schedule of evaluations with a stand-in model; and
a Server run with the key on.

Exact against the environment: physics, observations, actions.  Bounded: the reward -- EnvironmentPend squares with `**` (pow),
the oracle and the device with a product, and a reward lies in [-1.09, -1] where one ulp is 2^-52.  The totals
follow from the rewards, so they are compared bit for bit with the environment's own rewards fed to the oracle."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest

import ddpg_actors_oracle as do
import ddpg_eval_oracle as eo
import ddpg_oracle as o
import device_agents_oracle as ao
import device_pendulum_oracle as po

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ULP = 2.0 ** -52


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _eq(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _actor(seed, gain):
    """Test weights whose actor_output/W is scaled by `gain`: 0.003 leaves actions of a few hundredths, as a fresh network's are;
    at 1 tanh saturates on part of the states."""
    P = o.random_params(eo.S, eo.A, np.random.Generator(np.random.PCG64(seed)), stats=True)
    P["actor_output/W"] = (P["actor_output/W"] * gain).astype(np.float32).astype(np.float64)
    return P


@pytest.mark.parametrize("gain", [0.003, 1.0])
def test_oracle_follows_the_real_environment(gain):
    import ga3c_amd  # noqa: F401
    import EnvironmentPend
    P = _actor(5, gain)
    starts = eo.start_states(4321, 3)
    saturated = inside = 0
    for i, start in enumerate(starts):
        env = EnvironmentPend.Environment(i)
        env.game.state = np.array(start, np.float64)
        env.game.elapsed = 0
        env.current_state = np.asarray(env.game._obs(), np.float32).reshape(-1)
        phys, obs, actions, rewards, dones = [], [], [], [], []
        for t in range(200):
            phys.append(np.array(env.game.state, np.float64))
            obs.append(env.current_state.copy())
            action = eo.policy(P, env.current_state)
            reward, done = env.step(action)
            actions.append(action[0])
            rewards.append(float(reward))
            dones.append(bool(done))
        want = eo.rollout(P, start[None, :], 200)
        assert _eq(want["trace_phys"][0], np.array(phys))
        assert _eq(want["trace_obs"][0], np.array(obs, np.float32))
        assert _eq(want["trace_action"][0], np.array(actions, np.float32))
        assert _eq(want["phys"][0], np.array(env.game.state, np.float64))
        assert np.max(np.abs(want["trace_reward"][0] - np.array(rewards))) <= ULP
        assert np.all(want["trace_reward"] <= -1.0) and np.all(want["trace_reward"] >= -1.09)
        assert dones == [False] * 199 + [True] and np.array_equal(want["done"], dones)
        fed = eo.rollout(P, start[None, :], 200, rewards=np.array(rewards)[None, :])
        total = 0.0
        for r in rewards:
            total = total + r
        assert _eq(fed["total"], np.array([total]))
        saturated += int(np.sum(np.abs(want["trace_action"]) > 0.999))
        inside += int(np.sum(np.abs(want["trace_action"]) < 0.9))
    assert inside and (saturated > 0) == (gain == 1.0)


def test_step_many_is_the_actors_oracles_step():
    """The array form against ddpg_actors_oracle.env_step and PendulumEnv.observe, bit for bit: angles on both sides of +-pi and
    several turns out, speeds that the clip cuts, actions within [-1, 1] and beyond (the wrap, which evaluation cannot reach)."""
    rng = np.random.Generator(np.random.PCG64(17))
    n = 4000
    phys = np.stack([rng.uniform(-4 * np.pi, 4 * np.pi, n), rng.uniform(-8.0, 8.0, n)], axis=1)
    phys[:8, 0] = [np.pi, -np.pi, np.nextafter(np.pi, 4), np.nextafter(-np.pi, -4), 0.0, 3 * np.pi, -3 * np.pi, 2 * np.pi]
    action = rng.uniform(-1, 1, n).astype(np.float32)
    action[::7] = rng.uniform(-5, 5, len(action[::7])).astype(np.float32)
    action[:4] = [1.0, -1.0, 0.0, -0.0]
    got_phys, got_reward, got_obs = eo.step_many(phys, action)
    for i in range(n):
        want_phys, want_reward = do.env_step(phys[i], action[i:i + 1])
        assert _eq(got_phys[i], want_phys) and _eq(got_reward[i:i + 1], np.array([want_reward])), i
        assert _eq(got_obs[i], po.PendulumEnv.observe(want_phys)), i
    assert _eq(eo.observe_many(phys), np.array([po.PendulumEnv.observe(p) for p in phys]))


def test_start_states_are_reset_on_the_first_two_draws():
    for seed, n in ((12346, 1), (12346, 64), (-5, 17), (2 ** 40 + 3, 300)):
        got = eo.start_states(seed, n)
        assert got.shape == (n, 2) and got.dtype == np.float64
        for i in (0, n // 2, n - 1):
            rng = po.ResetRNG(seed, i)                      # Pendulum.reset on a fresh stream: draws 0 and 1
            assert _eq(got[i], po.PendulumEnv.reset(rng)) and rng.draws == 2
        assert np.all(np.abs(got[:, 0]) <= np.pi) and np.all(np.abs(got[:, 1]) <= 1.0)
    a, b = eo.start_states(12346, 64), eo.start_states(12346, 300)
    assert _eq(a, b[:64])                                   # an environment's start does not depend on how many there are
    assert not np.array_equal(a, eo.start_states(12345, 64))
    # the training actors of seed s start from draws 2..3 of the same streams: seed + 1 shares nothing with them
    assert not np.array_equal(a[:, 0], -np.pi + 2 * np.pi * ao.uniform(12345, np.arange(64), 2))
    assert eo.gym_return(-1.0 * 200 - 0.005 * 1234.5, 200) == pytest.approx(-1234.5, abs=1e-9)


BASE = dict(GAME='Pendulum-v0', USE_DDPG=True, DEVICE_AGENTS=64, DEVICE_DDPG=True, DEVICE_PENDULUM=False, DEVICE_DDPG_UPDATES=1,
            TRAINING_MIN_BATCH_SIZE=64, REPLAY_BUFFER_SIZE=1000000, PLAY_MODE=False, DYNAMIC_SETTINGS=False,
            DEVICE_AGENT_STEPS=32, DEVICE_DDPG_EVAL_ENVS=16, DEVICE_DDPG_EVAL_EVERY=1000, DEVICE_DDPG_EVAL_TARGET=False)
GATE = [
    (dict(DEVICE_DDPG_EVAL_ENVS=-1), "DEVICE_DDPG_EVAL_ENVS"),
    (dict(DEVICE_DDPG_EVAL_ENVS=4097), "DEVICE_DDPG_EVAL_ENVS"),
    (dict(DEVICE_DDPG_EVAL_ENVS=2.5), "DEVICE_DDPG_EVAL_ENVS"),
    (dict(DEVICE_DDPG_EVAL_ENVS=True), "DEVICE_DDPG_EVAL_ENVS"),
    (dict(DEVICE_DDPG_EVAL_EVERY=0), "DEVICE_DDPG_EVAL_EVERY"),
    (dict(DEVICE_DDPG_EVAL_EVERY=-3), "DEVICE_DDPG_EVAL_EVERY"),
    (dict(DEVICE_DDPG_EVAL_EVERY=1.5), "DEVICE_DDPG_EVAL_EVERY"),
    (dict(DEVICE_DDPG_EVAL_TARGET=1), "DEVICE_DDPG_EVAL_TARGET"),
    (dict(DEVICE_DDPG=False, DEVICE_AGENTS=0), "DEVICE_DDPG_EVAL_ENVS"),       # without DEVICE_DDPG the message names both keys
    (dict(DEVICE_DDPG=False, DEVICE_AGENTS=0), "DEVICE_DDPG "),
    (dict(DEVICE_DDPG=False, USE_DDPG=False, GAME='CartPole-v0', DEVICE_AGENTS=8), "DEVICE_DDPG_EVAL_ENVS"),
    (dict(DEVICE_DDPG=False, USE_DDPG=False, GAME='CartPole-v0', DEVICE_AGENTS=8), "DEVICE_DDPG "),
    (dict(DEVICE_DDPG=False, USE_DDPG=False, DEVICE_PENDULUM=True, DEVICE_AGENTS=8), "DEVICE_DDPG_EVAL_ENVS"),
]


@pytest.mark.parametrize("case", GATE, ids=["%s_%d" % (sorted(c[0].items())[0][0], i) for i, c in enumerate(GATE)])
def test_the_gate(case, monkeypatch):
    import ga3c_amd  # noqa: F401
    import Config as cfg
    settings, message = case
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    assert cfg.Config.DEVICE_DDPG_EVAL_ENVS == 0 and cfg.Config.DEVICE_DDPG_EVAL_EVERY == 1000
    assert cfg.Config.DEVICE_DDPG_EVAL_TARGET is False
    for k, v in BASE.items():
        monkeypatch.setattr(cfg.Config, k, v)
    cfg.resolve_device_agents()                       # the combination passes
    for extra in (dict(DEVICE_DDPG_EVAL_ENVS=1), dict(DEVICE_DDPG_EVAL_ENVS=4096), dict(DEVICE_DDPG_EVAL_EVERY=1),
                  dict(DEVICE_DDPG_EVAL_TARGET=True), dict(DEVICE_DDPG_EVAL_ENVS=4096, DEVICE_AGENTS=1),
                  dict(DEVICE_DDPG_EVAL_ENVS=0, DEVICE_DDPG_EVAL_EVERY=0, DEVICE_DDPG_EVAL_TARGET=None)):   # off: not looked at
        with monkeypatch.context() as mp:
            for k, v in extra.items():
                mp.setattr(cfg.Config, k, v)
            cfg.resolve_device_agents()
    for k, v in settings.items():
        monkeypatch.setattr(cfg.Config, k, v)
    with pytest.raises(ValueError, match=re.escape(message)):
        cfg.resolve_device_agents()


def test_the_defaults_leave_the_resolvers_alone(monkeypatch):
    """With DEVICE_DDPG_EVAL_ENVS = 0 every resolver accepts, refuses and sets what it did: the settings of the existing gates
    pass and fail as before (their own tests say so), nothing in Config moves, and the two other keys are not even read."""
    import ga3c_amd  # noqa: F401
    import Config as cfg
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    before = dict(vars(cfg.Config))
    cfg.resolve_action_space()
    cfg.resolve_ddpg()
    cfg.resolve_device_agents()
    assert dict(vars(cfg.Config)) == before
    for k, v in dict(BASE, DEVICE_DDPG_EVAL_ENVS=0, DEVICE_DDPG_EVAL_EVERY="x", DEVICE_DDPG_EVAL_TARGET="y", CONTINUOUS_INPUT=True,
                     DISCRATE_INPUT=False).items():
        monkeypatch.setattr(cfg.Config, k, v)
    for k in ("USE_REPLAY_MEMORY", "DISCOUNTING"):
        monkeypatch.setattr(cfg.Config, k, getattr(cfg.Config, k))
    cfg.resolve_ddpg()
    held = dict(vars(cfg.Config))
    cfg.resolve_device_agents()
    assert dict(vars(cfg.Config)) == held


def test_abi_entries():
    import ga3c_amd  # noqa: F401
    import _native as nat
    import NetworkDDPG
    text = open(os.path.join(ROOT, "include", "ga3c_abi.h")).read()
    lib = nat.hip_lib()
    for entry in ("create", "destroy", "run", "get", "set"):
        name = "ga3c_ddpg_eval_" + entry
        assert re.search(r"\bint %s\s*\(ga3c_ddpg\* net" % name, text), name
        assert name in nat.HIP_SIGNATURES and hasattr(lib, name), name
    sig = nat.HIP_SIGNATURES
    assert sig["ga3c_ddpg_eval_create"] == (C.c_int, [C.c_void_p, C.c_int32, C.c_int64, C.c_int32])
    assert sig["ga3c_ddpg_eval_run"] == (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, nat.f64p])
    assert sig["ga3c_ddpg_eval_destroy"] == sig["ga3c_ddpg_actors_destroy"]
    for entry in ("get", "set"):
        assert sig["ga3c_ddpg_eval_" + entry] == sig["ga3c_ddpg_actors_" + entry], entry
    assert re.search(r"int ga3c_ddpg_eval_create\(ga3c_ddpg\* net, int32_t n, int64_t seed, int32_t trace\);", text)
    assert re.search(r"int ga3c_ddpg_eval_run\(ga3c_ddpg\* net, int32_t steps, int32_t target, double\* total_reward\);", text)
    assert int(re.search(r"#define GA3C_DDPG_EVAL_MAX_ENVS (\d+)", text).group(1)) == 4096
    assert int(re.search(r"#define GA3C_DDPG_EVAL_MAX_STEPS (\d+)", text).group(1)) == 200 == NetworkDDPG.Network.EVAL_STEPS
    assert C.sizeof(nat.DdpgConfig) == 80             # attached to a live handle, no flag bit: the config did not grow
    assert "GA3C_DDPG_EVAL" not in re.sub(r"GA3C_DDPG_EVAL_MAX_(ENVS|STEPS)", "", text)
    for method in ("eval_create", "eval_run", "eval_get", "eval_set", "eval_destroy", "log_eval"):
        assert callable(getattr(NetworkDDPG.Network, method)), method
    assert set(NetworkDDPG.Network.EVAL_FIELDS) == {"start", "phys", "trace_phys", "trace_obs", "trace_action", "trace_reward"}


class _Model:
    """What ThreadDeviceAgents asks of a model: every actors_run is `calls_per_run` train steps; the loop is told to stop after
    `runs` of them.  The eval_* methods exist only `with_eval`; log_eval is NetworkDDPG.Network's own."""

    def __init__(self, agents, runs, calls_per_run, with_eval):
        self.agents, self.runs, self.calls_per_run = agents, runs, calls_per_run
        self.asked, self.model_name = [], "standin"
        self._log_lock = __import__("threading").Lock()
        if with_eval:
            import NetworkDDPG
            self.eval_create = lambda n, seed: self.asked.append(("eval_create", n, seed))
            self.eval_destroy = lambda: self.asked.append(("eval_destroy",))
            self.eval_run = self._eval_run
            self.log_eval = types.MethodType(NetworkDDPG.Network.log_eval, self)

    def _eval_run(self, steps, target):
        self.asked.append(("eval_run", steps, target, self.agents.server.training_step))
        return np.array([-200.0 - 0.005 * 100.0, -200.0 - 0.005 * 300.0])

    def actors_create(self, n, time_max, discount, seed):
        self.asked.append(("actors_create", n))

    def actors_run(self, steps, train=True):
        self.runs -= 1
        if self.runs == 0:
            self.agents.exit_flag = True
        return 4 * steps, self.calls_per_run, 8 * self.calls_per_run, 0

    def actors_episodes(self):
        return []

    def actors_destroy(self):
        self.asked.append(("actors_destroy",))


def _drive(monkeypatch, runs, calls_per_run, with_eval, **config):
    import ga3c_amd  # noqa: F401
    from Config import Config
    from ThreadDeviceAgents import ThreadDeviceAgents
    for k, v in dict(DEVICE_AGENTS=4, DEVICE_AGENT_STEPS=8, RANDOM_SEED=777, **config).items():
        monkeypatch.setattr(Config, k, v)
    value = lambda: types.SimpleNamespace(value=0)      # noqa: E731
    server = types.SimpleNamespace(training_step=0, frame_counter=0,
                                   stats=types.SimpleNamespace(training_count=value(), replay_memory_size=value()))
    agents = ThreadDeviceAgents(server)
    server.model = _Model(agents, runs, calls_per_run, with_eval)
    agents._run()
    return agents, server.model


def test_evaluations_at_step_zero_and_after_each_multiple(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    # 9 runs of 70 train steps: 0, then after 140 (passed 100), 210 (200), 350 (300), 420 (400), 560 (500), 630 (600)
    agents, model = _drive(monkeypatch, 9, 70, True, DEVICE_DDPG_EVAL_ENVS=2, DEVICE_DDPG_EVAL_EVERY=100,
                           DEVICE_DDPG_EVAL_TARGET=True)
    assert model.asked[:3] == [("actors_create", 4), ("eval_create", 2, 778), ("eval_run", 200, True, 0)]
    assert model.asked[-2:] == [("eval_destroy",), ("actors_destroy",)]
    at = [a[3] for a in model.asked if a[0] == "eval_run"]
    assert at == [0, 140, 210, 350, 420, 560, 630] and agents.evaluations == 7
    assert all(a[1:3] == (200, True) for a in model.asked if a[0] == "eval_run")
    lines = open(str(tmp_path / "logs" / "standin" / "eval.csv")).read().splitlines()
    assert len(lines) == 7
    rows = [ln.split(",") for ln in lines]
    assert [int(r[0]) for r in rows] == at and all(len(r) == 7 and (int(r[1]), int(r[2])) == (2, 200) for r in rows)
    mean, low, high, gym = (float(v) for v in rows[0][3:])
    assert (mean, low, high) == (-201.0, -201.5, -200.5)
    assert gym == (mean + 200) / 0.005 and gym == pytest.approx(-200.0, abs=1e-9)        # the two episodes' gym returns: -100, -300
    # a call that passes two multiples at once evaluates once
    agents, model = _drive(monkeypatch, 2, 250, True, DEVICE_DDPG_EVAL_ENVS=2, DEVICE_DDPG_EVAL_EVERY=100,
                           DEVICE_DDPG_EVAL_TARGET=False)
    assert [a[3] for a in model.asked if a[0] == "eval_run"] == [0, 250, 500]
    assert all(a[2] is False for a in model.asked if a[0] == "eval_run")


def test_no_evaluation_method_is_asked_for_with_the_key_off(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    agents, model = _drive(monkeypatch, 5, 300, False, DEVICE_DDPG_EVAL_ENVS=0, DEVICE_DDPG_EVAL_EVERY=1)
    assert model.asked == [("actors_create", 4), ("actors_destroy",)] and agents.evaluations == 0
    assert not os.path.exists(str(tmp_path / "logs"))
    for method in ("eval_create", "eval_run", "eval_destroy", "log_eval"):
        assert not hasattr(model, method)


def test_a_failed_evaluation_still_destroys_both(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    import ga3c_amd  # noqa: F401
    from Config import Config
    from ThreadDeviceAgents import ThreadDeviceAgents
    for k, v in dict(DEVICE_AGENTS=4, DEVICE_AGENT_STEPS=8, DEVICE_DDPG_EVAL_ENVS=2, DEVICE_DDPG_EVAL_EVERY=10).items():
        monkeypatch.setattr(Config, k, v)
    server = types.SimpleNamespace(training_step=0, frame_counter=0)
    agents = ThreadDeviceAgents(server)
    server.model = model = _Model(agents, 3, 5, True)

    def broken(steps, target):
        raise RuntimeError("no evaluation today")
    model.eval_run = broken
    with pytest.raises(RuntimeError, match="no evaluation today"):
        agents._run()
    assert model.asked[-2:] == [("eval_destroy",), ("actors_destroy",)]


@pytest.mark.timeout(120)
def test_server_run_with_the_key_on(tmp_path, monkeypatch):
    import ga3c_amd  # noqa: F401
    from Config import Config
    import NetworkDDPG
    from test_ddpg_actors_cpu import wide
    from test_device_agents_cpu import _StandInModel

    class StandIn(_StandInModel):
        """... with the oracle's DDPG actors behind actors_run and the oracle's rollout behind eval_run."""
        replay_capacity, model_name = 1000, "standin"
        log_eval = NetworkDDPG.Network.log_eval

        def __init__(self):
            super().__init__()
            self._log_lock = __import__("threading").Lock()
            self.evals, self.eval_destroyed, self.P = [], False, _actor(3, 1.0)

        def actors_create(self, n, time_max, discount, seed):
            self.created = (n, time_max, discount, seed)
            self.actors = do.Actors(n, seed)
            self.ring = do.Ring(self.replay_capacity)

        def replay_size(self):
            return self.ring.size, self.ring.total

        def actors_run(self, steps, train=True):
            self.calls.append((steps, train))
            calls = episodes = 0
            for _ in range(steps):
                rows, eps, _ = self.actors.step(np.array([wide(e.obs) for e in self.actors.env]) if self.actors.started else None)
                self.ring.add(rows)
                if train and self.ring.size > Config.TRAINING_MIN_BATCH_SIZE:
                    calls += 1
                self.pending += eps
                episodes += len(eps)
            return len(self.actors.env) * steps, calls, calls * Config.TRAINING_MIN_BATCH_SIZE, episodes

        def eval_create(self, n, seed):
            self.start = eo.start_states(seed, n)

        def eval_run(self, steps, target):
            self.evals.append((steps, target))
            return eo.rollout(self.P, self.start, steps)["total"]

        def eval_destroy(self):
            self.eval_destroyed = True

    monkeypatch.chdir(tmp_path)
    for k, v in dict(GAME='Pendulum-v0', USE_DDPG=True, DEVICE_AGENTS=6, DEVICE_DDPG=True, DEVICE_DDPG_UPDATES=1, DEVICE_PENDULUM=False,
                     DEVICE_AGENT_STEPS=4, TRAINING_MIN_BATCH_SIZE=8, REPLAY_BUFFER_SIZE=1000, DYNAMIC_SETTINGS=False,
                     SAVE_MODELS=False, PLAY_MODE=False, PRIORITIZED_REPLAY=False, DDPG_CRITIC_LOSS='fork',
                     DEVICE_DDPG_EVAL_ENVS=3, DEVICE_DDPG_EVAL_EVERY=8, DEVICE_DDPG_EVAL_TARGET=False).items():
        monkeypatch.setattr(Config, k, v)
    for k in ("AGENTS", "PREDICTORS", "TRAINERS", "CONTINUOUS_INPUT", "DISCRATE_INPUT", "RANDOM_SEED", "USE_REPLAY_MEMORY",
              "DISCOUNTING"):
        monkeypatch.setattr(Config, k, getattr(Config, k))
    import Server as server_module
    for cls in ("ProcessAgent", "ThreadPredictor", "ThreadTrainer", "ThreadReplay"):
        monkeypatch.setattr(server_module, cls, lambda *a, _c=cls, **k: pytest.fail(_c + " started"))
    model = StandIn()
    srv = server_module.Server(model=model)
    srv.main(max_seconds=3)
    assert srv.failure is None and model.destroyed and model.eval_destroyed
    agents = srv.device_agents
    assert agents.evaluations == len(model.evals) >= 2 and set(model.evals) == {(200, False)}
    rows = np.loadtxt(str(tmp_path / "logs" / "standin" / "eval.csv"), delimiter=",", ndmin=2)
    assert rows.shape == (agents.evaluations, 7) and rows[0, 0] == 0 and np.all(np.diff(rows[:, 0]) > 0)
    assert np.all(np.diff(rows[:, 0] // 8) >= 1)              # each after a multiple of 8 that the one before had not passed
    assert np.all(rows[:, 1] == 3) and np.all(rows[:, 2] == 200)
    want = eo.rollout(model.P, eo.start_states(Config.RANDOM_SEED + 1, 3), 200)["total"]
    assert np.all(rows[:, 3] == want.mean()) and np.all(rows[:, 4] == want.min()) and np.all(rows[:, 5] == want.max())
    assert np.all(rows[:, 6] == (want.mean() + 200) / 0.005) and np.all(rows[:, 6] < 0) and np.all(rows[:, 6] > -18000)
