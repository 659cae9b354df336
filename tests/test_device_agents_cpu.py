"""Device actors (Config.DEVICE_AGENTS) on the CPU: tests/device_agents_oracle.py -- the statement the device
is held to -- against the real ProcessAgent.run_episode over EnvironmentCart.Environment, bit for bit; then the Config
refusals, the header's constant against _native, and a Server run that starts the device-agent thread and nothing else."""
import os
import re

import numpy as np
import pytest

import device_agents_oracle as o

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED, GAMMA = 4242, 0.99


def balance(obs):
    """Stand-in policy of the observation that keeps the pole up: 0.97 on the side it leans to."""
    right = float(obs[2]) + 0.5 * float(obs[3]) + 0.02 * float(obs[0]) + 0.05 * float(obs[1]) > 0
    return np.array([0.03, 0.97] if right else [0.97, 0.03], np.float32)


def topple(obs):
    """... and one that pushes it over, mostly to the right, a little depending on the observation."""
    w = np.float32(0.8) + np.float32(0.1) * np.float32(np.tanh(np.float32(obs[1])))
    return np.array([np.float32(1.0) - w, w], np.float32)


def _host_run(policy, time_max, episodes, env_id=0, short_second_episode=False):
    """The real agent loop: ProcessAgent.run_episode and run()'s accounting over EnvironmentCart.Environment, with the
    oracle's uniforms behind both the action draw and the environment's reset -> (rollouts, episode records, steps)."""
    import ga3c_amd  # noqa: F401
    from Config import Config
    import EnvironmentCart
    import Transport as tp
    from ProcessAgent import ProcessAgent

    saved = {k: getattr(Config, k) for k in ("TIME_MAX", "GAME", "RETURN_MODE", "DISCOUNTING", "USE_INTERMEDIATE_REWARD",
                                             "CONTINUOUS_INPUT", "PLAY_MODE", "STATE_TRANSPORT")}
    Config.TIME_MAX, Config.GAME, Config.RETURN_MODE = time_max, 'CartPole-v0', 'fork'
    Config.DISCOUNTING, Config.USE_INTERMEDIATE_REWARD, Config.CONTINUOUS_INPUT, Config.PLAY_MODE = True, False, False, False
    try:
        agent = ProcessAgent(env_id, "unused", None, config={"DISCOUNT": GAMMA})
        env = EnvironmentCart.Environment(env_id)
        rng = o.CounterRNG(SEED, env_id)
        env.game.rng = rng
        env.reset()                                   # the reset that makes the environment: draws 0..3 (run_episode's: 4..7)
        agent.env, agent.num_actions, agent.actions = env, 2, np.arange(2)
        steps = [0]

        def predict_and_select(state, flags=0):
            p = policy(state)
            steps[0] += 1
            return p, np.float32(0.0), int(tp.select_action_index(p, rng.random()))
        agent.predict_and_select = predict_and_select
        step = env.step

        def counted_step(action):
            if action is None:
                steps[0] += 1
            return step(action)
        env.step = counted_step
        rollouts, records = [], []
        for ep in range(episodes):
            total_reward, total_length = 0, 0
            gen = agent.run_episode()
            if short_second_episode and ep == 1:      # one step before the time limit when the episode begins
                reset = env.reset

                def late_reset():
                    reset()
                    env.game.elapsed = o.TIME_LIMIT - 1
                env.reset = late_reset
            for experiences, reward_sum in gen:
                env.reset = type(env).reset.__get__(env)
                total_reward += reward_sum
                total_length += len(experiences) + 1
                x_, r_, a_, _, _ = agent.convert_data(experiences)
                rollouts.append((x_.astype(np.float32), a_, r_.astype(np.float32)))   # f64 -> f32 as ProcessAgent._ship stores it
            records.append((total_reward, total_length))
        return rollouts, records, steps[0]
    finally:
        for k, v in saved.items():
            setattr(Config, k, v)


def _oracle_run(policy, time_max, steps, env_id=0, short_second_episode=False):
    actor = o.Actor(SEED, env_id, time_max, GAMMA)
    rollouts, records = [], []
    for _ in range(steps):
        r = actor.step(policy(actor.obs))
        if r["cut"] is not None:
            rollouts.append(r["cut"])
        if r["episode"] is not None:
            records.append(r["episode"])
            if short_second_episode and len(records) == 1:
                actor.elapsed = o.TIME_LIMIT - 1
    return rollouts, records


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _same(host, oracle):
    (hr, he), (orr, oe) = host, oracle
    assert len(hr) == len(orr) and len(he) == len(oe)
    for k, (h, w) in enumerate(zip(hr, orr)):
        for name, hh, ww in zip(("states", "actions", "returns"), h, w):
            assert hh.dtype == ww.dtype == np.float32 and hh.shape == ww.shape, (k, name, hh.shape, ww.shape)
            assert np.array_equal(_bits(hh), _bits(ww)), (k, name)
    for (hr_, hl), (or_, ol) in zip(he, oe):
        assert np.float64(hr_).view(np.uint64) == np.float64(or_).view(np.uint64) and int(hl) == int(ol)


@pytest.mark.parametrize("time_max", [1, 2, 5])
@pytest.mark.parametrize("policy", [balance, topple], ids=["time_limit", "falls"])
def test_oracle_is_process_agent_bit_for_bit(policy, time_max):
    rollouts, records, steps = _host_run(policy, time_max, episodes=3)
    want = _oracle_run(policy, time_max, steps)
    _same((rollouts, records), want)
    # the first episode begins with the unpredicted step: 200 steps make elapsed 200 with 199 experiences
    if policy is balance:
        assert steps == 3 * o.TIME_LIMIT, "the balancing policy no longer reaches the 200-step limit"
    else:
        assert steps < 3 * 60, "the toppling policy no longer makes the pole fall"
    assert max(len(r[0]) for r in rollouts) == time_max + 1
    # the stale first observation: the first row of a later episode is the last observation of the one before
    firsts = [r[0][0] for r in rollouts]
    assert any(abs(float(f[2])) > 0.06 or abs(float(f[0])) > 0.06 for f in firsts[1:]), "no episode began on a stale observation"


def test_a_rollout_of_one_row():
    """An episode that ends on its first step: its one rollout has one row, whose return is its own reward."""
    rollouts, records, steps = _host_run(topple, 5, episodes=3, short_second_episode=True)
    want = _oracle_run(topple, 5, steps, short_second_episode=True)
    _same((rollouts, records), want)
    ones = [r for r in rollouts if len(r[0]) == 1]
    assert len(ones) == 1 and ones[0][2][0] == np.float32(1.0 * 0.005 - 1.0)
    assert records[1] == (1.0 * 0.005 - 1.0, 2)


def test_uniforms_are_the_documented_function():
    # splitmix64's finalizer on a known input (the first output of splitmix64 seeded with 0 is mix(0 + G))
    assert int(o.mix64(o.GOLDEN)[0]) == 0xE220A8397B1DCDAF
    u = o.uniform(12345, np.arange(300)[:, None], np.arange(50)[None, :])
    assert u.shape == (300, 50) and u.min() >= 0.0 and u.max() < 1.0 and len(np.unique(u)) == u.size
    assert abs(u.mean() - 0.5) < 0.01
    rng = o.CounterRNG(12345, 7)
    got = [rng.random() for _ in range(3)] + list(rng.uniform(-0.05, 0.05, size=(4,)))
    assert got[:3] == [float(u[7, k]) for k in range(3)]
    assert got[3:] == [-0.05 + (0.05 - -0.05) * float(u[7, k]) for k in range(3, 7)] and rng.draws == 7


def test_select_is_the_host_librarys():
    import ga3c_amd  # noqa: F401
    import Transport as tp
    rng = np.random.Generator(np.random.PCG64(3))
    for _ in range(500):
        p = rng.dirichlet(np.ones(2)).astype(np.float32)
        u = float(rng.random())
        assert o.select(p, u) == tp.select_action_index(p, u)
    p = np.array([0.25, 0.75], np.float32)
    assert o.select(p, 0.25) == 1 and o.select(p, np.nextafter(0.25, 0)) == 0 and o.select(p, 1.0) == 1


REFUSALS = [
    (dict(GAME='Pendulum-v0'), "CartPole-v0 only"),
    (dict(GAME='PongDeterministic-v4'), "CartPole-v0 only"),
    (dict(GAME='Pendulum-v0', USE_DDPG=True), "USE_DDPG"),
    (dict(RETURN_MODE='nstep'), "RETURN_MODE"),
    (dict(PLAY_MODE=True), "PLAY_MODE"),
    (dict(DYNAMIC_SETTINGS=True), "DYNAMIC_SETTINGS"),
    (dict(DEVICE_AGENTS=65536 // 6 + 1), "max_batch"),
    (dict(DEVICE_AGENTS=-1), "DEVICE_AGENTS=-1"),
    (dict(DISCOUNTING=False), "DISCOUNTING"),
    (dict(DEVICE_AGENT_STEPS=65), "DEVICE_AGENT_STEPS"),
]


@pytest.mark.parametrize("case", REFUSALS, ids=[sorted(c[0].items())[0][0] + "_%d" % i for i, c in enumerate(REFUSALS)])
def test_config_refusals(case):
    import ga3c_amd  # noqa: F401
    import Config as cfg
    settings, message = case
    base = dict(GAME='CartPole-v0', DEVICE_AGENTS=64, TIME_MAX=5, RETURN_MODE='fork', PLAY_MODE=False, DYNAMIC_SETTINGS=False,
                USE_DDPG=False, DISCOUNTING=True, USE_INTERMEDIATE_REWARD=False, DEVICE_AGENT_STEPS=32)
    saved = {k: getattr(cfg.Config, k) for k in base}
    try:
        for k, v in base.items():
            setattr(cfg.Config, k, v)
        cfg.resolve_device_agents()                   # the supported combination passes
        for k, v in settings.items():
            setattr(cfg.Config, k, v)
        with pytest.raises(ValueError, match=re.escape(message)):
            cfg.resolve_device_agents()
        cfg.Config.DEVICE_AGENTS = 0                  # off: nothing is checked
        cfg.resolve_device_agents()
    finally:
        for k, v in saved.items():
            setattr(cfg.Config, k, v)


def test_defaults_and_header_constants():
    import ga3c_amd  # noqa: F401
    from Config import Config
    import _native as nat
    assert Config.DEVICE_AGENTS == 0 and Config.DEVICE_AGENT_STEPS == 32
    text = open(os.path.join(ROOT, "include", "ga3c_abi.h")).read()
    assert int(re.search(r"#define GA3C_ACTORS_MAX_STEPS (\d+)", text).group(1)) == nat.ACTORS_MAX_STEPS == 64
    for entry in ("create", "destroy", "run", "episodes", "get", "set"):
        name = "ga3c_dmlp_actors_" + entry
        assert re.search(r"\b%s\s*\(" % name, text) and name in nat.HIP_SIGNATURES, name
    assert hasattr(nat.hip_lib(), "ga3c_dmlp_actors_run")


class _StandInModel:
    """What Server and ThreadDeviceAgents ask of the model, with the oracle's actors behind actors_run."""

    def __init__(self):
        self.learning_rate = self.beta = 0.0
        self.calls, self.rates, self.pending, self.actors, self.destroyed = [], [], [], None, False
        self.finished = []              # every episode, in the order they finished

    def actors_create(self, n, time_max, discount, seed):
        self.created = (n, time_max, discount, seed)
        self.actors = o.Actors(n, seed, time_max, discount)

    def actors_run(self, steps, train=True):
        self.calls.append((steps, train))
        self.rates.append((self.learning_rate, self.beta))
        calls = rows = episodes = 0
        for _ in range(steps):
            p = np.array([topple(e.obs) for e in self.actors.env])
            _, batch, eps = self.actors.step(p)
            if batch is not None:
                calls, rows = calls + 1, rows + len(batch[2])
            self.pending += eps
            self.finished += eps
            episodes += len(eps)
        return len(self.actors.env) * steps, calls, rows, episodes

    def actors_episodes(self):
        out, self.pending = self.pending, []
        return out

    def actors_destroy(self):
        self.destroyed = True

    def save(self, episode):
        pass


@pytest.mark.timeout(120)
def test_server_starts_the_device_agent_thread_and_nothing_else(tmp_path, monkeypatch):
    import ga3c_amd  # noqa: F401
    from Config import Config
    monkeypatch.chdir(tmp_path)
    keys = ("GAME", "DEVICE_AGENTS", "DEVICE_AGENT_STEPS", "TIME_MAX", "DYNAMIC_SETTINGS", "SAVE_MODELS", "AGENTS", "PREDICTORS",
            "TRAINERS", "CONTINUOUS_INPUT", "DISCRATE_INPUT", "RANDOM_SEED", "LEARNING_RATE_START", "LEARNING_RATE_END")
    saved = {k: getattr(Config, k) for k in keys}
    Config.GAME, Config.DEVICE_AGENTS, Config.DEVICE_AGENT_STEPS, Config.TIME_MAX = 'CartPole-v0', 6, 4, 5
    Config.DYNAMIC_SETTINGS, Config.SAVE_MODELS = False, False
    Config.LEARNING_RATE_START = Config.LEARNING_RATE_END = 0.0007
    try:
        import Server as server_module
        started = []
        for cls in ("ProcessAgent", "ThreadPredictor", "ThreadTrainer"):
            monkeypatch.setattr(server_module, cls, lambda *a, _c=cls, **k: started.append(_c))
        model = _StandInModel()
        srv = server_module.Server(model=model)
        srv.main(max_seconds=3)
        assert not started and not srv.agents and not srv.predictors and not srv.trainers
        assert srv.failure is None and not srv.dynamic_adjustment.is_alive() and srv.dynamic_adjustment.ident is None
        assert model.created == (6, 5, Config.DISCOUNT, Config.RANDOM_SEED) and model.destroyed
        assert model.calls and set(model.calls) == {(4, True)}
        assert (0.0007, Config.BETA_START) in [(round(lr, 7), b) for lr, b in model.rates[1:]]     # Server.main's annealing reaches it
        agents = srv.device_agents
        assert agents is not None and not agents.is_alive()
        assert agents.agent_steps == 6 * 4 * len(model.calls) and srv.predictions_served == agents.agent_steps - 6
        assert srv.training_step == srv.stats.training_count.value > 0 and srv.frame_counter > srv.training_step
        lines = open("results.txt").read().strip().splitlines()
        assert lines and all(re.match(r"^\d{4}-\d\d-\d\d \d\d:\d\d:\d\d, -?\d+, \d+$", ln) for ln in lines)
        # what the statistics process wrote before it was stopped is the head of the model's episode list: same episodes, same
        # order ('%d' of the reward and the length, ProcessStats.run)
        assert 0 < len(lines) <= agents.episodes <= len(model.finished)
        wrote = [tuple(int(t) for t in ln.split(", ")[1:]) for ln in lines]
        assert wrote == [(int(r), int(n)) for r, n in model.finished[:len(lines)]]
        assert len(set(wrote)) > 1, "every episode alike: the order is not told apart"
    finally:
        for k, v in saved.items():
            setattr(Config, k, v)
