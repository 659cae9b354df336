"""DDPG device actors (Config.DEVICE_DDPG) on the CPU: tests/ddpg_actors_oracle.py -- the statement the device is
held to -- against the real ProcessAgent.run_episode over EnvironmentPend.Environment under USE_DDPG; the wrap against
EnvironmentPend.check_bounds; the uniform draw; the Config gate; the six new ABI entries; and a Server run that starts the
device-agent thread and nothing else, no replay thread either.

Exact against the agent: states, the unwrapped action vectors, next states, done, physics, the length of every episode record.
Bounded: the reward.  EnvironmentPend squares with `**` (pow), the oracle and the device with a product; a reward lies in
[-1.09, -1], where one ulp is 2^-52: |r_oracle - r_env| <= 2^-52 on every step.  The ring's f32 rewards and the
episode totals follow from the rewards, so they are compared bit for bit with the environment's own rewards fed to the oracle."""
import os
import re

import numpy as np
import pytest

import ddpg_actors_oracle as do
import device_agents_oracle as o
import device_pendulum_oracle as po

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 4242
REWARD_BOUND = 2.0 ** -52


def wide(obs):
    """Stand-in policy of the observation: f32 multiples of 0.25 in [-3.5, 3.5] -- both wrap branches, more than a whole turn
    beyond either end, and exactly +-1."""
    t = np.float32(3.5) * np.float32(np.sin(np.float32(7.0) * np.float32(obs[2]) + np.float32(3.0) * np.float32(obs[1])))
    return np.array([np.round(t * np.float32(4.0)) / np.float32(4.0)], np.float32)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _host_run(policy, time_max, episodes, env_id=0):
    """The real agent loop under USE_DDPG with the oracle's counter uniforms behind the reset -> (rollouts as convert_data
    gives them, index of every episode's first rollout, episode records, per-step log [(physics, reward, done)])."""
    import ga3c_amd  # noqa: F401
    from Config import Config
    import EnvironmentPend
    from ProcessAgent import ProcessAgent

    saved = {k: getattr(Config, k) for k in ("TIME_MAX", "GAME", "RETURN_MODE", "DISCOUNTING", "USE_INTERMEDIATE_REWARD",
                                             "CONTINUOUS_INPUT", "PLAY_MODE", "STATE_TRANSPORT", "REWARD_CLIPPING", "USE_DDPG")}
    Config.TIME_MAX, Config.GAME, Config.RETURN_MODE, Config.USE_DDPG = time_max, 'Pendulum-v0', 'fork', True
    Config.DISCOUNTING, Config.USE_INTERMEDIATE_REWARD, Config.CONTINUOUS_INPUT, Config.PLAY_MODE = False, False, True, False
    try:
        agent = ProcessAgent(env_id, "unused", None, config={"DISCOUNT": 0.99})
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
        rollouts, firsts, records = [], [], []
        for _ in range(episodes):
            firsts.append(len(rollouts))
            total_reward, total_length = 0, 0
            for experiences, reward_sum in agent.run_episode():
                total_reward += reward_sum
                total_length += len(experiences) + 1
                rollouts.append(agent.convert_data(experiences))
            records.append((total_reward, total_length))
        return rollouts, firsts, records, log
    finally:
        for k, v in saved.items():
            setattr(Config, k, v)


def _oracle_run(policy, steps, env_id=0, rewards=None):
    actor = do.Actor(SEED, env_id)
    rows, records, log = [], [], []
    for k in range(steps):
        r = actor.step(None if k == 0 else policy(actor.obs), None if rewards is None else rewards[k])
        log.append((None if r["episode"] is not None else actor.phys.copy(), r["own_reward"], r["done"]))
        if r["row"] is not None:
            rows.append(r["row"])
        if r["episode"] is not None:
            records.append(r["episode"])
    assert actor.rng.draws == 4 + 2 * len(records)
    return rows, records, log


@pytest.mark.parametrize("time_max", [200, 5])
def test_oracle_is_process_agent(time_max):
    rollouts, firsts, records, log = _host_run(wide, time_max, episodes=3)
    steps = len(log)
    assert steps == 3 * po.TIME_LIMIT                 # step(None) and 199 transitions, then 200 and 200
    # the host's transition stream: at TIME_MAX < 200 row 0 of a re-used rollout is the last row of the one before, shipped twice
    host = []
    for k, (x_, r_, a_, x2_, done_) in enumerate(rollouts):
        reused = k not in firsts
        if reused:
            prev = rollouts[k - 1]
            assert all(np.array_equal(_bits(np.asarray(now[0], np.float64)), _bits(np.asarray(before[-1], np.float64)))
                       for now, before in zip((x_, r_, a_, x2_), prev[:4]))
        for t in range(1 if reused else 0, len(x_)):
            host.append((x_[t], a_[t], r_[t], done_[t], x2_[t]))
    if time_max == 200:
        assert len(rollouts) == 3 and firsts == [0, 1, 2]
    else:
        assert max(len(r[0]) for r in rollouts) == time_max + 1 and len(rollouts) > 100
    assert len(host) == steps - 1
    own, own_records, own_log = _oracle_run(wide, steps)
    assert len(own) == len(host) and len(own_records) == len(records) == 3
    actions = np.array([row[1][0] for row in own])
    assert (actions < -1).any() and (actions > 1).any() and (actions == 1).any() and (actions == -1).any()
    assert (actions > 3).any() and (actions < -3).any() and (np.abs(actions) < 1).any()
    for k, (h, w) in enumerate(zip(host, own)):
        for name, hh, ww in (("s", h[0], w[0]), ("a", h[1], w[1]), ("s2", h[4], w[4])):
            hh = np.asarray(hh)
            assert hh.dtype == np.float32 and np.array_equal(_bits(hh), _bits(ww)), (k, name)
        assert bool(h[3]) == bool(w[3]), k
    # the record is the one of an episode shipped as one rollout: at a smaller TIME_MAX the host counts len + 1 per rollout and
    # adds the rollouts' partial sums, which is another number (and another association)
    assert [n for _, n in own_records] == [200, 201, 201]
    if time_max == 200:
        assert [n for _, n in records] == [200, 201, 201]
    worst = 0.0
    for k, ((hp, hr, hd), (wp, wr, wd)) in enumerate(zip(log, own_log)):
        assert hd == wd, k
        if wp is not None:                            # (after a done the oracle holds the next episode's physics already)
            assert np.array_equal(_bits(hp), _bits(wp)), k
        worst = max(worst, abs(hr - wr))
        assert abs(hr - wr) <= REWARD_BOUND, (k, hr, wr)
    print("worst |r_oracle - r_env| = %.3e (bound %.3e)" % (worst, REWARD_BOUND))
    # fed the environment's own rewards, the ring's f32 rewards and the episode totals are the agent's bit for bit
    fed, fed_records, _ = _oracle_run(wide, steps, rewards=[r for _, r, _ in log])
    for k, (h, w) in enumerate(zip(host, fed)):
        assert np.float32(h[2]).view(np.uint32) == np.float32(w[2]).view(np.uint32), k      # _ship: returns[i] = e.reward
    for (hr_, hl), (or_, ol) in zip(records, fed_records):
        if time_max == 200:
            assert np.float64(hr_).view(np.uint64) == np.float64(or_).view(np.uint64) and int(hl) == int(ol)
        else:
            assert abs(hr_ - or_) <= 200 * 2.0 ** -45 and hl > ol       # the same rewards, summed in another order
    # the stale first observation: the first transition of a later episode starts from the last observation of the one before
    for ep in (1, 2):
        first = rollouts[firsts[ep]]
        assert np.array_equal(_bits(np.float32(first[0][0])), _bits(np.float32(rollouts[firsts[ep] - 1][3][-1])))


def test_wrap_is_check_bounds():
    import ga3c_amd  # noqa: F401
    import EnvironmentPend
    one = np.float32(1.0)
    inf = np.float32(np.inf)
    values = [one, -one, np.nextafter(one, inf), np.nextafter(-one, -inf), np.float32(3.0), np.float32(-3.0),
              np.float32(2.999999), np.float32(-2.999999), np.float32(0.0), np.float32(3.5), np.float32(-3.5), np.float32(5.25),
              np.float32(-7.75), np.nextafter(one, np.float32(0)), np.nextafter(-one, np.float32(0))]
    rng = np.random.Generator(np.random.PCG64(11))
    values += list(rng.uniform(-9, 9, 2000).astype(np.float32))
    for a in values:
        want = EnvironmentPend.check_bounds(np.array([a], np.float32), 1.0, -1.0, True)
        got = do.check_bounds(a)
        assert want.dtype == np.float64 and got.dtype == np.float64
        assert np.array_equal(_bits(want), _bits(np.array([got]))), a
        assert -1.0 <= got <= 1.0
        # ... after which the torque clip is an identity
        assert np.array_equal(_bits(np.clip(want * 2.0, -2.0, 2.0)), _bits(want * 2.0))
    assert do.check_bounds(np.float32(3.0)) == -1.0 and do.check_bounds(np.float32(-3.0)) == 1.0
    assert do.check_bounds(one) == 1.0 and do.check_bounds(-one) == -1.0


@pytest.mark.parametrize("size,batch", [(2, 1), (65, 64), (1000, 64), (1048576, 300)])
def test_uniform_draw_is_distinct_and_in_range(size, batch):
    for number in range(20):
        slots = do.uniform_slots(12345, number, size, batch)
        assert slots.dtype == np.int32 and slots.shape == (batch,)
        assert slots.min() >= 0 and slots.max() < size and len(set(slots.tolist())) == batch
        assert np.all(np.diff(slots) > 0)             # one per stratum, in order
    assert not np.array_equal(do.uniform_slots(12345, 0, size, batch), do.uniform_slots(12345, 1, size, batch)) or size == 2


def test_uniform_draw_is_uniform():
    """400 draws of 64 from 3000 slots, counted in 30 groups of 100 slots: 25600 draws, p = 1/30 each; every count within 5
    binomial standard deviations of its mean."""
    draws, batch, size, groups = 400, 64, 3000, 30
    counts = np.zeros(groups, np.int64)
    for number in range(draws):
        counts += np.bincount(do.uniform_slots(777, number, size, batch) // (size // groups), minlength=groups)
    n, p = draws * batch, 1.0 / groups
    sd = np.sqrt(n * p * (1 - p))
    assert counts.sum() == n and np.all(np.abs(counts - n * p) <= 5 * sd), counts


BASE = dict(GAME='Pendulum-v0', USE_DDPG=True, DEVICE_AGENTS=64, DEVICE_DDPG=True, DEVICE_PENDULUM=False, DEVICE_DDPG_UPDATES=1,
            TRAINING_MIN_BATCH_SIZE=64, REPLAY_BUFFER_SIZE=1000000, PLAY_MODE=False, DYNAMIC_SETTINGS=False,
            DEVICE_AGENT_STEPS=32, DISCOUNTING=False, RETURN_MODE='fork', USE_INTERMEDIATE_REWARD=False, TIME_MAX=5)
GATE = [
    (dict(USE_DDPG=False), "DEVICE_DDPG needs USE_DDPG"),
    (dict(DEVICE_AGENTS=0), "DEVICE_DDPG needs DEVICE_AGENTS"),
    (dict(GAME='CartPole-v0'), "Pendulum-v0"),
    (dict(GAME='PongDeterministic-v4'), "Pendulum-v0"),
    (dict(DEVICE_PENDULUM=True), "DEVICE_PENDULUM"),
    (dict(DEVICE_AGENTS=4097), "4096"),
    (dict(DEVICE_AGENTS=-1), "DEVICE_AGENTS=-1"),
    (dict(DEVICE_AGENTS=200, REPLAY_BUFFER_SIZE=199), "REPLAY_BUFFER_SIZE"),
    (dict(DEVICE_DDPG_UPDATES=0), "DEVICE_DDPG_UPDATES"),
    (dict(DEVICE_DDPG_UPDATES=17), "DEVICE_DDPG_UPDATES"),
    (dict(PLAY_MODE=True), "PLAY_MODE"),
    (dict(DYNAMIC_SETTINGS=True), "DYNAMIC_SETTINGS"),
    (dict(DEVICE_AGENT_STEPS=0), "DEVICE_AGENT_STEPS"),
    (dict(DEVICE_AGENT_STEPS=65), "DEVICE_AGENT_STEPS"),
    (dict(DEVICE_DDPG=False), "USE_DDPG"),            # without the key the refusal of today stands ...
    (dict(DEVICE_DDPG=False), "DEVICE_DDPG"),         # ... and names the key that lifts it
]


@pytest.mark.parametrize("case", GATE, ids=["%s_%d" % (sorted(c[0].items())[0][0], i) for i, c in enumerate(GATE)])
def test_the_gate(case, monkeypatch):
    import ga3c_amd  # noqa: F401
    import Config as cfg
    settings, message = case
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    assert cfg.Config.DEVICE_DDPG is False and cfg.Config.DEVICE_DDPG_UPDATES == 1
    for k, v in BASE.items():
        monkeypatch.setattr(cfg.Config, k, v)
    cfg.resolve_device_agents()                       # the combination passes with the key
    for extra in (dict(DEVICE_AGENTS=4096), dict(DEVICE_AGENTS=1), dict(DEVICE_DDPG_UPDATES=16), dict(TIME_MAX=0),
                  dict(RETURN_MODE='nstep'), dict(USE_INTERMEDIATE_REWARD=True), dict(DEVICE_AGENTS=4096, TIME_MAX=200),
                  dict(DEVICE_AGENTS=200, REPLAY_BUFFER_SIZE=200)):
        with monkeypatch.context() as mp:             # ... whatever the keys of the actor-critic regimes say
            for k, v in extra.items():
                mp.setattr(cfg.Config, k, v)
            cfg.resolve_device_agents()
    for k, v in settings.items():
        monkeypatch.setattr(cfg.Config, k, v)
    with pytest.raises(ValueError, match=re.escape(message)):
        cfg.resolve_device_agents()


def test_world_size_is_refused(monkeypatch):
    import ga3c_amd  # noqa: F401
    import Config as cfg
    for k, v in BASE.items():
        monkeypatch.setattr(cfg.Config, k, v)
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(ValueError, match="WORLD_SIZE"):
        cfg.resolve_device_agents()


def test_abi_entries():
    import ctypes as C
    import ga3c_amd  # noqa: F401
    import _native as nat
    import NetworkDDPG
    text = open(os.path.join(ROOT, "include", "ga3c_abi.h")).read()
    lib = nat.hip_lib()
    for entry in ("create", "destroy", "run", "episodes", "get", "set"):
        name = "ga3c_ddpg_actors_" + entry
        assert re.search(r"\bint %s\s*\(ga3c_ddpg\* net" % name, text), name
        assert name in nat.HIP_SIGNATURES and hasattr(lib, name), name
    sig = nat.HIP_SIGNATURES
    assert sig["ga3c_ddpg_actors_create"] == (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int64])
    assert sig["ga3c_ddpg_actors_run"] == (C.c_int, [C.c_void_p, C.c_int32, C.c_float, C.c_float, C.c_int32, C.c_int32, nat.f32p,
                                                     nat.i64p, nat.f32p])
    for entry in ("destroy", "episodes", "get", "set"):
        assert sig["ga3c_ddpg_actors_" + entry] == sig["ga3c_mlp_actors_" + entry], entry
    assert re.search(r"int ga3c_ddpg_actors_create\(ga3c_ddpg\* net, int32_t n, int32_t updates, int64_t seed\);", text)
    assert re.search(r"int ga3c_ddpg_actors_run\(ga3c_ddpg\* net, int32_t steps, float learning_rate, float beta_is, int32_t train, "
                     r"int32_t noise_mode,\s+const float\* noise, int64_t\* out_stats, float\* q_stats\);", text)
    assert C.sizeof(nat.DdpgConfig) == 80             # the actors are attached to a live handle: the config did not grow
    for method in ("actors_create", "actors_run", "actors_episodes", "actors_get", "actors_set", "actors_destroy"):
        assert callable(getattr(NetworkDDPG.Network, method)), method
    assert set(NetworkDDPG.Network.ACTOR_FIELDS) == {"phys", "elapsed", "draws", "obs", "action", "reward", "done", "slots"}


@pytest.mark.timeout(120)
def test_server_starts_the_device_agent_thread_and_nothing_else(tmp_path, monkeypatch):
    import ga3c_amd  # noqa: F401
    from Config import Config
    from test_device_agents_cpu import _StandInModel

    class StandIn(_StandInModel):
        """... with the oracle's DDPG actors and ring behind actors_run."""
        replay_capacity = 1000

        def actors_create(self, n, time_max, discount, seed):
            self.created = (n, time_max, discount, seed)
            self.actors = do.Actors(n, seed)
            self.ring = do.Ring(self.replay_capacity)

        def replay_size(self):
            return self.ring.size, self.ring.total

        def actors_run(self, steps, train=True):
            self.calls.append((steps, train))
            self.rates.append((self.learning_rate, self.beta))
            calls = episodes = 0
            for _ in range(steps):
                rows, eps, _ = self.actors.step(np.array([wide(e.obs) for e in self.actors.env]) if self.actors.started else None)
                self.ring.add(rows)
                if train and self.ring.size > Config.TRAINING_MIN_BATCH_SIZE:
                    calls += Config.DEVICE_DDPG_UPDATES
                self.pending += eps
                self.finished += eps
                episodes += len(eps)
            return len(self.actors.env) * steps, calls, calls * Config.TRAINING_MIN_BATCH_SIZE, episodes

    monkeypatch.chdir(tmp_path)
    for k, v in dict(GAME='Pendulum-v0', USE_DDPG=True, DEVICE_AGENTS=6, DEVICE_DDPG=True, DEVICE_DDPG_UPDATES=2, DEVICE_PENDULUM=False,
                     DEVICE_AGENT_STEPS=4, TRAINING_MIN_BATCH_SIZE=8, REPLAY_BUFFER_SIZE=1000, DYNAMIC_SETTINGS=False,
                     SAVE_MODELS=False, PLAY_MODE=False, PRIORITIZED_REPLAY=False, DDPG_CRITIC_LOSS='fork').items():
        monkeypatch.setattr(Config, k, v)
    for k in ("AGENTS", "PREDICTORS", "TRAINERS", "CONTINUOUS_INPUT", "DISCRATE_INPUT", "RANDOM_SEED", "USE_REPLAY_MEMORY",
              "DISCOUNTING"):
        monkeypatch.setattr(Config, k, getattr(Config, k))      # (Server resolves some of them: put back afterwards)
    import Server as server_module
    started = []
    for cls in ("ProcessAgent", "ThreadPredictor", "ThreadTrainer", "ThreadReplay"):
        monkeypatch.setattr(server_module, cls, lambda *a, _c=cls, **k: started.append(_c))
    model = StandIn()
    srv = server_module.Server(model=model)
    srv.main(max_seconds=3)
    assert Config.CONTINUOUS_INPUT is True and Config.DISCOUNTING is False
    assert not started and not srv.agents and not srv.predictors and not srv.trainers and srv.replay is None
    assert srv.failure is None and not srv.dynamic_adjustment.is_alive() and srv.dynamic_adjustment.ident is None
    assert model.created[0] == 6 and model.created[3] == Config.RANDOM_SEED and model.destroyed
    assert model.calls and set(model.calls) == {(4, True)}
    agents = srv.device_agents
    assert agents is not None and not agents.is_alive()
    assert agents.agent_steps == 6 * 4 * len(model.calls) and srv.predictions_served == agents.agent_steps - 6
    # 6 transitions per actor step from the second on; two train steps per actor step once the ring holds more than 8 rows
    assert model.ring.total == agents.agent_steps - 6
    actor_steps = 4 * len(model.calls)
    assert srv.training_step == srv.stats.training_count.value == 2 * (actor_steps - 2)
    assert srv.frame_counter == 8 * srv.training_step
    assert srv.stats.replay_memory_size.value == model.ring.size == min(1000, model.ring.total)
    assert len(model.finished) % 6 == 0
