"""GAME = 'CartPole-v0' without a GPU: the f64 statement of the discrete-action vector-state network
(tests/dmlp_oracle.py) against torch autograd and central differences in both wirings and both softmax branches, its
parameter table and initialisation, the restated CartPole-v0 and the reference's wrapper around it, the GAME / DENSE_LAYERS /
DENSE_STACK resolution, and a Server run with a stand-in model."""
import os

import numpy as np
import pytest

import ga3c_oracle as o
import dmlp_oracle as m

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (S, A, layers, wiring)
SHAPES = [(4, 2, (10, 10, 10, 10), "fork"), (4, 2, (10, 10, 10, 10), "chained"), (7, 5, (32, 16), "chained"),
          (3, 1, (10,), "fork")]
HEADS = [dict(use_log_softmax=False, min_policy=0.0), dict(use_log_softmax=True, min_policy=0.0),
         dict(use_log_softmax=False, min_policy=0.01)]


def _case(state_dim, num_actions, layers, stack, bsz, seed):
    params = m.init_params(state_dim, num_actions, layers, stack, seed=seed)
    rng = np.random.default_rng(seed)
    params["logits_p/w"] = params["logits_p/w"] * 4.0           # a policy that is not nearly uniform
    x = rng.uniform(-2, 2, size=(bsz, state_dim))
    y = rng.normal(size=bsz)
    a = np.eye(num_actions)[rng.integers(0, num_actions, bsz)]
    return params, x, y, a


def _max_rel(got, want):
    got, want = np.asarray(got).reshape(-1), np.asarray(want).reshape(-1)
    return np.max(np.abs(got - want)) / max(1.0, np.max(np.abs(want)))


def _torch_grads(params, x, y_r, a, beta, stack, use_log_softmax, min_policy, log_eps=1e-6):
    torch = pytest.importorskip("torch")
    t = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in params.items()}
    xt = torch.tensor(x, dtype=torch.float64)
    nl = (len(params) - 4) // 2
    h = xt
    for i in range(nl):                 # the reference's loop (:52-56): every layer is built, `h` is overwritten each time
        src = h if (stack == "chained" and i > 0) else xt
        h = torch.sigmoid(src @ t["dense1_%d_p/w" % (i + 1)] + t["dense1_%d_p/b" % (i + 1)])
    v = (h @ t["logits_v/w"] + t["logits_v/b"])[:, 0]
    z = h @ t["logits_p/w"] + t["logits_p/b"]
    yt, at = torch.tensor(y_r, dtype=torch.float64), torch.tensor(a, dtype=torch.float64)
    adv = yt - v.detach()
    if use_log_softmax:
        sp, ls = torch.softmax(z, 1), torch.log_softmax(z, 1)
        c1 = ((ls * at).sum(1) * adv).sum()
        c2 = (-beta * (ls * sp).sum(1)).sum()
    else:
        sp = (torch.softmax(z, 1) + min_policy) / (1.0 + min_policy * z.shape[1])
        eps = torch.tensor(log_eps, dtype=torch.float64)
        c1 = (torch.log(torch.maximum((sp * at).sum(1), eps)) * adv).sum()
        c2 = (-beta * (torch.log(torch.maximum(sp, eps)) * sp).sum(1)).sum()
    cv = 0.5 * ((yt - v) ** 2).sum()
    (-(c1 + c2) + cv).backward()
    return sp.detach().numpy(), (c1.item(), c2.item(), cv.item()), {k: (None if t[k].grad is None else t[k].grad.numpy())
                                                                    for k in t}


@pytest.mark.parametrize("head", HEADS, ids=["plain", "log_softmax", "min_policy"])
@pytest.mark.parametrize("state_dim,num_actions,layers,stack", SHAPES)
def test_oracle_matches_torch_autograd(state_dim, num_actions, layers, stack, head):
    params, x, y, a = _case(state_dim, num_actions, layers, stack, 9, 11 + state_dim + num_actions)
    sp, costs, tg = _torch_grads(params, x, y, a, 0.01, stack, **head)
    losses, g = m.loss_and_grads(params, x, y, a, 0.01, stack=stack, **head)
    assert np.max(np.abs(m.forward(params, x, stack, **head)["p"] - sp)) < 1e-12
    for got, want in zip((losses["cost_p_1_agg"], losses["cost_p_2_agg"], losses["cost_v"]), costs):
        assert abs(got - want) < 1e-10
    dead = m.dead_params(layers, stack)
    assert len(dead) == (2 * (len(layers) - 1) if stack == "fork" else 0)
    for k in m.param_order(layers):
        if k in dead:
            assert tg[k] is None and not np.any(g[k]) and g[k].shape == params[k].shape, k
        elif num_actions == 1 and k.startswith("logits_p/"):
            assert not np.any(g[k]), k               # the softmax over one action is 1 and has no gradient
            assert np.max(np.abs(tg[k])) < 1e-12
        else:
            assert _max_rel(g[k], tg[k]) < 1e-10, k


@pytest.mark.parametrize("head", HEADS, ids=["plain", "log_softmax", "min_policy"])
@pytest.mark.parametrize("state_dim,num_actions,layers,stack", SHAPES)
def test_oracle_matches_central_differences(state_dim, num_actions, layers, stack, head):
    params, x, y, a = _case(state_dim, num_actions, layers, stack, 5, 3 + state_dim)
    beta = 0.05
    adv = y - m.forward(params, x, stack)["v"]
    _, g = m.loss_and_grads(params, x, y, a, beta, stack=stack, **head)
    rng = np.random.default_rng(0)
    eps = 1e-6
    for k in m.param_order(layers):
        for idx in [tuple(rng.integers(0, s) for s in params[k].shape) for _ in range(3)]:
            save = params[k][idx]
            vals = []
            for d in (eps, -eps):
                params[k][idx] = save + d
                losses, _ = m.loss_and_grads(params, x, y, a, beta, stack=stack, adv_const=adv, **head)
                vals.append(losses["cost_all"])
            params[k][idx] = save
            fd = (vals[0] - vals[1]) / (2 * eps)
            assert abs(fd - g[k][idx]) < 1e-6 * max(1.0, abs(fd)), (k, idx, fd, g[k][idx])
            if k in m.dead_params(layers, stack):
                assert fd == 0.0 and g[k][idx] == 0.0


def test_float32_inputs_stay_float32():
    """The relative comparator measures e32 with this oracle run in float32: nothing in it may widen to float64."""
    for s, a_n, layers, stack in SHAPES:
        params, x, y, a = _case(s, a_n, layers, stack, 6, 2)
        p32 = {k: v.astype(np.float32) for k, v in params.items()}
        for head in HEADS:
            f = m.forward(p32, x.astype(np.float32), stack, **head)
            losses, g = m.loss_and_grads(p32, x.astype(np.float32), y.astype(np.float32), a.astype(np.float32), 0.01, stack=stack,
                                         **head)
            for k, val in list(f.items()) + list(g.items()) + list(losses.items()):
                assert np.asarray(val).dtype == np.float32, (k, np.asarray(val).dtype)


@pytest.mark.parametrize("stack", ["fork", "chained"])
@pytest.mark.parametrize("clip,momentum", [(None, 0.0), (40.0, 0.0), (None, 0.9), (0.05, 0.5)])
def test_one_rmsprop_step_matches_torch(clip, momentum, stack):
    """One TF-1 RMSProp step on the oracle's gradient (with clip_by_average_norm / momentum) against the same arithmetic on
    torch autograd's gradient; the dead variables and their slots keep their bits."""
    layers = (10, 10, 10, 10)
    params, x, y, a = _case(4, 2, layers, stack, 8, 5)
    _, _, tg = _torch_grads(params, x, y, a, 0.01, stack, False, 0.0)
    p1 = {k: v.copy() for k, v in params.items()}
    rng = np.random.default_rng(1)
    ms0 = {k: rng.uniform(0.5, 1.5, v.shape) for k, v in params.items()}
    mom0 = {k: rng.uniform(-0.1, 0.1, v.shape) for k, v in params.items()}
    ms1, mom1 = {k: v.copy() for k, v in ms0.items()}, {k: v.copy() for k, v in mom0.items()}
    m.train_step(p1, ms1, mom1, x, y, a, 1e-3, 0.01, stack=stack, momentum=momentum, clip=clip)
    dead = m.dead_params(layers, stack)
    assert (len(dead) == 6) == (stack == "fork")
    for k in m.param_order(layers):
        if k in dead:
            assert np.array_equal(p1[k], params[k]) and np.array_equal(ms1[k], ms0[k]) and np.array_equal(mom1[k], mom0[k]), k
            continue
        gt = tg[k] if clip is None else o.clip_by_average_norm(tg[k], clip)
        ms = 0.99 * ms0[k] + 0.01 * gt * gt
        step = 1e-3 * gt / np.sqrt(ms + 0.1)
        if momentum:
            step = momentum * mom0[k] + step
            assert np.max(np.abs(mom1[k] - step)) < 1e-12
        else:
            assert np.array_equal(mom1[k], mom0[k])
        assert np.max(np.abs(p1[k] - (params[k] - step))) < 1e-12, k
        assert np.max(np.abs(ms1[k] - ms)) < 1e-12


def test_parameter_table_order_and_init(monkeypatch):
    import ga3c_amd  # noqa: F401
    from Config import Config
    import NetworkVP_discrate as nd
    assert Config.DENSE_LAYERS == (10, 10, 10, 10) and Config.DENSE_STACK == 'fork'
    assert nd.param_order() == m.param_order() == (
        "dense1_1_p/w", "dense1_1_p/b", "dense1_2_p/w", "dense1_2_p/b", "dense1_3_p/w", "dense1_3_p/b", "dense1_4_p/w",
        "dense1_4_p/b", "logits_v/w", "logits_v/b", "logits_p/w", "logits_p/b")
    for num_actions in (1, 2, 5):
        shapes = nd.param_shapes(4, num_actions)
        assert all(shapes["dense1_%d_p/w" % i] == (4, 10) for i in range(1, 5))
        assert shapes["logits_v/w"] == (10, 1) and shapes["logits_p/w"] == (10, num_actions)
        assert sum(int(np.prod(v)) for v in shapes.values()) == 4 * 50 + 11 + 11 * num_actions
    assert nd.dead_params() == m.dead_params() == tuple("dense1_%d_p/%s" % (i, wb) for i in (1, 2, 3) for wb in ("w", "b"))
    for s, a, layers, stack in SHAPES:
        assert nd.param_order(layers) == m.param_order(layers)
        shapes = nd.param_shapes(s, a, layers, stack)
        assert shapes == m.param_shapes(s, a, layers, stack)
        assert nd.dead_params(layers, stack) == m.dead_params(layers, stack)
        theta = nd.initial_arena(s, a, 12345, layers, stack)
        assert theta.dtype == np.float32 and theta.size == m.param_count(s, a, layers, stack)
        assert np.array_equal(theta, m.flat(m.init_params(s, a, layers, stack, 12345)).astype(np.float32))
        assert np.array_equal(theta, nd.initial_arena(s, a, 12345, layers, stack))
        assert np.min(theta) >= np.float32(-0.3) and np.max(theta) <= np.float32(0.3)      # U[-0.3, 0.3), rounded to float32
        if theta.size > 200:
            assert np.min(theta) < -0.28 and np.max(theta) > 0.28
    assert nd.param_shapes(7, 5, (32, 16), "chained")["dense1_2_p/w"] == (32, 16)
    assert nd.param_shapes(7, 5, (32, 16), "fork")["dense1_2_p/w"] == (7, 16)
    for bad in ((), (10,) * 9, (0,), (257,)):
        with pytest.raises(ValueError):
            nd.param_order(bad)
    with pytest.raises(ValueError):
        nd.param_shapes(4, 2, (10,), "other")


# ---- CartPole-v0 and the reference's wrapper
def _restated_step(state, action):
    """An independent restatement of the issue's equations (names and grouping of its own)."""
    x, xd, th, thd = state
    f = 10.0 if action == 1 else -10.0
    temp = (f + 0.05 * thd * thd * np.sin(th)) / 1.1
    thacc = (9.8 * np.sin(th) - np.cos(th) * temp) / (0.5 * (4.0 / 3.0 - 0.1 * np.cos(th) ** 2 / 1.1))
    xacc = temp - 0.05 * thacc * np.cos(th) / 1.1
    nx, nxd, nth, nthd = x + 0.02 * xd, xd + 0.02 * xacc, th + 0.02 * thd, thd + 0.02 * thacc
    done = abs(nx) > 2.4 or abs(nth) > 12 * np.pi / 180
    return np.array([nx, nxd, nth, nthd]), done


def _cart_env(monkeypatch, seed=7):
    import ga3c_amd  # noqa: F401
    from Config import Config
    import EnvironmentCart as ec
    monkeypatch.setattr(Config, "RANDOM_SEED", seed)
    return ec, ec.Environment(0)


def _run(ec, policy, start=(0.0, 0.0, 0.0, 0.0)):
    game = ec.CartPole(np.random.default_rng(0))
    game.reset()
    game.state = np.array(start, dtype=np.float64)
    ref = np.array(start, dtype=np.float64)
    states = []
    for k in range(1000):
        obs, r, done = game.step(policy(k, game.state))
        ref, ref_done = _restated_step(ref, policy(k, ref))
        assert np.max(np.abs(obs - ref)) < 1e-12 and r == 1.0
        states.append(obs)
        if done:
            assert ref_done or k + 1 == 200
            return k + 1, np.array(states)
    raise AssertionError("never done")


def test_cartpole_step_values_and_step_counts(monkeypatch):
    ec, _ = _cart_env(monkeypatch)
    game = ec.CartPole(np.random.default_rng(0))
    game.state, game.elapsed = np.zeros(4), 0
    obs, r, done = game.step(1)
    assert np.allclose(obs, [0.0, 0.1951219512195122, 0.0, -0.2926829268292683], rtol=0, atol=1e-15) and r == 1.0 and not done
    n1, s1 = _run(ec, lambda k, s: 1)
    n0, s0 = _run(ec, lambda k, s: 0)
    assert n1 == 9 and n0 == 9
    assert np.array_equal(s0, -s1)                         # exact mirror symmetry: every component negated
    nalt, _ = _run(ec, lambda k, s: k % 2)
    assert nalt == 33
    with pytest.raises(ValueError):
        game.step(2)


def test_cartpole_random_policy_episode_lengths(monkeypatch):
    ec, _ = _cart_env(monkeypatch)
    rng = np.random.default_rng(5)
    game = ec.CartPole(np.random.default_rng(6))
    lengths = []
    for _ in range(2000):
        game.reset()
        n = 0
        done = False
        while not done:
            _, _, done = game.step(int(rng.integers(0, 2)))
            n += 1
        lengths.append(n)
    assert 20.0 < np.mean(lengths) < 24.0 and min(lengths) >= 7 and max(lengths) < 200      # the issue: mean 22, min 8, max 122


def test_cartpole_reset_range_and_time_limit(monkeypatch):
    ec, env = _cart_env(monkeypatch, seed=3)
    rng = np.random.Generator(np.random.PCG64(3))
    assert np.array_equal(env.game.state, rng.uniform(low=-0.05, high=0.05, size=(4,)))     # PCG64(seed + agent id)
    assert ec.Environment(1).game.state.tolist() != ec.Environment(0).game.state.tolist()
    for seed in range(20):
        game = ec.CartPole(np.random.Generator(np.random.PCG64(100 + seed)))
        obs = game.reset()
        assert obs.shape == (4,) and np.all(np.abs(obs) <= 0.05)
        ref = obs.copy()
        for k in range(1, 201):
            action = 1 if obs[2] + obs[3] > 0 else 0             # a policy that balances: `done` at 200 is the limit speaking
            ref, fell = _restated_step(ref, action)
            assert not fell
            obs, _, done = game.step(action)
            assert done == (k == 200), (seed, k)
        game.reset()
        assert game.elapsed == 0
    assert env.get_num_actions() == 2 and env.get_state_dim() == (4,) and env.vector_state and not env.on_device


def test_wrapper_first_step_stale_state_and_reward(monkeypatch):
    ec, env = _cart_env(monkeypatch)
    assert env.current_state is None and env.current_u8 is None
    start = env.game.state.copy()
    r, done = env.step(None)                                 # the agent's very first step: action 0
    want, _ = _restated_step(start, 0)
    assert np.array_equal(env.current_state, want.astype(np.float32)) and env.current_state.dtype == np.float32
    assert abs(r - (-0.995)) < 1e-15 and not done
    r, _ = env.step(1)
    assert abs(r - (0.005 * 1.0 - 1.0)) < 1e-15 and env.previous_state is not None
    last = env.current_state.copy()
    env.reset()
    # reset() keeps current_state: the next episode's first action is predicted from the last episode's last observation
    assert np.array_equal(env.current_state, last) and env.game.elapsed == 0


def test_agent_episode_starts_with_action_zero_and_a_stale_state(monkeypatch):
    """ProcessAgent.run_episode on the CartPole wrapper: the first episode begins with step(None); every later episode's
    first prediction is asked for the previous episode's last observation; actions are ints."""
    import ga3c_amd  # noqa: F401
    from Config import Config
    from ProcessAgent import ProcessAgent
    ec, env = _cart_env(monkeypatch)
    for k, v in (("CONTINUOUS_INPUT", False), ("DISCRATE_INPUT", True), ("TIME_MAX", 1000), ("PLAY_MODE", False)):
        monkeypatch.setattr(Config, k, v)
    asked = []

    class _T:
        def round_trip(self, agent, state, flags, timeout_ms, u, submit=True):
            asked.append(np.frombuffer(state.tobytes(), np.float32).copy())
            return 0, np.array([0.25, 0.75], np.float32), 0.0, len(asked) % 2

    ag = ProcessAgent.__new__(ProcessAgent)
    ag.transport, ag.id, ag.env, ag.requests = _T(), 0, env, 0
    ag.names_states, ag.discount_factor, ag.time_count = False, 0.99, 0
    ag.num_actions, ag.actions = 2, np.arange(2)
    steps = []
    orig = env.step
    monkeypatch.setattr(env, "step", lambda a: (steps.append(a), orig(a))[1])
    (rows, _), = list(ag.run_episode())
    assert steps[0] is None and all(type(s) is int and s in (0, 1) for s in steps[1:])
    assert len(rows) == len(steps) - 1 and rows[-1].done
    assert all(r.reward <= 0 for r in rows)
    x_, r_, a_, _, _ = ag.convert_data(rows)
    assert x_.shape == (len(rows), 4) and x_.dtype == np.float32
    assert a_.shape == (len(rows), 2) and a_.dtype == np.float32 and np.array_equal(a_.sum(1), np.ones(len(rows)))
    last = env.current_state.copy()
    asked.clear()
    list(ag.run_episode())
    assert np.array_equal(asked[0], last)                    # the stale first observation


# ---- configuration
_KEYS = ("CONTINUOUS_INPUT", "DISCRATE_INPUT", "GAME", "USE_DDPG", "USE_REPLAY_MEMORY", "DISCOUNTING", "DUAL_RMSPROP",
         "DENSE_STACK", "DENSE_LAYERS", "TRAINING_MIN_BATCH_SIZE", "AGENTS")


def _keep(monkeypatch):
    import ga3c_amd  # noqa: F401
    from Config import Config
    for k in _KEYS:
        monkeypatch.setattr(Config, k, getattr(Config, k))
    return Config


def test_game_sets_the_discrete_head_and_refuses_contradictions(monkeypatch):
    Config = _keep(monkeypatch)
    import Config as config_module
    import GA3C
    assert "CartPole-v0" in config_module.VECTOR_GAMES
    assert config_module.VECTOR_GAME_CONTINUOUS == {"Pendulum-v0": True, "CartPole-v0": False}
    Config.CONTINUOUS_INPUT, Config.DISCRATE_INPUT = True, False        # whatever was there before
    GA3C.apply_argv(["GAME=CartPole-v0"])
    assert config_module.vector_game() and config_module.discrete_vector_game()
    assert Config.DISCRATE_INPUT and not Config.CONTINUOUS_INPUT
    GA3C.apply_argv(["GAME=CartPole-v0", "CONTINUOUS_INPUT="])
    GA3C.apply_argv(["GAME=CartPole-v0", "DISCRATE_INPUT=True"])
    assert Config.DISCRATE_INPUT and not Config.CONTINUOUS_INPUT
    with pytest.raises(ValueError):
        GA3C.apply_argv(["GAME=CartPole-v0", "CONTINUOUS_INPUT=True"])
    Config.CONTINUOUS_INPUT = False
    with pytest.raises(ValueError):
        GA3C.apply_argv(["GAME=CartPole-v0", "DISCRATE_INPUT="])
    Config.DISCRATE_INPUT = True
    with pytest.raises(ValueError):
        GA3C.apply_argv(["GAME=CartPole-v0", "USE_DDPG=True", "TRAINING_MIN_BATCH_SIZE=64"])
    Config.USE_DDPG = False
    with pytest.raises(ValueError):
        GA3C.apply_argv(["GAME=CartPole-v0", "DUAL_RMSPROP=True"])
    Config.DUAL_RMSPROP = False
    with pytest.raises(ValueError):
        GA3C.apply_argv(["GAME=CartPole-v0", "DENSE_STACK=other"])
    GA3C.apply_argv(["GAME=CartPole-v0", "DENSE_STACK=chained", "DENSE_LAYERS=64,64"])
    assert Config.DENSE_STACK == "chained" and Config.DENSE_LAYERS == (64, 64)
    GA3C.apply_argv(["DENSE_LAYERS=7"])
    assert Config.DENSE_LAYERS == (7,)
    # every other key coerces as before; Pendulum's resolution is unchanged
    GA3C.apply_argv(["GAME=Pendulum-v0", "AGENTS=7"])
    assert Config.AGENTS == 7 and Config.CONTINUOUS_INPUT and not Config.DISCRATE_INPUT
    assert config_module.vector_game() and not config_module.discrete_vector_game()
    with pytest.raises(ValueError):
        GA3C.apply_argv(["GAME=Pendulum-v0", "CONTINUOUS_INPUT="])
    GA3C.apply_argv(["GAME=PongDeterministic-v4", "CONTINUOUS_INPUT="])
    assert Config.DISCRATE_INPUT and not Config.CONTINUOUS_INPUT and not config_module.vector_game()


class _CartStandIn:
    """A deterministic policy of the state that puts all its mass on one action, so a trainer can check that each row's
    one-hot action is what the agent was answered for exactly that state."""
    def __init__(self):
        self.learning_rate = self.beta = 0.0
        self.batches, self.mismatch, self.preds, self.bad_shape, self.seen = [], 0, 0, 0, set()

    @staticmethod
    def _policy(x):
        x = np.asarray(x, np.float32).reshape(-1, 4)
        right = (x[:, 2] + x[:, 3] > 0).astype(np.int64)
        return np.eye(2, dtype=np.float32)[right]

    def predict_p_and_v(self, x):
        self.preds += x.shape[0]
        return self._policy(x), np.zeros(x.shape[0], np.float32)

    def train(self, x, y_r, a, x2, done, tid):
        if not (x.dtype == np.float32 and x.shape[1:] == (4,) and a.dtype == np.float32 and a.shape == (x.shape[0], 2)):
            self.bad_shape += 1
        elif not np.array_equal(a, self._policy(x)):
            self.mismatch += 1
        self.seen.update(np.argmax(a, axis=1).tolist())
        self.batches.append(x.shape[0])

    def save(self, episode):
        pass

    def log(self, *a, **k):
        pass


@pytest.mark.parametrize("key,value", [("HOGWILD", True), ("FRONTEND", "device")])
def test_server_refuses_what_the_vector_net_lacks(monkeypatch, key, value):
    Config = _keep(monkeypatch)
    from Server import Server
    monkeypatch.setattr(Config, "GAME", "CartPole-v0")
    monkeypatch.setattr(Config, "CPU_AFFINITY", "off")
    monkeypatch.setattr(Config, key, value)
    with pytest.raises(ValueError):
        Server(model=_CartStandIn(), max_agents=4)


def test_server_refuses_data_parallel(monkeypatch):
    Config = _keep(monkeypatch)
    from Server import Server
    monkeypatch.setattr(Config, "GAME", "CartPole-v0")
    monkeypatch.setattr(Config, "CPU_AFFINITY", "off")
    with pytest.raises(ValueError, match="data-parallel"):
        Server(model=_CartStandIn(), max_agents=4, engine_group=object())


@pytest.mark.timeout(120)
def test_server_runs_cartpole_with_a_stand_in_model(tmp_path, monkeypatch):
    Config = _keep(monkeypatch)
    monkeypatch.chdir(tmp_path)
    for k, v in (("GAME", "CartPole-v0"), ("AGENTS", 3), ("PREDICTORS", 1), ("TRAINERS", 1), ("TIME_MAX", 5),
                 ("DYNAMIC_SETTINGS", False), ("SAVE_MODELS", False), ("TRAINING_MIN_BATCH_SIZE", 0),
                 ("CONTINUOUS_INPUT", True), ("DISCRATE_INPUT", False), ("CPU_AFFINITY", "off")):
        monkeypatch.setattr(Config, k, v)
    from Server import Server
    model = _CartStandIn()
    srv = Server(model=model, max_agents=8)
    assert Config.DISCRATE_INPUT and not Config.CONTINUOUS_INPUT and not srv.transport.float_actions
    assert srv.transport.state_bytes == 16 and srv.state_dim == (4,) and srv.num_actions == 2 and srv.vector
    srv.main(max_seconds=8)
    assert model.preds > 600 and model.batches
    assert model.bad_shape == 0 and model.mismatch == 0 and model.seen == {0, 1}
    with open(tmp_path / "results.txt") as f:
        lines = [ln for ln in f if ln.strip()]
    assert lines and all(int(ln.split(",")[2]) > 0 for ln in lines)
