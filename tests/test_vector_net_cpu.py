"""GAME = 'Pendulum-v0' without a GPU: the f64 statement of the vector-state network
(tests/mlp_oracle.py) against torch autograd and central differences, its parameter table and initialisation, the restated
Pendulum-v0 and the reference's wrapper around it, the GAME / CONTINUOUS_INPUT resolution, and a Server run with a stand-in
model."""
import os

import numpy as np
import pytest

import ga3c_oracle as o
import mlp_oracle as m

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _case(state_dim, num_actions, bsz, seed):
    params = m.init_params(state_dim, num_actions, seed=seed)
    rng = np.random.default_rng(seed)
    params["logits_p/out_x/b"] = rng.uniform(-2, 2, num_actions)
    params["logits_p/out_y/b"] = rng.uniform(-2, 2, num_actions)
    x = rng.uniform(-2, 2, size=(3 * bsz, state_dim))
    x = x[m.safe_rows(params, x, 1e-2)][:bsz]
    assert x.shape[0] == bsz
    y = rng.normal(size=bsz)
    a = rng.uniform(-1, 1, size=(bsz, num_actions))
    return params, x, y, a


def _max_rel(got, want):
    got, want = np.asarray(got).reshape(-1), np.asarray(want).reshape(-1)
    return np.max(np.abs(got - want)) / max(1.0, np.max(np.abs(want)))


def _torch_grads(params, x, y_r, a, beta):
    torch = pytest.importorskip("torch")
    t = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in params.items()}
    h = torch.tensor(x, dtype=torch.float64)
    for name, _, sig in m.TRUNK:
        h = h @ t[name + "/w"] + t[name + "/b"]
        if sig:
            h = torch.sigmoid(h)
    v = (h @ t["logits_v/w"] + t["logits_v/b"])[:, 0]
    X = torch.sigmoid(h @ t["logits_p/out_x/w"] + t["logits_p/out_x/b"]) - 0.5
    Y = torch.sigmoid(h @ t["logits_p/out_y/w"] + t["logits_p/out_y/b"]) - 0.5
    out = torch.atan2(Y, X) / np.pi
    yt, at = torch.tensor(y_r, dtype=torch.float64), torch.tensor(a, dtype=torch.float64)
    c1 = ((out * at).sum(1) * (yt - v.detach())).sum()
    c2 = (-beta * (out * out).sum(1)).sum()
    cv = 0.5 * ((yt - v) ** 2).sum()
    cost = -(c1 + c2) + cv
    cost.backward()
    return out.detach().numpy(), (c1.item(), c2.item(), cv.item()), {k: t[k].grad.numpy() for k in t}


@pytest.mark.parametrize("state_dim,num_actions", [(3, 1), (3, 3), (7, 1), (7, 3)])
def test_oracle_matches_torch_autograd(state_dim, num_actions):
    params, x, y, a = _case(state_dim, num_actions, 9, 11 + state_dim + num_actions)
    out, costs, tg = _torch_grads(params, x, y, a, 0.01)
    losses, g = m.loss_and_grads(params, x, y, a, 0.01)
    assert np.max(np.abs(m.forward(params, x)["o"] - out)) < 1e-12
    for got, want in zip((losses["cost_p_1_agg"], losses["cost_p_2_agg"], losses["cost_v"]), costs):
        assert abs(got - want) < 1e-10
    for k in m.PARAM_ORDER:
        assert _max_rel(g[k], tg[k]) < 1e-10, k


@pytest.mark.parametrize("state_dim,num_actions", [(3, 1), (7, 3)])
def test_oracle_matches_central_differences(state_dim, num_actions):
    params, x, y, a = _case(state_dim, num_actions, 5, 3 + state_dim)
    beta = 0.05
    adv = y - m.forward(params, x)["v"]
    _, g = m.loss_and_grads(params, x, y, a, beta)
    rng = np.random.default_rng(0)
    eps = 1e-6
    for k in m.PARAM_ORDER:
        for idx in [tuple(rng.integers(0, s) for s in params[k].shape) for _ in range(3)]:
            save = params[k][idx]
            vals = []
            for d in (eps, -eps):
                params[k][idx] = save + d
                losses, _ = m.loss_and_grads(params, x, y, a, beta, adv_const=adv)
                vals.append(losses["cost_all"])
            params[k][idx] = save
            fd = (vals[0] - vals[1]) / (2 * eps)
            assert abs(fd - g[k][idx]) < 1e-6 * max(1.0, abs(fd)), (k, idx, fd, g[k][idx])


@pytest.mark.parametrize("clip,momentum", [(None, 0.0), (40.0, 0.0), (None, 0.9), (0.05, 0.5)])
def test_one_rmsprop_step_matches_torch(clip, momentum):
    """One TF-1 RMSProp step on the oracle's gradient (with clip_by_average_norm / momentum) against the same arithmetic on
    torch autograd's gradient."""
    params, x, y, a = _case(3, 1, 8, 5)
    _, _, tg = _torch_grads(params, x, y, a, 0.01)
    _, g = m.loss_and_grads(params, x, y, a, 0.01)
    p1 = {k: v.copy() for k, v in params.items()}
    ms1 = {k: np.ones_like(v) for k, v in params.items()}
    mom1 = {k: np.zeros_like(v) for k, v in params.items()}
    m.rmsprop_update(p1, ms1, g, 1e-3, momentum=momentum, mom=mom1, clip=clip)
    for k in m.PARAM_ORDER:
        gt = tg[k] if clip is None else o.clip_by_average_norm(tg[k], clip)
        ms = 0.99 + 0.01 * gt * gt
        step = 1e-3 * gt / np.sqrt(ms + 0.1)
        want = params[k] - step           # mom starts at 0: the first step is the plain step with or without momentum
        assert np.max(np.abs(p1[k] - want)) < 1e-12, k
        assert np.max(np.abs(ms1[k] - ms)) < 1e-12
        if momentum:
            assert np.max(np.abs(mom1[k] - step)) < 1e-12


def test_parameter_table_order_and_init():
    import ga3c_amd  # noqa: F401
    import NetworkVP_vector as nv
    assert nv.param_order() == m.PARAM_ORDER
    assert len(m.PARAM_ORDER) == 16
    assert m.PARAM_ORDER[:4] == ("dense11_p/w", "dense11_p/b", "dense12_p/w", "dense12_p/b")
    assert m.PARAM_ORDER[-6:] == ("logits_v/w", "logits_v/b", "logits_p/out_x/w", "logits_p/out_x/b", "logits_p/out_y/w",
                                  "logits_p/out_y/b")
    for s, a in ((3, 1), (7, 3)):
        shapes = nv.param_shapes(s, a)
        assert shapes == m.param_shapes(s, a)
        assert sum(int(np.prod(v)) for v in shapes.values()) == m.param_count(s, a)
        theta = nv.initial_arena(s, a, 12345)
        assert theta.dtype == np.float32 and theta.size == m.param_count(s, a)
        assert np.array_equal(theta, m.flat(m.init_params(s, a, 12345)).astype(np.float32))
        assert np.max(np.abs(theta)) <= 0.3 and np.min(theta) < -0.29 and np.max(theta) > 0.29
    assert m.param_count(3, 1) == 99447


# ---- Pendulum-v0 and the reference's wrapper
def _pend_env(monkeypatch, seed=7):
    import ga3c_amd  # noqa: F401
    from Config import Config
    import EnvironmentPend as ep
    monkeypatch.setattr(Config, "RANDOM_SEED", seed)
    return ep, ep.Environment(0)


def test_pendulum_step_equations(monkeypatch):
    ep, env = _pend_env(monkeypatch)
    th, thdot = 0.7, -3.0
    env.game.state = np.array([th, thdot])
    r, done = env.step(np.array([0.4], np.float32))
    u = float(np.float32(0.4)) * 2.0                         # check_bounds, then the action bound
    cost = th ** 2 + 0.1 * thdot ** 2 + 0.001 * u * u
    nthdot = thdot + (-3 * 10.0 / 2 * np.sin(th + np.pi) + 3.0 * u) * 0.05
    nth = th + nthdot * 0.05
    assert np.allclose(env.game.state, [nth, nthdot], atol=1e-15, rtol=0)
    assert env.current_state.dtype == np.float32 and env.current_state.shape == (3,)
    assert np.allclose(env.current_state, np.float32([np.cos(nth), np.sin(nth), nthdot]))
    assert abs(r - (-cost * 0.005 - 1.0)) < 1e-12 and not done
    # angle normalisation in the cost
    env.game.state = np.array([2 * np.pi + 0.5, 0.0])
    r, _ = env.step(np.array([0.0]))
    assert abs(r - (-(0.5 ** 2) * 0.005 - 1.0)) < 1e-9


def test_pendulum_speed_clip_and_torque(monkeypatch):
    ep, env = _pend_env(monkeypatch)
    env.game.state = np.array([np.pi / 2, 7.9])              # gravity and torque push past max_speed
    env.step(np.array([1.0]))
    nthdot = 7.9 + (-15.0 * np.sin(np.pi / 2 + np.pi) + 3.0 * 2.0) * 0.05
    assert nthdot > 8.0 and env.game.state[1] == 8.0
    assert abs(env.game.state[0] - (np.pi / 2 + nthdot * 0.05)) < 1e-15     # th moves with the unclipped speed
    # check_bounds turns an out-of-range action around before the bound scales it; torque is clipped at 2
    assert np.allclose(ep.check_bounds(np.array([1.5]), 1.0, -1.0, True), [-0.5])
    assert np.allclose(ep.check_bounds(np.array([-1.25]), 1.0, -1.0, True), [0.75])
    assert np.allclose(ep.check_bounds(np.array([0.3]), 1.0, -1.0, True), [0.3])
    game = ep.Pendulum(np.random.default_rng(0))
    game.state = np.array([0.0, 0.0])
    _, r5, _ = game.step(np.array([5.0]))
    assert abs(r5 - (-0.001 * 4.0)) < 1e-15


def test_pendulum_reset_and_time_limit(monkeypatch):
    ep, env = _pend_env(monkeypatch, seed=3)
    rng = np.random.Generator(np.random.PCG64(3))
    th, thdot = rng.uniform(low=[-np.pi, -1.0], high=[np.pi, 1.0])
    assert np.array_equal(env.game.state, [th, thdot])       # reset: U(-pi, pi) x U(-1, 1) from PCG64(seed + agent id)
    assert env.current_state is None
    env.step(None)                                           # the agent's very first step: zero torque
    nthdot = thdot + (-15.0 * np.sin(th + np.pi)) * 0.05
    assert abs(env.game.state[1] - np.clip(nthdot, -8, 8)) < 1e-15
    for k in range(2, 201):
        _, done = env.step(np.array([0.1]))
        assert done == (k == 200)
    last = env.current_state.copy()
    env.reset()
    # reset() keeps current_state: the next episode's first action is predicted from the last episode's last observation
    assert env.current_state is not None and np.array_equal(env.current_state, last)
    for k in range(1, 201):
        _, done = env.step(np.array([0.0]))
        assert done == (k == 200)
    assert ep.Environment(1).game.state.tolist() != ep.Environment(0).game.state.tolist()
    assert env.get_num_actions() == 1 and env.get_state_dim() == (3,)


def test_agent_episode_starts_with_a_zero_torque_step_and_a_stale_state(monkeypatch):
    """ProcessAgent.run_episode on the Pendulum wrapper: the first episode begins with step(None); every later episode's
    first prediction is asked for the previous episode's last observation."""
    import ga3c_amd  # noqa: F401
    from Config import Config
    from ProcessAgent import ProcessAgent
    ep, env = _pend_env(monkeypatch)
    monkeypatch.setattr(Config, "CONTINUOUS_INPUT", True)
    monkeypatch.setattr(Config, "TIME_MAX", 1000)
    asked = []

    class _T:
        def round_trip(self, agent, state, flags, timeout_ms, u, submit=True):
            asked.append(np.frombuffer(state.tobytes(), np.float32).copy())
            return 0, np.array([0.5], np.float32), 0.0, -1

    ag = ProcessAgent.__new__(ProcessAgent)
    ag.transport, ag.id, ag.env, ag.requests = _T(), 0, env, 0
    ag.names_states, ag.discount_factor, ag.time_count = False, 0.99, 0
    steps = []
    orig = env.step
    monkeypatch.setattr(env, "step", lambda a: (steps.append(None if a is None else float(np.asarray(a)[0])), orig(a))[1])
    (rows, _), = list(ag.run_episode())
    assert steps[0] is None and all(s == 0.5 for s in steps[1:]) and len(steps) == 200
    assert len(rows) == 199 and rows[-1].done
    assert all(r.action.dtype == np.float32 and r.action.tolist() == [0.5] for r in rows)
    last = env.current_state.copy()
    asked.clear()
    (rows2, _), = list(ag.run_episode())
    assert np.array_equal(asked[0], last)                    # the stale first observation
    assert len(rows2) == 200


# ---- configuration
def test_game_sets_continuous_input_and_refuses_a_contradiction(monkeypatch):
    import ga3c_amd  # noqa: F401
    from Config import Config
    import GA3C
    for k in ("CONTINUOUS_INPUT", "DISCRATE_INPUT", "GAME"):
        monkeypatch.setattr(Config, k, getattr(Config, k))
    GA3C.apply_argv(["GAME=Pendulum-v0"])
    assert Config.CONTINUOUS_INPUT and not Config.DISCRATE_INPUT
    GA3C.apply_argv(["GAME=Pendulum-v0", "CONTINUOUS_INPUT=True"])
    assert Config.CONTINUOUS_INPUT
    GA3C.apply_argv(["GAME=Pendulum-v0", "DISCRATE_INPUT="])
    assert Config.CONTINUOUS_INPUT
    with pytest.raises(ValueError):
        GA3C.apply_argv(["GAME=Pendulum-v0", "CONTINUOUS_INPUT="])
    with pytest.raises(ValueError):
        GA3C.apply_argv(["GAME=Pendulum-v0", "DISCRATE_INPUT=True"])
    GA3C.apply_argv(["GAME=PongDeterministic-v4", "CONTINUOUS_INPUT="])
    assert Config.DISCRATE_INPUT and not Config.CONTINUOUS_INPUT


@pytest.mark.parametrize("key,value", [("HOGWILD", True), ("FRONTEND", "device")])
def test_server_refuses_what_the_vector_net_lacks(monkeypatch, key, value):
    import ga3c_amd  # noqa: F401
    from Config import Config
    from Server import Server
    monkeypatch.setattr(Config, "GAME", "Pendulum-v0")
    monkeypatch.setattr(Config, "CONTINUOUS_INPUT", Config.CONTINUOUS_INPUT)
    monkeypatch.setattr(Config, "DISCRATE_INPUT", Config.DISCRATE_INPUT)
    monkeypatch.setattr(Config, "CPU_AFFINITY", "off")
    monkeypatch.setattr(Config, key, value)
    with pytest.raises(ValueError):
        Server(model=_PendStandIn(), max_agents=4)


def test_server_refuses_data_parallel(monkeypatch):
    import ga3c_amd  # noqa: F401
    from Config import Config
    from Server import Server
    monkeypatch.setattr(Config, "GAME", "Pendulum-v0")
    monkeypatch.setattr(Config, "CONTINUOUS_INPUT", Config.CONTINUOUS_INPUT)
    monkeypatch.setattr(Config, "DISCRATE_INPUT", Config.DISCRATE_INPUT)
    monkeypatch.setattr(Config, "CPU_AFFINITY", "off")
    with pytest.raises(ValueError, match="data-parallel"):
        Server(model=_PendStandIn(), max_agents=4, engine_group=object())


class _PendStandIn:
    """A deterministic continuous policy of the state, so a trainer can check that each row's action is what the agent was
    answered for exactly that state."""
    def __init__(self):
        self.learning_rate = self.beta = 0.0
        self.batches, self.mismatch, self.preds, self.bad_shape = [], 0, 0, 0

    @staticmethod
    def _policy(x):
        x = np.asarray(x, np.float32).reshape(-1, 3)         # (row by row: a matmul's rounding may depend on the batch)
        return np.tanh(np.float32(0.7) * x[:, 0] - np.float32(0.4) * x[:, 1] + np.float32(0.2) * x[:, 2])[:, None]

    def predict_p_and_v(self, x):
        self.preds += x.shape[0]
        return self._policy(x), np.zeros(x.shape[0], np.float32)

    def train(self, x, y_r, a, x2, done, tid):
        if not (x.dtype == np.float32 and x.shape[1:] == (3,) and a.dtype == np.float32 and a.shape == (x.shape[0], 1)):
            self.bad_shape += 1
        elif not np.array_equal(a, self._policy(x)):
            self.mismatch += 1
        self.batches.append(x.shape[0])

    def save(self, episode):
        pass

    def log(self, *a, **k):
        pass


@pytest.mark.timeout(120)
def test_server_runs_pendulum_with_a_stand_in_model(tmp_path, monkeypatch):
    import ga3c_amd  # noqa: F401
    from Config import Config
    monkeypatch.chdir(tmp_path)
    for k, v in (("GAME", "Pendulum-v0"), ("AGENTS", 3), ("PREDICTORS", 1), ("TRAINERS", 1), ("TIME_MAX", 5),
                 ("DYNAMIC_SETTINGS", False), ("SAVE_MODELS", False), ("TRAINING_MIN_BATCH_SIZE", 0),
                 ("CONTINUOUS_INPUT", False), ("DISCRATE_INPUT", True), ("CPU_AFFINITY", "off")):
        monkeypatch.setattr(Config, k, v)
    from Server import Server
    model = _PendStandIn()
    srv = Server(model=model, max_agents=8)
    assert Config.CONTINUOUS_INPUT and srv.transport.float_actions
    assert srv.transport.state_bytes == 12 and srv.state_dim == (3,) and srv.num_actions == 1
    srv.main(max_seconds=8)
    assert model.preds > 600 and model.batches
    assert model.bad_shape == 0 and model.mismatch == 0
    with open(tmp_path / "results.txt") as f:
        lines = [ln for ln in f if ln.strip()]
    assert lines and all(int(ln.split(",")[2]) > 0 for ln in lines)
