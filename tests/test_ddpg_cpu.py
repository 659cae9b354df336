"""USE_DDPG without a GPU: the f64 statement of the DDPG step (tests/ddpg_oracle.py) against the same graph
under torch autograd, the replay thread and the ring's bookkeeping against what the reference's ReplayBuffer returned
(tests/golden/replay_buffer.json), the Config rules, and a Server run with a stand-in model over the real transport."""
import json
import os
import queue
import threading

import numpy as np
import pytest
import torch

import ddpg_oracle as o

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-10
SHAPES = [(3, 1), (7, 3)]


def _batch(S, A, B, rng):
    return (rng.uniform(-1.5, 1.5, (B, S)), rng.uniform(-1, 1, (B, A)), rng.uniform(-1, 0, B),
            (rng.uniform(size=B) < 0.3).astype(np.float64), rng.uniform(-1.5, 1.5, (B, S)))


def _t(P, grad=()):
    return {k: torch.tensor(v, dtype=torch.float64, requires_grad=k in grad) for k, v in P.items()}


def _bn(P, name, h):
    return P[name + "/gamma"] * (h - P[name + "/moving_mean"]) / torch.sqrt(P[name + "/moving_variance"] + o.BN_EPS) + P[name + "/beta"]


def _actor(P, x):
    a1 = torch.relu(_bn(P, "actor_norm1", x @ P["actor_fc1/W"] + P["actor_fc1/b"]))
    a2 = torch.relu(_bn(P, "actor_norm2", a1 @ P["actor_fc2/W"] + P["actor_fc2/b"]))
    return torch.tanh(a2 @ P["actor_output/W"] + P["actor_output/b"])


def _critic(P, x, a):
    c1 = torch.relu(_bn(P, "critic_norm1", x @ P["critic_fc1/W"] + P["critic_fc1/b"]))
    c2 = torch.relu(c1 @ P["critic_fc2/W"] + a @ P["critic_norm2/W"] + P["critic_norm2/b"])
    return c2 @ P["critic_output/W"] + P["critic_output/b"]                      # [B, 1]


def _close(got, want, tol=TOL):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape
    return np.max(np.abs(got - want)) <= tol * max(1.0, np.max(np.abs(want)))


@pytest.mark.parametrize("S,A", SHAPES)
@pytest.mark.parametrize("form", ["fork", "paired"])
def test_oracle_step_matches_torch_autograd(S, A, form):
    rng = np.random.default_rng(S + A)
    B = 9
    online, target = o.random_params(S, A, rng, stats=True), o.random_params(S, A, rng, stats=True)
    s, a, r, done, s2 = _batch(S, A, B, rng)
    ts, ta, tr, td, ts2 = (torch.tensor(v, dtype=torch.float64) for v in (s, a, r, done, s2))
    # steps 1-2
    T = _t(target)
    qt = _critic(T, ts2, _actor(T, ts2))[:, 0]
    y = torch.where(td != 0, tr, tr + 0.99 * qt)
    want_y, want_qt = o.targets(target, s2, r, done, 0.99)
    assert _close(want_y, y.numpy()) and _close(want_qt, qt.numpy())
    # step 3: the loss as the reference writes it, y of shape [B] against q of shape [B, 1]
    P = _t(online, grad=o.CRITIC_TRAINABLE)
    q = _critic(P, ts, ta)
    assert tuple(q.shape) == (B, 1) and tuple(y.shape) == (B,)
    if form == "fork":
        diff = y - q
        assert tuple(diff.shape) == (B, B)             # numpy's, TF's and torch's broadcasting: every pair
        loss = (diff ** 2).mean()
    else:
        loss = ((y.reshape(B, 1) - q) ** 2).mean()
    loss.backward()
    f, dq, g = o.critic_grads(online, s, a, want_y, form)
    for k in o.CRITIC_TRAINABLE:
        if k == o.DEAD:
            assert P[k].grad is None and not g[k].any()        # critic_fc2/b is in no forward pass
        else:
            assert _close(g[k].reshape(P[k].shape), P[k].grad.numpy()), k
    if form == "fork":
        assert _close(dq, (2.0 / B) * (q.detach().numpy()[:, 0] - want_y.mean()))
    # step 4: dq/da against autograd and against central differences
    noise = rng.normal(size=A) * 0.1
    a_out = (_actor(_t(online), ts) + torch.tensor(noise)).detach().requires_grad_(True)
    _critic(_t(online), ts, a_out).sum().backward()
    want_g = o.action_gradient(online, s, a_out.detach().numpy())
    assert _close(want_g, a_out.grad.numpy())
    base = a_out.detach().numpy()
    for i in range(A):
        d = np.zeros(A)
        d[i] = 1e-6
        num = (o.critic_forward(online, s, base + d)["q"] - o.critic_forward(online, s, base - d)["q"])[:, 0] / 2e-6
        assert np.max(np.abs(num - want_g[:, i])) <= 1e-6
    # step 5: d(out)/d(var) contracted with -g; the gradient flows through out without the noise
    PA = _t(online, grad=o.ACTOR_TRAINABLE)
    out = _actor(PA, ts)
    grads = torch.autograd.grad(out, [PA[k] for k in o.ACTOR_TRAINABLE], grad_outputs=-torch.tensor(want_g))
    _, ga = o.actor_grads(online, s, want_g)
    for k, gt in zip(o.ACTOR_TRAINABLE, grads):
        assert _close(ga[k].reshape(gt.shape), gt.numpy()), k


@pytest.mark.parametrize("cfg", [dict(), dict(critic_rmsprop=False), dict(clip=0.5, momentum=0.9)],
                         ids=["rmsprop", "adam", "clip-momentum"])
def test_oracle_optimizers_and_soft_update_match_torch(cfg):
    """Two whole steps: TF-1 RMSProp (with tf.clip_by_norm and momentum), TF's Adam, the soft update."""
    S, A, B, lr = 3, 1, 8, 3e-4
    rng = np.random.default_rng(1)
    online, target = o.random_params(S, A, rng), o.random_params(S, A, rng)
    st = o.new_state(online, target, critic_rmsprop=cfg.get("critic_rmsprop", True))
    O, T = _t(online), _t(target)
    sa = {k: torch.tensor(v) for k, v in st["slot_a"].items()}
    sb = {k: torch.tensor(v) for k, v in st["slot_b"].items()}

    def adam(k, g, rate, t):
        lr_t = rate * np.sqrt(1 - 0.999 ** t) / (1 - 0.9 ** t)
        sa[k] = 0.9 * sa[k] + 0.1 * g
        sb[k] = 0.999 * sb[k] + 0.001 * g * g
        O[k] = O[k] - lr_t * sa[k] / (torch.sqrt(sb[k]) + 1e-8)

    for t in (1, 2):
        s, a, r, done, s2 = _batch(S, A, B, rng)
        noise = rng.normal(size=A) * 0.1
        out = o.train_step(st, s, a, r.copy(), done, s2, lr, noise, **cfg)
        ts, ta, tr, td, ts2 = (torch.tensor(v, dtype=torch.float64) for v in (s, a, r, done, s2))
        y = torch.where(td != 0, tr, tr + 0.99 * _critic(T, ts2, _actor(T, ts2))[:, 0])
        P = {k: v.clone().requires_grad_(k in o.CRITIC_TRAINABLE) for k, v in O.items()}
        q = _critic(P, ts, ta)
        ((y - q) ** 2).mean().backward()
        assert _close(out["q"], q.detach().numpy()[:, 0]) and _close(out["q_max"], float(q.detach().max()))
        for k in o.CRITIC_TRAINABLE:
            g = P[k].grad
            if g is None:
                continue
            if cfg.get("clip"):
                g = g * cfg["clip"] / max(float(g.norm()), cfg["clip"])
            if cfg.get("critic_rmsprop", True):
                sa[k] = sa[k] + (g * g - sa[k]) * (1 - 0.99)
                sb[k] = sb[k] * cfg.get("momentum", 0.0) + g * (10.0 * lr) / torch.sqrt(0.1 + sa[k])
                O[k] = O[k] - sb[k]
            else:
                adam(k, g, 10.0 * lr, t)
        a_out = (_actor(O, ts) + torch.tensor(noise)).detach().requires_grad_(True)
        _critic(O, ts, a_out).sum().backward()
        PA = {k: v.clone().requires_grad_(k in o.ACTOR_TRAINABLE) for k, v in O.items()}
        grads = torch.autograd.grad(_actor(PA, ts), [PA[k] for k in o.ACTOR_TRAINABLE], grad_outputs=-a_out.grad)
        for k, g in zip(o.ACTOR_TRAINABLE, grads):
            adam(k, g, 1.0 * lr, t)
        for k in o.TRAINABLE:
            T[k] = 0.001 * O[k] + 0.999 * T[k]
    assert st["step"] == 2
    for k in o.TRAINABLE:
        assert _close(st["online"][k], O[k].numpy()), k
        assert _close(st["target"][k], T[k].numpy()), k
        assert _close(st["slot_a"][k], sa[k].numpy()) and _close(st["slot_b"][k], sb[k].numpy()), k
    assert np.array_equal(st["online"][o.DEAD], online[o.DEAD]) and not np.array_equal(st["target"][o.DEAD], target[o.DEAD])


def test_wrap_and_ou_recurrence():
    assert np.allclose(o.wrap([1.5, -1.5, 0.3, 3.25, -1.0, 1.0]), [-0.5, 0.5, 0.3, -0.75, -1.0, 1.0])
    assert np.isclose(o.ou_step(0.5, 2.0), 0.5 - 0.15 * 0.5 * 0.01 + 0.3 * 0.1 * 2.0)


# ---- the ring and the replay thread against the reference's ReplayBuffer

def _golden():
    with open(os.path.join(ROOT, "tests", "golden", "replay_buffer.json")) as f:
        return json.load(f)["cases"]


class _Transport:
    """Rollouts of `chunk` tagged rows; pop_rollout hands out one per call, then reports the shutdown."""

    def __init__(self, adds, chunk, S=3):
        self.S, self.todo, self.next_tag = S, [min(chunk, adds - i) for i in range(0, adds, chunk)], 0
        self.popped = self.released = 0
        self.current = None

    def pop_rollout(self, timeout_ms):
        assert self.popped == self.released, "a second rollout taken while one is held"
        if not self.todo:
            return -4
        n = self.todo.pop(0)
        row = np.zeros((n, 8), np.float32)
        row[:, 0] = row[:, 3] = np.arange(self.next_tag, self.next_tag + n)
        self.next_tag += n
        self.current = (row.view(np.uint8).reshape(n, 32), np.zeros(n, np.float32), np.zeros((n, 1), np.float32))
        self.popped += 1
        return 0

    def rows(self, slot):
        return self.current[0].shape[0]

    def rollout_views(self, slot):
        return self.current

    def release(self, slot):
        self.released += 1


class _RingModel:
    """Stand-in for the handle's ring: the rows by slot, and train_replay's refusal rule (include/ga3c_abi.h)."""

    def __init__(self, capacity):
        self.replay_capacity, self.total, self.slots = capacity, 0, {}
        self.events = []

    def replay_add(self, s, a, r, done, s2):
        for tag in s[:, 0]:
            self.slots[self.total % self.replay_capacity] = int(tag)
            self.total += 1
        self.events.append(("add", len(s)))
        return min(self.total, self.replay_capacity), self.total

    def stale(self, slot, stamp):
        last = (self.total - 1) - ((self.total - 1 - slot) % self.replay_capacity)
        return last >= stamp


class _Server:
    def __init__(self, model, q=None):
        self.model, self.replay_q, self.zero_copy, self.state_dim = model, q or queue.Queue(), False, (3,)
        self.stats = type("S", (), {"replay_memory_size": type("V", (), {"value": 0})()})()


@pytest.mark.parametrize("case", range(4))
def test_replay_thread_draws_the_reference_positions(case, monkeypatch):
    import ga3c_amd  # noqa: F401
    from Config import Config
    import ThreadReplay as tr
    c = _golden()[case]
    monkeypatch.setattr(Config, "TRAINING_MIN_BATCH_SIZE", c["batch"])
    monkeypatch.setattr(Config, "REPLAY_MIN_QUEUE_SIZE", 10 ** 9)        # the queue never looks full: one sample per pass
    monkeypatch.setattr(Config, "REPLAY_BUFFER_RANDOM_SEED", c["seed"])
    model = _RingModel(c["capacity"])

    class Q(queue.Queue):
        def put(self, item, *a, **k):
            model.events.append(("sample", item[1]))
            # the tags in the sampled slots, looked up at once, are the tags the reference drew
            self.drawn.append((item[1], [model.slots[int(s)] for s in item[0]]))
            super().put(item, *a, **k)
    q = Q()
    q.drawn = []
    srv = _Server(model, q)
    th = tr.ThreadReplay(srv, _Transport(c["adds"], c["chunk"]))
    th._run()
    # the thread samples at the top of a pass, the recording after each add: the buffers are the same ones, the last pass
    # (which finds the transport shut down) included
    want = [(s["total"], s["tags"]) for s in c["samples"]]
    assert q.drawn == want
    for s in c["samples"]:
        assert list(tr.ring_slots(s["positions"], s["total"], c["capacity"])) == \
            [t % c["capacity"] for t in s["tags"]]
    # eviction order: what the ring holds at the end, oldest first
    ring = o.Ring(c["capacity"])
    ring.add(c["adds"])
    assert [model.slots[ring.slot(j)] for j in range(ring.size)] == c["final_tags"] and ring.size == c["final_size"]
    assert srv.stats.replay_memory_size.value == c["final_size"]
    # one rollout per pass, released before the next is taken, sampling first
    kinds = [e[0] for e in model.events]
    assert "sample" in kinds and all(not (x == y == "sample") for x, y in zip(kinds, kinds[1:]))
    assert th.transport.popped == th.transport.released == len([e for e in kinds if e == "add"])


def test_more_than_a_batch_before_the_first_sample(monkeypatch):
    import ga3c_amd  # noqa: F401
    from Config import Config
    import ThreadReplay as tr
    monkeypatch.setattr(Config, "TRAINING_MIN_BATCH_SIZE", 12)
    monkeypatch.setattr(Config, "REPLAY_MIN_QUEUE_SIZE", 2)
    model = _RingModel(100)
    srv = _Server(model)
    th = tr.ThreadReplay(srv, _Transport(30, 6))
    th._run()
    # sizes at the sampling points: 0, 6, 12 (not MORE than 12: nothing), 18 (first batch), 24 (second; then the queue holds 2)
    assert [e for e in model.events if e[0] != "add"] == [] and srv.replay_q.qsize() == 2
    assert [srv.replay_q.get()[1] for _ in range(2)] == [18, 24]


def test_a_sampled_slot_overwritten_before_training_is_refused():
    """The overwrite rule: (slots, stamp) travels; a slot written after `stamp` is stale (GA3C_ELOST in the engine)."""
    model = _RingModel(10)
    model.replay_add(np.arange(10, dtype=np.float32).reshape(10, 1), None, None, None, None)
    stamp = model.total
    assert not any(model.stale(s, stamp) for s in range(10))
    model.replay_add(np.array([[10.0], [11.0]], np.float32), None, None, None, None)        # overwrites slots 0 and 1
    assert [model.stale(s, stamp) for s in range(10)] == [True, True] + [False] * 8
    assert not any(model.stale(s, model.total) for s in range(10))

    import ga3c_amd  # noqa: F401
    import _native as nat
    from Server import Server
    lost = []

    class M:
        def train_replay(self, slots, stamp):
            if any(model.stale(int(s), stamp) for s in slots):
                raise nat.StateLost("stale")
    srv = Server.__new__(Server)
    srv.model, srv.lost_train_batches = M(), 0
    srv._count_train_step = lambda *a, **k: lost.append("trained")
    srv.train_model_replay(np.array([0, 5], np.int32), stamp, 0)
    srv.train_model_replay(np.array([4, 5], np.int32), stamp, 0)
    assert srv.lost_train_batches == 1 and lost == ["trained"]


# ---- Config rules

@pytest.fixture
def ddpg_config(monkeypatch):
    import ga3c_amd  # noqa: F401
    from Config import Config
    for k, v in (("GAME", "Pendulum-v0"), ("USE_DDPG", True), ("CONTINUOUS_INPUT", True), ("DISCRATE_INPUT", False),
                 ("TRAINING_MIN_BATCH_SIZE", 64), ("USE_REPLAY_MEMORY", False), ("DISCOUNTING", True)):
        monkeypatch.setattr(Config, k, v)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    return Config


def test_use_ddpg_implies_the_reference_settings(ddpg_config):
    from Config import resolve_ddpg
    resolve_ddpg()
    c = ddpg_config
    assert c.USE_REPLAY_MEMORY and not c.DISCOUNTING and c.add_OUnoise and not c.add_uncertainity
    assert (c.REPLAY_BUFFER_SIZE, c.REPLAY_BUFFER_RANDOM_SEED, c.REPLAY_MIN_QUEUE_SIZE) == (1000000, 12345, 2)
    assert c.DDPG_FUTURE_REWARD_CALC and (c.tau, c.gamma, c.actor_lr, c.critic_lr, c.RMSPROP) == (0.001, 0.99, 1, 10, True)
    assert c.DDPG_CRITIC_LOSS == 'fork'


def test_without_use_ddpg_nothing_changes(monkeypatch):
    import ga3c_amd  # noqa: F401
    from Config import Config, resolve_ddpg
    monkeypatch.setattr(Config, "USE_DDPG", False)
    before = dict(vars(Config))
    resolve_ddpg()
    assert dict(vars(Config)) == before


@pytest.mark.parametrize("key,value", [("GAME", "PongDeterministic-v4"), ("DUAL_RMSPROP", True), ("HOGWILD", True),
                                       ("FRONTEND", "device"), ("add_uncertainity", True), ("TRAINING_MIN_BATCH_SIZE", 0),
                                       ("DDPG_CRITIC_LOSS", "mean"), ("WORLD_SIZE", "2")])
def test_refusals(ddpg_config, monkeypatch, key, value):
    from Config import resolve_ddpg
    if key == "WORLD_SIZE":
        monkeypatch.setenv("WORLD_SIZE", value)
    else:
        monkeypatch.setattr(ddpg_config, key, value)
    with pytest.raises(ValueError):
        resolve_ddpg()


def test_discrete_game_is_refused(ddpg_config, monkeypatch):
    from Config import resolve_ddpg
    monkeypatch.setattr(ddpg_config, "GAME", "PongDeterministic-v4")
    monkeypatch.setattr(ddpg_config, "CONTINUOUS_INPUT", False)
    with pytest.raises(ValueError, match="continuous"):
        resolve_ddpg()


def test_argv_applies_the_rules(ddpg_config, monkeypatch):
    import GA3C
    monkeypatch.setattr(ddpg_config, "USE_DDPG", False)
    GA3C.apply_argv(["GAME=Pendulum-v0", "USE_DDPG=True", "TRAINING_MIN_BATCH_SIZE=64"])
    assert ddpg_config.USE_REPLAY_MEMORY and not ddpg_config.DISCOUNTING
    with pytest.raises(ValueError, match="TRAINING_MIN_BATCH_SIZE"):
        GA3C.apply_argv(["GAME=Pendulum-v0", "USE_DDPG=True", "TRAINING_MIN_BATCH_SIZE=0"])


def test_initial_arena_is_one_soft_update_of_independent_targets():
    import ga3c_amd  # noqa: F401
    import NetworkDDPG as nd
    online, target = nd.initial_arena(3, 1, 12345, tau=0.001)
    again, _ = nd.initial_arena(3, 1, 12345, tau=0.001)
    assert all(np.array_equal(online[k], again[k]) for k in online)
    _, full = nd.initial_arena(3, 1, 12345, tau=1.0)
    _, none = nd.initial_arena(3, 1, 12345, tau=0.0)
    w = "actor_fc2/W"
    assert np.array_equal(full[w], online[w]) and not np.array_equal(none[w], online[w])
    assert np.allclose(target[w], 0.001 * online[w] + 0.999 * none[w], atol=1e-7)
    assert np.max(np.abs(online[w])) <= 0.04 + 1e-9 and abs(float(online[w].std()) - 0.0176) < 0.002     # truncated at 2 sigma
    assert np.max(np.abs(online["actor_output/W"])) <= 0.003 and not online["actor_fc1/b"].any()
    assert abs(float(online["actor_norm1/gamma"].mean()) - 1.0) < 0.001
    assert tuple(online) == nd.TRAINABLE == o.TRAINABLE and nd.param_shapes(3, 1) == {k: o.shapes(3, 1)[k] for k in o.TRAINABLE}


def test_ddpg_abi_is_declared_exported_and_bound():
    import re
    import ga3c_amd  # noqa: F401
    import _native as nat
    text = open(os.path.join(ROOT, "include", "ga3c_abi.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = sorted(set(re.findall(r"\b(ga3c_ddpg_[a-z0-9_]+)\s*\(", text)))
    assert len(names) >= 25 and "ga3c_ddpg_train_replay" in names
    lib = nat.hip_lib()
    for name in names:
        assert hasattr(lib, name) and name in nat.HIP_SIGNATURES, name
    import ctypes as C
    assert C.sizeof(nat.DdpgConfig) == 80


# ---- a Server run with a stand-in model over the real transport

class _DdpgStandIn:
    """Keeps every row the replay thread adds; trains on nothing.  No register_transport: the host path of ThreadReplay."""
    replay_capacity = 5000

    def __init__(self):
        self.rows, self.total, self.trained, self.lock = [], 0, 0, threading.Lock()
        self.learning_rate = self.beta = 0.0

    def predict_p_and_v(self, x):
        a = np.tanh(x[:, :1] * 0.5).astype(np.float32)
        return a, a

    def replay_add(self, s, a, r, done, s2):
        with self.lock:
            self.rows.append(tuple(np.array(t, copy=True) for t in (s, a, r, done, s2)))
            self.total += len(r)
        return min(self.total, self.replay_capacity), self.total

    def train_replay(self, slots, stamp):
        assert slots.dtype == np.int32 and slots.size == 16 and 0 <= slots.min() and slots.max() < min(self.total, 5000)
        assert stamp <= self.total
        self.trained += 1

    def save(self, episode):
        pass

    def log(self, *a, **k):
        pass


@pytest.mark.timeout(120)
def test_server_ships_s2_done_and_raw_rewards_to_the_replay_thread(tmp_path, monkeypatch):
    import ga3c_amd  # noqa: F401
    from Config import Config
    monkeypatch.chdir(tmp_path)
    for k, v in (("GAME", "Pendulum-v0"), ("USE_DDPG", True), ("AGENTS", 3), ("PREDICTORS", 1), ("TRAINERS", 1),
                 ("TIME_MAX", 5), ("DYNAMIC_SETTINGS", False), ("SAVE_MODELS", False), ("TRAINING_MIN_BATCH_SIZE", 16),
                 ("CONTINUOUS_INPUT", False), ("DISCRATE_INPUT", True), ("CPU_AFFINITY", "off"), ("DISCOUNTING", True),
                 ("USE_REPLAY_MEMORY", False)):
        monkeypatch.setattr(Config, k, v)
    from Server import Server
    model = _DdpgStandIn()
    srv = Server(model=model, max_agents=8)
    assert Config.USE_REPLAY_MEMORY and not Config.DISCOUNTING and srv.ddpg
    assert srv.transport.row_bytes == 32 and srv.transport.state_bytes == 12 and srv.transport.float_actions
    srv.main(max_seconds=8)
    assert model.trained > 0 and model.total > 200 and srv.stats.replay_memory_size.value == min(model.total, 5000)
    dones = 0
    for s, a, r, done, s2 in model.rows:
        assert s.shape == s2.shape == (len(r), 3) and a.shape == (len(r), 1) and set(np.unique(done)) <= {0.0, 1.0}
        assert np.array_equal(s2[:-1], s[1:]), "s2 of a row is not the next row's s"
        assert not done[:-1].any(), "done before a rollout's last row"
        dones += int(done[-1])
        # un-accumulated: the wrapper's r * 0.005 - 1 of one step lies in [-1.09, -1]; a discounted sum would not
        assert np.all(r <= -1.0 + 1e-6) and np.all(r >= -1.1)
        assert np.allclose(a[:, 0], np.tanh(s[:, 0] * 0.5), atol=1e-6)
    assert dones > 0
