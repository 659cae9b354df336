"""PRIORITIZED_REPLAY without a GPU: the numpy statement (tests/per_oracle.py) against what proportional
prioritised replay must do, its weighted loss against torch autograd, the Config rules, the replay thread's token, a Server run
with a stand-in model, and the new entries' declarations."""
import os
import random
import re
import threading

import numpy as np
import pytest
import torch

import ddpg_oracle as o
import per_oracle as per
from test_ddpg_cpu import _Server, _Transport, _critic, _t

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("ga3c_ddpg_priorities_create", "ga3c_ddpg_priorities_destroy", "ga3c_ddpg_priorities_get",
           "ga3c_ddpg_priorities_set", "ga3c_ddpg_sample_prioritized", "ga3c_ddpg_train_prioritized",
           "ga3c_ddpg_time_prioritized")


# ---- the statement itself

def test_draw_frequencies_follow_the_priorities():
    """400 samples of 64 from 3000 priorities in U(0.05, 3): the counts of 30 groups of 100 slots lie within 5 binomial
    standard deviations of N p (a stratified draw only tightens a binomial's spread)."""
    rng = np.random.default_rng(0)
    size, B, draws = 3000, 64, 400
    pa = rng.uniform(0.05, 3, size).astype(np.float32)
    counts = np.zeros(size)
    for n in range(draws):
        slots, _, _ = per.draw(pa, size, B, 7, n)
        assert slots.min() >= 0 and slots.max() < size
        np.add.at(counts, slots, 1)
    p = pa.astype(np.float64) / pa.astype(np.float64).sum()
    N = B * draws
    g, pg = counts.reshape(30, 100).sum(1), p.reshape(30, 100).sum(1)
    z = (g - N * pg) / np.sqrt(N * pg * (1 - pg))
    print("largest |z| over the groups: %.3f" % np.abs(z).max())
    assert np.abs(z).max() <= 5.0


def test_alpha_zero_is_uniform_with_unit_weights():
    size, B = 2500, 50
    td = np.random.default_rng(1).uniform(0, 4, size)
    pa = ((td + 0.01) ** 0.0).astype(np.float32)
    assert np.all(pa == 1.0)
    slots, w = per.sample(pa, size, B, 3, 0, beta_is=0.7)
    assert np.all(w == 1.0)
    # stratum k of B equal ones is [k size / B, (k + 1) size / B)
    assert np.all(slots // (size // B) == np.arange(B))


def test_a_heavy_slot_is_drawn_for_its_share():
    size, B = 2049, 64
    pa = np.full(size, 1e-3, np.float32)
    pa[700] = 50.0                                   # 50 / (50 + 2.048) = 96 % of the mass
    share = 50.0 / float(pa.astype(np.float64).sum())
    slots, total, _ = per.draw(pa, size, B, 5, 0)
    assert abs(total - float(pa.astype(np.float64).sum())) <= 1e-12 * total
    hits = int((slots == 700).sum())
    assert abs(hits - share * B) <= 2.0, hits      # 61.5 strata fit into the slot's mass; the one at each end is split
    w = per.weights(pa, size, slots, total, 1.0)
    assert w.max() == 1.0 and np.all(w[slots == 700] < 1e-4) and np.all(w[slots != 700] == 1.0)


def test_weights_are_the_normalised_inverse_probabilities():
    rng = np.random.default_rng(2)
    size = 1500
    pa = rng.uniform(0.01, 2, 2049).astype(np.float32) ** np.float32(0.6)
    slots, total, _ = per.draw(pa, size, 17, 9, 4)
    p = pa[slots].astype(np.float64) / total
    for beta in (0.0, 0.4, 1.0):
        want = (size * p) ** -beta
        assert np.allclose(per.weights(pa, size, slots, total, beta), want / want.max(), rtol=1e-6, atol=0)
    assert not np.array_equal(slots, per.draw(pa, size, 17, 9, 5)[0]), "the sample number does not reach the draw"
    assert np.array_equal(slots, per.draw(pa, size, 17, 9, 4)[0])


def test_the_clamp_on_made_up_sums():
    """A target the scanned sums promise but the walk never reaches: the chunk's last slot below size, and the last chunk when
    no scanned sum exceeds the target."""
    pa = np.full(1500, 0.25, np.float32)
    sc = np.array([256.0, 375.0])                    # the true sums
    assert per.walk(pa, 1500, sc, 255.9) == (1023, False)
    assert per.walk(pa, 1500, sc, 256.0) == (1024, False)
    high = np.array([256.5, 375.5])                  # as if the tree had rounded up: the walk ends at 256 / 375
    assert per.walk(pa, 1500, high, 256.25) == (1023, True)
    assert per.walk(pa, 1500, np.array([256.0, 375.5]), 375.25) == (1499, True)
    assert per.walk(pa, 1500, sc, 400.0) == (1499, True)
    assert per.walk(pa, 1500, sc, 0.0) == (0, False)


def test_chunk_sums_and_scan_are_sums():
    rng = np.random.default_rng(3)
    pa = rng.uniform(0.01, 2, 5000).astype(np.float32)
    for size in (1, 255, 1023, 1024, 1025, 4097, 5000):
        cs = per.chunk_sums(pa, size)
        assert cs.shape == ((size + 1023) // 1024,)
        want = [pa[c * 1024:min(size, (c + 1) * 1024)].astype(np.float64).sum() for c in range(len(cs))]
        assert np.allclose(cs, want, rtol=1e-13, atol=0)
        assert np.allclose(per.scan(cs), np.cumsum(want), rtol=1e-13, atol=0)


def test_update_last_row_wins_and_fill():
    pa = np.array([0.5, 0.5, 0.5, 0.5, 0.0, 0.0], np.float32)
    y = np.array([1.0, 2.0, 3.0, 0.0], np.float32)
    q = np.array([0.0, 0.0, 0.0, 0.0], np.float32)
    top = per.update(pa, 1.0, np.array([2, 0, 2, 3]), y, q, 0.01, 0.6)
    td, p = per.new_priorities(y, q, 0.01, 0.6)
    assert np.array_equal(td, [1.0, 2.0, 3.0, 0.0])
    assert pa[2] == np.float32(p[2]) and pa[0] == np.float32(p[1]) and pa[3] == np.float32(p[3]) and pa[1] == 0.5
    assert top == np.float32(p[2]) and abs(float(p[2]) - 3.01 ** 0.6) < 1e-6
    assert per.update(pa.copy(), 7.0, np.array([1]), y[:1], q[:1], 0.01, 0.6) == np.float32(7.0)      # never decreases
    per.fill(pa, 3.5, 4, 4)                          # rows 4 .. 7 of a ring of 6: slots 4, 5, 0, 1
    assert np.array_equal(pa == 3.5, [True, True, False, False, True, True])


@pytest.mark.parametrize("S,A", [(3, 1), (7, 3)])
def test_weighted_loss_gradient_matches_torch_autograd(S, A):
    """(2/B) w (q - y) and the critic's gradients under it against autograd of mean(w (y - q)^2) with paired shapes."""
    rng = np.random.default_rng(10 + S)
    B = 9
    P = o.random_params(S, A, rng, stats=True)
    s, a = rng.uniform(-1.5, 1.5, (B, S)), rng.uniform(-1, 1, (B, A))
    y, w = rng.uniform(-2, 0, B), rng.uniform(0.05, 1, B)
    tp = _t(P, grad=o.CRITIC_TRAINABLE)
    tq = _critic(tp, torch.tensor(s), torch.tensor(a))[:, 0]
    tq.retain_grad()
    loss = torch.mean(torch.tensor(w) * (torch.tensor(y) - tq) ** 2)
    loss.backward()
    f, dq, g = per.critic_grads(P, s, a, y, w)
    q = f["q"][:, 0]
    assert np.allclose(dq, tq.grad.numpy(), rtol=1e-10, atol=1e-13)
    assert np.allclose(dq, per.weighted_dq(q, y, w), rtol=1e-10, atol=1e-13)
    for k in o.CRITIC_TRAINABLE:
        if k == o.DEAD:
            continue
        want = tp[k].grad.numpy().reshape(g[k].shape)
        assert np.max(np.abs(g[k] - want)) <= 1e-10 * max(1.0, np.max(np.abs(want))), k
    # unit weights: the paired step itself
    _, dq1, _ = per.critic_grads(P, s, a, y, np.ones(B))
    assert np.allclose(dq1, o.critic_grads(P, s, a, y, "paired")[1], rtol=1e-12, atol=1e-15)


def test_weighted_train_step_with_unit_weights_is_the_paired_step():
    rng = np.random.default_rng(21)
    S, A, B = 3, 1, 12
    online, target = o.random_params(S, A, rng), o.random_params(S, A, rng)
    batch = (rng.uniform(-1.5, 1.5, (B, S)), rng.uniform(-1, 1, (B, A)), rng.uniform(-1, 0, B),
             (rng.uniform(size=B) < 0.3).astype(np.float64), rng.uniform(-1.5, 1.5, (B, S)))
    for kw in (dict(), dict(critic_rmsprop=False), dict(clip=40.0)):
        rms = kw.get("critic_rmsprop", True)
        a, b = o.new_state(online, target, rms), o.new_state(online, target, rms)
        o.train_step(a, *batch, 3e-4, None, form="paired", **kw)
        per.train_step(b, *batch, np.ones(B), 3e-4, None, **kw)
        for k in o.TRAINABLE:
            for part in ("online", "target", "slot_a", "slot_b"):
                assert np.allclose(a[part][k], b[part][k], rtol=1e-12, atol=1e-14), (part, k)
        assert a["step"] == b["step"] == 1


# ---- Config rules

@pytest.fixture
def per_config(monkeypatch):
    import ga3c_amd  # noqa: F401
    from Config import Config
    for k, v in (("GAME", "Pendulum-v0"), ("USE_DDPG", True), ("CONTINUOUS_INPUT", True), ("DISCRATE_INPUT", False),
                 ("TRAINING_MIN_BATCH_SIZE", 64), ("USE_REPLAY_MEMORY", False), ("DISCOUNTING", True),
                 ("PRIORITIZED_REPLAY", True), ("DDPG_CRITIC_LOSS", "paired")):
        monkeypatch.setattr(Config, k, v)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    return Config


def test_config_defaults_and_the_accepted_setting(per_config):
    from Config import Config, resolve_ddpg
    keys = {k for k in vars(Config) if k.startswith("PRIORITIZED_REPLAY")}
    assert keys == {"PRIORITIZED_REPLAY", "PRIORITIZED_REPLAY_ALPHA", "PRIORITIZED_REPLAY_BETA_START",
                          "PRIORITIZED_REPLAY_BETA_END", "PRIORITIZED_REPLAY_EPS"}
    assert (Config.PRIORITIZED_REPLAY_ALPHA, Config.PRIORITIZED_REPLAY_BETA_START, Config.PRIORITIZED_REPLAY_BETA_END,
            Config.PRIORITIZED_REPLAY_EPS) == (0.6, 0.4, 1.0, 0.01)
    resolve_ddpg()
    assert Config.USE_REPLAY_MEMORY and not Config.DISCOUNTING


def test_the_key_is_off_by_default():
    import ga3c_amd  # noqa: F401
    from Config import Config, resolve_ddpg
    assert Config.PRIORITIZED_REPLAY is False          # (the tests that switch it on do so through monkeypatch)
    before = dict(vars(Config))
    resolve_ddpg()
    assert dict(vars(Config)) == before


@pytest.mark.parametrize("key,value,match", [("USE_DDPG", False, "USE_DDPG"), ("DDPG_CRITIC_LOSS", "fork", "paired"),
                                             ("REPLAY_BUFFER_SIZE", 1048577, "1048576"),
                                             ("PRIORITIZED_REPLAY_ALPHA", 1.5, "ALPHA"), ("PRIORITIZED_REPLAY_EPS", 0.0, "EPS"),
                                             ("PRIORITIZED_REPLAY_BETA_START", -0.1, "BETA")])
def test_config_refusals(per_config, monkeypatch, key, value, match):
    from Config import resolve_ddpg
    monkeypatch.setattr(per_config, key, value)
    with pytest.raises(ValueError, match=match):
        resolve_ddpg()


def test_the_largest_ring_is_accepted(per_config, monkeypatch):
    from Config import resolve_ddpg
    monkeypatch.setattr(per_config, "REPLAY_BUFFER_SIZE", 1048576)
    resolve_ddpg()


def test_argv_sets_the_keys(per_config, monkeypatch):
    import GA3C
    monkeypatch.setattr(per_config, "PRIORITIZED_REPLAY", False)
    monkeypatch.setattr(per_config, "DDPG_CRITIC_LOSS", "fork")
    monkeypatch.setattr(per_config, "PRIORITIZED_REPLAY_ALPHA", 0.6)      # (apply_argv assigns it: restored afterwards)
    with pytest.raises(ValueError, match="paired"):
        GA3C.apply_argv(["GAME=Pendulum-v0", "USE_DDPG=True", "PRIORITIZED_REPLAY=True", "TRAINING_MIN_BATCH_SIZE=64"])
    GA3C.apply_argv(["GAME=Pendulum-v0", "USE_DDPG=True", "PRIORITIZED_REPLAY=True", "DDPG_CRITIC_LOSS=paired",
                     "TRAINING_MIN_BATCH_SIZE=64", "PRIORITIZED_REPLAY_ALPHA=0.5"])
    assert per_config.PRIORITIZED_REPLAY is True and per_config.PRIORITIZED_REPLAY_ALPHA == 0.5


# ---- the replay thread and the trainer path

class _CountingModel:
    def __init__(self, capacity):
        self.replay_capacity, self.total = capacity, 0

    def replay_add(self, s, a, r, done, s2):
        self.total += len(s)
        return min(self.total, self.replay_capacity), self.total


def test_replay_thread_queues_the_token_under_the_same_rules_and_draws_nothing(per_config, monkeypatch):
    import ThreadReplay as tr
    monkeypatch.setattr(per_config, "TRAINING_MIN_BATCH_SIZE", 12)
    monkeypatch.setattr(per_config, "REPLAY_MIN_QUEUE_SIZE", 2)
    srv = _Server(_CountingModel(100))
    th = tr.ThreadReplay(srv, _Transport(30, 6))
    th._run()
    # sizes at the sampling points: 0, 6, 12 (not MORE than 12: nothing), 18 (first token), 24 (second; then the queue holds 2)
    assert srv.replay_q.qsize() == 2 and th.batches == 2
    assert [srv.replay_q.get() for _ in range(2)] == [(None, 18), (None, 24)]
    assert th.random.getstate() == random.Random(per_config.REPLAY_BUFFER_RANDOM_SEED).getstate()
    # the uniform path on the same input does advance it
    monkeypatch.setattr(per_config, "PRIORITIZED_REPLAY", False)
    srv = _Server(_CountingModel(100))
    th = tr.ThreadReplay(srv, _Transport(30, 6))
    th._run()
    slots, stamp = srv.replay_q.get()
    assert slots.shape == (12,) and stamp == 18
    assert th.random.getstate() != random.Random(per_config.REPLAY_BUFFER_RANDOM_SEED).getstate()


def test_train_model_replay_lets_the_model_draw(per_config, monkeypatch):
    from Server import Server
    monkeypatch.setattr(per_config, "TRAINING_MIN_BATCH_SIZE", 48)
    calls = []

    class M:
        def train_prioritized(self, batch):
            calls.append(("prioritized", batch))

        def train_replay(self, slots, stamp):
            calls.append(("replay", len(slots), stamp))
    srv = Server.__new__(Server)
    srv.model, srv.lost_train_batches = M(), 0
    srv._count_train_step = lambda rows, *a, **k: calls.append(("counted", rows))
    srv.train_model_replay(None, 100, 0)
    srv.train_model_replay(np.arange(48, dtype=np.int32), 100, 0)
    assert calls == [("prioritized", 48), ("counted", 48), ("replay", 48, 100), ("counted", 48)] and srv.lost_train_batches == 0


class _PrioritizedStandIn:
    """Keeps count of what the replay thread adds and of the steps it is asked for; trains on nothing."""
    replay_capacity = 5000

    def __init__(self):
        self.total, self.betas, self.lock = 0, [], threading.Lock()
        self.learning_rate = self.beta = 0.0
        self.replay_beta = None

    def predict_p_and_v(self, x):
        a = np.tanh(x[:, :1] * 0.5).astype(np.float32)
        return a, a

    def replay_add(self, s, a, r, done, s2):
        with self.lock:
            self.total += len(r)
        return min(self.total, self.replay_capacity), self.total

    def train_prioritized(self, batch):
        assert batch == 16 and self.total > 16
        self.betas.append(self.replay_beta)

    def train_replay(self, slots, stamp):
        raise AssertionError("a host-drawn batch under PRIORITIZED_REPLAY")

    def save(self, episode):
        pass

    def log(self, *a, **k):
        pass


@pytest.mark.timeout(120)
def test_server_reaches_train_prioritized_with_an_annealed_beta(tmp_path, monkeypatch, per_config):
    from Config import Config
    monkeypatch.chdir(tmp_path)
    for k, v in (("AGENTS", 3), ("PREDICTORS", 1), ("TRAINERS", 1), ("TIME_MAX", 5), ("DYNAMIC_SETTINGS", False),
                 ("SAVE_MODELS", False), ("TRAINING_MIN_BATCH_SIZE", 16), ("CONTINUOUS_INPUT", False),
                 ("DISCRATE_INPUT", True), ("CPU_AFFINITY", "off"), ("ANNEALING_EPISODE_COUNT", 4),
                 ("PRIORITIZED_REPLAY_BETA_START", 0.25), ("PRIORITIZED_REPLAY_BETA_END", 0.75)):
        monkeypatch.setattr(Config, k, v)
    from Server import Server
    model = _PrioritizedStandIn()
    srv = Server(model=model, max_agents=8)
    assert srv.ddpg and Config.PRIORITIZED_REPLAY
    srv.main(max_seconds=8)
    assert len(model.betas) > 0 and srv.training_step == len(model.betas) and srv.lost_train_batches == 0
    # START + (END - START) / ANNEALING_EPISODE_COUNT * min(episodes, ANNEALING_EPISODE_COUNT - 1), as learning_rate
    allowed = [0.25 + 0.125 * step for step in range(4)]
    assert all(any(abs(b - a) < 1e-12 for a in allowed) for b in model.betas), sorted(set(model.betas))
    assert model.betas[0] == 0.25 and any(abs(model.replay_beta - a) < 1e-12 for a in allowed)


# ---- the C ABI

def test_new_entries_are_declared_bound_and_exported():
    import ctypes as C
    import ga3c_amd  # noqa: F401
    import _native as nat
    text = open(os.path.join(ROOT, "include", "ga3c_abi.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = nat.hip_lib()
    for name in ENTRIES:
        assert re.search(r"\bint %s\s*\(ga3c_ddpg\* net\b" % name, text), name
        assert name in nat.HIP_SIGNATURES and hasattr(lib, name), name
        res, args = nat.HIP_SIGNATURES[name]
        assert res is C.c_int and args[0] is C.c_void_p
        declared = re.search(r"\bint %s\s*\((.*?)\);" % name, text, flags=re.S).group(1)
        assert len(args) == declared.count(",") + 1, name
    sig = nat.HIP_SIGNATURES
    assert sig["ga3c_ddpg_priorities_create"][1][1:] == [C.c_float, C.c_float, C.c_int64]
    assert sig["ga3c_ddpg_train_prioritized"][1][1:] == [C.c_int32, C.c_float, C.c_float, C.c_int32, nat.f32p, nat.f32p, nat.i32p]
    assert sig["ga3c_ddpg_sample_prioritized"][1][1:] == [C.c_int32, C.c_float, nat.i32p, nat.f32p]
    # no new flag and no new field: prioritised replay is attached by its own call
    assert C.sizeof(nat.DdpgConfig) == 80 and "GA3C_DDPG_PRIORIT" not in text
    flags = re.findall(r"#define (GA3C_DDPG_[A-Z_]+) (\d+)u", text)
    assert sorted(int(v) for _, v in flags) == [1, 2, 4, 8, 16]
