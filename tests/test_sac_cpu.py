"""The soft actor-critic step's statement (tests/sac_oracle.py) without a GPU: against torch autograd in f64, its
log-density against torch.distributions and at saturation, its draws, the Config rules of DDPG_SOFT, the shapes, the ABI, and
the choice of rows of every case of tests/test_gpu_sac.py (tests/sac_cases.py)."""
import math

import numpy as np
import pytest
import torch

import ddpg_oracle as o
import sac_cases as sc
import sac_oracle as so
import td3_oracle as t3
from test_ddpg_cpu import _batch, _bn, _close, _critic, _t, ddpg_config  # noqa: F401

SHAPES = [(3, 1), (7, 3)]
LR = 3e-4


def _params(S, A, rng):
    return so.random_params(S, A, rng, stats=True), so.random_params(S, A, rng, stats=True)


def _raw(P, x):
    a1 = torch.relu(_bn(P, "actor_norm1", x @ P["actor_fc1/W"] + P["actor_fc1/b"]))
    a2 = torch.relu(_bn(P, "actor_norm2", a1 @ P["actor_fc2/W"] + P["actor_fc2/b"]))
    return a2 @ P["actor_output/W"] + P["actor_output/b"]


def _torch_sample(P, x, eps, ls_min, ls_max):
    """-> (a, logp) by torch: a TransformedDistribution's log_prob where it is finite is test_logp's business; here the plain
    formula with torch's clamp, whose gradient is zero outside the interval."""
    raw = _raw(P, x)
    A = raw.shape[1] // 2
    mu, ls = raw[:, :A], torch.clamp(raw[:, A:], ls_min, ls_max)
    u = mu + torch.exp(ls) * eps
    a = torch.tanh(u)
    logp = (-0.5 * eps * eps - ls - 0.5 * math.log(2 * math.pi) - 2.0 * (math.log(2.0) - u - torch.nn.functional.softplus(-2.0 * u))).sum(1)
    return a, logp


@pytest.mark.parametrize("S,A", SHAPES)
def test_oracle_step_matches_torch_autograd(S, A):
    rng = np.random.default_rng(10 + S + A)
    B, seed, step, ent = 12, 77, 3, -float(A)
    online, target = _params(S, A, rng)
    s, a, r, done, s2 = _batch(S, A, B, rng)
    # a clamp that bites on both sides (asserted below): bounds inside the spread of the head's raw ls on these rows
    ls_min, ls_max = (float(v) for v in np.quantile(so.head(online, s, -1e9, 1e9)["raw"][:, A:], [0.3, 0.7]))
    st = so.new_state(online, target)
    st["step"] = step
    eps2, eps = so.step_draws(seed, step + 1, B, A)
    out = so.train_step(st, s, a, r, done, s2, LR, policy_delay=2, seed=seed, ls_min=ls_min, ls_max=ls_max, stop_after=4)
    assert out["policy"] and np.array_equal(out["eps2"], eps2) and np.array_equal(out["eps"], eps)
    ts, ta, tr, td, ts2 = (torch.tensor(v, dtype=torch.float64) for v in (s, a, r, done, s2))
    te2, te = torch.tensor(eps2, dtype=torch.float64), torch.tensor(eps, dtype=torch.float64)
    alpha = float(np.exp(online[so.LOG_ALPHA][0]))
    # y: the online actor's sample at s2, the target critics' min, the entropy term
    O0, T = _t(online), _t(target)
    a2, logp2 = _torch_sample(O0, ts2, te2, ls_min, ls_max)
    qt = torch.minimum(_critic(T, ts2, a2)[:, 0], _critic(_t(t3.critic2(target)), ts2, a2)[:, 0])
    y = torch.where(td != 0, tr, tr + 0.99 * (qt - alpha * logp2))
    assert _close(out["y"], y.numpy()) and _close(out["qt"], qt.numpy()) and _close(out["logp2"], logp2.numpy())
    assert _close(out["a2"], a2.numpy()) and _close(out["vt"], (qt - alpha * logp2).numpy())
    # the policy step against the critics as the oracle's step 2 left them
    P = _t(st["online"], grad=o.ACTOR_TRAINABLE + (so.LOG_ALPHA,))
    pa, logp = _torch_sample(P, ts, te, ls_min, ls_max)
    q1, q2 = _critic(P, ts, pa)[:, 0], _critic(_t(t3.critic2(st["online"])), ts, pa)[:, 0]
    assert bool((q1 < q2).any()) and bool((q2 < q1).any()), "rows on both sides of the selection"
    J = (alpha * logp - torch.minimum(q1, q2)).mean()
    J.backward()
    for k in o.ACTOR_TRAINABLE:
        assert _close(out["actor_grads"][k].reshape(P[k].shape), P[k].grad.numpy(), 1e-9), k
    assert _close(out["fwd"]["logp"], logp.detach().numpy()) and _close(out["pq1"], q1.detach().numpy()) and _close(out["pq2"], q2.detach().numpy())
    assert abs(out["J"] - float(J.detach())) < 1e-9
    # dJ/dlog_alpha of the temperature's own loss, logp detached
    la = P[so.LOG_ALPHA]
    la.grad = None
    (-la[0] * (logp.detach().mean() + ent)).backward()
    assert abs(float(la.grad[0]) - out["dlog_alpha"]) < 1e-12
    # the clamp: raw ls outside the open interval on some rows and inside on others; no gradient reaches the former
    inside = out["fwd"]["inside"]
    assert inside.any() and (~inside).any()
    assert not out["do"][:, A:][~inside].any() and out["do"][:, A:][inside].all()
    assert np.array_equal(out["sel"], (q2 < q1).numpy())


def test_logp():
    rng = np.random.default_rng(5)
    B, A = 9, 3
    mu, ls, eps = rng.normal(size=(B, A)), rng.uniform(-2, 1, (B, A)), rng.normal(size=(B, A))
    u = mu + np.exp(ls) * eps
    base = torch.distributions.Normal(torch.tensor(mu), torch.tensor(np.exp(ls)))
    dist = torch.distributions.TransformedDistribution(base, [torch.distributions.transforms.TanhTransform(cache_size=1)])
    a = torch.tanh(torch.tensor(u))
    want = (base.log_prob(torch.tensor(u)) - torch.log1p(-a * a)).sum(1).numpy()            # moderate u: the naive form is fine
    assert _close(so.logp_of(eps, ls, u), want, 1e-10)
    assert _close(so.logp_of(eps, ls, u), dist.log_prob(a).sum(1).numpy(), 1e-6)
    # |u| = 12: tanh is 1 - 7.5e-11 in f64 and exactly 1 in f32; the closed form is ln(4) - 2 |u| up to exp(-4 |u|)
    for u12 in (12.0, -12.0):
        assert abs(float(so.log1mtanh2(np.array(u12))) - (math.log(4.0) - 24.0)) < 1e-9
        got32 = so.log1mtanh2(np.array(u12, np.float32))
        assert got32.dtype == np.float32 and np.isfinite(got32) and abs(float(got32) - (math.log(4.0) - 24.0)) < 1e-5
        assert np.tanh(np.float32(u12)) in (np.float32(1.0), np.float32(-1.0)), "the naive form would give -inf"
    # ls on and beyond both clamps: the clamped value enters, and the flag says where a gradient passes
    S = 3
    P = so.random_params(S, 4, rng)
    P["actor_output/W"][:, 4:] = 0.0
    P["actor_output/b"][4:] = [2.0, 7.0, -20.0, -33.0]
    f = so.sample(P, rng.normal(size=(5, S)), rng.normal(size=(5, 4)))
    assert np.array_equal(f["ls"], np.tile([2.0, 2.0, -20.0, -20.0], (5, 1))) and not f["inside"].any()
    assert np.all(np.isfinite(f["logp"]))
    P["actor_output/b"][4:] = [1.999, -19.999, 0.0, 0.0]
    assert so.sample(P, rng.normal(size=(5, S)), rng.normal(size=(5, 4)))["inside"].all()


def test_draws_are_reproducible_and_the_streams_distinct():
    B, A, seed, t = 33, 3, 12348, 7
    e2, e1 = so.step_draws(seed, t, B, A)
    again2, again1 = so.step_draws(seed, t, B, A)
    assert e2.dtype == np.float32 and e2.shape == (B, A) and np.array_equal(e2, again2) and np.array_equal(e1, again1)
    p0, p1 = so.predict_draws(seed, 0, B, A), so.predict_draws(seed, 1, B, A)
    flat = [v.reshape(-1) for v in (e2, e1, p0, p1)]
    for i in range(4):
        for j in range(i + 1, 4):
            assert not np.array_equal(flat[i], flat[j]) and abs(float(np.corrcoef(flat[i], flat[j])[0, 1])) < 0.35
    # numpy's restatement: j = k A + i on stream 2 t / 2 t + 1; row r, draw c A + i on stream r of seed + 1
    import device_agents_oracle as da
    k, i = 5, 2
    j = np.uint64(k * A + i)
    for stream, e in ((2 * t, e2), (2 * t + 1, e1)):
        n = np.sqrt(-2.0 * np.log(1.0 - da.uniform(seed, stream, 2 * j))) * np.cos(2.0 * np.pi * da.uniform(seed, stream, 2 * j + 1))
        assert e[k, i] == np.float32(n)
    j = np.uint64(1 * A + i)
    n = np.sqrt(-2.0 * np.log(1.0 - da.uniform(seed + 1, k, 2 * j))) * np.cos(2.0 * np.pi * da.uniform(seed + 1, k, 2 * j + 1))
    assert p1[k, i] == np.float32(n)
    assert not np.array_equal(e2, so.step_draws(seed, t + 1, B, A)[0])
    draws = np.concatenate([so.step_draws(seed, k, 4096, 1)[0].reshape(-1) for k in range(1, 9)]).astype(np.float64)
    assert abs(draws.mean()) < 0.02 and abs(draws.var() - 1.0) < 0.03 and np.abs(draws).max() > 3.5, "unclipped"
    # a step at count `step` draws streams 2 (step + 1) and 2 (step + 1) + 1
    rng = np.random.default_rng(0)
    online, target = _params(3, 1, rng)
    st = so.new_state(online, target)
    st["step"] = 6
    out = so.train_step(st, *_batch(3, 1, 5, rng), LR, policy_delay=1, seed=seed, stop_after=4)
    w2, w1 = so.step_draws(seed, 7, 5, 1)
    assert np.array_equal(out["eps2"], w2) and np.array_equal(out["eps"], w1)


def test_delayed_policy_step_and_fixed_temperature():
    S, A, B = 3, 1, 8
    rng = np.random.default_rng(3)
    online, target = _params(S, A, rng)
    for alpha_lr in (1.0, 0.0):
        st = so.new_state(online, target)
        for step in range(1, 5):
            before = {(w, k): st[w][k].copy() for w in ("online", "slot_a", "slot_b") for k in o.ACTOR_TRAINABLE + (so.LOG_ALPHA,)}
            before.update({("target", k): st["target"][k].copy() for k in so.ALL_VARS})
            out = so.train_step(st, *_batch(S, A, B, rng), LR, policy_delay=2, seed=5, alpha_lr=alpha_lr)
            same = all(np.array_equal(v, st[w][k]) for (w, k), v in before.items())
            assert out["policy"] == (step % 2 == 0) and same == (step % 2 == 1)
            assert np.array_equal(st["target"][so.LOG_ALPHA], target[so.LOG_ALPHA])
        moved = not np.array_equal(st["online"][so.LOG_ALPHA], online[so.LOG_ALPHA])
        assert moved == (alpha_lr > 0)


def test_soft_defaults_and_rules(ddpg_config, monkeypatch):  # noqa: F811
    from Config import resolve_ddpg, _resolve_device_ddpg
    c = ddpg_config
    assert (c.DDPG_SOFT, c.DDPG_SOFT_ALPHA, c.DDPG_SOFT_ALPHA_LR, c.DDPG_SOFT_TARGET_ENTROPY, c.DDPG_SOFT_LOG_STD_MIN,
            c.DDPG_SOFT_LOG_STD_MAX) == (False, 0.2, 1.0, None, -20.0, 2.0)
    monkeypatch.setattr(c, "DDPG_SOFT", True)
    with pytest.raises(ValueError, match="DDPG_TWIN"):
        resolve_ddpg()
    monkeypatch.setattr(c, "DDPG_TWIN", True)
    monkeypatch.setattr(c, "DDPG_CRITIC_LOSS", "paired")
    resolve_ddpg()
    resolve_ddpg(num_actions=16)
    with pytest.raises(ValueError, match="num_actions=17"):
        resolve_ddpg(num_actions=17)
    for key, bad in (("DDPG_SOFT_ALPHA", 0.0), ("DDPG_SOFT_ALPHA", -1.0), ("DDPG_SOFT_ALPHA", float("nan")),
                     ("DDPG_SOFT_ALPHA", float("inf")), ("DDPG_SOFT_ALPHA_LR", -0.5), ("DDPG_SOFT_ALPHA_LR", float("nan")),
                     ("DDPG_SOFT_TARGET_ENTROPY", float("inf")), ("DDPG_SOFT_TARGET_ENTROPY", "x"),
                     ("DDPG_SOFT_LOG_STD_MIN", 2.0), ("DDPG_SOFT_LOG_STD_MIN", float("nan")), ("DDPG_SOFT_LOG_STD_MAX", -20.0),
                     ("DDPG_SOFT_LOG_STD_MAX", float("inf"))):
        good = getattr(c, key)
        monkeypatch.setattr(c, key, bad)
        with pytest.raises(ValueError, match=key[:17]):
            resolve_ddpg()
        monkeypatch.setattr(c, key, good)
    for key, fine in (("DDPG_SOFT_ALPHA_LR", 0.0), ("DDPG_SOFT_TARGET_ENTROPY", -3.5), ("DDPG_SOFT_TARGET_ENTROPY", None)):
        monkeypatch.setattr(c, key, fine)
        resolve_ddpg()
    # the device actors: the policy's own sampling is already per environment
    for k, v in (("DEVICE_DDPG", True), ("DEVICE_AGENTS", 8), ("DYNAMIC_SETTINGS", False), ("PLAY_MODE", False),
                 ("REPLAY_BUFFER_SIZE", 4096)):
        monkeypatch.setattr(c, k, v)
    _resolve_device_ddpg(8, False)
    monkeypatch.setattr(c, "DEVICE_DDPG_NOISE", "per_env")
    with pytest.raises(ValueError, match="DDPG_SOFT"):
        _resolve_device_ddpg(8, False)
    monkeypatch.setattr(c, "DEVICE_DDPG_NOISE", "shared")
    monkeypatch.setattr(c, "USE_DDPG", False)
    with pytest.raises(ValueError, match="USE_DDPG"):
        resolve_ddpg()


def test_argv_sets_the_soft_keys(ddpg_config, monkeypatch):  # noqa: F811
    import GA3C
    monkeypatch.setattr(ddpg_config, "USE_DDPG", False)
    for k in ("DDPG_TWIN", "DDPG_CRITIC_LOSS", "DDPG_SOFT", "DDPG_SOFT_TARGET_ENTROPY", "DDPG_SOFT_ALPHA"):
        monkeypatch.setattr(ddpg_config, k, getattr(ddpg_config, k))          # restored afterwards
    base = ["GAME=Pendulum-v0", "USE_DDPG=True", "TRAINING_MIN_BATCH_SIZE=64", "DDPG_CRITIC_LOSS=paired"]
    GA3C.apply_argv(base + ["DDPG_TWIN=True", "DDPG_SOFT=True", "DDPG_SOFT_TARGET_ENTROPY=-2.5", "DDPG_SOFT_ALPHA=0.1"])
    assert ddpg_config.DDPG_SOFT is True and ddpg_config.DDPG_SOFT_TARGET_ENTROPY == -2.5 and ddpg_config.DDPG_SOFT_ALPHA == 0.1
    monkeypatch.setattr(ddpg_config, "DDPG_TWIN", False)
    with pytest.raises(ValueError, match="DDPG_TWIN"):
        GA3C.apply_argv(base + ["DDPG_SOFT=True"])


def test_param_shapes_and_initial_arena():
    import ga3c_amd  # noqa: F401
    import NetworkDDPG as nd
    assert nd.SOFT_LOG_ALPHA == so.LOG_ALPHA
    for S, A in SHAPES + [(3, 16)]:
        shapes = nd.param_shapes(S, A, twin=True, soft=True)
        assert all(shapes[k] == so.shapes(S, A)[k] for k in shapes)
        assert shapes["actor_output/W"] == (300, 2 * A) and shapes["actor_output/b"] == (2 * A,) and shapes[so.LOG_ALPHA] == (1,)
        plain = nd.param_shapes(S, A, twin=True)
        assert plain["actor_output/W"] == (300, A) and so.LOG_ALPHA not in plain
        assert all(shapes[k] == plain[k] for k in plain if not k.startswith("actor_output"))
        online, target = nd.initial_arena(S, A, 12345, tau=0.001, twin=True, soft=True)
        assert online["actor_output/W"].shape == (300, 2 * A) and np.max(np.abs(online["actor_output/W"])) <= 0.003
        assert not online["actor_output/b"].any() and online["actor_output/b"].shape == (2 * A,) and so.LOG_ALPHA not in online
        assert set(online) == set(nd.TRAINABLE + nd.TWIN_TRAINABLE)
    assert len(so.ALL_VARS) == 39 and so.ALL_VARS[:38] == t3.ALL_VARS and set(so.shapes(3, 1)) == set(so.ALL_VARS)


def test_soft_abi_is_declared_and_bound():
    import os
    import re
    import ga3c_amd  # noqa: F401
    import _native as nat
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "ga3c_abi.h")).read(), flags=re.S)
    for name in ("ga3c_ddpg_soft_create", "ga3c_ddpg_soft_destroy", "ga3c_ddpg_soft_info"):
        assert re.search(r"\b%s\s*\(" % name, text) and name in nat.HIP_SIGNATURES and hasattr(nat.hip_lib(), name)


# ---- the choice of rows of every GPU case: the cap of 4 B candidates holds for the oracle alone

@pytest.mark.parametrize("S,A,B", sc.EVERY_ROW)
def test_every_row_cases_find_their_rows(S, A, B):
    _, _, batch, tried = sc.every_row_case(S, A, B)
    assert batch[0].shape == (B, S) and batch[1].shape == (B, A) and B <= tried <= 4 * B


@pytest.mark.parametrize("way,delay", sc.STEP_CASES)
def test_step_cases_find_their_rows(way, delay):
    S, A = sc.STEPS_SHAPE
    _, _, st, rng = sc.steps_case(way, delay)
    kw = sc.steps_kw(way)
    for _ in range(sc.STEPS):
        b, tried = sc.select(st, sc.candidates(S, A, 4 * sc.STEPS_B, rng), sc.STEPS_B, delay, **kw)
        assert b[0].shape == (sc.STEPS_B, S) and tried <= 4 * sc.STEPS_B
        so.train_step(st, *sc.f64(b), sc.LR, policy_delay=delay, seed=sc.SOFT_SEED, **kw)
    assert st["step"] == sc.STEPS


def test_saturation_and_selection_cases_find_their_rows():
    online, _, batch, tried = sc.saturation_case()
    f = so.sample(online, np.asarray(batch[0], np.float64), so.step_draws(sc.SOFT_SEED, 1, 17, 5)[1])
    assert np.array_equal(f["raw"][:, 5:], np.tile(sc.SATURATION_LS, (17, 1))), "the raw ls are the bias exactly"
    assert np.array_equal(f["inside"][0], [False, False, False, False, True]) and np.abs(f["mu"][:, :4]).min() > 8.5
    assert tried <= 68
    for shift, want in ((10.0, False), (-10.0, True)):
        online, target, batch, tried = sc.selection_case(shift)
        st = so.new_state(online, target)
        out = so.train_step(st, *sc.f64(batch), sc.ROWS_LR, policy_delay=1, seed=sc.SOFT_SEED, stop_after=4)
        assert np.all(out["sel"] == want) and tried <= 68
