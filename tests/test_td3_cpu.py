"""The twin step's statement (tests/td3_oracle.py) without a GPU: against torch autograd in f64, its delayed
policy update, its reduction to ddpg_oracle's step, its smoothing draw, and the Config and initial-value rules of DDPG_TWIN."""
import numpy as np
import pytest
import torch

import ddpg_oracle as o
import device_agents_oracle as da
import td3_oracle as t3
from test_ddpg_cpu import _actor, _batch, _close, _critic, _t, ddpg_config  # noqa: F401

SHAPES = [(3, 1), (7, 3)]
LR = 3e-4


def _params(S, A, rng):
    return t3.random_params(S, A, rng, stats=True), t3.random_params(S, A, rng, stats=True)


@pytest.mark.parametrize("S,A", SHAPES)
def test_oracle_step_matches_torch_autograd(S, A):
    rng = np.random.default_rng(S + A)            # rows on both sides of the min and of both clips (asserted below)
    B = 12
    online, target = _params(S, A, rng)
    s, a, r, done, s2 = _batch(S, A, B, rng)
    sigma, c, seed, step = 1.0, 0.3, 77, 4
    eps = t3.smoothing_noise(seed, step + 1, B, A, sigma, c)
    # rows on both branches of each clip: the noise clip ...
    assert (np.abs(eps) == np.float32(c)).any() and (np.abs(eps) < np.float32(c)).any()
    ts, ta, tr, td, ts2 = (torch.tensor(v, dtype=torch.float64) for v in (s, a, r, done, s2))
    T = _t(target)
    raw = _actor(T, ts2) + torch.tensor(eps, dtype=torch.float64)
    # ... and the action clip (the target actor of U(-0.3, 0.3) weights saturates on some rows, not on all)
    assert bool((raw.abs() > 1).any()) and bool((raw.abs() < 1).any())
    at = torch.clamp(raw, -1.0, 1.0)
    T2 = _t(t3.critic2(target))
    qt1, qt2 = _critic(T, ts2, at)[:, 0], _critic(T2, ts2, at)[:, 0]
    y = torch.where(td != 0, tr, tr + 0.99 * torch.minimum(qt1, qt2)).detach()
    st = t3.new_state(online, target)
    st["step"] = step
    out = t3.train_step(st, s, a, r, done, s2, LR, None, policy_delay=2, sigma=sigma, noise_clip=c, seed=seed, stop_after=3)
    assert _close(out["y"], y.numpy()) and _close(out["qt1"], qt1.numpy()) and _close(out["qt2"], qt2.numpy())
    assert _close(out["t_a"], at.numpy()) and np.array_equal(out["t_eps"], eps)
    assert (qt1 < qt2).any() and (qt2 < qt1).any()
    # the loss: both critics on the same detached y
    P1, P2 = _t(online, grad=o.CRITIC_TRAINABLE), _t(t3.critic2(online), grad=o.CRITIC_TRAINABLE)
    q1, q2 = _critic(P1, ts, ta)[:, 0], _critic(P2, ts, ta)[:, 0]
    loss = ((q1 - y) ** 2).mean() + ((q2 - y) ** 2).mean()
    loss.backward()
    for P, g in ((P1, out["critic_grads"]), (P2, out["critic2_grads"])):
        for k in o.CRITIC_TRAINABLE:
            if k == o.DEAD:
                assert P[k].grad is None and not g[k].any()
            else:
                assert _close(g[k].reshape(P[k].shape), P[k].grad.numpy()), k
    assert _close(out["q"], q1.detach().numpy()) and _close(out["q2"], q2.detach().numpy())


def _snap(st, names, what=("target",)):
    return {(w, k): st[w][k].copy() for w in what for k in names}


def test_delayed_policy_update_leaves_targets_and_actor_slots_alone():
    S, A, B = 3, 1, 8
    rng = np.random.default_rng(3)
    online, target = _params(S, A, rng)
    st = t3.new_state(online, target)
    counts = []
    real = o.adam_step

    def counting(theta, m, v, g, lr, t):
        counts.append(t)
        return real(theta, m, v, g, lr, t)

    o.adam_step = counting
    try:
        for step in range(1, 5):
            before_t = _snap(st, t3.TRAINABLE)
            before_a = _snap(st, o.ACTOR_TRAINABLE, ("online", "slot_a", "slot_b"))
            before_c = _snap(st, o.CRITIC_TRAINABLE + t3.CRITIC2_TRAINABLE, ("online",))
            counts.clear()
            out = t3.train_step(st, *_batch(S, A, B, rng), LR, np.full(A, 0.05), policy_delay=2, seed=5)
            assert st["step"] == step and out["policy"] == (step % 2 == 0)
            same_t = all(np.array_equal(v, st[w][k]) for (w, k), v in before_t.items())
            same_a = all(np.array_equal(v, st[w][k]) for (w, k), v in before_a.items())
            if step % 2:
                assert same_t and same_a and not counts, "step %d is not a policy step" % step
            else:
                assert not same_t and not same_a
                assert set(counts) == {step // 2}, "the actor's Adam count"       # 1 then 2 (the critics are RMSProp's)
            moved = [k for (w, k), v in before_c.items() if not np.array_equal(v, st[w][k])]
            assert len(moved) == 18, "both critics step on every call, their dead variables never"
    finally:
        o.adam_step = real


@pytest.mark.parametrize("S,A", SHAPES)
@pytest.mark.parametrize("cfg", [dict(), dict(critic_rmsprop=False), dict(clip=0.5, momentum=0.9)], ids=["rmsprop", "adam", "clip"])
def test_delay_one_without_noise_and_equal_critics_is_ddpg(S, A, cfg):
    rng = np.random.default_rng(20 + S)
    online, target = o.random_params(S, A, rng, stats=True), o.random_params(S, A, rng, stats=True)
    both = []
    for P in (online, target):
        Q = dict(P)
        Q.update({"critic2_" + k[7:]: P[k].copy() for k in P if k.startswith("critic_")})
        both.append(Q)
    ref = o.new_state(online, target, critic_rmsprop=cfg.get("critic_rmsprop", True))
    st = t3.new_state(*both, critic_rmsprop=cfg.get("critic_rmsprop", True))
    for _ in range(3):
        batch = _batch(S, A, 8, rng)
        noise = rng.normal(size=A) * 0.1
        want = o.train_step(ref, *batch, LR, noise, form="paired", **cfg)
        got = t3.train_step(st, *batch, LR, noise, policy_delay=1, sigma=0.0, **cfg)
        assert not got["t_eps"].any() and _close(got["y"], want["y"], 1e-12)
    assert st["step"] == ref["step"] == 3
    for k in o.ALL_VARS:
        for w in ("online", "target") + (("slot_a", "slot_b") if k in o.TRAINABLE else ()):
            assert _close(st[w][k], ref[w][k], 1e-12), (w, k)
    for k in o.CRITIC_TRAINABLE:                              # same code, same data
        assert np.array_equal(st["online"]["critic2_" + k[7:]], st["online"][k])


def test_smoothing_draw():
    B, A, seed, sigma, c = 33, 3, 12345, 0.2, 0.5
    t = 7
    j = np.arange(B * A)
    u1 = 1.0 - da.uniform(seed, t, 2 * j)
    u2 = da.uniform(seed, t, 2 * j + 1)
    n = np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)
    assert np.all(u1 > 0.0) and np.all(np.isfinite(n))
    want = np.clip(np.float64(np.float32(sigma)) * n, -np.float64(np.float32(c)), np.float64(np.float32(c))).astype(np.float32)
    eps = t3.smoothing_noise(seed, t, B, A, sigma, c)
    assert eps.dtype == np.float32 and eps.shape == (B, A) and np.array_equal(eps.reshape(-1), want)
    assert eps[2, 1] == want[2 * A + 1]                                   # j = k A + i
    assert np.all(np.abs(eps) <= np.float32(c))
    big = t3.smoothing_noise(seed, t, B, A, 1.0, 0.3)
    assert np.all(np.abs(big) <= np.float32(0.3)) and (np.abs(big) == np.float32(0.3)).mean() > 0.5
    assert not t3.smoothing_noise(seed, t, B, A, 0.0, c).any()
    assert not np.array_equal(eps, t3.smoothing_noise(seed, t + 1, B, A, sigma, c))
    draws = np.concatenate([t3.smoothing_noise(seed, k, 4096, 1, 1.0, 100.0).reshape(-1) for k in range(1, 9)]).astype(np.float64)
    assert abs(draws.mean()) < 0.02 and abs(draws.var() - 1.0) < 0.03
    # the step's stream is t = step + 1: the oracle at step 6 draws stream 7
    rng = np.random.default_rng(0)
    online, target = _params(3, 1, rng)
    st = t3.new_state(online, target)
    st["step"] = 6
    out = t3.train_step(st, *_batch(3, 1, 5, rng), LR, None, policy_delay=2, sigma=sigma, noise_clip=c, seed=seed, stop_after=3)
    assert np.array_equal(out["t_eps"], t3.smoothing_noise(seed, 7, 5, 1, sigma, c))


# ---- Config rules

def test_twin_defaults_and_rules(ddpg_config, monkeypatch):  # noqa: F811
    from Config import resolve_ddpg
    c = ddpg_config
    assert (c.DDPG_TWIN, c.DDPG_POLICY_DELAY, c.DDPG_TARGET_NOISE, c.DDPG_TARGET_NOISE_CLIP) == (False, 2, 0.2, 0.5)
    monkeypatch.setattr(c, "DDPG_TWIN", True)
    with pytest.raises(ValueError, match="paired"):
        resolve_ddpg()                                                    # DDPG_CRITIC_LOSS is 'fork' by default
    monkeypatch.setattr(c, "DDPG_CRITIC_LOSS", "paired")
    resolve_ddpg()
    for key, bad in (("DDPG_POLICY_DELAY", 0), ("DDPG_POLICY_DELAY", 17), ("DDPG_TARGET_NOISE", -0.1),
                     ("DDPG_TARGET_NOISE_CLIP", -1.0), ("DDPG_TARGET_NOISE", float("nan"))):
        good = getattr(c, key)
        monkeypatch.setattr(c, key, bad)
        with pytest.raises(ValueError, match=key[:17]):
            resolve_ddpg()
        monkeypatch.setattr(c, key, good)
    for delay in (1, 16):
        monkeypatch.setattr(c, "DDPG_POLICY_DELAY", delay)
        resolve_ddpg()
    monkeypatch.setattr(c, "USE_DDPG", False)
    with pytest.raises(ValueError, match="USE_DDPG"):
        resolve_ddpg()


def test_argv_sets_the_twin(ddpg_config, monkeypatch):  # noqa: F811
    import GA3C
    monkeypatch.setattr(ddpg_config, "USE_DDPG", False)
    for k in ("DDPG_TWIN", "DDPG_CRITIC_LOSS", "DDPG_POLICY_DELAY"):
        monkeypatch.setattr(ddpg_config, k, getattr(ddpg_config, k))          # restored afterwards
    GA3C.apply_argv(["GAME=Pendulum-v0", "USE_DDPG=True", "TRAINING_MIN_BATCH_SIZE=64", "DDPG_TWIN=True",
                     "DDPG_CRITIC_LOSS=paired", "DDPG_POLICY_DELAY=3"])
    assert ddpg_config.DDPG_TWIN is True and ddpg_config.DDPG_POLICY_DELAY == 3
    with pytest.raises(ValueError, match="paired"):
        GA3C.apply_argv(["GAME=Pendulum-v0", "USE_DDPG=True", "TRAINING_MIN_BATCH_SIZE=64", "DDPG_TWIN=True",
                         "DDPG_CRITIC_LOSS=fork"])


def test_initial_arena_keeps_the_twenty_and_adds_critic_two():
    import ga3c_amd  # noqa: F401
    import NetworkDDPG as nd
    assert nd.TWIN_TRAINABLE == t3.CRITIC2_TRAINABLE and nd.TRAINABLE == o.TRAINABLE
    for S, A in SHAPES:
        online, target = nd.initial_arena(S, A, 12345, tau=0.001)
        online2, target2 = nd.initial_arena(S, A, 12345, tau=0.001, twin=True)
        assert tuple(online2) == nd.TRAINABLE + nd.TWIN_TRAINABLE == tuple(target2) and len(online2) == 30
        for k in nd.TRAINABLE:
            assert np.array_equal(online[k], online2[k]) and np.array_equal(target[k], target2[k]), k
        shapes = nd.param_shapes(S, A, twin=True)
        for k, k2 in zip(nd.CRITIC_TRAINABLE, nd.TWIN_TRAINABLE):
            assert online2[k2].shape == shapes[k2] == shapes[k] == online2[k].shape and online2[k2].dtype == np.float32
        w = "critic2_fc2/W"
        assert not np.array_equal(online2[w], online2["critic_fc2/W"]), "critic 2 is a draw of its own"
        _, none = nd.initial_arena(S, A, 12345, tau=0.0, twin=True)
        assert not np.array_equal(none[w], online2[w]), "its target starts from an independent draw"
        assert np.allclose(target2[w], 0.001 * online2[w] + 0.999 * none[w], atol=1e-7)
        assert np.max(np.abs(online2["critic2_output/W"])) <= 0.003 and not online2["critic2_fc1/b"].any()
        assert abs(float(online2["critic2_norm1/gamma"].mean()) - 1.0) < 0.001
    # with the two moving statistics the handle has 12 more variables than the 26
    assert len(t3.ALL_VARS) == 38 and t3.ALL_VARS[:26] == o.ALL_VARS and set(t3.shapes(3, 1)) == set(t3.ALL_VARS)


def test_twin_abi_is_declared_and_bound():
    import os
    import re
    import ga3c_amd  # noqa: F401
    import _native as nat
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "ga3c_abi.h")).read(), flags=re.S)
    for name in ("ga3c_ddpg_twin_create", "ga3c_ddpg_twin_destroy"):
        assert re.search(r"\b%s\s*\(" % name, text) and name in nat.HIP_SIGNATURES and hasattr(nat.hip_lib(), name)
