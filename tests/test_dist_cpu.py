"""The distributional step's statement (tests/dist_oracle.py) without a GPU: against torch autograd in f64, the
projection's properties, and the Config, ABI and initial-value rules of DDPG_DISTRIBUTIONAL."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import ddpg_oracle as o
import dist_oracle as d4
from test_ddpg_cpu import _actor, _batch, _close, _critic, _t, ddpg_config  # noqa: F401

SHAPES = [(3, 1), (7, 3)]
ATOMS = [2, 51]
LR = 3e-4
VMIN, VMAX = -3.0, 1.0          # narrow: rewards of U(-1, 0) and gamma z reach past both ends on some rows


def _params(S, A, N, rng):
    return d4.random_params(S, A, N, rng, stats=True), d4.random_params(S, A, N, rng, stats=True)


def _wide_batch(S, A, B, rng):
    """_batch with rewards wide enough for rows clipped at either end of [VMIN, VMAX]."""
    s, a, _, done, s2 = _batch(S, A, B, rng)
    return s, a, rng.uniform(-5.0, 3.0, B), done, s2


def _torch_project(pt, r, g, N):
    z, lo, hi, delta = d4.support(N, VMIN, VMAX)
    zt, k = torch.tensor(z), torch.arange(N, dtype=torch.float64)
    b = (torch.clamp(r[:, None] + g[:, None] * zt[None, :], lo, hi) - lo) / delta
    return torch.einsum("ij,ijk->ik", pt, torch.clamp(1.0 - (b[:, :, None] - k[None, None, :]).abs(), min=0.0))


@pytest.mark.parametrize("S,A", SHAPES)
@pytest.mark.parametrize("N", ATOMS)
def test_oracle_gradients_match_torch_autograd(S, A, N):
    rng = np.random.default_rng(S + A + N)
    B = 9
    online, target = _params(S, A, N, rng)
    s, a, r, done, s2 = _wide_batch(S, A, B, rng)
    w = rng.uniform(0.2, 1.0, B)
    z = torch.tensor(d4.support(N, VMIN, VMAX)[0])
    ts, ta, tr, td, ts2 = (torch.tensor(v, dtype=torch.float64) for v in (s, a, r, done, s2))
    T = _t(target)
    pt = torch.softmax(_critic(T, ts2, _actor(T, ts2)), dim=1)
    g = torch.where(td != 0, torch.zeros_like(tr), torch.full_like(tr, 0.99))
    m = _torch_project(pt, tr, g, N).detach()
    tg = d4.targets(target, s2, r, done, 0.99, N, VMIN, VMAX)
    assert _close(tg["pt"], pt.numpy()) and _close(tg["m"], m.numpy())
    assert _close(tg["y"], (m @ z).numpy()) and _close(tg["qt"], (pt @ z).numpy())
    # the critic's gradients of the weighted cross-entropy, the target detached
    P = _t(online, grad=o.CRITIC_TRAINABLE)
    logp = torch.log_softmax(_critic(P, ts, ta), dim=1)
    loss = (torch.tensor(w) * -(m * logp).sum(dim=1)).mean()
    loss.backward()
    f, gc = d4.critic_grads(online, s, a, tg["m"], N, VMIN, VMAX, w)
    assert _close([f["loss"]], [loss.item()])
    for k in o.CRITIC_TRAINABLE:
        if k == o.DEAD:
            assert P[k].grad is None and not gc[k].any()
        else:
            assert _close(gc[k].reshape(P[k].shape), P[k].grad.numpy()), k
    # the action gradient of the expected value
    P = _t(online)
    act = (_actor(P, ts) + 0.05).detach().requires_grad_(True)
    q = torch.softmax(_critic(P, ts, act), dim=1) @ z
    q.sum().backward()
    assert _close(d4.action_gradient(online, s, act.detach().numpy(), N, VMIN, VMAX), act.grad.numpy())
    assert _close(f["qv"], (torch.softmax(_critic(P, ts, ta), dim=1) @ z).detach().numpy())


def _torch_step(P, T, slots, t, batch, noise, N, cfg):
    """One whole step with torch autograd for the three gradients and ddpg_oracle's optimizer formulas for the updates."""
    s, a, r, done, s2 = (torch.tensor(v, dtype=torch.float64) for v in batch)
    z = torch.tensor(d4.support(N, VMIN, VMAX)[0])
    Tt = _t(T)
    pt = torch.softmax(_critic(Tt, s2, _actor(Tt, s2)), dim=1)
    g = torch.where(done != 0, torch.zeros_like(r), torch.full_like(r, 0.99))
    m = _torch_project(pt, r, g, N).detach()
    Pt = _t(P, grad=o.CRITIC_TRAINABLE)
    (-(m * torch.log_softmax(_critic(Pt, s, a), dim=1)).sum(dim=1)).mean().backward()
    for k in o.CRITIC_TRAINABLE:
        if k == o.DEAD:
            continue
        gk = Pt[k].grad.numpy().reshape(P[k].shape)
        if cfg.get("clip"):
            gk = o.clip_by_norm(gk, cfg["clip"])
        if cfg.get("critic_rmsprop", True):
            o.rmsprop_step(P[k], slots[0][k], slots[1][k], gk, 10.0 * LR, 0.99, cfg.get("momentum", 0.0), 0.1)
        else:
            o.adam_step(P[k], slots[0][k], slots[1][k], gk, 10.0 * LR, t)
    Pt = _t(P, grad=o.ACTOR_TRAINABLE)
    q = torch.softmax(_critic(Pt, s, _actor(Pt, s) + torch.tensor(noise)), dim=1) @ z
    (-q.sum()).backward()                  # sum over rows of d(out)/d(var) contracted with -dQ/da
    for k in o.ACTOR_TRAINABLE:
        o.adam_step(P[k], slots[0][k], slots[1][k], Pt[k].grad.numpy().reshape(P[k].shape), LR, t)
    o.soft_update(P, T, 0.001)


@pytest.mark.parametrize("S,A", SHAPES)
@pytest.mark.parametrize("N", ATOMS)
@pytest.mark.parametrize("cfg", [dict(), dict(critic_rmsprop=False), dict(clip=0.05, momentum=0.9)], ids=["rmsprop", "adam", "clip"])
def test_two_whole_steps_match_torch(S, A, N, cfg):
    rng = np.random.default_rng(40 + S + N)
    online, target = _params(S, A, N, rng)
    st = d4.new_state(online, target, critic_rmsprop=cfg.get("critic_rmsprop", True))
    ref = d4.new_state(online, target, critic_rmsprop=cfg.get("critic_rmsprop", True))
    noise = np.full(A, 0.05)
    for t in (1, 2):
        batch = _wide_batch(S, A, 8, rng)
        d4.train_step(st, *batch, LR, noise, atoms=N, vmin=VMIN, vmax=VMAX, **cfg)
        _torch_step(ref["online"], ref["target"], (ref["slot_a"], ref["slot_b"]), t, batch, noise, N, cfg)
    assert st["step"] == 2
    for k in o.TRAINABLE:
        for w in ("online", "target", "slot_a", "slot_b"):
            assert _close(st[w][k], ref[w][k], 1e-9), (w, k)


# ---- the projection

def _dists(B, N, rng):
    p = rng.uniform(0.0, 1.0, (B, N)) ** 3
    return p / p.sum(axis=1, keepdims=True)


@pytest.mark.parametrize("N", [2, 5, 51, 64])
def test_projection_keeps_the_mass_and_the_mean(N):
    rng = np.random.default_rng(N)
    B = 40
    pt, r, g = _dists(B, N, rng), rng.uniform(-5.0, 3.0, B), np.where(rng.uniform(size=B) < 0.3, 0.0, 0.99)
    m = d4.project(pt, r, g, N, VMIN, VMAX)
    assert np.all(m >= 0.0) and np.max(np.abs(m.sum(axis=1) - 1.0)) <= 1e-12
    z = d4.support(N, VMIN, VMAX)[0]
    tz = r[:, None] + g[:, None] * z[None, :]
    free = ((tz >= VMIN) & (tz <= VMAX)).all(axis=1)
    assert free.any() and not free.all()
    assert np.max(np.abs((m @ z)[free] - (r + g * (pt @ z))[free])) <= 1e-12
    # equal to the floor / ceil scatter where no b_j is an integer
    b = (np.clip(tz, VMIN, VMAX) - VMIN) / ((VMAX - VMIN) / (N - 1))
    whole = (b == np.round(b)).any(axis=1)
    assert (~whole).any()
    assert np.max(np.abs(m[~whole] - d4.project_scatter(pt, r, g, N, VMIN, VMAX)[~whole])) <= 1e-12


@pytest.mark.parametrize("N", [2, 51])
def test_projection_is_whole_where_b_is_an_integer(N):
    """A done row with r = z_k: every b_j = k exactly, which the floor / ceil scatter gives no mass at all."""
    rng = np.random.default_rng(3)
    z = d4.support(N, VMIN, VMAX)[0]
    ks = np.array([0, N // 2, N - 1])
    pt = _dists(3, N, rng)
    m = d4.project(pt, z[ks], np.zeros(3), N, VMIN, VMAX)
    assert np.max(np.abs(m.sum(axis=1) - 1.0)) <= 1e-12
    assert np.max(np.abs(m[np.arange(3), ks] - 1.0)) <= 1e-12
    assert np.max(np.abs(d4.project_scatter(pt, z[ks], np.zeros(3), N, VMIN, VMAX).sum(axis=1))) <= 1e-12
    # ... and the rule without future rewards is the same projection of r alone
    assert np.array_equal(d4.project(None, z[ks], None, N, VMIN, VMAX), (np.arange(N)[None, :] == ks[:, None]).astype(np.float64))


def test_mass_beyond_an_end_lands_on_the_end_atom():
    N = 51
    pt = _dists(2, N, np.random.default_rng(4))
    m = d4.project(pt, np.array([VMAX + 10.0, VMIN - 10.0]), np.full(2, 0.99), N, VMIN, VMAX)
    assert abs(m[0, -1] - 1.0) <= 1e-12 and abs(m[1, 0] - 1.0) <= 1e-12
    assert np.max(np.abs(m[0, :-1])) == 0.0 and np.max(np.abs(m[1, 1:])) == 0.0


def test_per_row_discounts_and_done_rows():
    rng = np.random.default_rng(5)
    S, A, N, B = 3, 1, 7, 6
    _, target = _params(S, A, N, rng)
    s, a, r, done, s2 = _batch(S, A, B, rng)
    done[:] = [0, 1, 0, 0, 1, 0]
    disc = rng.uniform(0.5, 0.99, B)
    tg = d4.targets(target, s2, r, done, disc, N, VMIN, VMAX)
    assert np.array_equal(tg["g"], np.where(done != 0, 0.0, disc))
    assert np.allclose(tg["m"], d4.project(tg["pt"], r, tg["g"], N, VMIN, VMAX), atol=0, rtol=0)
    none = d4.targets(target, s2, r, done, disc, N, VMIN, VMAX, future=False)
    assert not none["pt"].any() and not none["qt"].any()
    assert np.array_equal(none["m"], d4.project(None, r, None, N, VMIN, VMAX))


# ---- Config rules

def test_distributional_defaults_and_rules(ddpg_config, monkeypatch):  # noqa: F811
    from Config import resolve_ddpg
    c = ddpg_config
    assert (c.DDPG_DISTRIBUTIONAL, c.DDPG_ATOMS, c.DDPG_V_MIN, c.DDPG_V_MAX) == (False, 51, -100.0, 0.0)
    monkeypatch.setattr(c, "DDPG_DISTRIBUTIONAL", True)
    with pytest.raises(ValueError, match="paired"):
        resolve_ddpg()                                                    # DDPG_CRITIC_LOSS is 'fork' by default
    monkeypatch.setattr(c, "DDPG_CRITIC_LOSS", "paired")
    resolve_ddpg()
    monkeypatch.setattr(c, "DDPG_TWIN", True)
    with pytest.raises(ValueError, match="DDPG_TWIN"):
        resolve_ddpg()
    monkeypatch.setattr(c, "DDPG_TWIN", False)
    for key, bad in (("DDPG_ATOMS", 1), ("DDPG_ATOMS", 65), ("DDPG_ATOMS", 7.5), ("DDPG_V_MIN", 0.0), ("DDPG_V_MIN", 1.0),
                     ("DDPG_V_MAX", float("nan"))):
        good = getattr(c, key)
        monkeypatch.setattr(c, key, bad)
        with pytest.raises(ValueError, match=key[:9]):
            resolve_ddpg()
        monkeypatch.setattr(c, key, good)
    for n in (2, 64):
        monkeypatch.setattr(c, "DDPG_ATOMS", n)
        resolve_ddpg()
    monkeypatch.setattr(c, "USE_DDPG", False)
    with pytest.raises(ValueError, match="USE_DDPG"):
        resolve_ddpg()


def test_argv_sets_the_distributional_critic(ddpg_config, monkeypatch):  # noqa: F811
    import GA3C
    monkeypatch.setattr(ddpg_config, "USE_DDPG", False)
    for k in ("DDPG_DISTRIBUTIONAL", "DDPG_CRITIC_LOSS", "DDPG_ATOMS", "DDPG_V_MIN", "DDPG_V_MAX"):
        monkeypatch.setattr(ddpg_config, k, getattr(ddpg_config, k))          # restored afterwards
    base = ["GAME=Pendulum-v0", "USE_DDPG=True", "TRAINING_MIN_BATCH_SIZE=64", "DDPG_DISTRIBUTIONAL=True"]
    GA3C.apply_argv(base + ["DDPG_CRITIC_LOSS=paired", "DDPG_ATOMS=21", "DDPG_V_MIN=-50", "DDPG_V_MAX=-1.5"])
    c = ddpg_config
    assert c.DDPG_DISTRIBUTIONAL is True and (c.DDPG_ATOMS, c.DDPG_V_MIN, c.DDPG_V_MAX) == (21, -50.0, -1.5)
    with pytest.raises(ValueError, match="paired"):
        GA3C.apply_argv(base + ["DDPG_CRITIC_LOSS=fork"])


# ---- shapes, initial values, ABI

def test_shapes_and_initial_arena_with_atoms():
    import ga3c_amd  # noqa: F401
    import NetworkDDPG as nd
    for S, A in SHAPES:
        plain = nd.param_shapes(S, A)
        assert plain == {k: v for k, v in o.shapes(S, A).items() if k in o.TRAINABLE}
        assert nd.param_shapes(S, A, atoms=None) == plain and nd.param_shapes(S, A, False, None) == plain
        for N in (2, 51):
            sh = nd.param_shapes(S, A, atoms=N)
            assert tuple(sh) == tuple(plain) and sh == {k: v for k, v in d4.shapes(S, A, N).items() if k in o.TRAINABLE}
            assert [k for k in sh if sh[k] != plain[k]] == ["critic_output/W", "critic_output/b"]
            online0, target0 = nd.initial_arena(S, A, 12345, tau=0.001)
            online, target = nd.initial_arena(S, A, 12345, tau=0.001, atoms=N)
            assert tuple(online) == nd.TRAINABLE == tuple(target)
            for k in nd.TRAINABLE:
                assert online[k].shape == sh[k] == target[k].shape and online[k].dtype == np.float32
            # the stream is the same up to the head, which is drawn in its place
            for k in nd.TRAINABLE[:nd.TRAINABLE.index("critic_output/W")]:
                assert np.array_equal(online[k], online0[k]), k
            assert np.max(np.abs(online["critic_output/W"])) <= 0.003 and online["critic_output/W"].any()
            assert not online["critic_output/b"].any()
    a, b = nd.initial_arena(3, 1, 12345), nd.initial_arena(3, 1, 12345, atoms=None)
    assert all(np.array_equal(a[i][k], b[i][k]) for i in (0, 1) for k in nd.TRAINABLE)
    assert nd.param_shapes(3, 1, twin=True, atoms=5)["critic2_output/W"] == (300, 1)


def test_dist_abi_is_declared_and_bound():
    import ga3c_amd  # noqa: F401
    import _native as nat
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "ga3c_abi.h")).read(), flags=re.S)
    i32p, f32p = C.POINTER(C.c_int32), C.POINTER(C.c_float)
    want = {"ga3c_ddpg_dist_create": [C.c_void_p, C.c_int32, C.c_float, C.c_float], "ga3c_ddpg_dist_destroy": [C.c_void_p],
            "ga3c_ddpg_dist_info": [C.c_void_p, i32p, f32p, f32p]}
    for name, args in want.items():
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name
        assert nat.HIP_SIGNATURES[name] == (C.c_int, args)
        fn = getattr(nat.hip_lib(), name)
        assert fn.restype is C.c_int and list(fn.argtypes) == args
    assert re.search(r"#define\s+GA3C_DDPG_ATOMS_MAX\s+64\b", text)
