"""Config.DUAL_RMSPROP on the vector-state network without a GPU: the f64 statement tests/mlp_dual_oracle.py
checked four ways -- the two costs' gradients sum to mlp_oracle's, each equals torch autograd of its own cost (y_r - v
detached in cost_p) and agrees with central differences (adv_const frozen), and the regions without a path are exactly
zero -- then one two-optimizer step with clipping and momentum, and the configuration rules."""
import numpy as np
import pytest

import mlp_oracle as m
import mlp_dual_oracle as d

SHAPES = [(3, 1), (7, 3)]


def _case(state_dim, num_actions, bsz, seed):
    params = m.init_params(state_dim, num_actions, seed=seed)
    rng = np.random.default_rng(seed)
    params["logits_p/out_x/b"] = rng.uniform(-2, 2, num_actions)
    params["logits_p/out_y/b"] = rng.uniform(-2, 2, num_actions)
    x = rng.uniform(-2, 2, size=(3 * bsz + 16, state_dim))
    x = x[m.safe_rows(params, x, 1e-2)][:bsz]
    assert x.shape[0] == bsz
    y = rng.normal(size=bsz)
    a = rng.uniform(-1, 1, size=(bsz, num_actions))
    return params, x, y, a


@pytest.mark.parametrize("state_dim,num_actions", SHAPES)
def test_the_two_costs_sum_to_the_single_gradient_and_have_exact_zeros(state_dim, num_actions):
    worst = 0.0
    for bsz in (1, 17, 132, 201):
        params, x, y, a = _case(state_dim, num_actions, bsz, 40 + bsz)
        losses, gp, gv = d.dual_grads(params, x, y, a, 0.01)
        want_losses, g = m.loss_and_grads(params, x, y, a, 0.01)
        assert losses == want_losses
        for k in m.PARAM_ORDER + d.DELTAS + ("dv", "dz"):
            err = np.max(np.abs(gp[k] + gv[k] - g[k])) / np.max(np.abs(g[k]))
            worst = max(worst, err)
            assert err <= 1e-12, (bsz, k, err)
        for k in d.HEAD_V:
            assert gp[k].shape == params[k].shape and not np.any(gp[k]), k       # cost_p: no path to logits_v
        for k in d.HEAD_P:
            assert gv[k].shape == params[k].shape and not np.any(gv[k]), k       # cost_v: no path to logits_p/out_x, out_y
        assert not np.any(gp["dv"]) and not np.any(gv["dz"])
        for k in d.TRUNK_VARS:
            assert np.any(gp[k]) and np.any(gv[k]), k
    print("worst |g_p + g_v - g| / max|g| = %.2e" % worst)


def _torch_cost_grads(params, x, y_r, a, beta):
    torch = pytest.importorskip("torch")
    out = []
    for which in ("p", "v"):
        t = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in params.items()}
        h = torch.tensor(x, dtype=torch.float64)
        for name, _, sig in m.TRUNK:
            h = h @ t[name + "/w"] + t[name + "/b"]
            if sig:
                h = torch.sigmoid(h)
        v = (h @ t["logits_v/w"] + t["logits_v/b"])[:, 0]
        X = torch.sigmoid(h @ t["logits_p/out_x/w"] + t["logits_p/out_x/b"]) - 0.5
        Y = torch.sigmoid(h @ t["logits_p/out_y/w"] + t["logits_p/out_y/b"]) - 0.5
        o = torch.atan2(Y, X) / np.pi
        yt, at = torch.tensor(y_r, dtype=torch.float64), torch.tensor(a, dtype=torch.float64)
        c1 = ((o * at).sum(1) * (yt - v.detach())).sum()
        c2 = (-beta * (o * o).sum(1)).sum()
        cost = -(c1 + c2) if which == "p" else 0.5 * ((yt - v) ** 2).sum()
        cost.backward()
        out.append({k: None if t[k].grad is None else t[k].grad.numpy() for k in t})
    return out


@pytest.mark.parametrize("state_dim,num_actions", SHAPES)
def test_each_cost_matches_torch_autograd(state_dim, num_actions):
    params, x, y, a = _case(state_dim, num_actions, 9, 11 + state_dim)
    tp, tv = _torch_cost_grads(params, x, y, a, 0.01)
    _, gp, gv = d.dual_grads(params, x, y, a, 0.01)
    for k in m.PARAM_ORDER:
        for got, want, no_path in ((gp, tp, d.HEAD_V), (gv, tv, d.HEAD_P)):
            if k in no_path:                # autograd: None, the variable TF-1 gives that optimizer no slot for
                assert want[k] is None or not np.any(want[k]), k
                assert not np.any(got[k]), k
            else:
                err = np.max(np.abs(got[k] - want[k])) / max(1.0, np.max(np.abs(want[k])))
                assert err < 1e-10, (k, err)


@pytest.mark.parametrize("state_dim,num_actions", SHAPES)
def test_each_cost_matches_central_differences(state_dim, num_actions):
    params, x, y, a = _case(state_dim, num_actions, 5, 3 + state_dim)
    beta = 0.05
    adv = y - m.forward(params, x)["v"]
    _, gp, gv = d.dual_grads(params, x, y, a, beta)
    rng = np.random.default_rng(0)
    eps = 1e-6
    for k in m.PARAM_ORDER:
        for idx in [tuple(rng.integers(0, s) for s in params[k].shape) for _ in range(3)]:
            save = params[k][idx]
            vals = []
            for step in (eps, -eps):
                params[k][idx] = save + step
                losses, _ = m.loss_and_grads(params, x, y, a, beta, adv_const=adv)
                vals.append((-(losses["cost_p_1_agg"] + losses["cost_p_2_agg"]), losses["cost_v"]))
            params[k][idx] = save
            for c, g in enumerate((gp, gv)):
                fd = (vals[0][c] - vals[1][c]) / (2 * eps)
                assert abs(fd - g[k][idx]) < 1e-6 * max(1.0, abs(fd)), (k, idx, c, fd, g[k][idx])


def test_float32_weights_give_a_float32_restatement():
    params, x, y, a = _case(3, 1, 17, 5)
    p32 = {k: v.astype(np.float32) for k, v in params.items()}
    _, gp, gv = d.dual_grads(p32, x.astype(np.float32), y.astype(np.float32), a.astype(np.float32), 0.01)
    for g in (gp, gv):
        for k in m.PARAM_ORDER + d.DELTAS + ("dv", "dz"):
            assert np.asarray(g[k]).dtype == np.float32, k


def test_one_dual_step_with_clipping_and_momentum_keeps_the_slotless_regions():
    params, x, y, a = _case(3, 1, 8, 5)
    _, gp, gv = d.dual_grads(params, x, y, a, 0.01)
    clip, mu, lr = 0.05, 0.5, 1e-3
    p1 = {k: v.copy() for k, v in params.items()}
    slots = d.init_slots(params)
    d.dual_rmsprop_update(p1, slots, gp, gv, lr, momentum=mu, clip=clip)
    for k in m.PARAM_ORDER:
        want = params[k].copy()
        for cost, g, ms, mom, no_slot in (("v", gv, "ms_v", "mom_v", d.HEAD_P), ("p", gp, "ms_p", "mom_p", d.HEAD_V)):
            if k in no_slot:
                assert np.array_equal(slots[ms][k], np.ones_like(params[k])), (k, cost)
                assert np.array_equal(slots[mom][k], np.zeros_like(params[k])), (k, cost)
                continue
            gc = g[k] * clip / max(np.sqrt(np.sum(g[k] ** 2)), clip)
            assert np.sqrt(np.sum(gc ** 2)) <= clip * (1 + 1e-12)
            s = 0.99 + 0.01 * gc * gc
            step = lr * gc / np.sqrt(s + 0.1)          # mom starts at 0: the first step is the plain step
            want = want - step
            assert np.max(np.abs(slots[ms][k] - s)) < 1e-12 and np.max(np.abs(slots[mom][k] - step)) < 1e-12, (k, cost)
        assert np.max(np.abs(p1[k] - want)) < 1e-12, k
    mask = d.region_mask(3, 1, d.HEAD_P)
    assert mask.size == m.param_count(3, 1) and mask.sum() == 2 * (64 + 1) and not mask[:-130].any()


_KEYS = ("CONTINUOUS_INPUT", "DISCRATE_INPUT", "GAME", "USE_DDPG", "USE_REPLAY_MEMORY", "DISCOUNTING", "DUAL_RMSPROP",
         "TRAINING_MIN_BATCH_SIZE")


def test_pendulum_accepts_dual_and_the_other_vector_paths_still_refuse_it(monkeypatch):
    import ga3c_amd  # noqa: F401
    from Config import Config
    import GA3C
    for k in _KEYS:
        monkeypatch.setattr(Config, k, getattr(Config, k))
    GA3C.apply_argv(["GAME=Pendulum-v0", "DUAL_RMSPROP=True"])
    assert Config.DUAL_RMSPROP is True and Config.CONTINUOUS_INPUT and not Config.DISCRATE_INPUT and not Config.USE_DDPG
    import NetworkVP_vector
    import NetworkVP_discrate
    assert NetworkVP_vector.Network.DUAL_RMSPROP_REFUSAL is None
    assert NetworkVP_discrate.Network.DUAL_RMSPROP_REFUSAL
    Config.DUAL_RMSPROP = False
    with pytest.raises(ValueError):
        GA3C.apply_argv(["GAME=CartPole-v0", "DUAL_RMSPROP=True"])
    Config.DUAL_RMSPROP = False
    with pytest.raises(ValueError):
        GA3C.apply_argv(["GAME=Pendulum-v0", "USE_DDPG=True", "TRAINING_MIN_BATCH_SIZE=64", "DUAL_RMSPROP=True"])
