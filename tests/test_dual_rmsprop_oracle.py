"""Config.DUAL_RMSPROP's f64 statement (tests/dual_oracle.py) checked three ways, with no GPU: the two costs' gradients sum
to the oracle's gradient of cost_all, each equals torch autograd (CPU, f64) of its own cost, and each agrees with finite
differences of its own cost.  Also: the ABI flag the library and the binding agree on."""
import os
import re

import numpy as np
import pytest

import dual_oracle as d
import ga3c_oracle as o

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _case(num_actions, bsz, seed):
    params = o.init_params(num_actions)
    x = o.synthetic_states(bsz, seed=seed).astype(np.float64).reshape(bsz, 84, 84, 4)
    rng = np.random.default_rng(seed)
    y = rng.normal(size=bsz)
    a = np.eye(num_actions)[rng.integers(0, num_actions, bsz)]
    return params, x, y, a


def _max_rel(got, want):
    got, want = np.asarray(got).reshape(-1), np.asarray(want).reshape(-1)
    return np.max(np.abs(got - want)) / max(1.0, np.max(np.abs(want)))


@pytest.mark.parametrize("num_actions,bsz,use_log_softmax,min_policy", [(6, 3, False, 0.0), (18, 2, True, 0.0), (4, 2, False, 0.01)])
def test_parts_sum_to_the_cost_all_gradient(num_actions, bsz, use_log_softmax, min_policy):
    params, x, y, a = _case(num_actions, bsz, 11 + num_actions)
    kw = dict(min_policy=min_policy, use_log_softmax=use_log_softmax)
    _, g = o.loss_and_grads(params, x, y, a, 0.01, **kw)
    _, gp, gv = d.dual_grads(params, x, y, a, 0.01, **kw)
    for k in o.PARAM_ORDER:
        assert _max_rel(gp[k] + gv[k], g[k]) <= 1e-10, k
    for k in d.HEAD_V:                 # cost_p reaches the value head only through tf.stop_gradient
        assert not np.any(gp[k]), k
    for k in d.HEAD_P:                 # cost_v has no path to the policy head
        assert not np.any(gv[k]), k


def _torch_costs(params, x, y_r, a, beta, log_eps, min_policy, use_log_softmax, which):
    """cost_p or cost_v of the graph in torch (the statement of test_oracle_torch_crosscheck.py), differentiated alone."""
    torch = pytest.importorskip("torch")
    F = torch.nn.functional
    t = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in params.items()}
    xt = torch.tensor(x, dtype=torch.float64).permute(0, 3, 1, 2)

    def conv(inp, w, b, k, s):
        n = inp.shape[2]
        total = max((-(-n // s) - 1) * s + k - n, 0)
        lo, hi = total // 2, total - total // 2
        return F.conv2d(F.pad(inp, (lo, hi, lo, hi)), w.permute(3, 2, 0, 1), b, stride=s)

    n1 = torch.relu(conv(xt, t["conv11/w"], t["conv11/b"], 8, 4))
    n2 = torch.relu(conv(n1, t["conv12/w"], t["conv12/b"], 4, 2))
    d1 = torch.relu(n2.permute(0, 2, 3, 1).reshape(x.shape[0], -1) @ t["dense1/w"] + t["dense1/b"])
    v = (d1 @ t["logits_v/w"] + t["logits_v/b"])[:, 0]
    z = d1 @ t["logits_p/w"] + t["logits_p/b"]
    yt, at = torch.tensor(y_r, dtype=torch.float64), torch.tensor(a, dtype=torch.float64)
    adv = yt - v.detach()
    if use_log_softmax:
        ls = F.log_softmax(z, dim=1)
        s = F.softmax(z, dim=1)
        c1 = ((ls * at).sum(1) * adv).sum()
        c2 = (-beta * (ls * s).sum(1)).sum()
    else:
        p = (F.softmax(z, dim=1) + min_policy) / (1.0 + min_policy * z.shape[1])
        eps = torch.tensor(log_eps, dtype=torch.float64)
        c1 = (torch.log(torch.maximum((p * at).sum(1), eps)) * adv).sum()
        c2 = (-beta * (torch.log(torch.maximum(p, eps)) * p).sum(1)).sum()
    cost = -(c1 + c2) if which == "p" else 0.5 * ((yt - v) ** 2).sum()
    cost.backward()
    return {k: (t[k].grad.numpy() if t[k].grad is not None else np.zeros_like(params[k])) for k in t}


@pytest.mark.parametrize("num_actions,bsz,use_log_softmax,min_policy", [(6, 3, False, 0.0), (18, 2, True, 0.0), (4, 2, False, 0.01)])
def test_each_part_matches_autograd_of_its_own_cost(num_actions, bsz, use_log_softmax, min_policy):
    params, x, y, a = _case(num_actions, bsz, 40 + num_actions)
    _, gp, gv = d.dual_grads(params, x, y, a, 0.02, min_policy=min_policy, use_log_softmax=use_log_softmax)
    tp = _torch_costs(params, x, y, a, 0.02, 1e-6, min_policy, use_log_softmax, "p")
    tv = _torch_costs(params, x, y, a, 0.02, 1e-6, min_policy, use_log_softmax, "v")
    for k in o.PARAM_ORDER:
        assert _max_rel(gp[k], tp[k]) < 1e-10, ("cost_p", k)
        assert _max_rel(gv[k], tv[k]) < 1e-10, ("cost_v", k)


def test_each_part_matches_finite_differences():
    """Central differences of cost_p (advantage frozen, as tf.stop_gradient makes autodiff see it) and of cost_v."""
    num_actions, bsz = 5, 2
    params, x, y, a = _case(num_actions, bsz, 77)
    _, gp, gv = d.dual_grads(params, x, y, a, 0.05)
    adv = y - o.forward(params, x)["v"]

    def costs(pp):
        losses, _ = o.loss_and_grads(pp, x, y, a, 0.05, adv_const=adv)
        cost_p = -(losses["cost_p_1_agg"] + losses["cost_p_2_agg"])
        cost_v = 0.5 * np.sum((y - o.forward(pp, x)["v"]) ** 2)
        return cost_p, cost_v

    rng = np.random.default_rng(5)
    h = 1e-6
    for k in o.PARAM_ORDER:
        for _ in range(2):
            idx = tuple(int(rng.integers(0, s)) for s in params[k].shape)
            up = {kk: vv.copy() for kk, vv in params.items()}
            dn = {kk: vv.copy() for kk, vv in params.items()}
            up[k][idx] += h
            dn[k][idx] -= h
            (pu, vu), (pd, vd) = costs(up), costs(dn)
            for num, ana, name in (((pu - pd) / (2 * h), gp[k][idx], "cost_p"), ((vu - vd) / (2 * h), gv[k][idx], "cost_v")):
                assert abs(num - ana) <= 1e-5 * max(1.0, abs(ana)), (name, k, idx, num, ana)


def test_update_skips_heads_without_a_slot():
    """The value optimizer leaves its slots on logits_p/* alone, the policy optimizer its slots on logits_v/*; each head
    still moves (by its own optimizer), and the trunk moves by the two steps together."""
    num_actions, bsz = 6, 3
    params, x, y, a = _case(num_actions, bsz, 3)
    _, gp, gv = d.dual_grads(params, x, y, a, 0.01)
    for momentum in (0.0, 0.5):
        p1, s1 = {k: v.copy() for k, v in params.items()}, d.init_slots(params)
        d.dual_rmsprop_update(p1, s1, gp, gv, 1e-3, momentum=momentum)
        for k in d.HEAD_P:
            assert np.all(s1["ms_v"][k] == 1.0) and np.all(s1["mom_v"][k] == 0.0), k
            assert np.any(s1["ms_p"][k] != 1.0), k
        for k in d.HEAD_V:
            assert np.all(s1["ms_p"][k] == 1.0) and np.all(s1["mom_p"][k] == 0.0), k
            assert np.any(s1["ms_v"][k] != 1.0), k
        for k in o.PARAM_ORDER:
            assert np.any(p1[k] != params[k]), k
        # the trunk: the sum of two single-optimizer steps, each from its own fresh slots
        ms = {k: np.ones_like(v) for k, v in params.items()}
        pv = {k: v.copy() for k, v in params.items()}
        o.rmsprop_update(pv, ms, gv, 1e-3)
        ms = {k: np.ones_like(v) for k, v in params.items()}
        pp = {k: v.copy() for k, v in params.items()}
        o.rmsprop_update(pp, ms, gp, 1e-3)
        if momentum == 0.0:
            for k in ("conv11/w", "dense1/b"):
                want = params[k] - (params[k] - pv[k]) - (params[k] - pp[k])
                assert np.max(np.abs(p1[k] - want)) < 1e-15, k


def test_clip_by_norm_is_per_tensor_l2():
    g = np.array([3.0, 4.0])
    assert np.allclose(d.clip_by_norm(g, 1.0), [0.6, 0.8])
    assert np.array_equal(d.clip_by_norm(g, 10.0), g)


def test_abi_declares_the_dual_flag_the_binding_uses():
    import ga3c_amd  # noqa: F401  (puts the flat modules on sys.path)
    import _native
    with open(os.path.join(ROOT, "include", "ga3c_abi.h")) as fh:
        m = re.search(r"#define\s+GA3C_FLAG_DUAL_RMSPROP\s+(\d+)u", fh.read())
    assert m is not None
    assert int(m.group(1)) == _native.FLAG_DUAL_RMSPROP
    assert _native.FLAG_DUAL_RMSPROP not in (_native.FLAG_LOG_SOFTMAX, _native.FLAG_GRAD_CLIP)
