"""The cases of tests/test_gpu_vector_limits.py without a GPU (tests/vector_limit_cases.py builds them for both files): every
condition that makes them worth running, from the float64 oracle alone -- safe_rows keeps at least 90 % of the candidate rows
at every (shape, size), the saturated heads' logits reach past |z| = 17 (the float32 sigmoid is exactly 1) in a quarter of the
entries and past 88.8 (expf overflows, the sigmoid is exactly 0) in at least one while 2 % stay below 2, and no compared tensor
of the oracle is all zero.  Then the oracles themselves where the GPU tests lean on them and no older test took them:
mlp_oracle and mlp_dual_oracle against central differences of their own costs at A = 32, with the step and the bound of
tests/test_vector_net_cpu.py and tests/test_vector_dual_cpu.py."""
import numpy as np
import pytest

import mlp_dual_oracle as d
import mlp_oracle as m
import vector_limit_cases as vc

DELTAS = ("dv", "dz", "dd1", "dpd4", "dpd3", "dpd2", "dpd1")
EPS, FD_TOL, FD_BETA, FD_ROWS = 1e-6, 1e-6, 0.05, 5      # test_oracle_matches_central_differences' step, bound, beta and rows


@pytest.mark.parametrize("state_dim,num_actions", vc.SHAPES)
def test_safe_rows_keeps_the_batch_and_no_compared_tensor_is_all_zero(state_dim, num_actions):
    S, A = state_dim, num_actions
    params = vc.limit_params(S, A)
    for bsz in vc.SIZES:
        kept, total = vc.check_kept(S, A, bsz)
        print("vector S=%d A=%d B=%d: safe_rows keeps %d of %d candidate rows (%.1f %%)" % (S, A, bsz, kept, total,
                                                                                            100.0 * kept / total))
        x, y, a = vc.limit_batch(S, A, bsz)
        assert x.shape == (bsz, S) and a.shape == (bsz, A) and y.shape == (bsz,)
        f = m.forward(params, x.astype(np.float64))
        _, g = m.loss_and_grads(params, *vc.f64(x, y, a), vc.BETA)
        _, gp, gv = d.dual_grads(params, *vc.f64(x, y, a), vc.BETA)
        vc.no_zero_tensor(dict(f, p=f["o"]), ("x", "pd1", "pd2", "pd3", "pd4", "d1", "v", "p", "z"), (S, A, bsz))
        vc.no_zero_tensor(g, DELTAS + m.PARAM_ORDER, (S, A, bsz))
        vc.no_zero_tensor(gp, tuple(k for k in d.DELTAS + ("dz",) + m.PARAM_ORDER if k not in d.HEAD_V), (S, A, bsz, "p"))
        vc.no_zero_tensor(gv, tuple(k for k in d.DELTAS + ("dv",) + m.PARAM_ORDER if k not in d.HEAD_P), (S, A, bsz, "v"))


@pytest.mark.parametrize("state_dim,num_actions", vc.SATURATED)
def test_saturated_heads_leave_the_linear_range_both_ways(state_dim, num_actions):
    S, A = state_dim, num_actions
    s, (kept, total) = vc.check_saturated(S, A)
    print("saturated S=%d A=%d B=%d: max|z| %.1f, |z| > %g in %.1f %%, |z| > %g in %d entries, |z| < %g in %.1f %%, "
          "safe_rows keeps %d of %d" % (S, A, vc.SAT_B, s["max"], vc.ONE, 100 * s["one"], vc.OVERFLOW, s["overflow"], vc.LINEAR,
                                        100 * s["linear"], kept, total))
    params = vc.saturated_params(S, A)
    x, y, a = vc.saturated_batch(S, A)
    _, g = m.loss_and_grads(params, *vc.f64(x, y, a), vc.BETA)
    vc.no_zero_tensor(g, DELTAS + m.PARAM_ORDER, (S, A))
    if (S, A) == (64, 32):
        _, gp, gv = d.dual_grads(params, *vc.f64(x, y, a), vc.BETA)
        vc.no_zero_tensor(gp, tuple(k for k in m.PARAM_ORDER if k not in d.HEAD_V), (S, A, "p"))
        vc.no_zero_tensor(gv, tuple(k for k in m.PARAM_ORDER if k not in d.HEAD_P), (S, A, "v"))
    # the float32 run that supplies e32: sigmoids at exactly 0 and at exactly 1, every delta there exactly 0, all finite
    with np.errstate(over="ignore"):
        f32 = m.forward(vc.f32_params(params), x)
        _, g32 = m.loss_and_grads(vc.f32_params(params), x, y, a, vc.BETA)
    s32 = np.concatenate([f32["sx"], f32["sy"]], axis=1)
    assert s32.dtype == np.float32 and np.any(s32 == 0.0) and np.any(s32 == 1.0)
    assert not np.any(g32["dz"][(s32 == 0.0) | (s32 == 1.0)])
    assert all(np.all(np.isfinite(g32[k])) for k in g32)
    worst = max(np.max(np.abs(np.asarray(g32[k], np.float64) - g[k])) / np.max(np.abs(g[k])) for k in DELTAS + m.PARAM_ORDER)
    print("saturated S=%d A=%d: the float32 oracle's largest e32 is %.2e" % (S, A, worst))
    assert worst < 2e-5             # seen: 1.0e-5 and 9.5e-6; a fixture whose e32 drifts up would empty the bound 16 x e32


def _fd_indices(params, rng):
    return [(k, tuple(rng.integers(0, s) for s in params[k].shape)) for k in m.PARAM_ORDER for _ in range(3)]


@pytest.mark.parametrize("state_dim,num_actions", [(64, 32), (1, 32)])
def test_oracle_matches_central_differences_at_the_limits(state_dim, num_actions):
    S, A = state_dim, num_actions
    params = {k: v.copy() for k, v in vc.limit_params(S, A).items()}
    x, y, a = vc.f64(*vc.batch(params, FD_ROWS, S, A, 100 + FD_ROWS))
    adv = y - m.forward(params, x)["v"]
    _, g = m.loss_and_grads(params, x, y, a, FD_BETA)
    for k, idx in _fd_indices(params, np.random.default_rng(0)):
        save = params[k][idx]
        vals = []
        for step in (EPS, -EPS):
            params[k][idx] = save + step
            losses, _ = m.loss_and_grads(params, x, y, a, FD_BETA, adv_const=adv)
            vals.append(losses["cost_all"])
        params[k][idx] = save
        fd = (vals[0] - vals[1]) / (2 * EPS)
        assert abs(fd - g[k][idx]) < FD_TOL * max(1.0, abs(fd)), (k, idx, fd, g[k][idx])


def test_each_cost_matches_central_differences_at_the_limits():
    S, A = 64, 32
    params = {k: v.copy() for k, v in vc.limit_params(S, A).items()}
    x, y, a = vc.f64(*vc.batch(params, FD_ROWS, S, A, 100 + FD_ROWS))
    adv = y - m.forward(params, x)["v"]
    _, gp, gv = d.dual_grads(params, x, y, a, FD_BETA)
    for k in d.HEAD_V:
        assert not np.any(gp[k])
    for k in d.HEAD_P:
        assert not np.any(gv[k])
    for k, idx in _fd_indices(params, np.random.default_rng(0)):
        save = params[k][idx]
        vals = []
        for step in (EPS, -EPS):
            params[k][idx] = save + step
            losses, _ = m.loss_and_grads(params, x, y, a, FD_BETA, adv_const=adv)
            vals.append((-(losses["cost_p_1_agg"] + losses["cost_p_2_agg"]), losses["cost_v"]))
        params[k][idx] = save
        for c, g in enumerate((gp, gv)):
            fd = (vals[0][c] - vals[1][c]) / (2 * EPS)
            assert abs(fd - g[k][idx]) < FD_TOL * max(1.0, abs(fd)), (k, idx, c, fd, g[k][idx])
