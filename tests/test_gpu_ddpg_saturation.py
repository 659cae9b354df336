"""-m gpu: the DDPG handle's kernels (ga3c_ddpg.hip) where the other files of this handle do not take them: saturated tanh units of
the actor, a one-hot softmax of the atom head, and the largest and smallest shapes ga3c_ddpg_create admits.  The cases and what
makes them worth running are tests/ddpg_saturation_cases.py's and asserted on the oracle alone in test_ddpg_saturation_cpu.py;
the comparators are the other files', imported: 1e-4 x max(1, max|want|) per row tensor (test_gpu_ddpg._check) and closeness.py's
relative error per tensor with its bound from the float32 oracle.  B = 17 everywhere (a tile and one row), max_batch 32, a ring
of 64 rows; a case is one compute(..., 4) and its fetches.

What is new is element-wise, because a saturated unit's delta is far below its tensor's largest entry and no per-tensor norm
looks at it:
  * the actor's 1 - tanh^2, read back as r = -do / g per unit and held to 1 / cosh(h)^2 of the float64 oracle within
    exp(2 dh) - 1 + 2^-20 (ddpg_saturation_cases.dtanh_bound: dh is 16 x the float32 oracle's largest error of h);
  * the cross-entropy per row, within max(16 x e_row, 2^-20) of itself, e_row the float32 oracle's largest per-row error;
  * finiteness, signs and row sums of the head's rows on the fetched values.
No bound here is a literal: each is computed from the float32 and float64 runs of the oracle with closeness.py's 16 and 2^-20.

`pytest -s` prints every comparison, and per test the largest rel_err / bound it saw."""
import numpy as np
import pytest

import closeness as cl
import ddpg_oracle as o
import ddpg_saturation_cases as sc
import td3_oracle as t3
from test_gpu_ddpg import WTOL, _check, _compare_step4, _load, _net
from test_gpu_dist import DIST_FETCH, _args, _dnet, _single_draws as _dist_draws
from test_gpu_td3 import _check_eps, _load as _tload, _single_draws as _twin_draws, _tnet

pytestmark = pytest.mark.gpu

B = sc.B
MAXB, CAP = 32, 64


class _Relative:
    """closeness.py's comparison of a list of tensors, as test_gpu_ddpg.test_backward_tensors_relative_to_their_largest_entry
    makes it: every line printed, the failures collected, the worst rel_err / bound kept."""

    def __init__(self, label):
        self.label, self.failed, self.worst = label, [], (0.0, None)

    def hold(self, name, got, ref, ref32, draw=None):
        assert np.asarray(ref32).dtype == np.float32, name
        e32 = max(cl.rel_err(ref32, ref), draw or 0.0)
        err = cl.report(self.label, name, got, ref, e32, cl.bound(e32))
        if not err <= cl.bound(e32):
            self.failed.append((name, err, cl.bound(e32)))
        self.worst = max(self.worst, (err / cl.bound(e32), name))

    def done(self):
        print("%s: worst rel_err / bound %.2f (%s)" % ((self.label,) + self.worst))
        assert not self.failed, self.failed


def _scalar_tensors(out):
    fc, fa = out["critic_fwd"], out["actor_fwd"]
    t = {"dq": out["dq"], "c_dt": fc["dt"], "c_dn1": fc["dn1"], "g": out["g"], "do": fa["do"], "a_dn2": fa["dn2"], "a_dn1": fa["dn1"]}
    t.update({"grad " + k: out["critic_grads"][k] for k in o.CRITIC_TRAINABLE if k != o.DEAD})
    t.update({"grad " + k: out["actor_grads"][k] for k in o.ACTOR_TRAINABLE})
    return t


def _scalar_step(net, c, label):
    """test_gpu_ddpg.test_every_intermediate_and_gradient's comparison and the relative one, on the case's step."""
    _load(net, c.online, c.target)
    q_max, q_avg = net.compute(*_args(c.batch), 4, noise=c.noise)
    _check("q_max", [q_max], [c.out["q_max"]])
    _check("q_avg", [q_avg], [c.out["q_avg"]])
    _compare_step4(net, c.out, c.S, c.A, B)
    for k in o.CRITIC_TRAINABLE:
        _check("after step 3 " + k, net.get_variable_value(k, 0), c.st["online"][k], WTOL)
    assert net.get_global_step() == 0
    rel = _Relative(label)
    want, w32 = _scalar_tensors(c.out), _scalar_tensors(c.w32)
    for name, ref in want.items():
        got = net.get_variable_value(name[5:], 4) if name.startswith("grad ") else net.fetch(name, np.size(ref))
        rel.hold(name, got, ref, w32[name])
    rel.done()


def _dist_step(net, c, label):
    """test_gpu_dist.test_every_row_and_gradient's rows and gradients on the case's step -> the fetched head rows."""
    S, A, N, out, w32 = c.S, c.A, c.N, c.out, c.w32
    assert net.dist_info() == (N, c.vmin, c.vmax)
    _load(net, c.online, c.target)
    q_max, q_avg = net.compute(*_args(c.batch), 4, noise=c.noise)
    _check("q_max", [q_max], [out["q_max"]])
    _check("q_avg", [q_avg], [out["q_avg"]])
    fc, fa = out["critic_fwd"], out["actor_fwd"]
    rows = [("y", out["y"]), ("qt", out["qt"]), ("d_pt", out["pt"]), ("d_m", out["m"]), ("d_p", out["p"]), ("d_dz", out["dz"]),
            ("d_ce", out["ce"]), ("q", out["q"]), ("c_x", c.batch[0]), ("c_a", c.batch[1]), ("c_xh1", fc["xh1"]), ("c_c1", fc["c1"]),
            ("c_c2", fc["c2"]), ("c_dt", fc["dt"]), ("c_dn1", fc["dn1"]), ("c_dh1", fc["dh1"]),
            ("a_xh1", fa["xh1"]), ("a_a1", fa["a1"]), ("a_xh2", fa["xh2"]), ("a_a2", fa["a2"]), ("a_out", fa["out"]),
            ("a_noisy", out["a_out"]), ("g", out["g"]), ("do", fa["do"]), ("a_dn2", fa["dn2"]), ("a_dn1", fa["dn1"])]
    got = {}
    for name, want in rows:
        got[name] = net.fetch(name, np.size(want))
        _check(name, got[name], want)
    rel = _Relative(label)
    draws = _dist_draws(S, A, B, N, c.online, c.target, out, w32, c.kw)
    for k in o.CRITIC_TRAINABLE:
        grad = net.get_variable_value(k, 4)
        _check("grad " + k, grad, out["critic_grads"][k])
        if k != o.DEAD:
            rel.hold("grad " + k, grad, out["critic_grads"][k], w32["critic_grads"][k], draws[k])
    rel.hold("g", got["g"], out["g"], w32["g"])
    for k in o.ACTOR_TRAINABLE:
        _check("grad " + k, net.get_variable_value(k, 4), out["actor_grads"][k])
    rel.done()
    for k in o.CRITIC_TRAINABLE:
        _check("after step 3 " + k, net.get_variable_value(k, 0), c.st["online"][k], WTOL)
    assert net.get_global_step() == 0
    return got


# ---- 1. saturated units of the actor's output

@pytest.mark.parametrize("S,A,k", sc.ACTOR_CASES)
def test_saturated_actor_delta_unit_by_unit(S, A, k):
    c = sc.actor(S, A, k)
    ho = c.out["actor_fwd"]["ho"]
    dh, bound = sc.dtanh_bound(c.w32["actor_fwd"]["ho"], ho)
    net = _net(S, A, max_batch=MAXB, capacity=CAP)
    try:
        _scalar_step(net, c, "saturated actor S=%d A=%d k=%d" % (S, A, k))
        do, g = net.fetch("do", B * A).astype(np.float64), net.fetch("g", B * A).astype(np.float64)
        keep = g != 0
        assert keep.all(), "the oracle's g has no zero"
        err = sc.dtanh_err(-do[keep] / g[keep], ho.reshape(-1)[keep])
        print("saturated actor S=%d A=%d k=%d: max|h| %.1f  max|r / want - 1| %.3e  dh %.3e  bound %.3e  err/bound %.3f"
              % (S, A, k, np.abs(ho).max(), err, dh, bound, err / bound))
        assert err <= bound
        assert np.all(np.abs(net.fetch("a_out", B * A)) <= 1.0)
    finally:
        net.close()


# ---- 2. a saturated target actor under the twin's smoothing

def test_saturated_target_actor_under_smoothing_noise():
    S, A, k = sc.TWIN_CASE
    c = sc.twin(S, A, k)
    net = _tnet(S, A, delay=1, sigma=sc.TWIN["sigma"], c=sc.TWIN["noise_clip"], max_batch=MAXB, capacity=CAP)
    try:
        _tload(net, c.online, c.target)
        net.compute(*_args(c.batch), 4, noise=c.noise)
        eps = _check_eps(net, 1, B, A, sc.TWIN["sigma"], sc.TWIN["noise_clip"])
        _, out, _ = sc.twin_step(c, eps)
        at_clip = np.abs(out["t_a"]) == 1.0
        print("t_a: %d of %d entries at +-1" % (int(at_clip.sum()), at_clip.size))
        assert at_clip.any() and not at_clip.all()
        for name in ("t_eps", "t_a", "qt1", "qt2", "y"):
            _check(name, net.fetch(name, np.size(out[name])), out[name])
        assert np.all(np.abs(net.fetch("t_a", B * A)) <= 1.0)
    finally:
        net.close()


# ---- 3. a one-hot softmax of the atom head

def _head_rows_are_sane(got, N):
    for name in DIST_FETCH + ("q", "y", "qt", "g", "do"):
        assert np.all(np.isfinite(got[name])), name
    m, p = got["d_m"].reshape(B, N).astype(np.float64), got["d_p"].reshape(B, N).astype(np.float64)
    assert np.all(got["d_ce"] >= 0.0) and np.all(p >= 0.0) and np.all(m >= 0.0)
    assert np.max(np.abs(m.sum(axis=1) - 1.0)) <= 1e-5 and np.max(np.abs(p.sum(axis=1) - 1.0)) <= 1e-5


@pytest.mark.parametrize("S,A,N,k", sc.DIST_CASES)
def test_saturated_atom_head_rows_gradients_and_cross_entropy(S, A, N, k):
    c = sc.dist(S, A, N, k)
    label = "saturated head S=%d A=%d N=%d k=%d" % (S, A, N, k)
    net = _dnet(S, A, N, max_batch=MAXB, capacity=CAP)
    try:
        got = _dist_step(net, c, label)
        _head_rows_are_sane(got, N)
        zero = (got["d_p"].reshape(B, N) == 0).any(axis=1)
        print("%s: p has a zero in %d of %d fetched rows, max p %.7f, ce up to %.1f"
              % (label, int(zero.sum()), B, got["d_p"].max(), got["d_ce"].max()))
        e_row, bound = sc.ce_bound(c.w32["ce"], c.out["ce"])
        ce = c.out["ce"]
        err = float(np.max(np.abs(got["d_ce"].astype(np.float64) - ce) / np.abs(ce)))
        print("%s: ce per row rel_err %.3e  e_row %.3e  bound %.3e  err/bound %.3f" % (label, err, e_row, bound, err / bound))
        assert np.all(np.abs(got["d_ce"].astype(np.float64) - ce) <= bound * np.abs(ce))
    finally:
        net.close()


# ---- 4. the shapes ga3c_ddpg_create admits, at both ends (what it refuses beyond them: test_gpu_ddpg_host.py)

@pytest.mark.parametrize("S,A", sc.LIMITS)
def test_scalar_handle_at_the_shape_limits(S, A):
    c = sc.actor(S, A)
    s, a, r, done, s2 = c.batch
    net = _net(S, A, max_batch=MAXB, capacity=CAP)
    try:
        _scalar_step(net, c, "limits S=%d A=%d" % (S, A))
        _check("predict", net.predict(s2, noise=False), o.actor_forward(c.online, s2)["out"])      # compute(4) left the actor alone
        # the ring's rows of 2 S + A + 2 floats: first and last slot written, bit for bit
        assert net.replay_add(s, a, r, done, s2) == (B, B)
        for slot in (0, B - 1):
            row = net.replay_get(slot)
            assert all(np.array_equal(x, w[slot]) for x, w in zip(row, c.batch)), "slot %d" % slot
    finally:
        net.close()


@pytest.mark.parametrize("S,A", sc.LIMITS)
def test_twin_handle_at_the_shape_limits(S, A):
    c = sc.twin(S, A)
    net = _tnet(S, A, delay=1, sigma=sc.TWIN["sigma"], c=sc.TWIN["noise_clip"], max_batch=MAXB, capacity=CAP)
    try:
        _tload(net, c.online, c.target)
        net.compute(*_args(c.batch), 4, noise=c.noise)
        eps = _check_eps(net, 1, B, A, sc.TWIN["sigma"], sc.TWIN["noise_clip"])        # j = k A + i up to 17 x 32
        _, out, w32 = sc.twin_step(c, eps)
        for name in ("t_eps", "t_a", "qt1", "qt2", "qt", "y", "q", "q2", "g", "do"):
            want = out["actor_fwd"]["do"] if name == "do" else out[name]
            _check(name, net.fetch(name, np.size(want)), want)
        rel = _Relative("limits twin S=%d A=%d" % (S, A))
        draws = _twin_draws(S, A, B, c.online, c.target, c.batch, eps, out, w32)
        for pre, tag in (("critic_", "critic_grads"), ("critic2_", "critic2_grads")):
            for k in o.CRITIC_TRAINABLE:
                name = pre + k[len("critic_"):]
                got = net.get_variable_value(name, 4)
                _check("grad " + name, got, out[tag][k])
                if k != o.DEAD:
                    rel.hold("grad " + name, got, out[tag][k], w32[tag][k], draws[tag][k])
        rel.done()
        for k in o.ACTOR_TRAINABLE:
            _check("grad " + k, net.get_variable_value(k, 4), out["actor_grads"][k])
        assert len(net.get_variables_names()) == len(t3.ALL_VARS)
    finally:
        net.close()


@pytest.mark.parametrize("S,A", sc.LIMITS)
def test_distributional_handle_at_the_shape_limits(S, A):
    """N = 64 with S = 64: ddpg_dist_critic_kernel lays the tile's m [64][16] over the whole LDS buffer of the states."""
    N = sc.LIMIT_ATOMS
    c = sc.dist(S, A, N)
    net = _dnet(S, A, N, max_batch=MAXB, capacity=CAP)
    try:
        _head_rows_are_sane(_dist_step(net, c, "limits dist S=%d A=%d N=%d" % (S, A, N)), N)
    finally:
        net.close()
