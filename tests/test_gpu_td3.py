"""-m gpu: the DDPG handle's twin step (ga3c_ddpg_twin_create, Config.DDPG_TWIN) against its f64 statement
(tests/td3_oracle.py).

Tolerances are tests/test_gpu_ddpg.py's: 1e-4 x max(1, max|want|) on rows, 1e-5 on weights and optimizer slots after steps,
tests/closeness.py's relative error per gradient tensor (with its rule for tensors whose f32 error is a single draw,
_single_draws).  As there, a relu unit within 1e-4 of zero in the oracle could land on
the other side in f32, so rows with such a unit in any of the six evaluations of a twin step (td3_oracle.relu_margin) are left
out: 4 B candidate rows are drawn, the first B that qualify are kept, and the test asserts it found B.  The smoothing noise of a
row depends on its place in the batch, so a row that fails gives its place to the next candidate (_select).  The min and the
clips are continuous and need no margin.  The oracle is fed the noise the device drew (fetched "t_eps"), which is held to numpy's draw separately: 1e-6
absolute, since log, sqrt and cos are the device library's."""
import numpy as np
import pytest

import ddpg_oracle as o
import per_oracle as per
import td3_oracle as t3
from test_gpu_ddpg import LR, WTOL, _candidates, _cfg_kw, _check, _f64, _net

pytestmark = pytest.mark.gpu

SHAPES = [(3, 1), (7, 3)]
SIZES = [1, 15, 16, 17, 33, 132]
SEED = 12345                      # Config.RANDOM_SEED, which NetworkDDPG hands to twin_create
EINVAL, ESTATE = -1, -4
NEW_FETCH = ("qt1", "qt2", "t_eps", "t_a", "q2", "dq2", "c2_xh1", "c2_c1", "c2_dn1", "c2_dh1", "c2_c2", "c2_dt")


def _tnet(S, A, delay=2, sigma=0.2, c=0.5, max_batch=160, capacity=512, **kw):
    kw.setdefault("DDPG_CRITIC_LOSS", "paired")
    return _net(S, A, max_batch=max_batch, capacity=capacity, DDPG_TWIN=True, DDPG_POLICY_DELAY=delay, DDPG_TARGET_NOISE=sigma,
                DDPG_TARGET_NOISE_CLIP=c, RANDOM_SEED=SEED, **kw)


def _okw(cfg):
    """Config settings -> td3_oracle.train_step's keyword arguments."""
    return {k: v for k, v in _cfg_kw(cfg).items() if k != "form"}


def _load(net, online, target):
    for k in t3.ALL_VARS:
        net.set_variable_value(k, online[k], 0)
        net.set_variable_value(k, target[k], 1)


def _copy_state(st):
    return dict(st, online={k: v.copy() for k, v in st["online"].items()}, target=dict(st["target"]),
                slot_a={k: v.copy() for k, v in st["slot_a"].items()}, slot_b={k: v.copy() for k, v in st["slot_b"].items()})


def _select(st, cand, B, noise, tw, **kw):
    """B of the 4 B candidate rows, taken in order, that keep every relu unit of the step's six evaluations 1e-4 away from zero
    under the smoothing noise of their place in the batch, and, on a policy step, the units of critic 1's second layer where
    step 4 evaluates it after step 3 (test_gpu_ddpg._select's rule).  A row that fails is replaced in its place by the next
    candidate not yet tried, so the others keep their places and their noise; every candidate is tried once."""
    n, A = cand[1].shape
    assert n == 4 * B
    t = st["step"] + 1
    eps = t3.smoothing_noise(SEED, t, B, A, tw["sigma"], tw["noise_clip"])
    nz = 0.0 if noise is None else np.asarray(noise, np.float64)[None, :]
    place, tried = np.full(B, -1), 0
    for _ in range(60):
        need = np.flatnonzero(place < 0)
        assert tried + need.size <= n, "only %d of %d candidate rows qualify" % (B - need.size, n)
        place[need] = np.arange(tried, tried + need.size)
        tried += need.size
        rows = _f64(tuple(c[place] for c in cand))
        bad = t3.relu_margin(st["online"], st["target"], rows[0], rows[1], rows[4], eps) <= 1e-4
        if not bad.any() and t % tw["policy_delay"] == 0:
            trial = _copy_state(st)
            t3.train_step(trial, *rows, LR, None, eps=eps, stop_after=3, **tw, **kw)
            a_out = o.actor_forward(trial["online"], rows[0])["out"] + nz
            bad = np.abs(o.critic_forward(trial["online"], rows[0], a_out)["t"]).min(axis=1) <= 1e-4
        if not bad.any():
            print("rows: %d of the first %d candidates qualify" % (B, tried))
            return tuple(c[place] for c in cand)
        place[bad] = -1
    raise AssertionError("the choice of rows did not settle")


def _case(S, A, B, seed, tw, stats=False, noise=None, **kw):
    rng = np.random.Generator(np.random.PCG64(seed))
    online, target = t3.random_params(S, A, rng, stats=stats), t3.random_params(S, A, rng, stats=stats)
    st = t3.new_state(online, target, critic_rmsprop=kw.get("critic_rmsprop", True))
    return online, target, _select(st, _candidates(S, A, 4 * B, rng), B, noise, tw, **kw)


def _args(b):
    return b[0], b[2], b[1], b[4], b[3]          # Network.train's order: x, y_r, a, x2, done


def _check_eps(net, t, B, A, sigma, c):
    """-> the device's smoothing noise of step t, held to numpy's draw."""
    eps = net.fetch("t_eps", B * A).reshape(B, A)
    want = t3.smoothing_noise(SEED, t, B, A, sigma, c)
    err = float(np.max(np.abs(eps.astype(np.float64) - want)))
    print("t_eps: max |device - numpy| %.3e, %d of %d at the clip" % (err, int((np.abs(want) == np.float32(c)).sum()), want.size))
    assert err <= 1e-6 and np.all(np.abs(eps) <= np.float32(c))
    return eps


# ---- 1. one step, every row

def _single_draws(S, A, B, online, target, batch, eps, out, w32):
    """-> {critic tag: {variable: e32 or None}}: what replaces closeness.py's e32 where rel_err(g32, g64) is a SINGLE draw of
    the rounding error and 16 x it says nothing (closeness.e32_of_row_sum has the argument).  Everything here is the oracle's.
      * critic_output/b has one element, the sum of dq over the rows: closeness.e32_of_row_sum(dq32, dq64).
      * At B = 1 every gradient tensor is that one row's dq = 2 (q - y) times factors that carry no cancellation, so its
        relative error is dq's, and dq's is one draw of (error of q + error of y) / |q - y|.  What f32 costs q and y in some
        summation order is taken from many rows instead of one: the largest |q32 - q64| and |y32 - y64| of the oracle over 64
        rows drawn like the candidates, each under the noise of place 0.  e32 = (E_q + E_y) / |q - y| of the row.
    The caller takes the larger of this and the single draw."""
    import closeness as cl
    e = {}
    if B == 1:
        rng = np.random.Generator(np.random.PCG64(7))
        s, a, r, done, s2 = _candidates(S, A, 64, rng)
        e0 = np.repeat(eps[:1], 64, axis=0)
        f32 = lambda P: {k: v.astype(np.float32) for k, v in P.items()}     # noqa: E731
        y64 = t3.targets(target, *_f64((s2, r, done)), 0.99, e0)[0]
        y32 = t3.targets(f32(target), s2, r, done, 0.99, e0)[0]
        assert y32.dtype == np.float32
        e_y = float(np.max(np.abs(y32 - y64)))
    for tag, view in (("critic_grads", lambda P: P), ("critic2_grads", t3.critic2)):
        q_name, dq_name = ("q", "dq") if tag == "critic_grads" else ("q2", "dq2")
        e[tag] = {k: None for k in o.CRITIC_TRAINABLE}
        e[tag]["critic_output/b"] = cl.e32_of_row_sum(w32[dq_name], out[dq_name]) if B > 1 else None
        if B == 1:
            q64 = o.critic_forward(view(online), *_f64((s, a)))["q"][:, 0]
            q32 = o.critic_forward(view(f32(online)), s, a)["q"][:, 0]
            e_dq = (float(np.max(np.abs(q32 - q64))) + e_y) / abs(float(out[q_name][0] - out["y"][0]))
            print("B = 1, %s: E_q %.3e E_y %.3e |q - y| %.3e -> e32 %.3e" % (q_name, np.max(np.abs(q32 - q64)), e_y,
                                                                             abs(out[q_name][0] - out["y"][0]), e_dq))
            e[tag] = {k: e_dq for k in o.CRITIC_TRAINABLE}
    return e


def _every_row(S, A, B, sigma, c):
    import closeness as cl
    tw = dict(policy_delay=1, sigma=sigma, noise_clip=c)
    noise = np.linspace(-0.2, 0.3, A).astype(np.float32)
    online, target, batch = _case(S, A, B, 300 + B + S, tw, stats=True, noise=noise)
    net = _tnet(S, A, delay=1, sigma=sigma, c=c)
    try:
        _load(net, online, target)
        q_max, q_avg = net.compute(*_args(batch), 4, noise=noise)
        eps = _check_eps(net, 1, B, A, sigma, c)
        if sigma == 0:
            assert not eps.any()
        st = t3.new_state(online, target)
        out = t3.train_step(st, *_f64(batch), LR, noise.astype(np.float64), eps=eps, stop_after=4, **tw)
        f32 = lambda P: {k: v.astype(np.float32) for k, v in P.items()}     # noqa: E731
        w32 = t3.train_step(t3.new_state(f32(online), f32(target)), *batch, LR, noise, eps=eps, stop_after=4, **tw)
        clipped = np.abs(o.actor_forward(target, batch[4])["out"] + eps) > 1
        print("target action: %d of %d entries clipped to the unit box" % (int(clipped.sum()), clipped.size))
        _check("q_max", [q_max], [out["q_max"]])
        _check("q_avg", [q_avg], [out["q_avg"]])
        f1, f2, fa = out["critic_fwd"], out["critic2_fwd"], out["actor_fwd"]
        rows = [("y", out["y"]), ("qt", out["qt"]), ("qt1", out["qt1"]), ("qt2", out["qt2"]), ("t_a", out["t_a"]),
                ("q", out["q"]), ("dq", out["dq"]), ("c_xh1", f1["xh1"]), ("c_c1", f1["c1"]), ("c_c2", f1["c2"]), ("c_dt", f1["dt"]),
                ("c_dn1", f1["dn1"]), ("q2", out["q2"]), ("dq2", out["dq2"]), ("c2_xh1", f2["xh1"]), ("c2_c1", f2["c1"]),
                ("c2_c2", f2["c2"]), ("c2_dt", f2["dt"]), ("c2_dn1", f2["dn1"]),
                ("c2_dh1", f2["dn1"] * (online["critic2_norm1/gamma"] * f2["rs1"])),
                ("a_xh1", fa["xh1"]), ("a_a1", fa["a1"]), ("a_xh2", fa["xh2"]), ("a_a2", fa["a2"]), ("a_out", fa["out"]),
                ("a_noisy", out["a_out"]), ("g", out["g"]), ("do", fa["do"]), ("a_dn2", fa["dn2"]), ("a_dn1", fa["dn1"])]
        for name, want in rows:
            _check(name, net.fetch(name, np.size(want)), want)
        assert np.array_equal(net.fetch("qt", B), np.minimum(net.fetch("qt1", B), net.fetch("qt2", B)))
        failed = []
        draws = _single_draws(S, A, B, online, target, batch, eps, out, w32)
        for pre, tag in (("critic_", "critic_grads"), ("critic2_", "critic2_grads")):
            for k in o.CRITIC_TRAINABLE:
                name = pre + k[len("critic_"):]
                got = net.get_variable_value(name, 4)
                _check("grad " + name, got, out[tag][k])
                if k != o.DEAD:
                    assert w32[tag][k].dtype == np.float32
                    e32 = max(cl.rel_err(w32[tag][k], out[tag][k]), draws[tag][k] or 0.0)
                    err = cl.report("td3 S=%d A=%d B=%d" % (S, A, B), "grad " + name, got, out[tag][k], e32, cl.bound(e32))
                    if not err <= cl.bound(e32):
                        failed.append((name, err, cl.bound(e32)))
        for k in o.ACTOR_TRAINABLE:
            _check("grad " + k, net.get_variable_value(k, 4), out["actor_grads"][k])
        assert not failed, failed
        for k in o.CRITIC_TRAINABLE + t3.CRITIC2_TRAINABLE:
            _check("after step 3 " + k, net.get_variable_value(k, 0), st["online"][k], WTOL)
        assert net.get_global_step() == 0
    finally:
        net.close()


@pytest.mark.parametrize("S,A", SHAPES)
@pytest.mark.parametrize("B", SIZES)
def test_every_row_and_both_critics_gradients(S, A, B):
    _every_row(S, A, B, 0.2, 0.5)


@pytest.mark.parametrize("S,A", SHAPES)
@pytest.mark.parametrize("B", [17, 132])
@pytest.mark.parametrize("sigma,c", [(1.0, 0.3), (0.0, 0.5)], ids=["clip-bites", "sigma0"])
def test_every_row_with_a_biting_noise_clip_and_without_noise(S, A, B, sigma, c):
    _every_row(S, A, B, sigma, c)


# ---- 2. production steps

def _snapshot(net, names=t3.TRAINABLE):
    return {(k, w): net.get_variable_value(k, w) for k in names for w in (0, 1, 2, 3)}


def _same(a, b):
    return all(np.array_equal(a[k], b[k]) for k in a)


WAYS = [dict(), dict(RMSPROP_MOMENTUM=0.9), dict(USE_GRAD_CLIP=True), dict(RMSPROP=False)]


def _adam_shift(m, v, g, e_g, lr, t):
    """How far Adam's step on an element moves when its gradient moves by e_g either way (ddpg_oracle.adam_step's formula)."""
    lr_t = lr * np.sqrt(1.0 - o.ADAM_B2 ** t) / (1.0 - o.ADAM_B1 ** t)

    def step(gg):
        return lr_t * (m + (gg - m) * (1.0 - o.ADAM_B1)) / (np.sqrt(v + (gg * gg - v) * (1.0 - o.ADAM_B2)) + o.ADAM_EPS)

    return np.maximum(np.abs(step(g + e_g) - step(g)), np.abs(step(g - e_g) - step(g)))


def _abs_terms(P, f):
    """Per element of a critic's gradients (ddpg_oracle.critic_grads' forward dict f) the sum over the rows of the magnitudes
    of its terms: what a rounding error of the sum is relative to.  Zero where a unit is off in every row."""
    dq, dt, dn1 = np.abs(f["dq"])[:, None], np.abs(f["dt"]), np.abs(f["dn1"])
    dh1 = dn1 * np.abs(P["critic_norm1/gamma"] * f["rs1"])
    return {"critic_output/W": np.abs(f["c2"]).T @ dq, "critic_output/b": dq.sum(0), "critic_fc2/W": np.abs(f["c1"]).T @ dt,
            "critic_norm2/W": np.abs(f["a"]).T @ dt, "critic_norm2/b": dt.sum(0), "critic_norm1/beta": dn1.sum(0),
            "critic_norm1/gamma": (dn1 * np.abs(f["xh1"])).sum(0), "critic_fc1/W": np.abs(f["x"]).T @ dh1, "critic_fc1/b": dh1.sum(0)}


class _AdamCondition:
    """Which elements of an Adam critic's weights can be held to 1e-5 at all.  Adam's step is lr_t m / (sqrt(v) + 1e-8): on an
    element whose gradient is some 1e-6 or less (a sum over the rows that cancels) the 1e-8 decides the quotient, and the
    step, up to 3.2 lr_t = 1e-2 here, follows the gradient's RELATIVE error, which f32 does not keep for such a sum: the f32
    oracle itself is 9e-6 off the f64 one after one step of this test.  RMSProp divides by sqrt(0.1 + ms) and has no such
    element.  A condition, not a tolerance (as closeness.signed_or_magnitude's): an element is left out of the comparison of
    the online weights only if, in the oracle, its step moves by more than 1e-5 / 4 (four steps) when its gradient moves by
    bound(e32) x the sum of the magnitudes of its terms (_abs_terms), bound and e32 closeness.py's for its tensor, from the
    f32 oracle on the same rows; such elements must be at most 0.1 % of their tensor (or one) and stay within what four Adam
    steps can differ by at all.  Slots and targets are compared whole."""

    def __init__(self, st, st32):
        self.st, self.st32 = st, st32
        self.names = [k for k in o.CRITIC_TRAINABLE + t3.CRITIC2_TRAINABLE if k not in (o.DEAD, t3.DEAD2)]
        self.shaky = {k: np.zeros(st["online"][k].shape, bool) for k in self.names}

    def before(self):
        self.slots = {k: (self.st["slot_a"][k].copy(), self.st["slot_b"][k].copy()) for k in self.names}
        self.weights = {k: self.st["online"][k].copy() for k in o.ALL_VARS + t3.CRITIC2_TRAINABLE + t3.CRITIC2_STATS}

    def after(self, out, out32, lr, t):
        import closeness as cl
        for k in self.names:
            tag, kk = ("critic2_grads", "critic_" + k[len("critic2_"):]) if k.startswith("critic2_") else ("critic_grads", k)
            g = out[tag][kk].reshape(self.shaky[k].shape)
            P = t3.critic2(self.weights) if k.startswith("critic2_") else self.weights
            terms = _abs_terms(P, out[tag.replace("grads", "fwd")])[kk].reshape(g.shape)
            e_g = cl.bound(cl.rel_err(out32[tag][kk], g)) * terms
            self.shaky[k] |= _adam_shift(*self.slots[k], g, e_g, lr, t) > WTOL / 4

    def check(self, k, got, want, lr):
        keep = ~self.shaky[k]
        out = int((~keep).sum())
        print("%-28s %d of %d elements too small for Adam's quotient" % (k, out, keep.size))
        assert out <= max(1, keep.size // 1000), "%s: %d of %d elements" % (k, out, keep.size)
        _check("online " + k, got[keep], want[keep], WTOL)
        if not keep.all():
            assert np.max(np.abs(got[~keep] - want[~keep])) <= 4 * 2 * 3.2 * lr


@pytest.mark.parametrize("cfg", WAYS, ids=["plain", "momentum", "clip", "adam"])
@pytest.mark.parametrize("delay", [2, 3])
@pytest.mark.parametrize("S,A", SHAPES)
def test_four_production_steps(S, A, delay, cfg):
    B = 33
    tw = dict(policy_delay=delay, sigma=0.2, noise_clip=0.5)
    kw = _okw(cfg)
    noise = np.full(A, 0.05, np.float32)
    rng = np.random.Generator(np.random.PCG64(500 + S + delay))
    online, target = t3.random_params(S, A, rng), t3.random_params(S, A, rng)
    st = t3.new_state(online, target, critic_rmsprop=cfg.get("RMSPROP", True))
    adam = None
    if not cfg.get("RMSPROP", True):
        f32 = lambda P: {k: v.astype(np.float32) for k, v in P.items()}     # noqa: E731
        adam = _AdamCondition(st, t3.new_state(f32(online), f32(target), critic_rmsprop=False))
    net = _tnet(S, A, delay=delay, **cfg)
    try:
        _load(net, online, target)
        assert len(net.get_variables_names()) == 38
        for step in range(1, 5):
            b = _select(st, _candidates(S, A, 4 * B, rng), B, noise, tw, **kw)
            actor_and_targets = {(k, w): net.get_variable_value(k, w) for k in t3.TRAINABLE for w in (1,)}
            actor_and_targets.update({(k, w): net.get_variable_value(k, w) for k in o.ACTOR_TRAINABLE for w in (0, 2, 3)})
            q_max, q_avg = net.train(*_args(b), noise=noise)
            eps = _check_eps(net, step, B, A, 0.2, 0.5)
            if adam:
                adam.before()
            out = t3.train_step(st, *_f64(b), LR, noise.astype(np.float64), eps=eps, **tw, **kw)
            if adam:
                adam.after(out, t3.train_step(adam.st32, *b, LR, noise, eps=eps, **tw, **kw), 10.0 * LR, step)
            _check("step %d q_max" % step, [q_max], [out["q_max"]])
            _check("step %d q_avg" % step, [q_avg], [out["q_avg"]])
            unchanged = all(np.array_equal(v, net.get_variable_value(k, w)) for (k, w), v in actor_and_targets.items())
            assert out["policy"] == (step % delay == 0)
            assert unchanged != out["policy"], "step %d: targets and actor slots %s" % (step, "unchanged" if unchanged else "moved")
        assert net.get_global_step() == 4 and st["step"] == 4
        for k in t3.ALL_VARS:
            if adam and k in adam.shaky:
                adam.check(k, net.get_variable_value(k, 0), st["online"][k], 10.0 * LR)
            else:
                _check("online " + k, net.get_variable_value(k, 0), st["online"][k], WTOL)
            _check("target " + k, net.get_variable_value(k, 1), st["target"][k], WTOL)
        for k in t3.TRAINABLE:
            _check("slot a " + k, net.get_variable_value(k, 2), st["slot_a"][k], WTOL)
            _check("slot b " + k, net.get_variable_value(k, 3), st["slot_b"][k], WTOL)
        for k in t3.CRITIC2_STATS:          # the statistics have slots too, which nothing writes
            assert not net.get_variable_value(k, 2).any() and not net.get_variable_value(k, 3).any()
        for dead in (o.DEAD, t3.DEAD2):
            assert np.array_equal(net.get_variable_value(dead, 0), online[dead].astype(np.float32)), dead + " moved"
    finally:
        net.close()


# ---- 3. same code, same data

@pytest.mark.parametrize("cfg", [dict(), dict(USE_GRAD_CLIP=True)], ids=["plain", "clip"])
def test_critic_two_with_critic_ones_values_stays_bit_equal(cfg):
    S, A, B = 7, 3, 33
    rng = np.random.Generator(np.random.PCG64(9))
    online, target = t3.random_params(S, A, rng, stats=True), t3.random_params(S, A, rng, stats=True)
    pairs = [(k, "critic2_" + k[len("critic_"):]) for k in o.ALL_VARS if k.startswith("critic_")]
    net = _tnet(S, A, delay=2, **cfg)
    try:
        _load(net, online, target)
        for k, k2 in pairs:
            for w in (0, 1) + ((2, 3) if k in o.TRAINABLE else ()):
                net.set_variable_value(k2, net.get_variable_value(k, w), w)
        for step in range(3):
            b = _candidates(S, A, B, rng)
            net.train(*_args(b), noise=False)
            assert np.array_equal(net.fetch("qt1", B), net.fetch("qt2", B)) and np.array_equal(net.fetch("q", B), net.fetch("q2", B))
            for k, k2 in pairs:
                for w in (0, 1) + ((2, 3, 4) if k in o.TRAINABLE else ()):
                    assert np.array_equal(net.get_variable_value(k, w), net.get_variable_value(k2, w)), (step, k, w)
        assert not np.array_equal(net.get_variable_value("critic_fc1/W", 0), online["critic_fc1/W"].astype(np.float32))
    finally:
        net.close()


# ---- 4. the same calls give the same bits; train_replay is train

def test_repeated_calls_are_bit_identical_and_train_replay_is_train():
    S, A, B = 3, 1, 33
    rng = np.random.Generator(np.random.PCG64(11))
    online, target = t3.random_params(S, A, rng), t3.random_params(S, A, rng)
    s, a, r, done, s2 = _candidates(S, A, 128, rng)
    slots = np.random.default_rng(3).choice(128, B, replace=False).astype(np.int32)
    snaps = []
    for how in ("replay", "train", "replay"):
        net = _tnet(S, A)
        try:
            _load(net, online, target)
            assert net.replay_add(s, a, r, done, s2) == (128, 128)
            for _ in range(3):
                if how == "replay":
                    net.train_replay(slots, stamp=128, noise=[0.1])
                else:
                    net.train(s[slots], r[slots], a[slots], s2[slots], done[slots], noise=[0.1])
            snaps.append((_snapshot(net), net.fetch("y", B), net.fetch("t_a", B * A)))
        finally:
            net.close()
    for other in snaps[1:]:
        assert _same(snaps[0][0], other[0]) and np.array_equal(snaps[0][1], other[1]) and np.array_equal(snaps[0][2], other[2])


# ---- 5. priorities

def test_prioritized_twin_step():
    S, A, n, B = 3, 1, 128, 33
    alpha, eps_p = 0.6, 0.01
    tw = dict(policy_delay=1, sigma=0.2, noise_clip=0.5)
    noise = np.full(A, 0.05, np.float32)
    pa = np.zeros(n, np.float32)
    pa[:] = np.random.default_rng(5).uniform(0.01, 2, n).astype(np.float32) ** np.float32(0.6)
    want_slots, want_w = per.sample(pa, n, B, SEED, 0, 0.4)
    rng = np.random.Generator(np.random.PCG64(71))
    online, target = t3.random_params(S, A, rng), t3.random_params(S, A, rng)
    st = t3.new_state(online, target)
    # the batch is the draw's: choose its rows as _select does, then lay them into the ring at the drawn slots; a slot drawn
    # twice holds one row, so the rows are chosen for the distinct slots and the batch repeats them
    uniq, inverse = np.unique(want_slots, return_inverse=True)
    cand = _candidates(S, A, 4 * n, rng)
    eps = t3.smoothing_noise(SEED, 1, B, A, 0.2, 0.5)
    ok = np.ones(4 * n, bool)
    for _ in range(60):
        keep = np.flatnonzero(ok)[:uniq.size]
        assert keep.size == uniq.size
        rows = _f64(tuple(c[keep][inverse] for c in cand))
        bad = t3.relu_margin(online, target, rows[0], rows[1], rows[4], eps) <= 1e-4
        if not bad.any():
            trial = _copy_state(st)
            t3.train_step(trial, *rows, LR, None, eps=eps, per_w=want_w, stop_after=3, **tw)
            a_out = o.actor_forward(trial["online"], rows[0])["out"] + noise.astype(np.float64)[None, :]
            bad = np.abs(o.critic_forward(trial["online"], rows[0], a_out)["t"]).min(axis=1) <= 1e-4
        if not bad.any():
            break
        ok[keep[inverse[bad]]] = False
    else:
        raise AssertionError("the choice of rows did not settle")
    ring = [c[-n:].copy() for c in cand]                     # any rows; the drawn slots get the chosen ones
    for col, c in zip(ring, cand):
        col[uniq] = c[keep]
    net = _tnet(S, A, delay=1, capacity=n, PRIORITIZED_REPLAY=True, PRIORITIZED_REPLAY_ALPHA=alpha, PRIORITIZED_REPLAY_EPS=eps_p,
                REPLAY_BUFFER_RANDOM_SEED=SEED)
    try:
        _load(net, online, target)
        assert net.replay_add(*ring) == (n, n)
        net.set_priorities(pa, 0.05)
        net.replay_beta = 0.4
        net.train_prioritized(B, noise=noise)
        slots, w = net.last_slots, net.fetch("per_w", B)
        assert np.array_equal(slots, want_slots) and float(np.max(np.abs(w - want_w) / want_w)) <= 1e-6
        dev_eps = _check_eps(net, 1, B, A, 0.2, 0.5)
        batch = _f64(tuple(col[slots] for col in ring))
        out = t3.train_step(st, *batch, LR, noise.astype(np.float64), eps=dev_eps, per_w=w.astype(np.float64), **tw)
        for name in ("y", "q", "dq", "q2", "dq2"):
            _check(name, net.fetch(name, B), out[name])
        y, q, q2 = net.fetch("y", B), net.fetch("q", B), net.fetch("q2", B)
        assert np.array_equal(net.fetch("per_td", B), np.abs(y - q)), "per_td is critic 1's"
        for name, qq in (("dq", q), ("dq2", q2)):             # both critics' dq carry per_w
            plain = (2.0 / B) * (qq.astype(np.float64) - y)
            _check(name + " = per_w x the unweighted", net.fetch(name, B), w * plain)
            assert np.max(np.abs(net.fetch(name, B) - plain)) > 1e-4
        for k in t3.TRAINABLE:
            _check("online " + k, net.get_variable_value(k, 0), st["online"][k], WTOL)
            _check("target " + k, net.get_variable_value(k, 1), st["target"][k], WTOL)
        want_pa = pa.copy()
        top = per.update(want_pa, 0.05, slots, y, q, eps_p, alpha)
        got_pa, got_top = net.priorities()
        assert float(np.max(np.abs(got_pa - want_pa) / want_pa)) <= 1e-6 and abs(float(got_top) - float(top)) <= 1e-6 * float(top)
    finally:
        net.close()


# ---- 6. device actors

def test_device_actors_run_the_twin_step():
    import ddpg_actors_oracle as do
    S, A, n, B, steps, capacity = do.S, do.A, 17, 16, 6, 400
    rng = np.random.Generator(np.random.PCG64(31))
    online, target = t3.random_params(S, A, rng), t3.random_params(S, A, rng)
    net, other = (_tnet(S, A, max_batch=64, capacity=capacity) for _ in range(2))
    try:
        for h in (net, other):
            _load(h, online, target)
        net.actors_create(n, seed=5, updates=1, batch=B, draw_seed=24680)
        assert net.actors_run(1, train=True, noise=[0.3]) == (n, 0, 0, 0)         # step(None): no transition
        drawn = []
        for k in range(steps):
            stats = net.actors_run(1, train=True, noise=[0.3])
            assert stats[0] == n and stats[1] == 1
            drawn.append(net.actors_get("slots").copy())
        rows = np.array([do.pack(net.replay_get(i)) for i in range(n * steps)], np.float32).reshape(n * steps, do.ROWF)
        for k in range(steps):
            f = rows[k * n:(k + 1) * n]
            size, _ = other.replay_add(f[:, :S], f[:, S:S + A], f[:, S + A], f[:, S + A + 1], f[:, S + A + 2:])
            assert size == n * (k + 1) > B
            other.train_replay(drawn[k], noise=[0.3])
        assert net.get_global_step() == other.get_global_step() == steps
        assert len(net.get_variables_names()) == 38
        for k in t3.ALL_VARS:
            for w in (0, 1, 2, 3):
                assert np.array_equal(net.get_variable_value(k, w), other.get_variable_value(k, w)), (k, w)
    finally:
        net.close()
        other.close()


# ---- 7. return codes

def test_return_codes():
    import _native as nat
    S, A, B = 3, 1, 16
    lib = nat.hip_lib()
    plain = _net(S, A, max_batch=32, capacity=64, DDPG_CRITIC_LOSS="paired")
    fork = _net(S, A, max_batch=32, capacity=64)
    try:
        h = plain._h
        create = lib.ga3c_ddpg_twin_create
        for args in ((0, 0.2, 0.5), (17, 0.2, 0.5), (-1, 0.2, 0.5), (2, -0.1, 0.5), (2, float("nan"), 0.5), (2, 0.2, -0.5),
                     (2, 0.2, float("nan"))):
            assert create(h, args[0], args[1], args[2], 1) == EINVAL, args
        assert create(fork._h, 2, 0.2, 0.5, 1) == ESTATE
        assert lib.ga3c_ddpg_twin_destroy(h) == ESTATE
        assert len(plain.get_variables_names()) == 26 == len(plain.get_target_names())
        buf = np.zeros(B * 400 + 1, np.float32)          # the widest fetch below, and one more
        rng = np.random.default_rng(0)
        b = _candidates(S, A, B, rng)
        for _ in range(2):
            plain.train(*_args(b), noise=False)

        def refused_without_the_twin():
            for k in t3.CRITIC2_TRAINABLE + t3.CRITIC2_STATS:
                assert lib.ga3c_ddpg_get_param(h, k.encode(), 0, nat.ptr(buf), 400) == EINVAL, k
            for name in NEW_FETCH:
                assert lib.ga3c_ddpg_fetch(h, name.encode(), nat.ptr(buf), B) == ESTATE, name
            assert lib.ga3c_ddpg_fetch(h, b"nothing", nat.ptr(buf), B) == EINVAL

        refused_without_the_twin()
        before = {(k, w): plain.get_variable_value(k, w) for k in o.ALL_VARS for w in (0, 1, 2, 3)}
        assert create(h, 2, 0.2, 0.5, 1) == 0
        assert create(h, 2, 0.2, 0.5, 1) == ESTATE
        names = plain.get_variables_names()
        assert names == [k + ":0" for k in t3.ALL_VARS]
        targets = plain.get_target_names()
        assert len(targets) == 38 and targets[26] == "critic2_fc1_1/W:0" and targets[37] == "critic2_norm1_1/moving_variance:0"
        assert all(np.array_equal(v, plain.get_variable_value(k, w)) for (k, w), v in before.items()), "the 26 keep their values"
        rms = {k: plain.get_variable_value(k, 2) for k in t3.CRITIC2_TRAINABLE}
        for k in t3.CRITIC2_TRAINABLE:            # as ga3c_ddpg_create leaves the others: zero, ms one
            assert not plain.get_variable_value(k, 0).any() and not plain.get_variable_value(k, 1).any()
            assert np.all(rms[k] == 1.0) and not plain.get_variable_value(k, 3).any() and not plain.get_variable_value(k, 4).any()
            assert plain.get_variable_value(k, 0).shape == t3.shapes(S, A)[k] and plain._param_info(k)[2]
        for w in (0, 1):
            assert not plain.get_variable_value(t3.CRITIC2_STATS[0], w).any()
            assert np.all(plain.get_variable_value(t3.CRITIC2_STATS[1], w) == 1.0)
        assert not plain._param_info(t3.CRITIC2_STATS[0])[2]
        # off a policy step (t = 3 at delay 2) compute's stop_after = 4 does what 3 does: no actor row is written
        a_out = plain.fetch("a_out", B * A)
        plain.compute(*_args(_candidates(S, A, B, rng)), 4, noise=False)
        assert np.array_equal(plain.fetch("a_out", B * A), a_out) and plain.get_global_step() == 2
        widths = dict(qt1=1, qt2=1, t_eps=A, t_a=A, q2=1, dq2=1, c2_xh1=400, c2_c1=400, c2_dn1=400, c2_dh1=400, c2_c2=300, c2_dt=300)
        for name in NEW_FETCH:
            width = widths[name]
            assert lib.ga3c_ddpg_fetch(h, name.encode(), nat.ptr(buf), B * width) == 0, name
            assert lib.ga3c_ddpg_fetch(h, name.encode(), nat.ptr(buf), B * width + 1) == EINVAL, name
        before = {(k, w): plain.get_variable_value(k, w) for k in o.ALL_VARS for w in (0, 1, 2, 3)}     # (compute stepped the critic)
        assert lib.ga3c_ddpg_twin_destroy(h) == 0
        assert len(plain.get_variables_names()) == 26
        refused_without_the_twin()
        assert all(np.array_equal(v, plain.get_variable_value(k, w)) for (k, w), v in before.items())
        assert create(h, 16, 0.0, 0.0, -7) == 0       # the limits, and a fresh critic 2
        assert not plain.get_variable_value("critic2_fc1/W", 0).any() and len(plain.get_variables_names()) == 38
        plain.train(*_args(b), noise=False)
    finally:
        plain.close()             # destroys the twin with the handle
        fork.close()


# ---- 8. checkpoints

def test_checkpoint_members_round_trip_resume_and_cross_refusals(tmp_path):
    S, A, B = 3, 1, 17
    rng = np.random.Generator(np.random.PCG64(51))
    online, target = t3.random_params(S, A, rng), t3.random_params(S, A, rng)
    batches = [_candidates(S, A, B, rng) for _ in range(4)]
    path, path3, plain_path = str(tmp_path / "td3.npz"), str(tmp_path / "td3b.npz"), str(tmp_path / "ddpg.npz")
    net = _tnet(S, A, delay=2)
    try:
        _load(net, online, target)
        for b in batches[:3]:
            net.train(*_args(b), noise=False)
        net._lib.ga3c_ddpg_save(net._h, path.encode())
        three = _snapshot(net)
        net.train(*_args(batches[3]), noise=False)            # step 4: a policy step, Adam's count 2
        four = _snapshot(net)
        with np.load(path) as z:
            assert int(z["step"]) == 3
            names = set(z.files)
            for k, t in zip(net.get_variables_names(), net.get_target_names()):
                assert k in names and t in names, (k, t)
            for k in ("critic2_fc1/W:0", "critic2_fc1_1/W:0", "critic2_output_1/b:0", "critic2_fc1/W/RMSProp:0",
                      "critic2_fc2/b/RMSProp_1:0", "critic2_norm1/moving_mean:0", "critic2_norm1_1/moving_variance:0",
                      "critic_fc1/W/RMSProp:0", "actor_fc1/W/Adam_1:0"):
                assert k in names, k
            assert len(names) == 1 + 2 * 38 + 2 * 30 and "critic2_norm1/moving_mean/RMSProp:0" not in names
            assert np.array_equal(z["critic2_fc2/W:0"], three[("critic2_fc2/W", 0)])
            np.savez(path3, **{k: z[k] for k in z.files})     # through numpy and back
    finally:
        net.close()
    adam = _tnet(S, A, RMSPROP=False)
    try:
        apath = str(tmp_path / "adam.npz")
        adam._lib.ga3c_ddpg_save(adam._h, apath.encode())
        with np.load(apath) as z:
            assert "critic2_fc1/W/Adam:0" in z.files and "critic2_fc1/W/Adam_1:0" in z.files and "critic2_fc1/W/RMSProp:0" not in z.files
    finally:
        adam.close()
    fresh, plain = _tnet(S, A, delay=2), _net(S, A, max_batch=160, capacity=512, DDPG_CRITIC_LOSS="paired")
    try:
        fresh.load_file(path3)
        assert fresh.get_global_step() == 3 and _same(three, _snapshot(fresh))
        fresh.train(*_args(batches[3]), noise=False)          # resumed at step 3: the next step equals the uninterrupted run's
        assert _same(four, _snapshot(fresh))
        plain.train(*_args(batches[0]), noise=False)
        plain._lib.ga3c_ddpg_save(plain._h, plain_path.encode())
        with np.load(plain_path) as z:
            assert len(z.files) == 1 + 2 * 26 + 2 * 20 and not any(k.startswith("critic2") for k in z.files)
        # a twin handle loads only a twin handle's file, a plain handle refuses one; both stay as they were
        before_f, before_p = _snapshot(fresh), _snapshot(plain, o.TRAINABLE)
        assert fresh._lib.ga3c_ddpg_load(fresh._h, plain_path.encode()) == ESTATE
        assert plain._lib.ga3c_ddpg_load(plain._h, path.encode()) == ESTATE
        assert _same(before_f, _snapshot(fresh)) and fresh.get_global_step() == 4
        assert _same(before_p, _snapshot(plain, o.TRAINABLE)) and plain.get_global_step() == 1
        plain.load_file(plain_path)
        assert _same(before_p, _snapshot(plain, o.TRAINABLE))
    finally:
        fresh.close()
        plain.close()


# ---- 9. a Server run

@pytest.mark.timeout(120)
def test_server_trains_pendulum_with_the_twin(tmp_path, monkeypatch):
    import ga3c_amd  # noqa: F401
    from Config import Config
    monkeypatch.chdir(tmp_path)
    for k, v in (("GAME", "Pendulum-v0"), ("USE_DDPG", True), ("DDPG_TWIN", True), ("DDPG_CRITIC_LOSS", "paired"), ("AGENTS", 4),
                 ("PREDICTORS", 1), ("TRAINERS", 1), ("TIME_MAX", 5), ("DYNAMIC_SETTINGS", False), ("SAVE_MODELS", False),
                 ("TRAINING_MIN_BATCH_SIZE", 64), ("REPLAY_BUFFER_SIZE", 2000), ("CONTINUOUS_INPUT", Config.CONTINUOUS_INPUT),
                 ("DISCRATE_INPUT", Config.DISCRATE_INPUT), ("DISCOUNTING", Config.DISCOUNTING),
                 ("USE_REPLAY_MEMORY", Config.USE_REPLAY_MEMORY)):
        monkeypatch.setattr(Config, k, v)
    from Server import Server
    import NetworkDDPG
    srv = Server(max_agents=8)
    assert isinstance(srv.model, NetworkDDPG.Network) and srv.ddpg and srv.model.twin
    assert len(srv.model.get_variables_names()) == 38
    start = srv.model.get_variable_value("critic2_fc1/W", 0)
    assert start.any(), "critic 2 starts from initial_arena's draw"
    srv.main(max_seconds=5)
    assert srv.failure is None and srv.training_step > 10 and srv.predictions_served > 100
    assert srv.model.get_global_step() == srv.training_step
    assert not np.array_equal(start, srv.model.get_variable_value("critic2_fc1/W", 0)), "critic 2 did not train"
    for k in ("actor_fc1/W", "critic_fc1/W", "critic2_fc1/W"):
        assert np.all(np.isfinite(srv.model.get_variable_value(k, 0))) and np.all(np.isfinite(srv.model.get_variable_value(k, 1)))
    lines = open("results.txt").read().strip().splitlines()
    assert lines and all(len(line.split(",")) == 3 for line in lines), "results.txt keeps its format"
    srv.model.close()
