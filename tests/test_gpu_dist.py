"""-m gpu: the DDPG handle's distributional step (ga3c_ddpg_dist_create, Config.DDPG_DISTRIBUTIONAL) against its f64
statement (tests/dist_oracle.py).

Tolerances are tests/test_gpu_ddpg.py's, imported: 1e-4 x max(1, max|want|) on rows (_check), WTOL on weights and optimizer
slots after steps, tests/closeness.py's relative error per gradient tensor of the critic with e32 from an f32 run of the oracle.
Two kinds of tensor have an e32 that is a single draw of the rounding error, of which 16 x says nothing
(closeness.e32_of_row_sum has the argument); what stands in for it is the oracle's too (_single_draws).

As in test_gpu_ddpg.py, a relu unit within 1e-4 of zero in the oracle could land on the other side in f32: 4 B candidate rows
are drawn, the first B whose units keep that margin in every evaluation of the step are kept (_dselect), and the test asserts it
found B.  The head has no relu, and the softmax, the projection and the clip are continuous: they get no margin.  The support is
the narrow [-3, 1] with rewards drawn from [-5, 3], so that rows are clipped at either end; every fifth candidate is a done row
whose reward is (the f32 nearest to) an atom."""
import numpy as np
import pytest

import ddpg_actors_oracle as do
import ddpg_oracle as o
import dist_oracle as d4
import per_oracle as per
from test_gpu_ddpg import LR, WTOL, _candidates, _check, _f64, _load, _net, _same, _snapshot
from test_gpu_prioritized_replay import PTOL, SEED as PER_SEED, _check_update, _per_net, _random_priorities, _rel

pytestmark = pytest.mark.gpu

SHAPES = [(3, 1), (7, 3)]
VMIN, VMAX = -3.0, 1.0
EINVAL, ESTATE = -1, -4
DIST_FETCH = ("d_pt", "d_m", "d_p", "d_dz", "d_ce")
# every B at N = 51, every N at B = 17: 16 is the tile, 2 and 64 the ends of the atom count, 51 its odd default
CASES = [(B, 51) for B in (1, 15, 16, 17, 33)] + [(17, 2), (17, 64)]


def _dnet(S, A, N, max_batch=64, capacity=256, vmin=VMIN, vmax=VMAX, **kw):
    kw.setdefault("DDPG_CRITIC_LOSS", "paired")
    return _net(S, A, max_batch=max_batch, capacity=capacity, DDPG_DISTRIBUTIONAL=True, DDPG_ATOMS=N, DDPG_V_MIN=vmin,
                DDPG_V_MAX=vmax, **kw)


def _okw(cfg, N):
    """Config settings -> dist_oracle.train_step's keyword arguments."""
    return dict(atoms=N, vmin=VMIN, vmax=VMAX, critic_rmsprop=cfg.get("RMSPROP", True), momentum=cfg.get("RMSPROP_MOMENTUM", 0.0),
                clip=40.0 if cfg.get("USE_GRAD_CLIP") else None, future=cfg.get("DDPG_FUTURE_REWARD_CALC", True))


def _dcandidates(S, A, n, N, rng):
    s, a, _, done, s2 = _candidates(S, A, n, rng)
    r = rng.uniform(-5.0, 3.0, n).astype(np.float32)
    on = np.arange(n) % 5 == 0
    done[on] = 1.0
    r[on] = d4.support(N, VMIN, VMAX)[0][rng.integers(0, N, int(on.sum()))].astype(np.float32)
    return s, a, r, done, s2


def _dselect(st, cand, B, noise, **kw):
    """test_gpu_ddpg._select with the distributional step: the first B candidates whose relu units keep 1e-4 away from zero in
    the four nets, and in the critic's second layer where step 4 evaluates it after step 3 on the chosen rows."""
    s, a, r, done, s2 = cand
    ok = d4.relu_margin(st["online"], st["target"], s, a, s2) > 1e-4
    nz = 0.0 if noise is None else np.asarray(noise, np.float64)[None, :]
    for _ in range(20):
        keep = np.flatnonzero(ok)[:B]
        assert keep.size == B, "only %d of %d candidate rows qualify" % (keep.size, ok.size)
        trial = dict(st, online={k: v.copy() for k, v in st["online"].items()},
                     slot_a={k: v.copy() for k, v in st["slot_a"].items()}, slot_b={k: v.copy() for k, v in st["slot_b"].items()})
        rows = tuple(np.asarray(t[keep], np.float64) for t in cand)
        d4.train_step(trial, *rows, LR, None, stop_after=3, **kw)
        a_out = o.actor_forward(trial["online"], rows[0])["out"] + nz
        bad = np.abs(o.critic_forward(trial["online"], rows[0], a_out)["t"]).min(axis=1) <= 1e-4
        if not bad.any():
            return tuple(t[keep] for t in cand)
        ok[keep[bad]] = False
    raise AssertionError("the choice of rows did not settle")


def _dcase(S, A, B, N, seed, stats=False, noise=None, **kw):
    rng = np.random.Generator(np.random.PCG64(seed))
    online, target = d4.random_params(S, A, N, rng, stats=stats), d4.random_params(S, A, N, rng, stats=stats)
    st = d4.new_state(online, target, critic_rmsprop=kw.get("critic_rmsprop", True))
    return online, target, _dselect(st, _dcandidates(S, A, 4 * B, N, rng), B, noise, **kw)


def _args(b):
    return b[0], b[2], b[1], b[4], b[3]          # Network.train's order: x, y_r, a, x2, done


def _f32(P):
    return {k: v.astype(np.float32) for k, v in P.items()}


def _kinds(batch, N, gamma=0.99):
    """-> per row: done, clipped at the lower end, at the upper end, done with r on an atom (each a boolean [B])."""
    z = d4.support(N, VMIN, VMAX)[0]
    r, done = batch[2].astype(np.float64), batch[3] != 0
    tz = r[:, None] + np.where(done, 0.0, gamma)[:, None] * z[None, :]
    on = done & (np.abs(r[:, None] - z[None, :]).min(axis=1) <= 1e-6)
    return done, (tz < VMIN).any(axis=1), (tz > VMAX).any(axis=1), on


# ---- 1. one step, every row

def _single_draws(S, A, B, N, online, target, out, w32, kw):
    """-> {variable: e32 or None}: what replaces closeness.py's e32 where rel_err(g32, g64) is a SINGLE draw of the rounding
    error.  Everything here is the oracle's.
      * critic_output/b is, per atom, the sum of dz over the rows; at N = 2 its two entries are each other's negative (p and m
        both sum to one), so the tensor is one draw.  closeness.e32_of_row_sum's argument per column: each of the B terms carries
        an error of up to rel_err(dz32, dz64) x max|dz|, errors of mixed sign add like sqrt(B), and the result is measured against
        the tensor's largest entry: e32 = sqrt(B) x rel_err(dz32, dz64) x max|dz| / max_k |sum_i dz_ik|.
      * At B = 1 every gradient tensor is one row's dz pushed through the backward pass, and its rel_err one draw relative to
        that row's own magnitudes.  What f32 costs such a tensor is taken from many rows instead of one: the largest
        rel_err(g32, g64) over 64 rows drawn like the candidates, each stepped alone under the same weights.
    The caller takes the larger of this and the single draw."""
    import closeness as cl
    e = {k: None for k in o.CRITIC_TRAINABLE}
    if B > 1:
        dz64, dz32 = out["dz"], w32["dz"]
        e["critic_output/b"] = float(np.sqrt(B) * cl.rel_err(dz32, dz64) * np.max(np.abs(dz64)) / np.max(np.abs(dz64.sum(0))))
        return e
    rng = np.random.Generator(np.random.PCG64(7))
    cand = _dcandidates(S, A, 64, N, rng)
    e = {k: 0.0 for k in o.CRITIC_TRAINABLE}
    for i in range(64):
        row = tuple(t[i:i + 1] for t in cand)
        g64 = d4.train_step(d4.new_state(online, target), *_f64(row), LR, None, stop_after=3, **kw)["critic_grads"]
        g32 = d4.train_step(d4.new_state(_f32(online), _f32(target)), *row, LR, None, stop_after=3, **kw)["critic_grads"]
        for k in o.CRITIC_TRAINABLE:
            if k != o.DEAD and np.any(g64[k]):
                e[k] = max(e[k], cl.rel_err(g32[k], g64[k]))
    return e


@pytest.mark.parametrize("S,A", SHAPES)
@pytest.mark.parametrize("B,N", CASES)
def test_every_row_and_gradient(S, A, B, N):
    import closeness as cl
    kw = _okw({}, N)
    noise = np.linspace(-0.2, 0.3, A).astype(np.float32)
    online, target, batch = _dcase(S, A, B, N, 300 + B + S + N, stats=True, noise=noise, **kw)
    kinds = _kinds(batch, N)
    print("rows: %d done, %d clipped below, %d above, %d done on an atom" % tuple(int(k.sum()) for k in kinds))
    assert B == 1 or all(k.any() for k in kinds)
    net = _dnet(S, A, N)
    try:
        assert net.dist_info() == (N, VMIN, VMAX) and len(net.get_variables_names()) == 26
        _load(net, online, target)
        q_max, q_avg = net.compute(*_args(batch), 4, noise=noise)
        st = d4.new_state(online, target)
        out = d4.train_step(st, *_f64(batch), LR, noise.astype(np.float64), stop_after=4, **kw)
        w32 = d4.train_step(d4.new_state(_f32(online), _f32(target)), *batch, LR, noise, stop_after=4, **kw)
        _check("q_max", [q_max], [out["q_max"]])
        _check("q_avg", [q_avg], [out["q_avg"]])
        fc, fa = out["critic_fwd"], out["actor_fwd"]
        rows = [("y", out["y"]), ("qt", out["qt"]), ("d_pt", out["pt"]), ("d_m", out["m"]), ("d_p", out["p"]), ("d_dz", out["dz"]),
                ("d_ce", out["ce"]), ("q", out["q"]), ("c_x", batch[0]), ("c_a", batch[1]), ("c_xh1", fc["xh1"]), ("c_c1", fc["c1"]),
                ("c_c2", fc["c2"]), ("c_dt", fc["dt"]), ("c_dn1", fc["dn1"]), ("c_dh1", fc["dh1"]),
                ("a_xh1", fa["xh1"]), ("a_a1", fa["a1"]), ("a_xh2", fa["xh2"]), ("a_a2", fa["a2"]), ("a_out", fa["out"]),
                ("a_noisy", out["a_out"]), ("g", out["g"]), ("do", fa["do"]), ("a_dn2", fa["dn2"]), ("a_dn1", fa["dn1"])]
        for name, want in rows:
            _check(name, net.fetch(name, np.size(want)), want)
        m = net.fetch("d_m", B * N).reshape(B, N)
        assert np.max(np.abs(m.astype(np.float64).sum(axis=1) - 1.0)) <= 1e-5 and np.all(m >= 0.0)
        failed = []
        draws = _single_draws(S, A, B, N, online, target, out, w32, kw)
        for k in o.CRITIC_TRAINABLE:
            got = net.get_variable_value(k, 4)
            _check("grad " + k, got, out["critic_grads"][k])
            if k != o.DEAD:
                assert w32["critic_grads"][k].dtype == np.float32
                e32 = max(cl.rel_err(w32["critic_grads"][k], out["critic_grads"][k]), draws[k] or 0.0)
                err = cl.report("dist S=%d A=%d B=%d N=%d" % (S, A, B, N), "grad " + k, got, out["critic_grads"][k], e32, cl.bound(e32))
                if not err <= cl.bound(e32):
                    failed.append((k, err, cl.bound(e32)))
        for k in o.ACTOR_TRAINABLE:
            _check("grad " + k, net.get_variable_value(k, 4), out["actor_grads"][k])
        assert not failed, failed
        for k in o.CRITIC_TRAINABLE:
            _check("after step 3 " + k, net.get_variable_value(k, 0), st["online"][k], WTOL)
        assert net.get_global_step() == 0
    finally:
        net.close()


# ---- 2. production steps

WAYS = [dict(), dict(RMSPROP_MOMENTUM=0.9), dict(USE_GRAD_CLIP=True), dict(RMSPROP=False)]
STEPS = 3


def _abs_terms(P, f):
    """test_gpu_td3._abs_terms for this critic (dist_oracle.critic_grads' forward dict f): per element of its gradients the sum
    over the rows of the magnitudes of its terms, what a rounding error of the sum is relative to."""
    dz, dt, dn1 = np.abs(f["dz"]), np.abs(f["dt"]), np.abs(f["dn1"])
    dh1 = dn1 * np.abs(P["critic_norm1/gamma"] * f["rs1"])
    return {"critic_output/W": np.abs(f["c2"]).T @ dz, "critic_output/b": dz.sum(0), "critic_fc2/W": np.abs(f["c1"]).T @ dt,
            "critic_norm2/W": np.abs(f["a"]).T @ dt, "critic_norm2/b": dt.sum(0), "critic_norm1/beta": dn1.sum(0),
            "critic_norm1/gamma": (dn1 * np.abs(f["xh1"])).sum(0), "critic_fc1/W": np.abs(f["x"]).T @ dh1, "critic_fc1/b": dh1.sum(0)}


class _AdamCondition:
    """test_gpu_td3._AdamCondition for this critic: which elements of an Adam critic's weights can be held to WTOL at all.
    Adam's step is lr_t m / (sqrt(v) + 1e-8): on an element whose gradient is a sum over the rows that cancels to some 1e-6 or
    less the 1e-8 decides the quotient, and the step follows the gradient's RELATIVE error, which f32 does not keep for such a
    sum: the f32 oracle itself is 3.1e-5 off the f64 one in critic_fc2/W after the first step of the (7, 3) case here.  A
    condition, not a tolerance: an element is left out of the comparison of the online weights only if, in the oracle, its step
    moves by more than WTOL / STEPS when its gradient moves by bound(e32) x the sum of the magnitudes of its terms, bound and
    e32 closeness.py's for its tensor from the f32 oracle on the same rows; such elements must be fewer than 1 % of their
    tensor (or one; closeness.signed_or_magnitude's share for entries too small to carry a sign: a first-layer unit that is on
    in almost no row puts its S weights among them at once, 23 of critic_fc1/W's 2800 at S = 7 by the oracle alone) and stay
    within what the steps can differ by at all.  Slots and targets are compared whole."""

    def __init__(self, st):
        self.st = st
        self.names = [k for k in o.CRITIC_TRAINABLE if k != o.DEAD]
        self.shaky = {k: np.zeros(st["online"][k].shape, bool) for k in self.names}

    def before(self):
        self.slots = {k: (self.st["slot_a"][k].copy(), self.st["slot_b"][k].copy()) for k in self.names}
        self.weights = {k: v.copy() for k, v in self.st["online"].items()}

    def after(self, out, out32, lr, t):
        import closeness as cl
        from test_gpu_td3 import _adam_shift
        terms = _abs_terms(self.weights, out["critic_fwd"])
        for k in self.names:
            g = out["critic_grads"][k].reshape(self.shaky[k].shape)
            e_g = cl.bound(cl.rel_err(out32["critic_grads"][k], g)) * terms[k].reshape(g.shape)
            self.shaky[k] |= _adam_shift(*self.slots[k], g, e_g, lr, t) > WTOL / STEPS

    def check(self, k, got, want, lr):
        keep = ~self.shaky[k]
        out = int((~keep).sum())
        print("%-28s %d of %d elements too small for Adam's quotient" % (k, out, keep.size))
        assert out <= max(1, keep.size // 100), "%s: %d of %d elements" % (k, out, keep.size)
        _check("online " + k, got[keep], want[keep], WTOL)
        if not keep.all():
            assert np.max(np.abs(got[~keep] - want[~keep])) <= STEPS * 2 * 3.2 * lr


@pytest.mark.parametrize("cfg", WAYS, ids=["plain", "momentum", "clip", "adam"])
@pytest.mark.parametrize("S,A", SHAPES)
def test_three_production_steps(S, A, cfg):
    B, N = 33, 51
    kw = _okw(cfg, N)
    noise = np.full(A, 0.05, np.float32)
    rng = np.random.Generator(np.random.PCG64(500 + S))
    online, target = d4.random_params(S, A, N, rng), d4.random_params(S, A, N, rng)
    st = d4.new_state(online, target, critic_rmsprop=cfg.get("RMSPROP", True))
    adam, st32 = None, None
    if not cfg.get("RMSPROP", True):
        adam, st32 = _AdamCondition(st), d4.new_state(_f32(online), _f32(target), critic_rmsprop=False)
    net = _dnet(S, A, N, **cfg)
    try:
        _load(net, online, target)
        for step in range(1, STEPS + 1):
            b = _dselect(st, _dcandidates(S, A, 4 * B, N, rng), B, noise, **kw)
            q_max, q_avg = net.train(*_args(b), noise=noise)
            if adam:
                adam.before()
            out = d4.train_step(st, *_f64(b), LR, noise.astype(np.float64), **kw)
            if adam:
                adam.after(out, d4.train_step(st32, *b, LR, noise, **kw), 10.0 * LR, step)
            _check("step %d q_max" % step, [q_max], [out["q_max"]])
            _check("step %d q_avg" % step, [q_avg], [out["q_avg"]])
        assert net.get_global_step() == STEPS and st["step"] == STEPS
        for k in o.ALL_VARS:
            if adam and k in adam.shaky:
                adam.check(k, net.get_variable_value(k, 0), st["online"][k], 10.0 * LR)
            else:
                _check("online " + k, net.get_variable_value(k, 0), st["online"][k], WTOL)
            _check("target " + k, net.get_variable_value(k, 1), st["target"][k], WTOL)
        for k in o.TRAINABLE:
            _check("slot a " + k, net.get_variable_value(k, 2), st["slot_a"][k], WTOL)
            _check("slot b " + k, net.get_variable_value(k, 3), st["slot_b"][k], WTOL)
        assert np.array_equal(net.get_variable_value(o.DEAD, 0), online[o.DEAD].astype(np.float32)), "critic_fc2/b moved"
    finally:
        net.close()


def test_without_future_rewards_the_target_is_the_projection_of_r():
    S, A, B, N = 3, 1, 17, 51
    cfg = dict(DDPG_FUTURE_REWARD_CALC=False)
    kw = _okw(cfg, N)
    online, target, batch = _dcase(S, A, B, N, 77, **kw)
    net = _dnet(S, A, N, **cfg)
    try:
        _load(net, online, target)
        net.compute(*_args(batch), 3, noise=False)
        out = d4.train_step(d4.new_state(online, target), *_f64(batch), LR, None, stop_after=3, **kw)
        want = d4.project(None, batch[2], None, N, VMIN, VMAX)
        assert np.array_equal(out["m"], want)
        _check("d_m", net.fetch("d_m", B * N), want)
        assert not net.fetch("d_pt", B * N).any() and not net.fetch("qt", B).any()
        for name, ref in (("y", out["y"]), ("q", out["q"]), ("d_dz", out["dz"]), ("d_ce", out["ce"])):
            _check(name, net.fetch(name, np.size(ref)), ref)
        for k in o.CRITIC_TRAINABLE:
            _check("grad " + k, net.get_variable_value(k, 4), out["critic_grads"][k])
    finally:
        net.close()


# ---- 3. bits

def test_train_replay_is_train_on_the_same_rows_and_the_same_call_gives_the_same_bits():
    S, A, B, N = 3, 1, 33, 51
    rng = np.random.Generator(np.random.PCG64(11))
    online, target = d4.random_params(S, A, N, rng), d4.random_params(S, A, N, rng)
    s, a, r, done, s2 = _dcandidates(S, A, 64, N, rng)
    slots = np.random.default_rng(3).choice(64, B, replace=False).astype(np.int32)
    snaps, rows = [], []
    for how in ("replay", "train", "replay"):
        net = _dnet(S, A, N)
        try:
            _load(net, online, target)
            assert net.replay_add(s, a, r, done, s2) == (64, 64)
            for _ in range(2):
                if how == "replay":
                    net.train_replay(slots, stamp=64, noise=[0.1])
                else:
                    net.train(s[slots], r[slots], a[slots], s2[slots], done[slots], noise=[0.1])
            snaps.append(_snapshot(net))
            rows.append({k: net.fetch(k, B * (1 if k in ("d_ce", "y", "q") else N)) for k in DIST_FETCH + ("y", "q")})
        finally:
            net.close()
    assert _same(snaps[0], snaps[1]) and _same(rows[0], rows[1]), "train_replay differs from train on the same rows"
    assert _same(snaps[0], snaps[2]) and _same(rows[0], rows[2]), "the same calls on a fresh handle gave other bits"


# ---- 4. with priorities

def test_prioritized_step_weights_the_delta_and_sets_the_priorities():
    S, A, n, B, N, beta = 3, 1, 128, 33, 51, 0.4
    kw = _okw({}, N)
    rng = np.random.Generator(np.random.PCG64(43))
    online, target = d4.random_params(S, A, N, rng), d4.random_params(S, A, N, rng)
    cand = _dcandidates(S, A, 3 * n, N, rng)
    keep = np.flatnonzero(d4.relu_margin(online, target, cand[0], cand[1], cand[4]) > 1e-4)[:n]
    assert keep.size == n
    rows = tuple(t[keep] for t in cand)
    pa = _random_priorities(n, n, np.random.default_rng(5))
    want_slots, want_w = per.sample(pa, n, B, PER_SEED, 0, beta)
    net = _per_net(n, max_batch=64, DDPG_DISTRIBUTIONAL=True, DDPG_ATOMS=N, DDPG_V_MIN=VMIN, DDPG_V_MAX=VMAX)
    try:
        _load(net, online, target)
        assert net.replay_add(*(t[:64] for t in rows))[0] == 64 and net.replay_add(*(t[64:] for t in rows)) == (n, n)
        net.set_priorities(pa, 0.05)
        net.replay_beta = beta
        net.train_prioritized(B, noise=[0.05])
        slots, w = net.last_slots, net.fetch("per_w", B)
        assert np.array_equal(slots, want_slots) and _rel(w, want_w) <= PTOL
        assert len(np.unique(w)) > 1
        batch = _f64(tuple(t[slots] for t in rows))
        out = d4.train_step(d4.new_state(online, target), *batch, LR, None, stop_after=3, w=w.astype(np.float64), **kw)
        for name, ref in (("y", out["y"]), ("q", out["q"]), ("d_m", out["m"]), ("d_p", out["p"]), ("d_dz", out["dz"]), ("d_ce", out["ce"])):
            _check(name, net.fetch(name, np.size(ref)), ref)
        plain = (out["p"] - out["m"]) / B
        assert np.max(np.abs(plain - out["dz"])) > 10 * 1e-4 * np.max(np.abs(plain)), "the weights did not reach the oracle's delta"
        for k in o.CRITIC_TRAINABLE:
            _check("grad " + k, net.get_variable_value(k, 4), out["critic_grads"][k])
        _check_update(net, pa, np.float32(0.05), slots, B)              # pa[slot] = (|y - q| + eps)^alpha on the expectations
    finally:
        net.close()


# ---- 5. with n-step returns

def test_per_slot_discounts_reach_the_projection():
    S, A, B, N = 3, 1, 17, 51
    kw = _okw({}, N)
    rng = np.random.Generator(np.random.PCG64(61))
    online, target = d4.random_params(S, A, N, rng), d4.random_params(S, A, N, rng)
    cand = _dcandidates(S, A, 4 * B, N, rng)
    keep = np.flatnonzero(d4.relu_margin(online, target, cand[0], cand[1], cand[4]) > 1e-4)[:B]
    assert keep.size == B
    batch = tuple(t[keep] for t in cand)
    capacity = B + 5
    disc = np.full(capacity, np.float32(0.99), np.float32)
    disc[:B] = (np.float32(0.99) ** np.arange(1, B + 1)).astype(np.float32)
    net = _dnet(S, A, N, capacity=capacity)
    try:
        net.nstep_create(5)
        _load(net, online, target)
        assert net.replay_add(*batch) == (B, B)
        net.set_nstep_discounts(disc)
        # train and compute have no slot: the scalar gamma, and fetch says so
        net.compute(*_args(batch), 3, noise=False)
        assert np.all(net.fetch("disc", B) == np.float32(0.99))
        _check("d_m under gamma", net.fetch("d_m", B * N), d4.targets(target, *(_f64(batch)[i] for i in (4, 2, 3)), 0.99, N, VMIN, VMAX)["m"])
        _load(net, online, target)                  # compute stepped the critic; the rows below do not read the slots
        slots = rng.permutation(B).astype(np.int32)
        net.train_replay(slots, noise=[0.05])
        assert np.array_equal(net.fetch("disc", B), disc[slots])
        rows = _f64(tuple(t[slots] for t in batch))
        out = d4.train_step(d4.new_state(online, target), *rows, LR, None, stop_after=3,
                            **dict(kw, gamma=disc[slots].astype(np.float64)))
        for name, ref in (("d_pt", out["pt"]), ("d_m", out["m"]), ("y", out["y"]), ("qt", out["qt"]), ("d_dz", out["dz"])):
            _check(name, net.fetch(name, np.size(ref)), ref)
        scalar = d4.targets(target, rows[4], rows[2], rows[3], 0.99, N, VMIN, VMAX)["m"]
        assert np.max(np.abs(scalar - out["m"])) > 10 * 1e-4, "the discounts did not reach the oracle's projection"
    finally:
        net.close()


# ---- 6. with device actors

def test_device_actors_train_the_distributional_step():
    S, A, n, B, N, capacity, noise = 3, 1, 5, 16, 51, 400, [0.3]
    rng = np.random.Generator(np.random.PCG64(71))
    online, target = d4.random_params(S, A, N, rng), d4.random_params(S, A, N, rng)
    net, twin = (_dnet(S, A, N, capacity=capacity, vmin=-100.0, vmax=0.0) for _ in range(2))
    try:
        for h in (net, twin):
            _load(h, online, target)
        net.actors_create(n, seed=5, updates=1, batch=B, draw_seed=2468)
        stats = [net.actors_run(20, train=True, noise=noise) for _ in range(2)]
        adds = 39                                   # the first actor step is step(None): no transition
        assert net.replay_size() == (n * adds, n * adds)
        calls = sum(1 for k in range(1, adds + 1) if n * k > B)
        assert stats[0][1] + stats[1][1] == calls > 20 and net.get_global_step() == calls
        ring = np.stack([np.concatenate([np.atleast_1d(c) for c in net.replay_get(i)]) for i in range(n * adds)])
        sample, last, q_twin = 0, None, None
        for k in range(adds):
            f = ring[k * n:(k + 1) * n]
            size, _ = twin.replay_add(f[:, :S], f[:, S:S + A], f[:, S + A], f[:, S + A + 1], f[:, S + A + 2:])
            if size > B:
                last = do.uniform_slots(2468, sample, size, B)
                q_twin = twin.train_replay(last, noise=noise)
                sample += 1
        assert sample == calls and np.array_equal(net.actors_get("slots"), last)
        assert net.logging == q_twin and np.all(np.isfinite(net.logging)) and -100.0 <= net.logging[1] <= 0.0
        assert _same(_snapshot(net), _snapshot(twin))
        for k in DIST_FETCH:
            c = B * (1 if k == "d_ce" else N)
            assert np.array_equal(net.fetch(k, c), twin.fetch(k, c)), k
    finally:
        net.close()
        twin.close()


# ---- 7. return codes

def test_return_codes():
    import _native as nat
    lib = nat.hip_lib()
    net = _net(3, 1, max_batch=16, capacity=32, DDPG_CRITIC_LOSS="paired")
    fork = _net(3, 1, max_batch=16, capacity=32)
    try:
        h = net._h
        create, destroy = lib.ga3c_ddpg_dist_create, lib.ga3c_ddpg_dist_destroy
        assert net.dist_info() == (1, 0.0, 0.0)
        buf = np.zeros(64, np.float32)
        for name in DIST_FETCH:
            assert lib.ga3c_ddpg_fetch(h, name.encode(), nat.ptr(buf), 1) == ESTATE, name
        assert destroy(h) == ESTATE
        for atoms, lo, hi in ((1, -1.0, 1.0), (65, -1.0, 1.0), (0, -1.0, 1.0), (51, 1.0, 1.0), (51, 2.0, 1.0),
                              (51, float("nan"), 1.0), (51, -1.0, float("nan")), (51, -float("inf"), 1.0), (51, -1.0, float("inf"))):
            assert create(h, atoms, lo, hi) == EINVAL, (atoms, lo, hi)
        assert create(fork._h, 51, -1.0, 1.0) == ESTATE                 # without GA3C_DDPG_LOSS_PAIRED
        before = {k: net.get_variable_value(k, 0) for k in o.ALL_VARS}
        assert create(h, 51, -2.0, 1.0) == 0
        assert create(h, 51, -2.0, 1.0) == ESTATE                       # a second create
        assert net.dist_info() == (51, -2.0, 1.0)
        assert lib.ga3c_ddpg_twin_create(h, 2, 0.2, 0.5, 1) == ESTATE   # twin on a distributional handle
        names = net.get_variables_names()
        assert len(names) == 26 and [k[:-2] for k in names] == list(o.ALL_VARS)
        assert net.get_variable_value("critic_output/W", 0).shape == (300, 51)
        assert net.get_variable_value("critic_output/b", 1).shape == (51,)
        # every other variable kept its value; the head is as create leaves variables: zero, the RMSProp ms slot one
        for k in o.ALL_VARS:
            if not k.startswith("critic_output"):
                assert np.array_equal(net.get_variable_value(k, 0), before[k]), k
        for which, fill in ((0, 0.0), (1, 0.0), (2, 1.0), (3, 0.0), (4, 0.0)):
            assert np.all(net.get_variable_value("critic_output/W", which) == fill), which
        assert lib.ga3c_ddpg_fetch(h, b"d_m", nat.ptr(buf), 7) == EINVAL          # no step yet: 0 floats
        assert destroy(h) == 0 and destroy(h) == ESTATE
        assert len(net.get_variables_names()) == 26 and net.get_variable_value("critic_output/W", 0).shape == (300, 1)
        assert not net.get_variable_value("critic_output/W", 0).any() and net.dist_info()[0] == 1
        for k in o.ALL_VARS:
            if not k.startswith("critic_output"):
                assert np.array_equal(net.get_variable_value(k, 0), before[k]), k
        # the other order: a distributional critic on a twin handle
        assert lib.ga3c_ddpg_twin_create(h, 2, 0.2, 0.5, 1) == 0
        assert create(h, 51, -2.0, 1.0) == ESTATE
        assert lib.ga3c_ddpg_twin_destroy(h) == 0 and create(h, 2, -2.0, 1.0) == 0
    finally:
        net.close()                     # destroy with the feature attached
        fork.close()


# ---- 8. checkpoints

def _arenas(net):
    return {(k, w): net.get_variable_value(k, w) for k in o.ALL_VARS for w in (0, 1, 2, 3)}


@pytest.mark.parametrize("cfg", [dict(), dict(RMSPROP=False)], ids=["rmsprop", "adam"])
def test_checkpoint_round_trip_resume_and_refusals(cfg, tmp_path):
    S, A, B, N = 3, 1, 17, 51
    rng = np.random.Generator(np.random.PCG64(51))
    online, target = d4.random_params(S, A, N, rng), d4.random_params(S, A, N, rng)
    batch = _dcandidates(S, A, B, N, rng)
    path = str(tmp_path / "dist.npz")
    net = _dnet(S, A, N, **cfg)
    try:
        _load(net, online, target)
        for _ in range(3):
            net.train(*_args(batch), noise=False)
        assert net._lib.ga3c_ddpg_save(net._h, path.encode()) == 0
        three = _arenas(net)
        net.train(*_args(batch), noise=False)
        four = _arenas(net)
    finally:
        net.close()
    slot = ("critic_fc1/W/RMSProp:0", "critic_fc1/W/RMSProp_1:0") if cfg.get("RMSPROP", True) else ("critic_fc1/W/Adam:0", "critic_fc1/W/Adam_1:0")
    with np.load(path) as z:
        assert int(z["step"]) == 3 and z["dist_support"].dtype == np.float32
        assert np.array_equal(z["dist_support"], np.array([VMIN, VMAX], np.float32))
        assert z["critic_output/W:0"].shape == (300, N) and z["critic_output_1/b:0"].shape == (N,)
        for name in slot + ("actor_fc1/W/Adam:0", "actor_fc1/W/Adam_1:0", "critic_output/W/" + slot[0].split("/")[-1]):
            assert name in z.files, name
        assert np.array_equal(z["critic_output/W:0"], three[("critic_output/W", 0)])
        assert np.array_equal(z[slot[0]], three[("critic_fc1/W", 2)]) and np.array_equal(z[slot[1]], three[("critic_fc1/W", 3)])
        assert len(z.files) == 2 + 2 * 26 + 2 * 20
    fresh = _dnet(S, A, N, **cfg)
    try:
        fresh.load_file(path)
        assert fresh.get_global_step() == 3 and _same(three, _arenas(fresh))
        fresh.train(*_args(batch), noise=False)
        assert _same(four, _arenas(fresh)), "the resumed run differs from the uninterrupted one"
    finally:
        fresh.close()
    if cfg:
        return
    # the four cross-refusals leave the arenas as they were
    plain_path = str(tmp_path / "plain.npz")
    plain = _net(S, A, DDPG_CRITIC_LOSS="paired")
    try:
        assert plain._lib.ga3c_ddpg_save(plain._h, plain_path.encode()) == 0
        before = _arenas(plain)
        assert plain._lib.ga3c_ddpg_load(plain._h, path.encode()) == ESTATE          # a distributional file into a plain handle
        assert _same(before, _arenas(plain)) and plain.get_global_step() == 0
    finally:
        plain.close()
    for other, bad in ((dict(N=N), plain_path), (dict(N=21), path), (dict(N=N, vmax=2.0), path), (dict(N=N, vmin=-3.5), path)):
        h = _dnet(S, A, other["N"], vmin=other.get("vmin", VMIN), vmax=other.get("vmax", VMAX))
        try:
            before = _arenas(h)
            assert h._lib.ga3c_ddpg_load(h._h, bad.encode()) == ESTATE, other
            assert _same(before, _arenas(h)) and h.get_global_step() == 0
        finally:
            h.close()


# ---- 9. the server

@pytest.mark.timeout(120)
def test_server_runs_the_device_actors_with_a_distributional_critic(tmp_path, monkeypatch):
    import ga3c_amd  # noqa: F401
    from Config import Config
    monkeypatch.chdir(tmp_path)
    for k, v in (("GAME", "Pendulum-v0"), ("USE_DDPG", True), ("DEVICE_AGENTS", 64), ("DEVICE_DDPG", True),
                 ("DYNAMIC_SETTINGS", False), ("SAVE_MODELS", False), ("TRAINING_MIN_BATCH_SIZE", 64),
                 ("DDPG_CRITIC_LOSS", "paired"), ("DDPG_DISTRIBUTIONAL", True), ("CONTINUOUS_INPUT", Config.CONTINUOUS_INPUT),
                 ("DISCRATE_INPUT", Config.DISCRATE_INPUT), ("DISCOUNTING", Config.DISCOUNTING),
                 ("USE_REPLAY_MEMORY", Config.USE_REPLAY_MEMORY)):
        monkeypatch.setattr(Config, k, v)
    from Server import Server
    srv = Server()
    try:
        assert srv.model.dist and srv.model.dist_info() == (51, -100.0, 0.0)
        srv.main(max_seconds=4)
        assert srv.failure is None and srv.training_step > 0 and srv.model.get_global_step() == srv.training_step
        assert open("results.txt").read().strip(), "no episode was logged"
        q_max, q_avg = srv.model.logging
        assert np.isfinite(q_max) and np.isfinite(q_avg) and Config.DDPG_V_MIN <= q_avg <= q_max <= Config.DDPG_V_MAX
    finally:
        srv.model.close()
