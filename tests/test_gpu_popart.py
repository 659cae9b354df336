"""-m gpu: PopArt on the DDPG handle's critic (Config.DDPG_POPART, ga3c_ddpg_popart_*) against
tests/popart_oracle.py, which tests/test_popart_cpu.py holds to tests/ddpg_oracle.py and to autograd.

Exact (bits): a popart handle at beta = 0 against a plain paired handle; ddpg_popart_kernel's rescale and yn against the oracle's
expressions on the statistics the kernel stored; two fresh runs; a resumed run; the device actors at beta = 0.  Bounded: the
statistics within one f32 spacing of the oracle's (the sums are f64 in another order), full steps at tests/test_gpu_ddpg.py's own
TOL and WTOL, and the preserved outputs at four times what the oracle's own mixed form loses (profiles/popart_closeness.md has the ratio).
Rows follow test_gpu_ddpg's rule: 2 B candidates, the first B whose relu units keep 1e-4 from zero in the oracle, in all four
nets and where step 4 evaluates the updated critic; the test asserts it found B."""
import os

import numpy as np
import pytest

import ddpg_oracle as o
import per_oracle as per
import popart_oracle as po
from test_gpu_ddpg import LR, TOL, WTOL, _candidates, _cfg_kw, _check, _f64, _load, _net
from test_gpu_ddpg_actors import DRAW_SEED, _eq, _ring_rows, _weights
from test_gpu_prioritized_replay import SEED as PER_SEED, _random_priorities

pytestmark = pytest.mark.gpu

SHAPES = [(3, 1), (7, 3)]
SIZES = [1, 17, 33]             # one valid row of a tile, a second tile with one row, three tiles
EINVAL, ESTATE = -1, -4
MU, NU = "critic_popart/mu", "critic_popart/nu"
ROWS = ("y", "qt", "q", "dq", "c_x", "c_a", "c_xh1", "c_c1", "c_dn1", "c_dh1", "c_c2", "c_dt", "a_xh1", "a_a1", "a_dn1", "a_dh1",
        "a_xh2", "a_a2", "a_dn2", "a_dh2", "a_out", "a_noisy", "g", "do")
WIDTH = {"c_x": "S", "c_a": "A", "a_out": "A", "a_noisy": "A", "g": "A", "do": "A"}


def _pnet(S, A, beta=0.1, popart=True, **kw):
    kw.setdefault("DDPG_CRITIC_LOSS", "paired")
    return _net(S, A, DDPG_POPART=popart, DDPG_POPART_BETA=beta, **kw)


def _okw(cfg):
    return {k: v for k, v in _cfg_kw(dict(cfg, DDPG_CRITIC_LOSS="paired")).items() if k != "form"}


def _copy(st):
    return dict(st, **{k: {n: v.copy() for n, v in st[k].items()} for k in ("online", "target", "slot_a", "slot_b")})


def _select(st, cand, B, step):
    """test_gpu_ddpg._select's rule with the popart step: step(trial, rows) runs steps 1-4 on a copy of the state."""
    s, a, r, done, s2 = cand
    ok = o.relu_margin(st["online"], st["target"], s, a, s2) > 1e-4
    for _ in range(20):
        keep = np.flatnonzero(ok)[:B]
        assert keep.size == B, "only %d of %d candidate rows qualify" % (keep.size, ok.size)
        trial = _copy(st)
        rows = _f64(tuple(t[keep] for t in cand))
        out = step(trial, rows)
        bad = np.abs(o.critic_forward(trial["online"], rows[0], out["a_out"])["t"]).min(axis=1) <= 1e-4
        if not bad.any():
            return tuple(t[keep] for t in cand)
        ok[keep[bad]] = False
    raise AssertionError("the choice of rows did not settle")


def _fetch_all(net, S, A, B, names=ROWS):
    out = {}
    for name in names:
        wd = {"S": S, "A": A}.get(WIDTH.get(name), 400 if name[-1] == "1" else 300 if name[-1] == "2" or name == "c_dt" else 1)
        out[name] = net.fetch(name, B * wd)
    return out


def _arenas(net, names=o.ALL_VARS, which=(0, 1, 2, 3, 4)):
    return {(k, w): net.get_variable_value(k, w) for k in names for w in which}


def _same(a, b):
    return a.keys() == b.keys() and all(_eq(a[k], b[k]) for k in a)


def _stats(net):
    return float(net.get_variable_value(MU)[0]), float(net.get_variable_value(NU)[0])


def _set_stats(net, mu, nu):
    for which in (0, 1):
        net.set_variable_value(MU, [mu], which)
        net.set_variable_value(NU, [nu], which)


# ---- 1. beta = 0 is the plain step

@pytest.mark.parametrize("S,A", SHAPES)
@pytest.mark.parametrize("B", SIZES)
def test_beta_zero_is_the_plain_paired_step_bit_for_bit(S, A, B):
    rng = np.random.Generator(np.random.PCG64(300 + B + S))
    online, target = o.random_params(S, A, rng, stats=True), o.random_params(S, A, rng, stats=True)
    rows = tuple(t[:3 * B] for t in _candidates(S, A, 6 * B, rng))
    noise = np.linspace(-0.2, 0.3, A).astype(np.float32)
    got = []
    for popart in (True, False):
        net = _pnet(S, A, beta=0.0, popart=popart)
        try:
            _load(net, online, target)
            assert len(net.get_variables_names()) == (28 if popart else 26) == len(net.get_target_names())
            assert net.replay_add(*rows) == (3 * B, 3 * B)
            steps = []
            for i in range(3):
                q = net.train_replay(np.arange(i * B, (i + 1) * B, dtype=np.int32), noise=noise)
                steps.append((q, _fetch_all(net, S, A, B)))
                if popart:
                    assert _eq(net.fetch("yn", B), steps[-1][1]["y"])
                    assert _stats(net) == (0.0, 1.0) and net.popart_info() == (0.0, 0.0, 1.0, 1.0)
                    assert _eq(net.get_variable_value(MU, 1), np.zeros(1, np.float32))
                    assert _eq(net.get_variable_value(NU, 1), np.ones(1, np.float32))
            got.append((steps, _arenas(net), net.get_global_step()))
        finally:
            net.close()
    (psteps, parena, pstep), (steps, arena, step) = got
    assert pstep == step == 3 and _same(parena, arena)
    for (pq, prow), (q, row) in zip(psteps, steps):
        assert pq == q and _same(prow, row)


# ---- 2. the kernel alone

def _kernel_case(S, A, B, offset, seed):
    """y = r exactly: rewards offset + 0.09 u, u in (-1, 0), as the wrapper's r 0.005 - 1 spreads them.  At B = 1 the reward has
    eight significant bits, so that its square is an f32 and nu' - mu'^2 is exactly zero: sigma resolves no finer than
    sqrt(half a spacing of nu), 0.02 at -100."""
    rng = np.random.Generator(np.random.PCG64(seed))
    online, target = o.random_params(S, A, rng, stats=True), o.random_params(S, A, rng, stats=True)
    s, a, r, done, s2 = tuple(t[:B] for t in _candidates(S, A, 2 * B, rng))
    r = (np.float32(offset) + np.float32(0.09) * r).astype(np.float32)
    if B == 1:
        r = (np.round(r * 16) / 16).astype(np.float32)
    return online, target, (s, a, r, done, s2)


@pytest.mark.parametrize("S,A", SHAPES)
@pytest.mark.parametrize("B", SIZES)
@pytest.mark.parametrize("beta", [0.5, 1.0])
@pytest.mark.parametrize("offset,mu,nu", [(-1.0, -0.8, 0.9), (-100.0, -97.0, 9500.0)], ids=["near-1", "near-100"])
def test_the_kernel_alone(S, A, B, beta, offset, mu, nu):
    online, target, batch = _kernel_case(S, A, B, offset, 400 + B + S)
    s, a, r, done, s2 = batch
    net = _pnet(S, A, beta=beta, DDPG_FUTURE_REWARD_CALC=False)
    try:
        _load(net, online, target)
        _set_stats(net, mu, nu)
        mu, nu = np.float32(mu), np.float32(nu)
        net.learning_rate = 0.0
        net.compute(s, r, a, s2, done, 3, noise=False)
        y = net.fetch("y", B)
        assert _eq(y, r)
        mu1, nu1 = (np.float32(v) for v in _stats(net))
        want_mu, want_nu = po.update_mixed(mu, nu, y, beta)
        print("mu' %.9g (oracle %.9g)  nu' %.9g (oracle %.9g)" % (mu1, want_mu, nu1, want_nu))
        assert abs(float(mu1) - float(want_mu)) <= np.spacing(np.abs(want_mu))
        assert abs(float(nu1) - float(want_nu)) <= np.spacing(np.abs(want_nu))
        assert _eq(net.get_variable_value(MU, 1)[0], mu1) and _eq(net.get_variable_value(NU, 1)[0], nu1)     # the target copy mirrors
        # ... and from the stored statistics on, the oracle's expressions give the kernel's bits
        ratio, shift, muf, isig, sigma, sigma1 = po.constants(mu, nu, mu1, nu1)
        for which, P in ((0, online), (1, target)):
            W, b = po.rescale(P[po.WO].astype(np.float32), P[po.BO].astype(np.float32), ratio, shift)
            assert _eq(net.get_variable_value(po.WO, which), W), which
            assert _eq(net.get_variable_value(po.BO, which), b), which
        yn = net.fetch("yn", B)
        assert _eq(yn, po.normalise(y, muf, isig))
        info = net.popart_info()
        assert info[1:3] == (float(mu1), float(nu1)) and info[3] == float(np.float32(sigma1))
        everything = [yn, net.fetch("q", B), net.fetch("dq", B)] + [net.get_variable_value(k, w) for k in o.CRITIC_TRAINABLE
                                                                    for w in (0, 1, 2, 3, 4)]
        assert all(np.all(np.isfinite(v)) for v in everything)
        if B == 1 and beta == 1.0:              # zero variance: sigma sits at its lower clamp
            assert sigma1 == po.bounds32()[0] and info[3] == np.float32(po.SIGMA_MIN) and float(mu1) == float(y[0])
            assert _eq(yn, np.zeros(1, np.float32))
        else:                                   # (a batch's spread of 0.03 at -100 is below sigma's resolution: the clamp may hold it)
            assert po.bounds32()[0] <= sigma1 < po.bounds32()[1]
    finally:
        net.close()


# ---- 3. outputs are preserved

@pytest.mark.parametrize("S,A", SHAPES)
@pytest.mark.parametrize("B", [17, 33])
def test_the_rescale_preserves_the_critics_outputs(S, A, B):
    """sigma' n' + mu' of the step that moved the statistics against sigma n + mu of the same rows under the old ones (a handle
    at beta = 0, whose rescale is the identity).  Bound: four times the largest such difference in the oracle's own runs, mixed
    and float64, on the same case -- what f32 weights and an f32 sum lose, times 4 for the order of the sum."""
    beta, mu, nu = 0.5, np.float32(-97.0), np.float32(9500.0)
    online, target, batch = _kernel_case(S, A, B, -100.0, 500 + B + S)
    s, a, r, done, s2 = batch
    n, stats = [], []
    for b in (0.0, beta):
        net = _pnet(S, A, beta=b, DDPG_FUTURE_REWARD_CALC=False)
        try:
            _load(net, online, target)
            _set_stats(net, mu, nu)
            net.learning_rate = 0.0
            net.compute(s, r, a, s2, done, 3, noise=False)
            n.append(net.fetch("q", B).astype(np.float64))
            stats.append(net.popart_info())
        finally:
            net.close()
    lo, hi = po.bounds32()
    assert stats[0][1:3] == (float(mu), float(nu)) and stats[1][1:3] != stats[0][1:3]
    before = po.sigma_of(mu, nu, lo, hi) * n[0] + float(mu)
    after = po.sigma_of(stats[1][1], stats[1][2], lo, hi) * n[1] + stats[1][1]
    err = float(np.max(np.abs(after - before)))
    own = []
    for mixed in (True, False):
        P = {k: v.astype(np.float32) for k, v in online.items()} if mixed else online
        c2 = o.critic_forward(P, s, a)["c2"]
        b0, b1, _ = po.preserved((P[po.WO], P[po.BO]), c2, mu, nu, r, beta, mixed=mixed)
        own.append(float(np.max(np.abs(b1 - b0))))
    bound = 4.0 * max(own)
    print("S=%d A=%d B=%d: outputs near %.4g moved by %.3e; the oracle's mixed form %.3e, float64 %.3e; ratio to the bound %.3f"
          % (S, A, B, float(np.max(np.abs(before))), err, own[0], own[1], err / bound))
    assert err <= bound


# ---- 4. full steps against the oracle

def _compare_rows(net, out, B, names=("y", "qt", "yn", "q", "dq")):
    for name in names:
        _check(name, net.fetch(name, np.size(out[name])), out[name])


FULL = [("rmsprop", dict()), ("adam-clip", dict(RMSPROP=False, USE_GRAD_CLIP=True))]


def _f32(P):
    return {k: v.astype(np.float32) for k, v in P.items()}


def _full_case(S, A, B, cfg, beta, noise, base, steps=3, tries=40):
    """-> (online, target, the steps' batches, e32).  Two conditions on the rows, both the oracle's alone.  The relu margin
    (_select), at every step.  And Adam's conditioning: its step is lr m / (sqrt(v) + 1e-8), of size lr whatever the gradient's,
    so an element whose gradient lies within f32's reach of zero moves by a fraction of lr = 3e-4 that no f32 sum can be held
    to.  The oracle's own float32 restatement of the three steps (e32: its largest weight or slot error against float64, in
    _check's measure) says whether the rows have such elements, and it often does, up to 9e-5; a case is kept when
    e32 <= WTOL / 4, the 4 for the order of the device's sums, as in the test above.  The first seed of base, base + 1000, ...
    that meets both is the case; the search runs here on the CPU and knows nothing of the device."""
    kw = dict(_okw(cfg), beta=beta)
    rms = cfg.get("RMSPROP", True)
    nz = noise.astype(np.float64)
    for k in range(tries):
        rng = np.random.Generator(np.random.PCG64(base + 1000 * k))
        online, target = o.random_params(S, A, rng), o.random_params(S, A, rng)
        st, s32 = po.new_state(online, target, critic_rmsprop=rms), po.new_state(_f32(online), _f32(target), critic_rmsprop=rms)
        s32["slot_a"], s32["slot_b"] = _f32(s32["slot_a"]), _f32(s32["slot_b"])
        batches = []
        try:
            for _ in range(steps):
                b = _select(st, _candidates(S, A, 2 * B, rng), B,
                            lambda trial, rows: po.train_step(trial, *rows, LR, nz, stop_after=4, **kw))
                po.train_step(st, *_f64(b), LR, nz, **kw)
                po.train_step(s32, *b, np.float32(LR), noise, mixed=True, **kw)
                batches.append(b)
        except AssertionError:
            continue
        e32 = max(float(np.max(np.abs(s32[p][v].astype(np.float64) - st[p][v]))) / max(1.0, float(np.max(np.abs(st[p][v]))))
                  for p in ("online", "target", "slot_a", "slot_b") for v in o.TRAINABLE)
        if e32 <= WTOL / 4:
            return online, target, batches, e32
    raise AssertionError("no seed in %d gave rows that meet both conditions" % tries)


@pytest.mark.parametrize("S,A", SHAPES)
@pytest.mark.parametrize("B", SIZES)
@pytest.mark.parametrize("case", FULL, ids=[c[0] for c in FULL])
def test_three_full_steps(S, A, B, case):
    cfg, beta = case[1], 0.1
    kw = dict(_okw(cfg), beta=beta, mixed=False)
    noise = np.full(A, 0.05, np.float32)
    online, target, batches, e32 = _full_case(S, A, B, cfg, beta, noise, 604 + B + S)
    print("the oracle's own float32 run is within %.3e of its float64 run on these rows" % e32)
    st = po.new_state(online, target, critic_rmsprop=cfg.get("RMSPROP", True))
    net = _pnet(S, A, beta=beta, **cfg)
    try:
        _load(net, online, target)
        for i, b in enumerate(batches):
            out = po.train_step(st, *_f64(b), LR, noise.astype(np.float64), **kw)
            assert net.replay_add(*b) == ((i + 1) * B, (i + 1) * B)
            q_max, q_avg = net.train_replay(np.arange(i * B, (i + 1) * B, dtype=np.int32), noise=noise)
            _compare_rows(net, out, B)
            _check("g", net.fetch("g", B * A), out["g"])
            _check("step %d q_max" % i, [q_max], [out["q_max"]])          # return units
            _check("step %d q_avg" % i, [q_avg], [out["q_avg"]])
            for k in o.CRITIC_TRAINABLE:
                _check("grad " + k, net.get_variable_value(k, 4), out["critic_grads"][k])
            mu, nu = _stats(net)
            _check("mu", [mu], [st["mu"]], WTOL)
            _check("nu", [nu], [st["nu"]], WTOL)
        assert net.get_global_step() == 3 and st["mu"] != 0.0
        for k in o.TRAINABLE:
            _check("online " + k, net.get_variable_value(k, 0), st["online"][k], WTOL)
            _check("target " + k, net.get_variable_value(k, 1), st["target"][k], WTOL)
            _check("slot a " + k, net.get_variable_value(k, 2), st["slot_a"][k], WTOL)
            _check("slot b " + k, net.get_variable_value(k, 3), st["slot_b"][k], WTOL)
    finally:
        net.close()


def test_a_step_on_rows_with_their_own_discounts():
    S, A, B, beta = 3, 1, 17, 0.1
    noise = np.full(A, 0.05, np.float32)
    rng = np.random.Generator(np.random.PCG64(71))
    disc = (np.float32(0.99) ** rng.integers(1, 6, B)).astype(np.float32)
    online, target = o.random_params(S, A, rng), o.random_params(S, A, rng)
    st = po.new_state(online, target, mu=-1.5, nu=3.0)
    kw = dict(_okw({}), beta=beta, disc=disc.astype(np.float64))
    b = _select(st, _candidates(S, A, 2 * B, rng), B,
                lambda trial, rows: po.train_step(trial, *rows, LR, noise.astype(np.float64), stop_after=4, **kw))
    net = _pnet(S, A, beta=beta)
    try:
        net.nstep_create(5)
        _load(net, online, target)
        _set_stats(net, -1.5, 3.0)
        assert net.replay_add(*b) == (B, B)
        full = np.full(net.replay_capacity, np.float32(0.99), np.float32)
        full[:B] = disc
        net.set_nstep_discounts(full)
        out = po.train_step(st, *_f64(b), LR, noise.astype(np.float64), **kw)
        q_max, q_avg = net.train_replay(np.arange(B, dtype=np.int32), noise=noise)
        assert _eq(net.fetch("disc", B), disc)
        _compare_rows(net, out, B)
        _check("q_max", [q_max], [out["q_max"]])
        _check("q_avg", [q_avg], [out["q_avg"]])
        for k in o.TRAINABLE:
            _check("online " + k, net.get_variable_value(k, 0), st["online"][k], WTOL)
            _check("target " + k, net.get_variable_value(k, 1), st["target"][k], WTOL)
    finally:
        net.close()


def test_a_prioritised_step():
    S, A, n, B, beta, beta_is = 3, 1, 64, 33, 0.1, 0.4
    noise = np.full(A, 0.05, np.float32)
    pa = _random_priorities(n, n, np.random.default_rng(5))
    slots, w = per.sample(pa, n, B, PER_SEED, 0, beta_is)
    rng = np.random.Generator(np.random.PCG64(73))
    online, target = o.random_params(S, A, rng), o.random_params(S, A, rng)
    kw = dict(_okw({}), beta=beta)
    # n ring rows with the margin under the initial weights; the batch rows[slots] keeps it after step 3 as well
    cand = _candidates(S, A, 3 * n, rng)
    ok = o.relu_margin(online, target, cand[0], cand[1], cand[4]) > 1e-4
    for _ in range(50):
        keep = np.flatnonzero(ok)[:n]
        assert keep.size == n, "only %d of %d candidate rows qualify" % (keep.size, ok.size)
        rows = tuple(t[keep] for t in cand)
        batch = _f64(tuple(t[slots] for t in rows))
        trial = po.new_state(online, target)
        out = po.train_step(trial, *batch, LR, noise.astype(np.float64), w=w.astype(np.float64), stop_after=4, **kw)
        bad = np.abs(o.critic_forward(trial["online"], batch[0], out["a_out"])["t"]).min(axis=1) <= 1e-4
        if not bad.any():
            break
        ok[keep[slots[bad]]] = False
    else:
        raise AssertionError("the choice of rows did not settle")
    net = _pnet(S, A, beta=beta, PRIORITIZED_REPLAY=True, PRIORITIZED_REPLAY_ALPHA=0.6, PRIORITIZED_REPLAY_EPS=0.01,
                REPLAY_BUFFER_RANDOM_SEED=PER_SEED, capacity=n)
    try:
        _load(net, online, target)
        assert net.replay_add(*rows) == (n, n)
        net.set_priorities(pa, 2.0)
        net.replay_beta = beta_is
        q_max, q_avg = net.train_prioritized(B, noise=noise)
        w_dev = net.fetch("per_w", B)
        assert np.array_equal(net.last_slots, slots) and np.allclose(w_dev, w, rtol=1e-6, atol=0.0)
        st = po.new_state(online, target)
        out = po.train_step(st, *batch, LR, noise.astype(np.float64), w=w_dev.astype(np.float64), **kw)
        _compare_rows(net, out, B)
        _check("q_max", [q_max], [out["q_max"]])
        _check("q_avg", [q_avg], [out["q_avg"]])
        yn, q = net.fetch("yn", B), net.fetch("q", B)
        td = net.fetch("per_td", B)
        assert _eq(td, np.abs(yn - q))                                    # scale-free: the normalised TD error
        got_pa, top = net.priorities()
        want_pa = pa.copy()
        want_top = per.update(want_pa, 2.0, slots, yn, q, 0.01, 0.6)
        assert top == want_top and np.max(np.abs(got_pa - want_pa) / np.maximum(want_pa, 1e-30)) <= 1e-6
        for k in o.TRAINABLE:
            _check("online " + k, net.get_variable_value(k, 0), st["online"][k], WTOL)
    finally:
        net.close()


# ---- 5. determinism, 6. checkpoints

def _state(net):
    """Everything a checkpoint holds but the step: the writable arenas of the 26 and both copies of the statistics."""
    return {**_arenas(net, which=(0, 1, 2, 3)), **_arenas(net, (MU, NU), (0, 1))}


def _three_steps(net, rows, B, noise, first=0, last=3):
    for i in range(first, last):
        net.train_replay(np.arange(i * B, (i + 1) * B, dtype=np.int32), noise=noise)
    return _state(net)


def test_determinism_checkpoints_and_cross_refusals(tmp_path):
    S, A, B, beta = 3, 1, 17, 0.1
    rng = np.random.Generator(np.random.PCG64(81))
    online, target = o.random_params(S, A, rng), o.random_params(S, A, rng)
    rows = tuple(t[:3 * B] for t in _candidates(S, A, 6 * B, rng))
    noise = np.full(A, 0.05, np.float32)
    path, plain_path = str(tmp_path / "popart.npz"), str(tmp_path / "plain.npz")
    runs = []
    for _ in range(2):
        net = _pnet(S, A, beta=beta)
        try:
            _load(net, online, target)
            net.replay_add(*rows)
            two = _three_steps(net, rows, B, noise, 0, 2)
            if not runs:
                net._lib.ga3c_ddpg_save(net._h, path.encode())
            runs.append((two, _three_steps(net, rows, B, noise, 2, 3), net.fetch("yn", B), net.logging))
        finally:
            net.close()
    assert _same(runs[0][0], runs[1][0]) and _same(runs[0][1], runs[1][1]) and _eq(runs[0][2], runs[1][2]) and runs[0][3] == runs[1][3]
    assert float(runs[0][1][(MU, 0)][0]) != 0.0 and not _same(runs[0][0], runs[0][1])
    with np.load(path) as z:
        assert int(z["step"]) == 2 and len(z.files) == 1 + 2 * 26 + 2 * 20 + 4
        for name, key in (("critic_popart/mu:0", (MU, 0)), ("critic_popart_1/mu:0", (MU, 1)), ("critic_popart/nu:0", (NU, 0)),
                          ("critic_popart_1/nu:0", (NU, 1))):
            assert z[name].shape == (1,) and _eq(z[name], runs[0][0][key]), name
    fresh, plain = _pnet(S, A, beta=beta), _pnet(S, A, popart=False)
    try:
        fresh.load_file(path)
        assert fresh.get_global_step() == 2
        assert _same(runs[0][0], _state(fresh))
        fresh.replay_add(*rows)
        assert _same(runs[0][1], _three_steps(fresh, rows, B, noise, 2, 3)) and _eq(fresh.fetch("yn", B), runs[0][2])
        # cross-refusals, handles untouched
        _load(plain, online, target)
        plain._lib.ga3c_ddpg_save(plain._h, plain_path.encode())
        with np.load(plain_path) as z:
            assert len(z.files) == 1 + 2 * 26 + 2 * 20
        before, before_plain = _arenas(fresh, o.ALL_VARS + (MU, NU), (0, 1, 2, 3)), _arenas(plain, which=(0, 1, 2, 3))
        with pytest.raises(RuntimeError, match="critic_popart/mu"):
            fresh.load_file(plain_path)
        with pytest.raises(RuntimeError, match="PopArt"):
            plain.load_file(path)
        assert _same(before, _arenas(fresh, o.ALL_VARS + (MU, NU), (0, 1, 2, 3))) and fresh.get_global_step() == 3
        assert _same(before_plain, _arenas(plain, which=(0, 1, 2, 3))) and plain.get_global_step() == 0
    finally:
        fresh.close()
        plain.close()


# ---- 7. return codes

def test_return_codes():
    import ga3c_amd  # noqa: F401
    import _native as nat
    lib = nat.hip_lib()
    S, A = 3, 1
    net, fork = _pnet(S, A, popart=False, max_batch=32, capacity=64), _pnet(S, A, popart=False, DDPG_CRITIC_LOSS="fork")
    twin, dist = _pnet(S, A, popart=False, DDPG_TWIN=True), _pnet(S, A, popart=False, DDPG_DISTRIBUTIONAL=True)
    buf = np.zeros(64, np.float32)
    f = nat.ptr(buf)
    try:
        h = net._h
        create, destroy, info = lib.ga3c_ddpg_popart_create, lib.ga3c_ddpg_popart_destroy, lib.ga3c_ddpg_popart_info
        # without it: GA3C_ESTATE, and no such variable
        assert destroy(h) == ESTATE and info(h, f, f, f, f) == ESTATE
        assert lib.ga3c_ddpg_fetch(h, b"yn", f, 1) == ESTATE
        assert lib.ga3c_ddpg_get_param(h, MU.encode(), 0, f, 1) == EINVAL and lib.ga3c_ddpg_num_params(h) == 26
        nan, inf = float("nan"), float("inf")
        for bad in ((-0.1, 1e-4, 1e6), (1.5, 1e-4, 1e6), (nan, 1e-4, 1e6), (inf, 1e-4, 1e6), (0.1, 0.0, 1e6), (0.1, -1.0, 1e6),
                    (0.1, 2.0, 2.0), (0.1, 2.0, 1.0), (0.1, nan, 1e6), (0.1, 1e-4, nan), (0.1, 1e-4, inf), (0.1, inf, inf)):
            assert create(h, *bad) == EINVAL, bad
        assert create(None, 0.1, 1e-4, 1e6) == EINVAL and lib.ga3c_ddpg_num_params(h) == 26
        assert create(fork._h, 0.1, 1e-4, 1e6) == ESTATE
        assert create(twin._h, 0.1, 1e-4, 1e6) == ESTATE and lib.ga3c_ddpg_num_params(twin._h) == 38
        assert create(dist._h, 0.1, 1e-4, 1e6) == ESTATE and lib.ga3c_ddpg_num_params(dist._h) == 26
        for beta in (0.0, 1.0):                 # the ends of the range are taken
            assert create(h, beta, 1e-4, 1e6) == 0 and destroy(h) == 0
        assert create(h, 0.25, 1e-3, 1e3) == 0 and create(h, 0.25, 1e-3, 1e3) == ESTATE
        assert lib.ga3c_ddpg_num_params(h) == 28
        assert [lib.ga3c_ddpg_param_name(h, i).decode() for i in (26, 27)] == [MU, NU]
        assert net.get_target_names()[26:] == ["critic_popart_1/mu:0", "critic_popart_1/nu:0"]
        assert net._param_info(MU) == (1, (1,), False) and net._param_info(NU) == (1, (1,), False)
        assert net._param_info("critic_output/W")[2] and not net._param_info("critic_norm1/moving_mean")[2]
        for which, want in ((0, (0.0, 1.0)), (1, (0.0, 1.0)), (2, (0.0, 0.0)), (3, (0.0, 0.0)), (4, (0.0, 0.0))):
            assert (float(net.get_variable_value(MU, which)[0]), float(net.get_variable_value(NU, which)[0])) == want, which
        assert lib.ga3c_ddpg_twin_create(h, 2, 0.2, 0.5, 1) == ESTATE and lib.ga3c_ddpg_dist_create(h, 51, -100.0, 0.0) == ESTATE
        assert lib.ga3c_ddpg_num_params(h) == 28
        assert info(h, None, None, None, None) == 0 and info(None, f, f, f, f) == EINVAL
        assert net.popart_info() == (0.25, 0.0, 1.0, 1.0)
        _set_stats(net, -3.0, 9.0)              # zero variance: the lower clamp
        assert net.popart_info() == (0.25, -3.0, 9.0, float(np.float32(1e-3)))
        _set_stats(net, 0.0, 1e12)
        assert net.popart_info()[3] == 1e3
        _set_stats(net, 0.0, 1.0)
        rows = _candidates(S, A, 16, np.random.default_rng(0))
        net.train(rows[0], rows[2], rows[1], rows[4], rows[3], noise=False)
        assert lib.ga3c_ddpg_fetch(h, b"yn", f, 17) == EINVAL and lib.ga3c_ddpg_fetch(h, b"yn", f, 16) == 0
        # priorities, n-step returns and device actors attach to it; destroy gives the 26 back
        assert lib.ga3c_ddpg_priorities_create(h, 0.6, 0.01, 1) == 0 and lib.ga3c_ddpg_nstep_create(h, 3) == 0
        assert lib.ga3c_ddpg_actors_create(h, 4, 1, 1) == 0 and lib.ga3c_ddpg_actors_destroy(h) == 0
        assert destroy(h) == 0 and destroy(h) == ESTATE and lib.ga3c_ddpg_num_params(h) == 26
        assert lib.ga3c_ddpg_get_param(h, MU.encode(), 0, f, 1) == EINVAL and lib.ga3c_ddpg_fetch(h, b"yn", f, 16) == ESTATE
        assert lib.ga3c_ddpg_twin_create(h, 2, 0.2, 0.5, 1) == 0      # ... and what it excluded is possible again
        assert create(h, 0.1, 1e-4, 1e6) == ESTATE
        assert lib.ga3c_ddpg_twin_destroy(h) == 0 and create(h, 0.1, 1e-4, 1e6) == 0
    finally:
        for n in (net, fork, twin, dist):
            n.close()              # destroy with PopArt attached


# ---- 8. device actors

def _actor_run(beta, popart=True):
    net = _pnet(3, 1, beta=beta, popart=popart, max_batch=16, capacity=256)
    try:
        online, target = _weights(31)
        for P in (online, target):              # a critic that starts near zero, as the product's does: y is near r
            for k in (po.WO, po.BO):
                P[k] = (P[k] * 0.01).astype(np.float32).astype(np.float64)
        _load(net, online, target)
        net.actors_create(5, seed=5, updates=2, batch=16, draw_seed=DRAW_SEED)
        stats = [net.actors_run(20, train=True, noise=[0.3]) for _ in range(2)]
        fields = {k: net.actors_get(k) for k in ("phys", "elapsed", "draws", "obs", "action", "reward", "done", "slots")}
        size, total = net.replay_size()
        out = dict(stats=stats, fields=fields, ring=_ring_rows(net, range(size)), arenas=_arenas(net), logging=net.logging,
                   step=net.get_global_step(), episodes=net.actors_episodes())
        if popart:
            out["popart"] = (net.popart_info(), net.fetch("yn", 16), net.get_variable_value(MU, 1), net.get_variable_value(NU, 1))
        return out
    finally:
        net.close()


def test_device_actors_with_popart():
    plain, zero = _actor_run(0.0, popart=False), _actor_run(0.0)
    assert plain["stats"][0][1] > 0 and plain["stats"][1] == (100, 40, 640, 0) and plain["step"] == zero["step"] > 40
    for k in ("stats", "logging", "step", "episodes"):
        assert plain[k] == zero[k], k
    assert _same(plain["fields"], zero["fields"]) and _eq(plain["ring"], zero["ring"]) and _same(plain["arenas"], zero["arenas"])
    assert zero["popart"][0] == (0.0, 0.0, 1.0, 1.0)
    a, b = _actor_run(0.1), _actor_run(0.1)
    for k in ("stats", "logging", "step", "episodes"):
        assert a[k] == b[k], k
    assert _same(a["fields"], b["fields"]) and _eq(a["ring"], b["ring"]) and _same(a["arenas"], b["arenas"])
    assert a["popart"][0] == b["popart"][0] and all(_eq(x, y) for x, y in zip(a["popart"][1:], b["popart"][1:]))
    (_, mu, nu, sigma) = a["popart"][0]
    rewards = a["ring"][:, 4]
    print("mu %.6g nu %.6g sigma %.6g; the ring's rewards average %.6g; Q %r" % (mu, nu, sigma, rewards.mean(), a["logging"]))
    assert rewards.max() < 0.0 and 2.0 * rewards.mean() < mu < 0.5 * rewards.mean()      # from 0 to y = r + gamma q', q' still small
    assert _eq(a["popart"][2], np.array([mu], np.float32)) and _eq(a["popart"][3], np.array([nu], np.float32))
    assert all(np.all(np.isfinite(v)) for v in a["arenas"].values()) and np.all(np.isfinite(a["popart"][1]))
    assert np.all(np.isfinite(a["logging"])) and not _same(a["arenas"], zero["arenas"])


# ---- 9. the server

@pytest.mark.timeout(120)
def test_server_runs_the_device_actors_with_popart(tmp_path, monkeypatch):
    import ga3c_amd  # noqa: F401
    from Config import Config
    monkeypatch.chdir(tmp_path)
    for k, v in (("GAME", "Pendulum-v0"), ("USE_DDPG", True), ("DEVICE_AGENTS", 64), ("DEVICE_DDPG", True),
                 ("DYNAMIC_SETTINGS", False), ("SAVE_MODELS", False), ("TRAINING_MIN_BATCH_SIZE", 64),
                 ("DDPG_CRITIC_LOSS", "paired"), ("DDPG_POPART", True), ("CONTINUOUS_INPUT", Config.CONTINUOUS_INPUT),
                 ("DISCRATE_INPUT", Config.DISCRATE_INPUT), ("DISCOUNTING", Config.DISCOUNTING),
                 ("USE_REPLAY_MEMORY", Config.USE_REPLAY_MEMORY)):
        monkeypatch.setattr(Config, k, v)
    from Server import Server
    srv = Server()
    try:
        model = srv.model
        assert model.popart and model.popart_info() == (float(np.float32(3e-4)), 0.0, 1.0, 1.0)
        assert model.get_variables_names()[26:] == [MU + ":0", NU + ":0"]
        srv.main(max_seconds=4)
        assert srv.failure is None and srv.training_step > 0 and model.get_global_step() == srv.training_step
        assert open("results.txt").read().strip(), "no episode was logged"
        _, mu, nu, sigma = model.popart_info()
        q_max, q_avg = model.logging
        assert mu < 0.0 and np.isfinite([mu, nu, sigma, q_max, q_avg]).all()
        # Q is logged in return units: sigma n + mu of the last step's normalised predictions
        n = model.fetch("q", 64).astype(np.float64)
        _check("q_max", [q_max], [sigma * n.max() + mu])
        _check("q_avg", [q_avg], [sigma * n.mean() + mu])
        model.log(training_step=srv.training_step)
        scalars = np.loadtxt(os.path.join("logs", model.model_name, "scalars.csv"), delimiter=",", ndmin=2)
        assert scalars.shape == (1, 4) and np.allclose(scalars[0, 2:], [q_max, q_avg], rtol=1e-6)
        stats = np.loadtxt(os.path.join("logs", model.model_name, "popart.csv"), delimiter=",", ndmin=2)
        assert stats.shape == (1, 4) and np.allclose(stats[0, 1:], [mu, nu, sigma], rtol=1e-6)
    finally:
        srv.model.close()
