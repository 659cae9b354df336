"""-m gpu: the device actors for Pendulum-v0 (Config.DEVICE_PENDULUM, ga3c_mlp_actors_*) against
tests/device_pendulum_oracle.py, which tests/test_device_pendulum_cpu.py holds to the real ProcessAgent.  The Pendulum
network, S = 3 and A = 1; N on both sides of the 16-row tile of the network's kernels, in one and in two workgroups of the
step kernel; N = 1025 and 2500 for the one-workgroup scan with two and three environments per thread.

Exact: done, elapsed, counters, u == -1, draws (they move only at a reset), the action (the prediction row, bit for bit), the
reward (products and one fmod on the device's own pre-step physics and action: no transcendental function), the thdot
observation (the f32 cast), rollout rows, action rows, y_r, batch order, episode records, reset physics, and the arenas after
a train step against ga3c_mlp_train on the same batch.  Bounded: the new physics and the cos / sin observations, whose sin
and cos are the device library's and not numpy's -- PHYS_BOUND and OBS_BOUND below."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import device_agents_oracle as o
import device_pendulum_oracle as po
import mlp_oracle as m
from test_gpu_device_agents import SCAN_SIZES, _forced

pytestmark = pytest.mark.gpu

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ga3c_amd")
SIZES = [1, 15, 16, 17, 33, 300]
GAMMA = 0.99
TOL = 1e-4
S, A = 3, 1
# worst |got - want| / max(1, |want|) over the inputs of test_one_forced_step, measured on an MI355X: of the
# f64 physics after one step (PHYS_MEASURED) and of the f32 cos / sin observations against numpy's on the device's own new
# physics (OBS_MEASURED).  The assertions are at 8 times the measured value, under caps of 1e-12 and 2^-22; a measured 0
# asserts bits.  Measured: the physics 2.193e-16 at N = 300 and 0 at every other N (one ulp of a thdot' near 1.5, from one sin
# that rounds the other way); the observations 0 at every N -- on these inputs the device library's cos and sin, cast to
# f32, are numpy's.
PHYS_MEASURED = 2.193e-16
OBS_MEASURED = 0.0
PHYS_BOUND = 8 * PHYS_MEASURED
OBS_BOUND = 8 * OBS_MEASURED
assert PHYS_BOUND <= 1e-12 and OBS_BOUND <= 2.0 ** -22


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _rel(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(np.max(np.abs(got - want) / np.maximum(1.0, np.abs(want)))) if got.size else 0.0


@pytest.fixture(scope="module")
def params():
    p = m.init_params(S, A, seed=777)
    rng = np.random.default_rng(5)                    # head biases wide enough for a policy that is not nearly constant
    p["logits_p/out_x/b"] = rng.uniform(-1.5, 1.5, A).astype(np.float32).astype(np.float64)
    p["logits_p/out_y/b"] = rng.uniform(-1.5, 1.5, A).astype(np.float32).astype(np.float64)
    return p


def _net(params, max_batch, clip=False, dual=False, state_dim=S, num_actions=A):
    import ga3c_amd  # noqa: F401
    from Config import Config
    from NetworkVP_vector import Network
    saved = {k: getattr(Config, k) for k in ("DUAL_RMSPROP", "USE_GRAD_CLIP", "GRAD_CLIP_NORM")}
    Config.DUAL_RMSPROP, Config.USE_GRAD_CLIP, Config.GRAD_CLIP_NORM = dual, clip, 1.0
    try:
        net = Network("gpu:0", "pendulum_actors", num_actions, (state_dim,), max_batch=max_batch, predict_lanes=1)
    finally:
        for k, v in saved.items():
            setattr(Config, k, v)
    if params is not None:
        net.set_arena(0, m.flat(params))
    return net


def _cases(rng, count):
    """Physics for forced steps -> (phys[count,2], elapsed, started).  th 2e-6 on both sides of +-pi; th several turns from
    0; thdot where the step lands beyond the +-8 clip, short of it, and at 8 exactly with no gravity term to speak of (the
    action's sign decides the side); elapsed = 199 and 198; first ever steps (one at elapsed = 199: its done is ignored)."""
    phys = np.stack([rng.uniform(-np.pi, np.pi, size=count), rng.uniform(-6.0, 6.0, size=count)], axis=1)
    elapsed = rng.integers(0, 190, size=count).astype(np.int32)
    started = np.ones(count, np.int32)
    fixed = [(s * (np.pi + d), w) for s in (1.0, -1.0) for d in (-2e-6, 2e-6) for w in (0.3,)]
    fixed += [(25.0, -1.0), (-40.0, 2.0), (7 * np.pi + 0.1, 0.5), (-9 * np.pi - 0.2, -0.5)]
    fixed += [(s * np.pi / 2, s * 7.9) for s in (1.0, -1.0)] + [(s * np.pi / 2, s * 6.5) for s in (1.0, -1.0)]
    fixed += [(0.0, 8.0), (0.0, -8.0)]
    for k, (th, thdot) in enumerate(fixed):
        if k < count:
            phys[k] = [th, thdot]
    for idx, (el, st) in zip(range(len(fixed), len(fixed) + 4), ((199, 1), (198, 1), (199, 0), (5, 0))):
        if idx < count:
            elapsed[idx], started[idx] = el, st
    return phys, elapsed, started


def _safe_obs(params, rng, n):
    """n observations away from the atan2 branch cut, where the f32 head and the f64 oracle may land on opposite sides."""
    x = rng.uniform(-1.5, 1.5, size=(3 * n + 16, S)).astype(np.float32)
    x = x[m.safe_rows(params, x.astype(np.float64), 1e-3)][:n]
    assert x.shape[0] == n
    return x


@pytest.mark.parametrize("n", SIZES)
def test_one_forced_step(params, n, capsys):
    time_max, seed = 5, 2024 + n
    net = _net(params, max(16, n * (time_max + 1)))
    rng = np.random.Generator(np.random.PCG64(n))
    total = max(24, n)
    phys_all, elapsed_all, started_all = _cases(rng, total)
    worst_phys = worst_obs = 0.0
    clipped = unclipped = 0
    try:
        for lo in range(0, total, n):
            idx = np.arange(lo, lo + n) % total
            phys, elapsed, started = phys_all[idx].copy(), elapsed_all[idx].copy(), started_all[idx].copy()
            tc = rng.integers(0, time_max + 1, size=n).astype(np.int32)
            draws = 2 * rng.integers(2, 1 << 39, size=n).astype(np.uint64)
            obs = _safe_obs(params, rng, n)
            net.actors_create(n, time_max, GAMMA, seed)
            for name, val in (("phys", phys), ("elapsed", elapsed), ("started", started), ("time_count", tc), ("draws", draws),
                              ("obs", obs)):
                net.actors_set(name, val)
                assert _same(net.actors_get(name), val), name
            on = started == 1
            want_done = elapsed + 1 >= po.TIME_LIMIT
            reset = on & want_done                                  # a first ever step's done is ignored
            assert net.actors_run(1, train=False) == (n, 0, 0, int(reset.sum()))
            g = {k: net.actors_get(k) for k in ("phys", "elapsed", "time_count", "started", "draws", "obs", "p", "v", "u", "action",
                                                 "reward", "done", "cut", "rollout_len")}
            assert g["p"].shape == g["action"].shape == (n, A) and g["phys"].shape == (n, 2) and g["obs"].shape == (n, S)
            # predictions: the network's own kernel on the observation buffer
            p_ref, v_ref, _ = net.predict_p_v_logits(obs)
            assert _same(g["p"], p_ref) and _same(g["v"], v_ref)
            f = m.forward(params, obs.astype(np.float64))
            assert np.max(np.abs(g["p"] - f["o"])) <= TOL and np.max(np.abs(g["v"] - f["v"])) <= TOL * max(1.0, np.max(np.abs(f["v"])))
            assert np.all(np.abs(g["p"]) <= 1.0)
            # the action is the prediction row, the zero vector on a first ever step; no draw for it
            assert _same(g["action"], np.where(on[:, None], g["p"], np.float32(0.0)))
            assert np.all(g["u"] == -1.0)
            assert np.array_equal(g["draws"], draws + np.uint64(2) * reset.astype(np.uint64))
            assert np.array_equal(g["done"] != 0, want_done) and np.all(g["started"] == 1)
            assert np.array_equal(g["elapsed"], np.where(reset, 0, elapsed + 1))
            cut = on & (want_done | (tc == time_max))
            assert np.array_equal(g["cut"], cut.astype(np.int32))
            assert np.array_equal(g["time_count"], np.where(~on, tc, np.where(want_done, 0, np.where(cut, 1, tc + 1))))
            assert np.array_equal(g["rollout_len"], np.where(on & ~want_done, 1, 0))
            assert net.actors_get("batch_rows") == int(cut.sum())
            # the oracle's step on the device's own pre-step physics and action
            stepped, reward = zip(*[po.PendulumEnv.step(phys[i], g["action"][i]) for i in range(n)])
            stepped, reward = np.array(stepped), np.array(reward, np.float64)
            assert _same(g["reward"], reward)
            assert np.all(reward <= -1.0) and np.all(reward >= -1.09)
            keep = ~reset
            worst_phys = max(worst_phys, _rel(g["phys"][keep], stepped[keep]))
            clipped += int(np.sum(np.abs(g["phys"][keep][:, 1]) == 8.0))
            unclipped += int(np.sum(np.abs(g["phys"][keep][:, 1]) < 8.0))
            assert np.all(np.abs(g["phys"][keep][:, 1]) <= 8.0)
            # observations: thdot the exact cast of the device's physics, cos / sin against numpy's on the same physics
            assert _same(g["obs"][keep][:, 2], g["phys"][keep][:, 1].astype(np.float32))
            want_obs = np.array([po.PendulumEnv.observe(ph) for ph in g["phys"]])
            worst_obs = max(worst_obs, _rel(g["obs"][keep][:, :2], want_obs[keep][:, :2]))
            if reset.any():
                # the physics are the reset's own draws, bit for bit; the observation is of the stepped physics it replaced
                k = draws[reset]
                u0, u1 = (o.uniform(seed, np.arange(n)[reset], k + np.uint64(j)) for j in (0, 1))
                assert _same(g["phys"][reset], np.stack([-np.pi + (np.pi - -np.pi) * u0, -1.0 + (1.0 - -1.0) * u1], axis=1))
                gone = np.array([po.PendulumEnv.observe(ph) for ph in stepped[reset]])
                worst_obs = max(worst_obs, _rel(g["obs"][reset], gone))
            net.actors_destroy()
        with capsys.disabled():
            print("\n[device pendulum] N=%d: worst physics error %.3e (bound %.3e), worst cos / sin observation error %.3e "
                  "(bound %.3e); thdot at the clip %d, inside %d" % (n, worst_phys, PHYS_BOUND, worst_obs, OBS_BOUND, clipped, unclipped))
        assert worst_phys <= PHYS_BOUND
        assert worst_obs <= OBS_BOUND
        assert clipped >= 2 and unclipped >= 2
    finally:
        net.close()


@pytest.mark.parametrize("time_max", [2, 5])
@pytest.mark.parametrize("n", SIZES)
def test_forty_steps_follow_the_oracle(params, n, time_max):
    seed = 99 + n
    net = _net(params, max(16, n * (time_max + 1)))
    try:
        net.actors_create(n, time_max, GAMMA, seed)
        net.learning_rate, net.beta = 0.0, 0.01
        ora = po.PendulumActors(n, seed, time_max, GAMMA)
        assert _same(net.actors_get("phys"), np.array([e.phys for e in ora.env]))
        assert np.all(net.actors_get("draws") == 4) and not net.actors_get("started").any()
        elapsed = net.actors_get("elapsed")
        # these episodes end inside the run, on different steps; 171: 28 experiences, a last rollout short of TIME_MAX + 1 rows
        # at TIME_MAX 2 and 5; 199: a rollout of one row
        elapsed[::3] = 171 + (7 * np.arange(len(elapsed[::3]))) % 29
        net.actors_set("elapsed", elapsed)
        for e, el in zip(ora.env, elapsed):
            e.elapsed = int(el)
        theta0 = net.get_arena(0)
        stale, carried, carried_a = {}, {}, {}                      # env -> the observation / row / action row its next rollout must begin with
        seen = dict(stale=0, carried=0, limit=0, short=0, ends=set())
        for step in range(40):
            phys = net.actors_get("phys")
            for e, ph in zip(ora.env, phys):                        # re-seeded from the device's physics before every step
                e.phys = ph.copy()
            draws = net.actors_get("draws")
            stats = net.actors_run(1, train=True)
            g = {k: net.actors_get(k) for k in ("phys", "elapsed", "obs", "p", "u", "action", "reward", "done", "cut", "draws",
                                                 "time_count")}
            res, batch, episodes = ora.step(g["p"], actions=g["action"], dones=g["done"], rewards=g["reward"])
            rows = net.actors_get("batch_rows")
            assert stats == (n, int(rows > 0), rows, len(episodes))
            at = 0
            bx, by, ba = (net.actors_get(k) for k in ("batch_x", "batch_y_r", "batch_a")) if rows else (None, None, None)
            for i, (r, e) in enumerate(zip(res, ora.env)):
                assert g["u"][i] == -1.0 == r["u"], (step, i)
                assert r["own_done"] == bool(g["done"][i]), (step, i)
                assert _same(np.float64(r["own_reward"]), g["reward"][i]), (step, i)
                assert _same(r["own_action"], g["p"][i] if step else np.zeros(A, np.float32)) and _same(r["own_action"], g["action"][i])
                assert e.elapsed == g["elapsed"][i] and e.time_count == g["time_count"][i] and e.rng.draws == int(g["draws"][i])
                if r["episode"] is not None:                        # the reset: draws 2k and 2k + 1, the same bits
                    assert _same(e.phys, g["phys"][i])
                    k = int(draws[i])
                    assert k % 2 == 0 and int(g["draws"][i]) == k + 2
                    want = [-np.pi + (np.pi - -np.pi) * float(o.uniform(seed, i, k)), -1.0 + (1.0 - -1.0) * float(o.uniform(seed, i, k + 1))]
                    assert _same(g["phys"][i], np.array(want))
                    seen["limit"] += 1
                    seen["ends"].add(step)
                else:
                    assert int(g["draws"][i]) == int(draws[i])
                e.obs = g["obs"][i].copy()                          # the device's own observation (test_one_forced_step bounds it)
                if r["cut"] is not None:
                    T = len(r["cut"][2])
                    assert g["cut"][i] == T <= time_max + 1
                    x = bx[at:at + T]
                    if i in stale:                                  # the first action of an episode was predicted from the last
                        assert _same(x[0], stale.pop(i))            # observation of the episode before
                        seen["stale"] += 1
                    if i in carried:                                # the last row of a rollout is row 0 of the next
                        assert _same(x[0], carried.pop(i)) and T >= 2
                        assert _same(ba[at], carried_a.pop(i))
                        seen["carried"] += 1
                    seen["short"] += T < time_max + 1
                    if r["episode"] is None:
                        carried[i] = x[-1].copy()
                        carried_a[i] = ba[at + T - 1].copy()
                    at += T
                else:
                    assert g["cut"][i] == 0
                if r["episode"] is not None:
                    stale[i] = g["obs"][i].copy()
            if rows:
                assert at == rows
                for name, got, want in zip(("x", "a", "y_r"), (bx, ba, by), batch):
                    assert _same(got, want), (step, name)
            else:
                assert batch is None
            got_eps = net.actors_episodes()
            assert len(got_eps) == len(episodes)
            for (gr, gl), (wr, wl) in zip(got_eps, episodes):
                assert np.float64(gr).view(np.uint64) == np.float64(wr).view(np.uint64) and gl == wl
        assert _same(net.get_arena(0), theta0)                      # learning rate 0
        assert seen["stale"] and seen["carried"] and seen["limit"] and seen["short"], seen
        if n >= 15:
            assert len(seen["ends"]) > 1, "every episode ended on the same step"
    finally:
        net.close()


@pytest.mark.parametrize("n", SCAN_SIZES)
def test_the_scan_with_several_environments_per_thread(params, n):
    """The first cut at TIME_MAX = 2 is the fourth step, 3 rows of every environment; the forced episodes end on it.  The
    physics differ by environment (the seed's draws), so the rows and the records do: their order is held."""
    time_max, seed = 2, 7 + n
    net = _net(params, 3 * n)
    forced = _forced(n)
    try:
        net.actors_create(n, time_max, GAMMA, seed)
        ora = po.PendulumActors(n, seed, time_max, GAMMA)
        for step in range(4):
            if step == 3:
                elapsed = net.actors_get("elapsed")
                elapsed[forced] = 199
                net.actors_set("elapsed", elapsed)
                for i in forced:
                    ora.env[i].elapsed = 199
            for e, ph in zip(ora.env, net.actors_get("phys")):       # re-seeded from the device's physics before every step
                e.phys = ph.copy()
            stats = net.actors_run(1, train=False)
            g = {k: net.actors_get(k) for k in ("obs", "p", "action", "reward", "done", "elapsed", "draws")}
            res, batch, episodes = ora.step(g["p"], actions=g["action"], dones=g["done"], rewards=g["reward"])
            for i, (r, e) in enumerate(zip(res, ora.env)):
                assert r["own_done"] == bool(g["done"][i]) and e.elapsed == g["elapsed"][i] and e.rng.draws == int(g["draws"][i])
                assert _same(np.float64(r["own_reward"]), g["reward"][i]), (step, i)
                e.obs = g["obs"][i].copy()
            rows = net.actors_get("batch_rows")
            assert stats == (n, 0, 0, len(episodes))
            got_eps = net.actors_episodes()
            assert len(got_eps) == len(episodes)
            for (gr, gl), (wr, wl) in zip(got_eps, episodes):
                assert np.float64(gr).view(np.uint64) == np.float64(wr).view(np.uint64) and gl == wl
            if step < 3:
                assert rows == 0 and batch is None and not episodes
                continue
            assert rows == 3 * n and len(episodes) == len(forced) == len(set(episodes))
            assert np.array_equal(np.flatnonzero(g["done"]), forced)
            for name, want in zip(("batch_x", "batch_a", "batch_y_r"), batch):
                assert _same(net.actors_get(name), want), name
            assert len(np.unique(batch[0], axis=0)) > n              # the rows tell the environments apart
    finally:
        net.close()


@pytest.mark.parametrize("kind", ["plain", "grad_clip", "dual"])
def test_the_train_step_is_ga3c_mlp_train_on_the_fetched_batch(params, kind):
    n, time_max = 33, 2
    kw = dict(clip=kind == "grad_clip", dual=kind == "dual")
    arenas = range(7) if kind == "dual" else range(4)
    state = (0, 1, 2, 4, 5) if kind == "dual" else (0, 1, 2)
    net, twin = _net(params, 128, **kw), _net(params, 128, **kw)
    try:
        net.actors_create(n, time_max, GAMMA, 5)
        net.learning_rate, net.beta = 1e-2, 0.01
        twin.learning_rate, twin.beta = 1e-2, 0.01
        assert net.actors_run(3, train=True) == (3 * n, 0, 0, 0)    # the unpredicted step, then time_count 0 and 1: nothing cut
        before = {k: net.get_arena(k) for k in state}
        for k in state:
            twin.set_arena(k, before[k])
        assert net.actors_run(1, train=True) == (n, 1, n * (time_max + 1), 0)
        x, y, a = (net.actors_get(k) for k in ("batch_x", "batch_y_r", "batch_a"))
        assert x.shape == (99, S) and a.shape == (99, A) and y.shape == (99,)
        assert len(np.unique(a)) > 33 and np.all(np.abs(a) <= 1.0)  # action vectors, not one-hot rows
        twin.train(x, y, a)
        for k in arenas:
            assert _same(net.get_arena(k), twin.get_arena(k)), k
        assert not _same(net.get_arena(0), before[0]) and net.get_global_step() == twin.get_global_step() == 1
        if kind == "dual":
            assert not _same(net.get_arena(4), before[4])
    finally:
        net.close()
        twin.close()


def test_same_seed_same_bits_and_train_0_trains_nothing(params):
    n, time_max = 33, 5
    out = []
    for seed in (11, 11, 12):
        net = _net(params, n * (time_max + 1))
        try:
            net.actors_create(n, time_max, GAMMA, seed)
            net.learning_rate, net.beta = 1e-3, 0.01
            elapsed = net.actors_get("elapsed")
            elapsed[:] = 150 + np.arange(n) % 40                    # episodes finish inside the run
            net.actors_set("elapsed", elapsed)
            theta = net.get_arena(0)
            stats = net.actors_run(20, train=False)
            assert stats[:3] == (20 * n, 0, 0) and net.get_global_step() == 0
            assert all(_same(net.get_arena(k), w) for k, w in ((0, theta), (1, np.ones_like(theta)), (2, np.zeros_like(theta))))
            stats = net.actors_run(50, train=True)
            assert stats[0] == 50 * n and stats[1] == net.get_global_step() > 0 and stats[2] > stats[1] and stats[3] > 0
            out.append([net.get_arena(k) for k in range(3)] + [net.actors_get("phys"), net.actors_get("draws"),
                                                               np.array(net.actors_episodes())])
            assert not _same(out[-1][0], theta) and len(out[-1][5]) >= stats[3]
        finally:
            net.close()
    assert all(_same(a, b) for a, b in zip(out[0], out[1]))
    assert not _same(out[0][0], out[2][0]) and not _same(out[0][3], out[2][3])


def test_refusals_return_their_codes(params):
    import ga3c_amd  # noqa: F401
    import _native as nat
    lib = nat.hip_lib()
    EINVAL, ESTATE = -1, -4
    net = _net(params, 64)
    h = net._h
    buf = np.zeros(64, np.float64)
    vp = buf.ctypes.data_as(C.c_void_p)
    stats = np.zeros(4, np.int64)
    count = C.c_int32()
    try:
        assert lib.ga3c_mlp_actors_run(h, 1, 0.0, 0.0, 1, nat.ptr(stats, nat.i64p)) == ESTATE
        assert lib.ga3c_mlp_actors_destroy(h) == ESTATE
        assert lib.ga3c_mlp_actors_get(h, b"phys", vp, 16) == ESTATE
        assert lib.ga3c_mlp_actors_set(h, b"phys", vp, 16) == ESTATE
        assert lib.ga3c_mlp_actors_episodes(h, nat.ptr(buf, nat.f64p), nat.ptr(stats, nat.i64p), 4, C.byref(count)) == ESTATE
        assert lib.ga3c_mlp_actors_create(None, 4, 5, GAMMA, 1) == EINVAL
        for n, time_max in ((0, 5), (-1, 5), (4, 0), (11, 5), (64, 1)):          # 11 x 6 and 64 x 2 rows exceed max_batch 64
            assert lib.ga3c_mlp_actors_create(h, n, time_max, GAMMA, 1) == EINVAL, (n, time_max)
        assert b"max_batch" in lib.ga3c_last_error()
        assert lib.ga3c_mlp_actors_create(h, 10, 5, GAMMA, 1) == 0
        assert lib.ga3c_mlp_actors_create(h, 10, 5, GAMMA, 1) == ESTATE
        for steps in (0, -1, nat.ACTORS_MAX_STEPS + 1):
            assert lib.ga3c_mlp_actors_run(h, steps, 0.0, 0.0, 1, None) == EINVAL
        assert lib.ga3c_mlp_actors_run(h, nat.ACTORS_MAX_STEPS, 0.0, 0.0, 0, None) == 0
        assert lib.ga3c_mlp_actors_get(h, b"nothing", vp, 16) == EINVAL
        assert lib.ga3c_mlp_actors_get(h, b"phys", vp, 10 * 16 - 8) == EINVAL
        assert lib.ga3c_mlp_actors_get(h, b"phys", vp, 10 * 32) == EINVAL        # two f64 per environment, not CartPole's four
        assert lib.ga3c_mlp_actors_get(h, b"phys", None, 10 * 16) == EINVAL
        assert lib.ga3c_mlp_actors_get(h, b"phys", vp, 10 * 16) == 0
        assert lib.ga3c_mlp_actors_get(h, b"action", vp, 10 * 4) == 0            # f32 [n, 1]
        assert lib.ga3c_mlp_actors_set(h, b"p", vp, 10 * 4) == EINVAL            # read only
        assert lib.ga3c_mlp_actors_set(h, b"action", vp, 10 * 4) == EINVAL
        assert lib.ga3c_mlp_actors_set(h, b"batch_x", vp, 0) == EINVAL
        bad = np.full(10, 6, np.int32)
        assert lib.ga3c_mlp_actors_set(h, b"time_count", bad.ctypes.data_as(C.c_void_p), 40) == EINVAL
        bad[:] = -1
        assert lib.ga3c_mlp_actors_set(h, b"elapsed", bad.ctypes.data_as(C.c_void_p), 40) == EINVAL
        assert lib.ga3c_mlp_actors_episodes(h, None, None, 4, C.byref(count)) == EINVAL
        assert lib.ga3c_mlp_actors_destroy(h) == 0
        assert lib.ga3c_mlp_actors_destroy(h) == ESTATE
    finally:
        net.close()
    for state_dim, num_actions in ((4, 1), (3, 2)):                               # Pendulum has three state floats and one action
        other = _net(None, 64, state_dim=state_dim, num_actions=num_actions)
        try:
            assert lib.ga3c_mlp_actors_create(other._h, 4, 5, GAMMA, 1) == EINVAL
        finally:
            other.close()


def test_destroy_with_live_actors(params):
    import ga3c_amd  # noqa: F401
    import _native as nat
    net = _net(params, 64)
    net.actors_create(8, 5, GAMMA, 3)
    assert net.actors_run(7, train=True)[0] == 56
    h, net._h = net._h, None
    assert nat.hip_lib().ga3c_mlp_destroy(h) == 0     # frees the actors with the handle
    again = _net(params, 64)
    try:
        again.actors_create(8, 5, GAMMA, 3)
        assert again.actors_run(1, train=False) == (8, 0, 0, 0)
    finally:
        again.close()


@pytest.mark.timeout(120)
def test_train_script_runs_device_pendulum(tmp_path):
    env = dict(os.environ, PYTHONUNBUFFERED="1")
    run = subprocess.run(["timeout", "-k", "10", "90", "sh", os.path.join(PKG, "_train.sh"), "GAME=Pendulum-v0", "DEVICE_AGENTS=64",
                          "DEVICE_PENDULUM=True", "MAX_SECONDS=5"],
                         cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=110)
    assert run.returncode == 0, run.stdout[-3000:] + run.stderr[-3000:]
    assert "died" not in run.stdout + run.stderr
    status = [ln for ln in run.stdout.splitlines() if "TPS:" in ln]
    assert status and re.search(r"\[NT:  0 NP:  0 NA: 64\]", status[-1]), run.stdout[-2000:]
    tps = [int(t) for t in re.findall(r"TPS:\s*(\d+)\]", run.stdout)]
    assert max(tps) > 0
    lines = open(os.path.join(str(tmp_path), "results.txt")).read().strip().splitlines()
    # an episode is 200 steps; len(rollout) + 1 per rollout of TIME_MAX = 5 new steps and one carried row
    assert lines and all(1 <= int(ln.split(",")[2]) <= 200 + 2 * (200 // 5 + 1) for ln in lines)
    # the reward of a step lies in [-1.09, -1]
    assert all(-1.09 * 200 <= float(ln.split(",")[1]) <= -199 for ln in lines)
