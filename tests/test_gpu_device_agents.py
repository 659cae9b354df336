"""-m gpu: the device actors (Config.DEVICE_AGENTS, ga3c_dmlp_actors_*) against tests/device_agents_oracle.py,
which tests/test_device_agents_cpu.py holds to the real ProcessAgent.  Default network, S = 4 and A = 2; N on both sides of
the 16-row tile of the network's kernels, in one and in several workgroups of the step kernel; N = 1025 and 2500 for the
one-workgroup scan with two and three environments per thread.

Exact: uniforms, done, elapsed, rewards, counters, observations (the f32 cast of the device's own physics), rollout rows,
y_r, one-hot rows, batch order, episode records, and the arenas after a train step against ga3c_dmlp_train on the same
batch.  Bounded: the f64 physics, whose sin / cos are the device library's and not numpy's -- PHYS_BOUND below."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import device_agents_oracle as o
import dmlp_oracle as m

pytestmark = pytest.mark.gpu

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ga3c_amd")
SIZES = [1, 15, 16, 17, 33, 300]
GAMMA = 0.99
TOL = 1e-4
# worst |got - want| / max(1, |want|) of one physics step over the inputs of test_one_forced_step, measured on an MI355X
# (DESIGN.md 8i): PHYS_MEASURED; the assertion is at 8 times that, and the issue's cap on it is 1e-12.  Measured: 0 at every
# N -- on these inputs the device library's sin and cos round as glibc's do -- so the physics is held to the oracle's bits.
PHYS_MEASURED = 0.0
PHYS_BOUND = 8 * PHYS_MEASURED
assert PHYS_BOUND <= 1e-12
EDGE = 1e-9                 # a draw this close to a cdf edge is left out of the action comparison (at most 1 % may be)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


@pytest.fixture(scope="module")
def params():
    p = m.init_params(4, 2, seed=777)
    p["logits_p/w"] = (p["logits_p/w"] * 4.0).astype(np.float32).astype(np.float64)      # a policy that is not nearly uniform
    return p


def _net(params, max_batch, clip=False):
    import ga3c_amd  # noqa: F401
    from Config import Config
    from NetworkVP_discrate import Network
    saved = {k: getattr(Config, k) for k in ("DENSE_LAYERS", "DENSE_STACK", "USE_LOG_SOFTMAX", "MIN_POLICY", "DUAL_RMSPROP",
                                             "USE_GRAD_CLIP")}
    Config.DENSE_LAYERS, Config.DENSE_STACK, Config.USE_LOG_SOFTMAX, Config.MIN_POLICY = m.DEFAULT_LAYERS, "fork", False, 0.0
    Config.DUAL_RMSPROP, Config.USE_GRAD_CLIP = False, clip
    try:
        net = Network("gpu:0", "actors", 2, (4,), max_batch=max_batch, predict_lanes=1)
    finally:
        for k, v in saved.items():
            setattr(Config, k, v)
    net.set_arena(0, m.flat(params))
    return net


def _cases(rng, count):
    """Physics for forced steps -> (phys[count,4], elapsed, started).  The first 8 sit 2e-6 inside / outside each limit with
    the velocity that would move them zero, so the step leaves that coordinate where it is; then elapsed = 199; then first
    ever steps (one of them at elapsed = 199: its done is ignored); the rest are ordinary states."""
    phys = rng.uniform(-0.05, 0.05, size=(count, 4))
    phys[:, 0] = rng.uniform(-2.0, 2.0, size=count)
    phys[:, 1] = rng.uniform(-1.5, 1.5, size=count)
    phys[:, 2] = rng.uniform(-0.18, 0.18, size=count)
    phys[:, 3] = rng.uniform(-1.5, 1.5, size=count)
    elapsed = rng.integers(0, 190, size=count).astype(np.int32)
    started = np.ones(count, np.int32)
    k = 0
    for coord, limit in ((0, o.X_LIMIT), (2, o.THETA_LIMIT)):
        for sign in (1.0, -1.0):
            for margin in (-2e-6, 2e-6):
                if k < count:
                    phys[k] = [0.0, 0.0, 0.0, 0.0]
                    phys[k, coord] = sign * (limit + margin)
                    if coord == 0:
                        phys[k, 2], phys[k, 3] = 0.01, 0.2
                    k += 1
    for idx, (el, st) in zip(range(8, 12), ((199, 1), (198, 1), (199, 0), (5, 0))):
        if idx < count:
            elapsed[idx], started[idx] = el, st
    return phys, elapsed, started


@pytest.mark.parametrize("n", SIZES)
def test_one_forced_step(params, n, capsys):
    time_max, seed = 5, 2024 + n
    net = _net(params, max(16, n * (time_max + 1)))
    rng = np.random.Generator(np.random.PCG64(n))
    total = max(24, n)
    phys_all, elapsed_all, started_all = _cases(rng, total)
    worst, left_out, compared = 0.0, 0, 0
    try:
        for lo in range(0, total, n):
            idx = np.arange(lo, lo + n) % total
            phys, elapsed, started = phys_all[idx].copy(), elapsed_all[idx].copy(), started_all[idx].copy()
            tc = rng.integers(0, time_max + 1, size=n).astype(np.int32)
            draws = rng.integers(8, 1 << 40, size=n).astype(np.uint64)
            obs = rng.uniform(-1.5, 1.5, size=(n, 4)).astype(np.float32)
            net.actors_create(n, time_max, GAMMA, seed)
            for name, val in (("phys", phys), ("elapsed", elapsed), ("started", started), ("time_count", tc), ("draws", draws),
                              ("obs", obs)):
                net.actors_set(name, val)
                assert _same(net.actors_get(name), val), name
            assert net.actors_run(1, train=False) == (n, 0, 0, int(net.actors_get("done")[started == 1].sum()))
            g = {k: net.actors_get(k) for k in ("phys", "elapsed", "time_count", "started", "draws", "obs", "p", "v", "u", "action",
                                                 "reward", "done", "cut", "rollout_len")}
            # predictions: the network's own kernel on the observation buffer
            p_ref, v_ref, _ = net.predict_p_v_logits(obs)
            assert _same(g["p"], p_ref) and _same(g["v"], v_ref)
            f = m.forward(params, obs.astype(np.float64))
            assert np.max(np.abs(g["p"] - f["p"])) <= TOL and np.max(np.abs(g["v"] - f["v"])) <= TOL * max(1.0, np.max(np.abs(f["v"])))
            on = started == 1
            # uniforms, bit for bit; none on a first ever step
            want_u = np.where(on, o.uniform(seed, np.arange(n), draws), -1.0)
            assert _same(g["u"], want_u)
            for i in range(n):
                if not on[i]:
                    assert g["action"][i] == 0
                    continue
                if np.min(np.abs(o.cdf_edges(g["p"][i]) - g["u"][i])) <= EDGE:
                    left_out += 1
                    continue
                compared += 1
                assert g["action"][i] == o.select(g["p"][i], g["u"][i]), i
            stepped = np.array([o.physics(phys[i], g["action"][i]) for i in range(n)])
            want_done = np.array([o.fell(stepped[i]) or elapsed[i] + 1 >= o.TIME_LIMIT for i in range(n)])
            assert np.array_equal(g["done"] != 0, want_done)
            reset = on & want_done                                  # a first ever step's done is ignored
            assert np.all(g["reward"] == 1.0 * 0.005 - 1.0) and np.all(g["started"] == 1)
            assert np.array_equal(g["elapsed"], np.where(reset, 0, elapsed + 1))
            assert np.array_equal(g["draws"], draws + on.astype(np.uint64) + np.uint64(4) * reset.astype(np.uint64))
            cut = on & (want_done | (tc == time_max))
            assert np.array_equal(g["cut"], cut.astype(np.int32))
            assert np.array_equal(g["time_count"], np.where(~on, tc, np.where(want_done, 0, np.where(cut, 1, tc + 1))))
            assert np.array_equal(g["rollout_len"], np.where(on & ~want_done, 1, 0))
            # the physics: where the episode went on, what the device holds; where it was reset, the reset's own draws
            keep = ~reset
            err = np.abs(g["phys"][keep] - stepped[keep]) / np.maximum(1.0, np.abs(stepped[keep]))
            worst = max(worst, float(err.max()) if err.size else 0.0)
            assert _same(g["obs"][keep], g["phys"][keep].astype(np.float32))
            if reset.any():
                base = draws[reset] + np.uint64(1)
                want = -0.05 + (0.05 - -0.05) * o.uniform(seed, np.arange(n)[reset][:, None], base[:, None] + np.arange(4, dtype=np.uint64))
                assert _same(g["phys"][reset], want)
                # the observation is the stepped physics, which the reset has replaced: held to the oracle's at f32 rounding
                w32 = stepped[reset]
                assert np.all(np.abs(g["obs"][reset] - w32) <= 2.0 ** -23 * np.maximum(1.0, np.abs(w32)))
            assert net.actors_get("batch_rows") == int(cut.sum())
            net.actors_destroy()
        with capsys.disabled():
            print("\n[device actors] N=%d: worst physics error %.3e (bound %.3e); %d draws compared, %d left out"
                  % (n, worst, PHYS_BOUND, compared, left_out))
        assert worst <= PHYS_BOUND
        assert left_out <= 0.01 * (compared + left_out)
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
        ora = o.Actors(n, seed, time_max, GAMMA)
        assert _same(net.actors_get("phys"), np.array([e.phys for e in ora.env]))
        assert np.all(net.actors_get("draws") == 8) and not net.actors_get("started").any()
        elapsed = net.actors_get("elapsed")
        elapsed[::3] = 190                                          # some episodes end at the 200-step limit
        net.actors_set("elapsed", elapsed)
        for e, el in zip(ora.env, elapsed):
            e.elapsed = int(el)
        theta0 = net.get_arena(0)
        stale, carried = {}, {}                                     # env -> the observation / row its next rollout must begin with
        seen = dict(stale=0, carried=0, limit=0, fell=0, short=0, left_out=0, compared=0)
        for step in range(40):
            phys = net.actors_get("phys")
            for e, ph in zip(ora.env, phys):                        # re-seeded from the device's physics before every step
                e.phys = ph.copy()
            stats = net.actors_run(1, train=True)
            g = {k: net.actors_get(k) for k in ("phys", "elapsed", "obs", "p", "u", "action", "done", "cut", "draws", "time_count")}
            first = step == 0
            res, batch, episodes = ora.step(g["p"], actions=g["action"], dones=None if first else g["done"])
            rows = net.actors_get("batch_rows")
            assert stats == (n, int(rows > 0), rows, len(episodes))
            at = 0
            bx, by, ba = (net.actors_get(k) for k in ("batch_x", "batch_y_r", "batch_a")) if rows else (None, None, None)
            for i, (r, e) in enumerate(zip(res, ora.env)):
                assert np.float64(r["u"]).view(np.uint64) == g["u"][i:i + 1].view(np.uint64)[0], (step, i)
                assert r["own_done"] == bool(g["done"][i]), (step, i)
                if not first:
                    if np.min(np.abs(o.cdf_edges(g["p"][i]) - g["u"][i])) <= EDGE:
                        seen["left_out"] += 1
                    else:
                        seen["compared"] += 1
                        assert r["own_action"] == g["action"][i], (step, i)
                assert e.elapsed == g["elapsed"][i] and e.time_count == g["time_count"][i] and e.rng.draws == int(g["draws"][i])
                if r["episode"] is not None:                        # the reset: the same draws, the same bits
                    assert _same(e.phys, g["phys"][i])
                    seen["limit" if not o.fell(o.physics(phys[i], g["action"][i])) else "fell"] += 1
                e.obs = g["obs"][i].copy()                          # the f32 cast of the device's own physics (test_one_forced_step)
                if r["cut"] is not None:
                    T = len(r["cut"][2])
                    assert g["cut"][i] == T <= time_max + 1
                    x = bx[at:at + T]
                    if i in stale:                                  # the first action of an episode was predicted from the last
                        assert _same(x[0], stale.pop(i))            # observation of the episode before
                        seen["stale"] += 1
                    if i in carried:                                # the last row of a rollout is row 0 of the next
                        assert _same(x[0], carried.pop(i)) and T >= 2
                        seen["carried"] += 1
                    seen["short"] += T < time_max + 1
                    if r["episode"] is None:
                        carried[i] = x[-1].copy()
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
        assert seen["left_out"] <= 0.01 * (seen["left_out"] + seen["compared"])
        if n >= 15:
            assert seen["stale"] and seen["carried"] and seen["limit"] and seen["fell"] and seen["short"], seen
    finally:
        net.close()


SCAN_SIZES = [1025, 2500]   # environments per thread of the 1024-thread scan: 2 (thread 512 owns the last alone), 3 (thread 833 owns
                            # the last alone, the 190 threads after it none)


def _forced(n):
    """The environments whose episodes a scan test ends by elapsed = 199: the first, two in one thread's chunk (thread 5), the
    last of a chunk and the first of the next (threads 6 and 7), one far inside, the last."""
    chunk = -(-n // 1024)
    assert chunk >= 2
    return np.array([0, 5 * chunk, 5 * chunk + 1, 7 * chunk - 1, 7 * chunk, 600 * (chunk - 1) + 1, n - 1])


@pytest.mark.parametrize("n", SCAN_SIZES)
def test_the_scan_with_several_environments_per_thread(params, n):
    """The first cut at TIME_MAX = 2 is the fourth step, 3 rows of every environment; the forced episodes end on it.  The
    physics differ by environment (the seed's draws), so the batch's x rows do and their order is held; a CartPole record is
    (3 rewards of -0.995, 4) whichever environment it is of, so of the records it is the count that is held here."""
    time_max, seed = 2, 7 + n
    net = _net(params, 3 * n)
    forced = _forced(n)
    try:
        net.actors_create(n, time_max, GAMMA, seed)
        ora = o.Actors(n, seed, time_max, GAMMA)
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
            g = {k: net.actors_get(k) for k in ("obs", "p", "action", "done", "elapsed", "draws")}
            res, batch, episodes = ora.step(g["p"], actions=g["action"], dones=None if step == 0 else g["done"])
            for i, (r, e) in enumerate(zip(res, ora.env)):
                assert r["own_done"] == bool(g["done"][i]) and e.elapsed == g["elapsed"][i] and e.rng.draws == int(g["draws"][i])
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
            assert rows == 3 * n and len(episodes) == len(forced)
            assert np.array_equal(np.flatnonzero(g["done"]), forced)
            for name, want in zip(("batch_x", "batch_a", "batch_y_r"), batch):
                assert _same(net.actors_get(name), want), name
            assert len(np.unique(batch[0], axis=0)) > n              # the rows tell the environments apart
    finally:
        net.close()


@pytest.mark.parametrize("clip", [False, True], ids=["plain", "grad_clip"])
def test_the_train_step_is_ga3c_dmlp_train_on_the_fetched_batch(params, clip):
    n, time_max = 33, 2
    net, twin = _net(params, 128, clip), _net(params, 128, clip)
    try:
        net.actors_create(n, time_max, GAMMA, 5)
        net.learning_rate, net.beta = 1e-2, 0.01
        twin.learning_rate, twin.beta = 1e-2, 0.01
        assert net.actors_run(3, train=True) == (3 * n, 0, 0, 0)    # the unpredicted step, then time_count 0 and 1: nothing cut
        before = [net.get_arena(k) for k in range(3)]
        for k in range(3):
            twin.set_arena(k, before[k])
        assert net.actors_run(1, train=True) == (n, 1, n * (time_max + 1), 0)
        x, y, a = (net.actors_get(k) for k in ("batch_x", "batch_y_r", "batch_a"))
        assert x.shape == (99, 4) and np.all(a.sum(axis=1) == 1.0)
        want_y = np.tile(o.returns_fork([-0.995] * 3, GAMMA, -0.995).astype(np.float32), n)
        assert _same(y, want_y)
        twin.train(x, y, a)
        for k in range(3):
            assert _same(net.get_arena(k), twin.get_arena(k)), k
        assert not _same(net.get_arena(0), before[0]) and net.get_global_step() == twin.get_global_step() == 1
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
            theta = net.get_arena(0)
            stats = net.actors_run(20, train=False)
            assert stats[:3] == (20 * n, 0, 0) and net.get_global_step() == 0
            assert all(_same(net.get_arena(k), w) for k, w in ((0, theta), (1, np.ones_like(theta)), (2, np.zeros_like(theta))))
            stats = net.actors_run(50, train=True)
            assert stats[0] == 50 * n and stats[1] == net.get_global_step() > 0 and stats[2] > stats[1]
            out.append([net.get_arena(k) for k in range(3)] + [net.actors_get("phys"), net.actors_get("draws")])
            assert not _same(out[-1][0], theta)
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
        assert lib.ga3c_dmlp_actors_run(h, 1, 0.0, 0.0, 1, nat.ptr(stats, nat.i64p)) == ESTATE
        assert lib.ga3c_dmlp_actors_destroy(h) == ESTATE
        assert lib.ga3c_dmlp_actors_get(h, b"phys", vp, 32) == ESTATE
        assert lib.ga3c_dmlp_actors_set(h, b"phys", vp, 32) == ESTATE
        assert lib.ga3c_dmlp_actors_episodes(h, nat.ptr(buf, nat.f64p), nat.ptr(stats, nat.i64p), 4, C.byref(count)) == ESTATE
        assert lib.ga3c_dmlp_actors_create(None, 4, 5, GAMMA, 1) == EINVAL
        for n, time_max in ((0, 5), (-1, 5), (4, 0), (11, 5), (64, 1)):          # 11 x 6 and 64 x 2 rows exceed max_batch 64
            assert lib.ga3c_dmlp_actors_create(h, n, time_max, GAMMA, 1) == EINVAL, (n, time_max)
        assert b"max_batch" in lib.ga3c_last_error()
        assert lib.ga3c_dmlp_actors_create(h, 10, 5, GAMMA, 1) == 0
        assert lib.ga3c_dmlp_actors_create(h, 10, 5, GAMMA, 1) == ESTATE
        for steps in (0, -1, nat.ACTORS_MAX_STEPS + 1):
            assert lib.ga3c_dmlp_actors_run(h, steps, 0.0, 0.0, 1, None) == EINVAL
        assert lib.ga3c_dmlp_actors_run(h, nat.ACTORS_MAX_STEPS, 0.0, 0.0, 0, None) == 0
        assert lib.ga3c_dmlp_actors_get(h, b"nothing", vp, 32) == EINVAL
        assert lib.ga3c_dmlp_actors_get(h, b"phys", vp, 10 * 32 - 8) == EINVAL
        assert lib.ga3c_dmlp_actors_get(h, b"phys", None, 10 * 32) == EINVAL
        assert lib.ga3c_dmlp_actors_get(h, b"phys", vp, 10 * 32) == 0
        assert lib.ga3c_dmlp_actors_set(h, b"p", vp, 10 * 8) == EINVAL            # read only
        assert lib.ga3c_dmlp_actors_set(h, b"batch_x", vp, 0) == EINVAL
        bad = np.full(10, 6, np.int32)
        assert lib.ga3c_dmlp_actors_set(h, b"time_count", bad.ctypes.data_as(C.c_void_p), 40) == EINVAL
        bad[:] = -1
        assert lib.ga3c_dmlp_actors_set(h, b"elapsed", bad.ctypes.data_as(C.c_void_p), 40) == EINVAL
        assert lib.ga3c_dmlp_actors_episodes(h, None, None, 4, C.byref(count)) == EINVAL
        assert lib.ga3c_dmlp_actors_destroy(h) == 0
        assert lib.ga3c_dmlp_actors_destroy(h) == ESTATE
    finally:
        net.close()
    import NetworkVP_discrate
    other = NetworkVP_discrate.Network("gpu:0", "three_actions", 3, (4,), max_batch=64, predict_lanes=1)
    try:
        assert lib.ga3c_dmlp_actors_create(other._h, 4, 5, GAMMA, 1) == EINVAL    # CartPole has two actions
    finally:
        other.close()


@pytest.mark.timeout(120)
def test_train_script_runs_device_agents(tmp_path):
    env = dict(os.environ, PYTHONUNBUFFERED="1")
    run = subprocess.run(["sh", os.path.join(PKG, "_train.sh"), "GAME=CartPole-v0", "DEVICE_AGENTS=64", "MAX_SECONDS=5"],
                         cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=100)
    assert run.returncode == 0, run.stdout[-3000:] + run.stderr[-3000:]
    assert "died" not in run.stdout + run.stderr
    status = [ln for ln in run.stdout.splitlines() if "TPS:" in ln]
    assert status and re.search(r"\[NT:  0 NP:  0 NA: 64\]", status[-1]), run.stdout[-2000:]
    tps = [int(t) for t in re.findall(r"TPS:\s*(\d+)\]", run.stdout)]
    assert max(tps) > 0
    lines = open(os.path.join(str(tmp_path), "results.txt")).read().strip().splitlines()
    # an episode is at most 200 steps; len(rollout) + 1 per rollout of TIME_MAX = 5 new steps and one carried row
    assert lines and all(1 <= int(ln.split(",")[2]) <= 200 + 2 * (200 // 5 + 1) for ln in lines)
