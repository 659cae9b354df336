"""-m gpu: the DDPG device actors (Config.DEVICE_DDPG, ga3c_ddpg_actors_*) against tests/ddpg_actors_oracle.py,
which tests/test_ddpg_actors_cpu.py holds to the real ProcessAgent.  S = 3 and A = 1; N on both sides of the 16-row tile of the
predict kernel, in one and in two workgroups of the step kernel; N = 1025 and 2500 for the one-workgroup episode scan with two
and three environments per thread.

Exact: the action (ga3c_ddpg_predict's bits on the same observations and noise), the reward (the wrap, products and one fmod on
the device's own pre-step physics and action: no transcendental function), done, elapsed, draws, reset physics, the thdot
observation (the f32 cast), every field of the ring rows, slot order, episode records, the slots of a train step's draw, and the
arenas after train steps against a twin handle that is fed the fetched rows by replay_add and stepped by train_replay (or
train_prioritized) on the same slots.  Bounded: the new physics and the cos / sin observations, whose sin and cos are the
device library's and not numpy's -- PHYS_BOUND and OBS_BOUND below."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import ddpg_actors_oracle as do
import ddpg_oracle as o
import device_agents_oracle as ao
import device_pendulum_oracle as po
from test_gpu_ddpg import PKG, _load, _net, _same, _snapshot
from test_gpu_device_agents import SCAN_SIZES, _forced
from test_gpu_device_pendulum import _cases
from test_gpu_prioritized_replay import _per_net

pytestmark = pytest.mark.gpu

S, A = do.S, do.A
SIZES = [1, 15, 16, 17, 33, 300]
EINVAL, ESTATE = -1, -4
DRAW_SEED = 24680
# worst |got - want| / max(1, |want|) over the inputs of test_one_forced_step, measured on an MI355X: of the
# f64 physics after one step (PHYS_MEASURED) and of the f32 cos / sin observations against numpy's on the device's own new
# physics (OBS_MEASURED).  The assertions are at 8 times the measured value, under caps of 1e-12 and 2^-22; a measured 0
# asserts bits.  Measured: the physics 2.140e-16 at N = 300 and 0 at every other N (one ulp of one value, from a sin that rounds
# the other way); the observations 0 at every N -- on these inputs the device library's cos and sin, cast to f32, are numpy's.
PHYS_MEASURED = 2.140e-16
OBS_MEASURED = 0.0
PHYS_BOUND = 8 * PHYS_MEASURED
OBS_BOUND = 8 * OBS_MEASURED
assert PHYS_BOUND <= 1e-12 and OBS_BOUND <= 2.0 ** -22
NOISES = (0.8, -0.8, 3.2, -3.2, 0.0)        # tanh + noise: beyond +1, beyond -1, more than a turn beyond either, within


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _eq(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _rel(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(np.max(np.abs(got - want) / np.maximum(1.0, np.abs(want)))) if got.size else 0.0


def _weights(seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    online, target = o.random_params(S, A, rng), o.random_params(S, A, rng)
    online["actor_output/W"] = (online["actor_output/W"] * 3).astype(np.float32).astype(np.float64)    # a tanh output that varies
    return online, target


def _ring_rows(net, slots):
    return np.array([do.pack(net.replay_get(int(k))) for k in slots], np.float32).reshape(len(slots), do.ROWF)


@pytest.mark.parametrize("n", SIZES)
def test_one_forced_step(n, capsys):
    seed = 2024 + n
    net = _net(S, A, max_batch=max(16, n), capacity=2 * n + 3)
    _load(net, *_weights(n))
    rng = np.random.Generator(np.random.PCG64(n))
    total = max(24, n)
    phys_all, elapsed_all, _ = _cases(rng, total)
    worst_phys = worst_obs = 0.0
    below = above = within = turns = resets = 0
    try:
        count = max(len(NOISES), -(-total // n))      # every case and every noise at least once
        groups = [((g * n) % total, NOISES[g % len(NOISES)]) for g in range(count)]
        for lo, nz in groups:
            idx = np.arange(lo, lo + n) % total
            phys, elapsed = phys_all[idx].copy(), elapsed_all[idx].copy()
            draws = 2 * rng.integers(2, 1 << 39, size=n).astype(np.uint64)
            obs = rng.uniform(-1.5, 1.5, size=(n, S)).astype(np.float32)
            net.actors_create(n, seed=seed, batch=1, updates=1)
            base = net.replay_size()[1]
            assert net.actors_run(1, train=False, noise=[nz]) == (n, 0, 0, 0)          # step(None): no transition
            assert net.replay_size()[1] == base and np.all(net.actors_get("action") == 0.0)
            assert np.all(net.actors_get("elapsed") == 1) and np.all(net.actors_get("draws") == 4)
            for name, val in (("phys", phys), ("elapsed", elapsed), ("draws", draws), ("obs", obs)):
                net.actors_set(name, val)
                assert _eq(net.actors_get(name), val), name
            want_done = elapsed + 1 >= po.TIME_LIMIT
            assert net.actors_run(1, train=False, noise=[nz]) == (n, 0, 0, int(want_done.sum()))
            g = {k: net.actors_get(k) for k in ("phys", "elapsed", "draws", "obs", "action", "reward", "done")}
            assert g["action"].shape == (n, A) and g["phys"].shape == (n, 2) and g["obs"].shape == (n, S)
            # the action: the predict entry's bits on the same observations and noise
            assert _eq(g["action"], net.predict(obs, noise=[nz]))
            act = g["action"][:, 0]
            below, above, within = below + int((act < -1).sum()), above + int((act > 1).sum()), within + int((np.abs(act) <= 1).sum())
            turns += int((np.abs(act) > 3).sum())
            # the oracle's step on the device's own pre-step physics and action
            stepped, reward = zip(*[do.env_step(phys[i], g["action"][i]) for i in range(n)])
            stepped, reward = np.array(stepped), np.array(reward, np.float64)
            assert _eq(g["reward"], reward)
            assert np.all(reward <= -1.0) and np.all(reward >= -1.09)
            assert np.array_equal(g["done"] != 0, want_done)
            assert np.array_equal(g["elapsed"], np.where(want_done, 0, elapsed + 1))
            assert np.array_equal(g["draws"], draws + np.uint64(2) * want_done.astype(np.uint64))
            keep = ~want_done
            worst_phys = max(worst_phys, _rel(g["phys"][keep], stepped[keep]))
            assert np.all(np.abs(g["phys"][keep][:, 1]) <= 8.0)
            assert _eq(g["obs"][keep][:, 2], g["phys"][keep][:, 1].astype(np.float32))
            want_obs = np.array([po.PendulumEnv.observe(ph) for ph in g["phys"]])
            worst_obs = max(worst_obs, _rel(g["obs"][keep][:, :2], want_obs[keep][:, :2]))
            if want_done.any():
                resets += int(want_done.sum())
                k = draws[want_done]
                u0, u1 = (ao.uniform(seed, np.arange(n)[want_done], k + np.uint64(j)) for j in (0, 1))
                assert _eq(g["phys"][want_done], np.stack([-np.pi + (np.pi - -np.pi) * u0, -1.0 + (1.0 - -1.0) * u1], axis=1))
                gone = np.array([po.PendulumEnv.observe(ph) for ph in stepped[want_done]])
                worst_obs = max(worst_obs, _rel(g["obs"][want_done], gone))
            # the ring rows: s the observation before, a as predicted, the f32 reward, done, s2 the observation after
            size, ring_total = net.replay_size()
            assert ring_total == base + n
            slots = (base + np.arange(n)) % net.replay_capacity
            want_rows = np.concatenate([obs, g["action"], reward.astype(np.float32)[:, None],
                                        want_done.astype(np.float32)[:, None], g["obs"]], axis=1)
            assert _eq(_ring_rows(net, slots), want_rows)
            # an episode that ends here began with this transition: its reward, and 1 + 1
            assert net.actors_episodes() == [(float(reward[i]), 2) for i in np.flatnonzero(want_done)]
            net.actors_destroy()
        with capsys.disabled():
            print("\n[ddpg actors] N=%d: worst physics error %.3e (bound %.3e), worst cos / sin observation error %.3e (bound %.3e); "
                  "actions below -1: %d, above 1: %d, within: %d, beyond +-3: %d; resets %d"
                  % (n, worst_phys, PHYS_BOUND, worst_obs, OBS_BOUND, below, above, within, turns, resets))
        assert below and above and within and turns
        assert worst_phys <= PHYS_BOUND
        assert worst_obs <= OBS_BOUND
    finally:
        net.close()


def _capacities(n):
    return [("full", n, False), ("odd", 2 * n + 3, False), ("odd-per", 2 * n + 3, True), ("large", 5000, False)]


@pytest.mark.parametrize("kind", ["full", "odd", "odd-per", "large"])
@pytest.mark.parametrize("n", SIZES)
def test_forty_steps_follow_the_oracle(n, kind):
    _, capacity, prioritized = next(c for c in _capacities(n) if c[0] == kind)
    seed = 99 + n
    net = _per_net(capacity, max_batch=max(16, n)) if prioritized else _net(S, A, max_batch=max(16, n), capacity=capacity)
    _load(net, *_weights(7))
    try:
        net.actors_create(n, seed=seed, batch=1, updates=1)
        ora = do.Actors(n, seed)
        ring = do.Ring(capacity, prioritized)
        assert _eq(net.actors_get("phys"), np.array([e.phys for e in ora.env]))
        assert np.all(net.actors_get("draws") == 4) and np.all(net.actors_get("elapsed") == 0)
        # these episodes end inside the run, on different steps
        elapsed = np.zeros(n, np.int32)
        for i in range(n):
            if i % 3 != 2:
                elapsed[i] = po.TIME_LIMIT - 3 - (7 * i) % 31
        net.actors_set("elapsed", elapsed)
        for e, el in zip(ora.env, elapsed):
            e.elapsed = int(el)
        pa0 = None
        if prioritized:
            pa0 = np.random.default_rng(3).uniform(0.1, 1.5, capacity).astype(np.float32)
            net.set_priorities(pa0, 2.0)
            ring.pa[:], ring.max_pa = pa0, np.float32(2.0)
        records, finished_on = [], set()
        for step in range(40):
            nz = NOISES[step % len(NOISES)] * (0.5 + 0.01 * step)
            before_phys, before_obs = net.actors_get("phys"), net.actors_get("obs")
            stats = net.actors_run(1, train=False, noise=[nz])
            g = {k: net.actors_get(k) for k in ("phys", "obs", "action", "reward", "done", "elapsed", "draws")}
            # the oracle re-seeded from the device's physics and observation, stepped with the device's action
            for i, e in enumerate(ora.env):
                e.phys, e.obs = before_phys[i].copy(), before_obs[i].copy()
            rows, eps, outs = ora.step(None if step == 0 else g["action"])
            assert stats == (n, 0, 0, len(eps))
            assert _eq(g["reward"], np.array([r["reward"] for r in outs], np.float64))
            assert np.array_equal(g["done"] != 0, np.array([r["done"] for r in outs]))
            assert np.array_equal(g["elapsed"], np.array([e.elapsed for e in ora.env], np.int32))
            assert np.array_equal(g["draws"], np.array([e.rng.draws for e in ora.env], np.uint64))
            ended = np.array([r["episode"] is not None for r in outs])
            assert _eq(g["phys"][ended], np.array([e.phys for e in ora.env])[ended].reshape(-1, 2))       # the reset's draws
            assert _rel(g["phys"][~ended], np.array([e.phys for e in ora.env])[~ended]) <= PHYS_BOUND
            if step:
                assert _eq(g["action"], net.predict(before_obs, noise=[nz]))
                # the rows as the device must have written them: the oracle's, with the device's own new observation as s2
                ring.add([(row[0], row[1], row[2], row[3], g["obs"][i]) for i, row in enumerate(rows)])
            assert net.replay_size() == (ring.size, ring.total)
            records += eps
            if eps:
                finished_on.add(step)
            assert net.actors_episodes() == eps       # environment order, bit for bit
            if prioritized and step in (1, 2, 39):
                pa, top = net.priorities()
                assert top == np.float32(2.0) and _eq(pa, ring.pa)
                if step == 1:
                    assert np.all(pa[:n] == 2.0) and _eq(pa[n:], pa0[n:])
        assert ring.total == 39 * n and (ring.total > capacity or kind == "large")       # a full ring was overwritten whole
        assert _eq(_ring_rows(net, range(ring.size)), ring.rows[:ring.size])
        assert len(records) == int(np.sum(elapsed > 0)) and len(finished_on) >= (2 if n > 1 else 1)
    finally:
        net.close()


@pytest.mark.parametrize("n", SCAN_SIZES)
def test_the_episode_scan_with_several_environments_per_thread(n):
    """step(None), then one step on which the forced episodes end.  The physics differ by environment (the seed's draws), so
    the rewards, the rows and the records do: their order is held."""
    seed, capacity, nz = 31 + n, 2 * n + 3, 0.8
    net = _net(S, A, max_batch=n, capacity=capacity)
    _load(net, *_weights(7))
    forced = _forced(n)
    try:
        net.actors_create(n, seed=seed, batch=1, updates=1)
        ora, ring = do.Actors(n, seed), do.Ring(capacity)
        assert net.actors_run(1, train=False, noise=[nz]) == (n, 0, 0, 0)
        ora.step(None)
        assert net.replay_size() == (0, 0) and net.actors_episodes() == []
        elapsed = net.actors_get("elapsed")
        elapsed[forced] = 199
        net.actors_set("elapsed", elapsed)
        # the oracle re-seeded from the device's physics and observation, stepped with the device's action
        for e, ph, ob, el in zip(ora.env, net.actors_get("phys"), net.actors_get("obs"), elapsed):
            e.phys, e.obs, e.elapsed = ph.copy(), ob.copy(), int(el)
        stats = net.actors_run(1, train=False, noise=[nz])
        g = {k: net.actors_get(k) for k in ("obs", "action", "reward", "done", "elapsed", "draws")}
        rows, eps, outs = ora.step(g["action"])
        assert _eq(g["reward"], np.array([r["reward"] for r in outs], np.float64))
        assert np.array_equal(np.flatnonzero(g["done"]), forced)
        assert np.array_equal(g["elapsed"], np.array([e.elapsed for e in ora.env], np.int32))
        assert np.array_equal(g["draws"], np.array([e.rng.draws for e in ora.env], np.uint64))
        assert len(eps) == len(forced) == len(set(eps)) and stats == (n, 0, 0, len(eps))
        assert net.actors_episodes() == eps               # environment order, bit for bit
        # the rows as the device must have written them: the oracle's, with the device's own new observation as s2
        ring.add([(row[0], row[1], row[2], row[3], g["obs"][i]) for i, row in enumerate(rows)])
        assert net.replay_size() == (n, n) == (ring.size, ring.total)
        assert _eq(_ring_rows(net, range(n)), ring.rows[:n])
        assert len(np.unique(ring.rows[:n], axis=0)) == n
    finally:
        net.close()


def _train_sizes(n, batch, adds, updates):
    """-> [ring size at each train step] after `adds` actor steps that each added n rows: ThreadReplay's rule."""
    return [n * k for k in range(1, adds + 1) if n * k > batch for _ in range(updates)]


TRAIN = [("plain", dict(), 1, False), ("clip", dict(USE_GRAD_CLIP=True), 1, False), ("adam", dict(RMSPROP=False), 1, False),
         ("updates3", dict(), 3, False), ("per", dict(), 1, True), ("per-clip-updates3", dict(USE_GRAD_CLIP=True), 3, True)]


@pytest.mark.parametrize("B", [1, 16, 17, 64])
@pytest.mark.parametrize("case", TRAIN, ids=[c[0] for c in TRAIN])
def test_train_steps_are_the_twins(case, B):
    """The ring is large enough to keep every row, so the twin can be fed the run's rows afterwards, n after n, and take a train
    step wherever the rule says the device took one: train_replay on the oracle's slots, or train_prioritized."""
    _, cfg, updates, prioritized = case
    n, capacity, steps, noise = 17, 400, 8, [0.3]
    if prioritized:
        net, twin = (_per_net(capacity, max_batch=64, **cfg) for _ in range(2))
        net.replay_beta = twin.replay_beta = 0.4
    else:
        net, twin = (_net(S, A, max_batch=64, capacity=capacity, **cfg) for _ in range(2))
    online, target = _weights(31)
    try:
        for h in (net, twin):
            _load(h, online, target)
        start = _snapshot(net)
        net.actors_create(n, seed=5, updates=updates, batch=B, draw_seed=DRAW_SEED)
        assert net.actors_get("batch") == B and net.actors_get("draw_seed") == DRAW_SEED
        # while the ring holds at most B rows nothing trains: B = 16 and 17 sit on both sides of the 17 rows of one actor step
        quiet = 1 + B // n
        assert net.actors_run(quiet, train=True, noise=noise) == (n * quiet, 0, 0, 0)
        assert net.replay_size()[0] == n * (quiet - 1) <= B and net.get_global_step() == 0 and _same(start, _snapshot(net))
        adds = quiet - 1 + steps
        sizes = _train_sizes(n, B, adds, updates)
        assert len(sizes) == steps * updates
        assert net.actors_run(steps, train=True, noise=noise) == (n * steps, len(sizes), len(sizes) * B, 0)
        assert net.replay_size() == (n * adds, n * adds) and n * adds < capacity
        rows = _ring_rows(net, range(n * adds))
        sample, q_twin, last_slots = 0, None, None
        for k in range(adds):
            f = rows[k * n:(k + 1) * n]
            size, _ = twin.replay_add(f[:, :S], f[:, S:S + A], f[:, S + A], f[:, S + A + 1], f[:, S + A + 2:])
            if size > B:
                for _ in range(updates):
                    assert size == sizes[sample]
                    if prioritized:
                        q_twin = twin.train_prioritized(B, noise=noise)
                        last_slots = twin.last_slots
                    else:
                        last_slots = do.uniform_slots(DRAW_SEED, sample, size, B)
                        q_twin = twin.train_replay(last_slots, noise=noise)
                    sample += 1
        assert sample == len(sizes)
        assert np.array_equal(net.actors_get("slots"), last_slots)
        assert net.logging == q_twin
        assert _same(_snapshot(net), _snapshot(twin))
        assert net.get_global_step() == twin.get_global_step() == len(sizes)
        assert not _same(start, _snapshot(net))
        if prioritized:
            (pa, top), (tpa, ttop) = net.priorities(), twin.priorities()
            assert top == ttop and _eq(pa, tpa)
    finally:
        net.close()
        twin.close()


def test_the_same_seed_gives_the_same_bits_and_train_zero_trains_nothing():
    online, target = _weights(41)
    snaps, rings, eps = [], [], []
    for _ in range(2):
        net = _net(S, A, max_batch=64, capacity=500)
        try:
            _load(net, online, target)
            net.actors_create(33, seed=77, updates=2, batch=16, draw_seed=DRAW_SEED)
            net.actors_set("elapsed", np.full(33, 190, np.int32))
            start = _snapshot(net)
            assert net.actors_run(12, train=False) == (33 * 12, 0, 0, 33)       # the handle's own noise process
            assert net.get_global_step() == 0 and _same(start, _snapshot(net))  # train = 0: the rows are written, nothing trains
            assert net.replay_size() == (33 * 11, 33 * 11)
            stats = net.actors_run(20, train=True)
            assert stats == (33 * 20, 40, 40 * 16, 0) and net.get_global_step() == 40
            assert not _same(start, _snapshot(net))
            snaps.append(_snapshot(net))
            rings.append(_ring_rows(net, range(500)))
            eps.append(net.actors_episodes())
        finally:
            net.close()                               # destroy with live actors
    assert _same(snaps[0], snaps[1]) and _eq(rings[0], rings[1]) and eps[0] == eps[1] and len(eps[0]) == 33
    assert all(length == 10 for _, length in eps[0])  # elapsed 190 -> 191 at step(None), then 9 transitions: 9 + 1


def test_refusals():
    import ga3c_amd  # noqa: F401
    import _native as nat
    lib = nat.hip_lib()
    net = _net(S, A, max_batch=32, capacity=20)
    wide = _net(7, 3, max_batch=32, capacity=64)
    stats, q = np.zeros(4, np.int64), np.zeros(2, np.float32)
    buf = np.zeros(64, np.float64)
    noise = np.zeros(1, np.float32)
    count = C.c_int32()

    def run(h, steps=1, mode=1, nz=noise):
        return lib.ga3c_ddpg_actors_run(h._h, steps, 1e-4, 0.4, 1, mode, nat.ptr(nz) if nz is not None else None,
                                        nat.ptr(stats, nat.i64p), nat.ptr(q))
    try:
        h = net._h
        # without actors: GA3C_ESTATE from every call
        assert lib.ga3c_ddpg_actors_destroy(h) == ESTATE and run(net) == ESTATE
        assert lib.ga3c_ddpg_actors_episodes(h, nat.ptr(buf, nat.f64p), nat.ptr(stats, nat.i64p), 4, C.byref(count)) == ESTATE
        assert lib.ga3c_ddpg_actors_get(h, b"phys", buf.ctypes.data_as(C.c_void_p), 16) == ESTATE
        assert lib.ga3c_ddpg_actors_set(h, b"phys", buf.ctypes.data_as(C.c_void_p), 16) == ESTATE
        # create: n in [1, min(max_batch 32, replay_capacity 20)], updates in [1, 16], a 3-float state and one action
        for n, updates in ((0, 1), (21, 1), (-1, 1), (4, 0), (4, 17)):
            assert lib.ga3c_ddpg_actors_create(h, n, updates, 1) == EINVAL, (n, updates)
        assert lib.ga3c_ddpg_actors_create(wide._h, 4, 1, 1) == EINVAL
        assert lib.ga3c_ddpg_actors_create(h, 20, 16, 1) == 0
        assert lib.ga3c_ddpg_actors_create(h, 20, 16, 1) == ESTATE
        assert run(net, steps=0) == EINVAL and run(net, steps=65) == EINVAL
        assert run(net, mode=3) == EINVAL and run(net, mode=-1) == EINVAL and run(net, mode=1, nz=None) == EINVAL
        assert net.replay_size() == (0, 0)            # ... and none of them stepped anything
        ptr = buf.ctypes.data_as(C.c_void_p)
        assert lib.ga3c_ddpg_actors_get(h, b"nothing", ptr, 8) == EINVAL
        assert lib.ga3c_ddpg_actors_get(h, b"phys", ptr, 20 * 16 - 8) == EINVAL
        assert lib.ga3c_ddpg_actors_get(h, b"phys", ptr, 20 * 16) == 0
        for name, size in ((b"action", 80), (b"reward", 160), (b"done", 80), (b"slots", 0)):
            assert lib.ga3c_ddpg_actors_set(h, name, ptr, size) == EINVAL, name       # read only
        for batch in (0, 33):
            value = np.array([batch], np.int32)
            assert lib.ga3c_ddpg_actors_set(h, b"batch", value.ctypes.data_as(C.c_void_p), 4) == EINVAL
        assert net.actors_get("batch") == 32          # max_batch until it is set
        bad = np.full(20, -1, np.int32)
        assert lib.ga3c_ddpg_actors_set(h, b"elapsed", bad.ctypes.data_as(C.c_void_p), 80) == EINVAL
        assert run(net, steps=64) == 0 and stats[0] == 20 * 64
        assert lib.ga3c_ddpg_actors_destroy(h) == 0 and lib.ga3c_ddpg_actors_destroy(h) == ESTATE
    finally:
        net.close()
        wide.close()


LINES = [("uniform", []), ("prioritized", ["PRIORITIZED_REPLAY=True", "DDPG_CRITIC_LOSS=paired"])]


@pytest.mark.timeout(120)
@pytest.mark.parametrize("line", LINES, ids=[c[0] for c in LINES])
def test_train_script_runs_device_ddpg(line, tmp_path):
    env = dict(os.environ, PYTHONUNBUFFERED="1")
    run = subprocess.run(["timeout", "-k", "10", "90", "sh", os.path.join(PKG, "_train.sh"), "GAME=Pendulum-v0", "USE_DDPG=True",
                          "TRAINING_MIN_BATCH_SIZE=64", "DEVICE_AGENTS=64", "DEVICE_DDPG=True", "MAX_SECONDS=5"] + line[1],
                         cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=110)
    assert run.returncode == 0, run.stdout[-3000:] + run.stderr[-3000:]
    assert "died" not in run.stdout + run.stderr
    status = [ln for ln in run.stdout.splitlines() if "TPS:" in ln]
    assert status and re.search(r"\[NT:  0 NP:  0 NA: 64\]", status[-1]), run.stdout[-2000:]
    tps = [int(t) for t in re.findall(r"TPS:\s*(\d+)\]", run.stdout)]
    assert max(tps) > 0
    lines = open(os.path.join(str(tmp_path), "results.txt")).read().strip().splitlines()
    # the first episode is step(None) and 199 transitions, every later one 200: transitions + 1
    assert lines and all(int(ln.split(",")[2]) in (200, 201) for ln in lines)
    assert all(-1.09 * 200 <= float(ln.split(",")[1]) <= -199 for ln in lines)
