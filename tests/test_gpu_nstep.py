"""-m gpu: n-step returns of the DDPG device actors (Config.DDPG_NSTEP, ga3c_ddpg_nstep_*) against
tests/nstep_oracle.py, which tests/test_nstep_cpu.py holds to the per-episode definition.  S = 3 and A = 1 throughout.

Exact (bits): the ring rows, their order, disc by slot, replay_size, the pa slots written and the episode records over forty
steps (the rewards, the discounts and the n-step sum contain no transcendental function); at n = 1 the whole ring against a
handle without n-step state; the arenas after train steps against a second handle that is fed the fetched rows and discounts
and stepped on the same slots.  Bounded, at test_gpu_ddpg.py's own TOL and WTOL: y, q', q, dq and the critics' gradients of one
train step whose rows carry a mix of gamma^1 .. gamma^16, against the f64 oracles called with the per-row discounts."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import ddpg_actors_oracle as do
import ddpg_oracle as o
import device_pendulum_oracle as po
import nstep_oracle as ns
import per_oracle as per
import td3_oracle as t3
import test_gpu_ddpg as gd
import test_gpu_td3 as gt
from test_gpu_ddpg import LR, PKG, TOL, WTOL, _cfg_kw, _check, _f64, _load, _net, _same, _snapshot
from test_gpu_ddpg_actors import DRAW_SEED, NOISES, PHYS_BOUND, _eq, _rel, _ring_rows, _train_sizes, _weights
from test_gpu_prioritized_replay import SEED as PER_SEED, _per_net, _random_priorities, _ring_for_batch

pytestmark = pytest.mark.gpu

S, A = do.S, do.A
GAMMA = 0.99
EINVAL, ESTATE = -1, -4


def _powers():
    """(f32) g_m for m = 1..16 as the kernel forms them: sequential f64 products of the f32 gamma."""
    g64, g, out = ns.gamma64(GAMMA), 1.0, []
    for _ in range(16):
        g = g * g64
        out.append(np.float32(g))
    return np.array(out, np.float32)


def _nnet(n, capacity, max_batch, prioritized=False, twin=False, **kw):
    if twin:
        net = gt._tnet(S, A, max_batch=max_batch, capacity=capacity, **kw)
    elif prioritized:
        net = _per_net(capacity, max_batch=max_batch, **kw)
    else:
        net = _net(S, A, max_batch=max_batch, capacity=capacity, **kw)
    if n is not None:
        net.nstep_create(n)
    return net


# ---- 1. rows

KINDS = {"full": (lambda n: n, False), "odd": (lambda n: 2 * n + 3, False), "odd-per": (lambda n: 2 * n + 3, True),
         "large": (lambda n: 5000, False)}
ROWS = ([(N, n, kind) for N in (1, 17) for n in (1, 2, 5, 16) for kind in KINDS]
        + [(300, 1, "full"), (300, 2, "odd"), (300, 5, "odd-per"), (300, 16, "large"), (300, 16, "full"), (300, 5, "odd"),
           (300, 2, "odd-per"), (300, 1, "large")]
        + [(1025, 5, "odd")])            # more than one environment per thread of the episode scan


@pytest.mark.parametrize("N,n,kind", ROWS, ids=["N%d-n%d-%s" % c for c in ROWS])
def test_forty_steps_follow_the_delay_line(N, n, kind):
    capacity, prioritized = KINDS[kind][0](N), KINDS[kind][1]
    seed = 99 + N
    net = _nnet(n, capacity, max(16, N), prioritized)
    plain = _nnet(None, capacity, max(16, N), prioritized) if n == 1 else None
    handles = [net] + ([plain] if plain else [])
    try:
        for h in handles:
            _load(h, *_weights(7))
            h.actors_create(N, seed=seed, batch=1, updates=1)
        assert net.actors_get("nstep") == n and net.actors_get("nstep_count") == 0
        assert plain is None or plain.actors_get("nstep") == 1
        ora = ns.Actors(N, seed, n, GAMMA)
        ring = ns.Ring(capacity, prioritized, GAMMA)
        assert _eq(net.nstep_discounts(), ring.disc)                       # gamma in every slot at create
        # these episodes end inside the run, on different steps
        elapsed = np.zeros(N, np.int32)
        for i in range(N):
            if i % 3 != 2:
                elapsed[i] = po.TIME_LIMIT - 3 - (7 * i) % 31
        for h in handles:
            h.actors_set("elapsed", elapsed)
        for e, el in zip(ora.env, elapsed):
            e.elapsed = int(el)
        pa0 = None
        if prioritized:
            pa0 = np.random.default_rng(3).uniform(0.1, 1.5, capacity).astype(np.float32)
            for h in handles:
                h.set_priorities(pa0, 2.0)
            ring.pa[:], ring.max_pa = pa0, np.float32(2.0)
        records, ones, shorts = [], 0, 0
        for step in range(40):
            nz = NOISES[step % len(NOISES)] * (0.5 + 0.01 * step)
            if step in (9, 10, 11, 12, 25):
                # every fourth environment ends on this step, on four consecutive steps: episodes of one transition in a window
                forced = net.actors_get("elapsed")
                forced[1::4] = po.TIME_LIMIT - 1
                for h in handles:
                    h.actors_set("elapsed", forced)
                for e, el in zip(ora.env, forced):
                    e.elapsed = int(el)
            before_phys, before_obs = net.actors_get("phys"), net.actors_get("obs")
            stats = net.actors_run(1, train=False, noise=[nz])
            if plain:
                assert plain.actors_run(1, train=False, noise=[nz]) == stats
            g = {k: net.actors_get(k) for k in ("phys", "obs", "action", "reward", "done", "elapsed", "draws")}
            # the oracle re-seeded from the device's physics and observation, stepped with the device's action, keeping the
            # device's own new observation as s2
            for i, e in enumerate(ora.env):
                e.phys, e.obs = before_phys[i].copy(), before_obs[i].copy()
            pairs, eps, outs = ora.step(None if step == 0 else g["action"], s2=g["obs"])
            assert stats == (N, 0, 0, len(eps))
            assert _eq(g["reward"], np.array([r["reward"] for r in outs], np.float64))
            assert np.array_equal(g["done"] != 0, np.array([r["done"] for r in outs]))
            assert np.array_equal(g["elapsed"], np.array([e.elapsed for e in ora.env], np.int32))
            assert np.array_equal(g["draws"], np.array([e.rng.draws for e in ora.env], np.uint64))
            ended = np.array([r["episode"] is not None for r in outs])
            assert _rel(g["phys"][~ended], np.array([e.phys for e in ora.env])[~ended]) <= PHYS_BOUND
            if step:
                assert _eq(g["action"], net.predict(before_obs, noise=[nz]))
            assert len(pairs) == (N if step >= n else 0)                    # step(None), then n - 1 silent transition steps
            ring.add([p[0] for p in pairs], [p[1] for p in pairs])
            shorts += sum(1 for p in pairs if p[1] != _powers()[n - 1])
            assert net.replay_size() == (ring.size, ring.total) and ring.total == max(0, step - n + 1) * N
            assert net.actors_get("nstep_count") == step
            records += eps
            ones += sum(1 for _, length in eps if length == 2)
            assert net.actors_episodes() == eps                             # per step and unchanged: environment order, bits
            if plain:
                assert plain.actors_episodes() == eps
            if prioritized and step in (1, n - 1, n, n + 1, 39):
                pa, top = net.priorities()
                assert top == np.float32(2.0) and _eq(pa, ring.pa)
                if step < n:
                    assert _eq(pa, pa0)
        assert ring.total == (40 - n) * N and (ring.total > capacity or kind == "large")
        assert _eq(_ring_rows(net, range(ring.size)), ring.rows[:ring.size])
        disc = net.nstep_discounts()
        assert _eq(disc, ring.disc)
        if N > 1:
            assert ones >= 3 * len(range(1, N, 4)), "episodes of one transition"
        short = disc[:ring.size] != _powers()[n - 1]
        assert np.all(ring.rows[:ring.size][short, S + A + 1] == 1.0)         # a shortened horizon ends its episode
        assert (shorts > 0) == (n > 1), "shortened horizons"
        assert n > 1 or np.all(disc == np.float32(GAMMA))
        if plain:
            assert plain.replay_size() == net.replay_size()
            assert _eq(_ring_rows(plain, range(ring.size)), ring.rows[:ring.size])
            if prioritized:
                assert _eq(plain.priorities()[0], net.priorities()[0])
    finally:
        for h in handles:
            h.close()


# ---- 2. the target against the f64 oracles

def _mixed(count, rng):
    """`count` discounts out of gamma^1 .. gamma^16, every power present when count allows."""
    p = _powers()
    idx = np.concatenate([np.arange(16), rng.integers(0, 16, max(0, count - 16))])[:count]
    return p[rng.permutation(idx)]


@pytest.mark.parametrize("B", [1, 16, 17, 64])
def test_target_with_per_row_discounts(B):
    rng = np.random.Generator(np.random.PCG64(500 + B))
    noise = np.full(A, 0.05, np.float32)
    gam = _mixed(B, rng)
    online, target, batch = gd._case(S, A, B, 700 + B, noise=noise, gamma=gam.astype(np.float64))
    capacity = B + 5
    net = _nnet(5, capacity, 64)
    try:
        _load(net, online, target)
        assert net.replay_add(*batch) == (B, B)
        assert np.all(net.nstep_discounts() == np.float32(GAMMA))          # rows added by hand are one-step rows
        disc = np.full(capacity, np.float32(GAMMA), np.float32)
        disc[:B] = gam
        net.set_nstep_discounts(disc)
        assert _eq(net.nstep_discounts(), disc)
        slots = rng.permutation(B).astype(np.int32)
        q_max, q_avg = net.train_replay(slots, noise=noise)
        assert _eq(net.fetch("disc", B), disc[slots])
        st = o.new_state(online, target)
        rows = _f64(tuple(t[slots] for t in batch))
        out = o.train_step(st, *rows, LR, noise.astype(np.float64), gamma=disc[slots].astype(np.float64))
        done = rows[3] != 0
        print("B=%d: %d rows done, %d discounts" % (B, int(done.sum()), len(np.unique(gam))))
        for name in ("y", "qt", "q", "dq"):
            _check(name, net.fetch(name, B), out[name])
        _check("q_max", [q_max], [out["q_max"]])
        _check("q_avg", [q_avg], [out["q_avg"]])
        if B > 1:
            scalar = rows[2] + np.where(done, 0.0, GAMMA * out["qt"])
            assert np.max(np.abs(scalar - out["y"])) > 10 * TOL, "the discounts did not reach the oracle's target"
        for k in o.CRITIC_TRAINABLE:
            _check("grad " + k, net.get_variable_value(k, 4), out["critic_grads"][k])
        for k in o.TRAINABLE:
            _check("online " + k, net.get_variable_value(k, 0), st["online"][k], WTOL)
        # train and compute have no slot: the scalar gamma, and fetch says so
        net.compute(batch[0], batch[2], batch[1], batch[4], batch[3], 3, noise=noise)
        assert np.all(net.fetch("disc", B) == np.float32(GAMMA))
    finally:
        net.close()


def test_twin_target_with_per_row_discounts():
    B = 17
    rng = np.random.Generator(np.random.PCG64(41))
    tw = dict(policy_delay=1, sigma=0.2, noise_clip=0.5)
    noise = np.full(A, 0.05, np.float32)
    gam = _mixed(B, rng)
    online, target, batch = gt._case(S, A, B, 900, tw, noise=noise, gamma=gam.astype(np.float64))
    net = _nnet(16, B, 64, twin=True, delay=1)
    try:
        gt._load(net, online, target)
        assert net.replay_add(*batch) == (B, B)
        net.set_nstep_discounts(gam)
        net.train_replay(np.arange(B, dtype=np.int32), noise=noise)
        assert _eq(net.fetch("disc", B), gam)
        eps = gt._check_eps(net, 1, B, A, 0.2, 0.5)
        st = t3.new_state(online, target)
        out = t3.train_step(st, *_f64(batch), LR, noise.astype(np.float64), eps=eps, gamma=gam.astype(np.float64), **tw)
        for name in ("y", "qt", "qt1", "qt2", "q", "dq", "q2", "dq2"):
            _check(name, net.fetch(name, B), out[name])
        for pre, tag in (("critic_", "critic_grads"), ("critic2_", "critic2_grads")):
            for k in o.CRITIC_TRAINABLE:
                _check("grad " + pre + k[len("critic_"):], net.get_variable_value(pre + k[len("critic_"):], 4), out[tag][k])
        for k in t3.TRAINABLE:
            _check("online " + k, net.get_variable_value(k, 0), st["online"][k], WTOL)
    finally:
        net.close()


def test_prioritized_target_with_per_row_discounts():
    n, B, beta = 128, 64, 0.4
    rng = np.random.Generator(np.random.PCG64(43))
    noise = np.full(A, 0.05, np.float32)
    pa = _random_priorities(n, n, np.random.default_rng(5))
    want_slots, want_w = per.sample(pa, n, B, PER_SEED, 0, beta)
    disc = _mixed(n, rng)
    okw = dict({k: v for k, v in _cfg_kw({}).items() if k != "form"}, gamma=disc[want_slots].astype(np.float64))
    online, target, rows = _ring_for_batch(n, 71, want_slots, want_w, noise, **okw)
    net = _nnet(3, n, 320, prioritized=True)
    try:
        _load(net, online, target)
        assert net.replay_add(*rows) == (n, n)
        net.set_priorities(pa, 0.05)
        net.set_nstep_discounts(disc)
        net.replay_beta = beta
        net.train_prioritized(B, noise=noise)
        slots, w = net.last_slots, net.fetch("per_w", B)
        assert np.array_equal(slots, want_slots)
        assert _eq(net.fetch("disc", B), disc[slots])
        st = o.new_state(online, target)
        batch = _f64(tuple(t[slots] for t in rows))
        out = per.train_step(st, *batch, w.astype(np.float64), LR, noise.astype(np.float64), **okw)
        for name in ("y", "q", "dq"):
            _check(name, net.fetch(name, B), out[name])
        _check("qt", net.fetch("qt", B), o.targets(target, batch[4], batch[2], batch[3], okw["gamma"])[1])
        for k in o.CRITIC_TRAINABLE:
            _check("grad " + k, net.get_variable_value(k, 4), out["critic_grads"][k])
        y, q = net.fetch("y", B), net.fetch("q", B)
        assert np.array_equal(net.fetch("per_td", B), np.abs(y - q))        # the new priorities come from the n-step target
    finally:
        net.close()


# ---- 3. train steps are the twin's

TRAIN = [("plain", dict(), 1, False, False), ("clip", dict(USE_GRAD_CLIP=True), 1, False, False),
         ("adam", dict(RMSPROP=False), 1, False, False), ("updates3", dict(), 3, False, False), ("per", dict(), 1, True, False),
         ("twin", dict(), 1, False, True)]


@pytest.mark.parametrize("B", [1, 16, 17, 64])
@pytest.mark.parametrize("case", TRAIN, ids=[c[0] for c in TRAIN])
def test_train_steps_are_the_twins(case, B):
    """test_gpu_ddpg_actors' test of the same name at n = 3: the second handle is fed the run's ring rows by replay_add and
    its discounts by nstep_set, and takes a train step wherever the rule says the device took one."""
    _, cfg, updates, prioritized, twin = case
    N, n, capacity, steps, noise = 17, 3, 400, 8, [0.3]
    net, other = (_nnet(n, capacity, 64, prioritized, twin, **cfg) for _ in range(2))
    if prioritized:
        net.replay_beta = other.replay_beta = 0.4
    online, target = _weights(31)
    if twin:
        rng = np.random.Generator(np.random.PCG64(31))
        online, target = t3.random_params(S, A, rng), t3.random_params(S, A, rng)
    names = t3.TRAINABLE if twin else o.TRAINABLE
    snap = lambda h: gt._snapshot(h, names)        # noqa: E731
    try:
        for h in (net, other):
            (gt._load if twin else _load)(h, online, target)
        start = snap(net)
        net.actors_create(N, seed=5, updates=updates, batch=B, draw_seed=DRAW_SEED)
        net.actors_set("elapsed", np.where(np.arange(N) % 2, po.TIME_LIMIT - 10, 0).astype(np.int32))    # ends inside the second run
        # while the ring holds at most B rows nothing trains: step(None), the n - 1 silent steps, then B // N adding ones
        quiet = 1 + (n - 1) + B // N
        assert net.actors_run(quiet, train=True, noise=noise) == (N * quiet, 0, 0, 0)
        assert net.replay_size()[0] == N * (B // N) <= B and net.get_global_step() == 0 and _same(start, snap(net))
        adds = B // N + steps
        sizes = _train_sizes(N, B, adds, updates)
        assert len(sizes) == steps * updates
        stats = net.actors_run(steps, train=True, noise=noise)
        assert stats[:3] == (N * steps, len(sizes), len(sizes) * B) and stats[3] == N // 2
        assert net.replay_size() == (N * adds, N * adds) and N * adds < capacity
        rows, disc = _ring_rows(net, range(N * adds)), net.nstep_discounts()
        assert len(np.unique(disc[:N * adds])) > 1 and np.any(rows[:, S + A + 1] == 1.0)
        sample, q_other, last_slots = 0, None, None
        for k in range(adds):
            f = rows[k * N:(k + 1) * N]
            size, _ = other.replay_add(f[:, :S], f[:, S:S + A], f[:, S + A], f[:, S + A + 1], f[:, S + A + 2:])
            other.set_nstep_discounts(disc)
            if size > B:
                for _ in range(updates):
                    assert size == sizes[sample]
                    if prioritized:
                        q_other = other.train_prioritized(B, noise=noise)
                        last_slots = other.last_slots
                    else:
                        last_slots = do.uniform_slots(DRAW_SEED, sample, size, B)
                        q_other = other.train_replay(last_slots, noise=noise)
                    sample += 1
        assert sample == len(sizes)
        assert np.array_equal(net.actors_get("slots"), last_slots)
        assert _eq(net.fetch("disc", B), other.fetch("disc", B)) and _eq(net.fetch("disc", B), disc[last_slots])
        assert net.logging == q_other
        assert _same(snap(net), snap(other))
        assert net.get_global_step() == other.get_global_step() == len(sizes)
        assert not _same(start, snap(net))
        if prioritized:
            (pa, top), (opa, otop) = net.priorities(), other.priorities()
            assert top == otop and _eq(pa, opa)
    finally:
        net.close()
        other.close()


# ---- 4. one is today

def test_one_step_state_changes_nothing():
    online, target = _weights(41)
    out = []
    for n in (1, None):
        net = _nnet(n, 400, 64)
        try:
            _load(net, online, target)
            net.actors_create(17, seed=77, updates=2, batch=16, draw_seed=DRAW_SEED)
            net.actors_set("elapsed", np.full(17, po.TIME_LIMIT - 6, np.int32))
            stats = net.actors_run(8, train=True, noise=[0.3])
            assert stats == (17 * 8, 14, 14 * 16, 17)
            arenas = {(k, w): net.get_variable_value(k, w) for k in o.ALL_VARS for w in (0, 1, 2, 3, 4)}
            out.append((arenas, _ring_rows(net, range(17 * 7)), net.actors_episodes(), net.logging, net.get_global_step()))
            if n:
                assert np.all(net.nstep_discounts() == np.float32(GAMMA)) and np.all(net.fetch("disc", 16) == np.float32(GAMMA))
        finally:
            net.close()
    assert _same(out[0][0], out[1][0]) and _eq(out[0][1], out[1][1]) and out[0][2:] == out[1][2:]


# ---- 5. determinism, return codes, the product line

def test_the_same_seed_gives_the_same_bits():
    online, target = _weights(41)
    snaps, rings, discs, eps = [], [], [], []
    for _ in range(2):
        net = _nnet(5, 1000, 64)
        try:
            _load(net, online, target)
            net.actors_create(33, seed=77, updates=2, batch=16, draw_seed=DRAW_SEED)
            net.actors_set("elapsed", np.full(33, 190, np.int32))
            start = _snapshot(net)
            assert net.actors_run(12, train=False) == (33 * 12, 0, 0, 33)      # the handle's own noise process
            assert net.get_global_step() == 0 and _same(start, _snapshot(net))
            assert net.replay_size() == (33 * 7, 33 * 7)                       # 11 transitions, the first 4 silent
            stats = net.actors_run(20, train=True)
            assert stats == (33 * 20, 40, 40 * 16, 0) and net.get_global_step() == 40
            snaps.append(_snapshot(net))
            rings.append(_ring_rows(net, range(33 * 27)))
            discs.append(net.nstep_discounts())
            eps.append(net.actors_episodes())
        finally:
            net.close()                               # destroy with live actors and n-step state
    assert _same(snaps[0], snaps[1]) and _eq(rings[0], rings[1]) and _eq(discs[0], discs[1]) and eps[0] == eps[1]
    assert len(eps[0]) == 33 and len(np.unique(discs[0])) == 5


def test_return_codes():
    import ga3c_amd  # noqa: F401
    import _native as nat
    lib = nat.hip_lib()
    net = _net(S, A, max_batch=32, capacity=20)
    nofuture = _net(S, A, max_batch=32, capacity=20, DDPG_FUTURE_REWARD_CALC=False)
    buf = np.full(64, 0.5, np.float32)
    try:
        h = net._h
        create, destroy, get, put = (getattr(lib, "ga3c_ddpg_nstep_" + k) for k in ("create", "destroy", "get", "set"))
        # without n-step: GA3C_ESTATE from every call, and from fetch for "disc"
        assert destroy(h) == ESTATE and get(h, nat.ptr(buf), 20) == ESTATE and put(h, nat.ptr(buf), 20) == ESTATE
        assert lib.ga3c_ddpg_fetch(h, b"disc", nat.ptr(buf), 1) == ESTATE
        for n in (0, 17, -1):
            assert create(h, n) == EINVAL, n
        assert create(nofuture._h, 5) == ESTATE
        assert create(None, 5) == EINVAL
        # the window is sized at actors_create: n-step comes first
        assert lib.ga3c_ddpg_actors_create(h, 4, 1, 1) == 0
        assert create(h, 5) == ESTATE
        assert net.actors_get("nstep") == 1
        assert lib.ga3c_ddpg_actors_destroy(h) == 0
        assert create(h, 16) == 0 and create(h, 16) == ESTATE
        assert get(h, nat.ptr(buf), 19) == EINVAL and get(h, nat.ptr(buf), 21) == EINVAL and get(h, None, 20) == EINVAL
        assert get(h, nat.ptr(buf), 20) == 0 and np.all(buf[:20] == np.float32(GAMMA)) and np.all(buf[20:] == 0.5)
        for bad in (float("nan"), -0.01, 1.5, float("inf")):
            v = np.full(20, 0.5, np.float32)
            v[7] = bad
            assert put(h, nat.ptr(v), 20) == EINVAL, bad
        assert put(h, nat.ptr(buf), 21) == EINVAL and put(h, None, 20) == EINVAL
        edge = np.linspace(0, 1, 20).astype(np.float32)
        assert put(h, nat.ptr(edge), 20) == 0 and _eq(net.nstep_discounts(), edge)      # 0 and 1 themselves are taken
        net.train(*gt._args(gd._candidates(S, A, 16, np.random.default_rng(0))), noise=False)
        assert lib.ga3c_ddpg_fetch(h, b"disc", nat.ptr(buf), 17) == EINVAL
        assert lib.ga3c_ddpg_fetch(h, b"disc", nat.ptr(buf), 16) == 0 and np.all(buf[:16] == np.float32(GAMMA))      # no slot
        # destroy: refused while actors live
        assert lib.ga3c_ddpg_actors_create(h, 4, 1, 1) == 0
        assert net.actors_get("nstep") == 16 and net.actors_get("nstep_count") == 0
        for name, size in ((b"nstep", 4), (b"nstep_count", 8)):
            assert lib.ga3c_ddpg_actors_set(h, name, buf.ctypes.data_as(C.c_void_p), size) == EINVAL, name      # read only
        assert lib.ga3c_ddpg_actors_get(h, b"nstep", buf.ctypes.data_as(C.c_void_p), 8) == EINVAL
        assert destroy(h) == ESTATE
        assert net.actors_run(3, train=False, noise=[0.1]) == (12, 0, 0, 0) and net.actors_get("nstep_count") == 2
        assert lib.ga3c_ddpg_actors_destroy(h) == 0
        assert destroy(h) == 0 and destroy(h) == ESTATE
        assert create(h, 1) == 0
        assert lib.ga3c_ddpg_actors_create(h, 4, 1, 1) == 0
    finally:
        net.close()              # destroy with live actors and n-step state
        nofuture.close()


LINES = [("alone", []), ("prioritized-twin", ["PRIORITIZED_REPLAY=True", "DDPG_TWIN=True", "DDPG_CRITIC_LOSS=paired"])]


@pytest.mark.timeout(120)
@pytest.mark.parametrize("line", LINES, ids=[c[0] for c in LINES])
def test_train_script_runs_nstep(line, tmp_path):
    env = dict(os.environ, PYTHONUNBUFFERED="1")
    run = subprocess.run(["timeout", "-k", "10", "90", "sh", os.path.join(PKG, "_train.sh"), "GAME=Pendulum-v0", "USE_DDPG=True",
                          "TRAINING_MIN_BATCH_SIZE=64", "DEVICE_AGENTS=64", "DEVICE_DDPG=True", "DDPG_NSTEP=3", "MAX_SECONDS=5"] + line[1],
                         cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=110)
    assert run.returncode == 0, run.stdout[-3000:] + run.stderr[-3000:]
    assert "died" not in run.stdout + run.stderr
    status = [ln for ln in run.stdout.splitlines() if "TPS:" in ln]
    assert status and re.search(r"\[NT:  0 NP:  0 NA: 64\]", status[-1]), run.stdout[-2000:]
    tps = [int(t) for t in re.findall(r"TPS:\s*(\d+)\]", run.stdout)]
    assert max(tps) > 0
    lines = open(os.path.join(str(tmp_path), "results.txt")).read().strip().splitlines()
    # the episode records are per step and unchanged: step(None) and 199 transitions, every later one 200
    assert lines and all(int(ln.split(",")[2]) in (200, 201) for ln in lines)
    assert all(-1.09 * 200 <= float(ln.split(",")[1]) <= -199 for ln in lines)
