"""-m gpu: prioritised replay on the DDPG handle (ga3c_ddpg_priorities_* / _sample_prioritized / _train_prioritized, DESIGN.md
8j) against its numpy statement (tests/per_oracle.py).  S = 3, A = 1.

Slots are held to the oracle exactly: every operation that decides one is an f64 add, product, quotient or compare in a
stated order.  Weights and new priorities carry one pow each, then a cast to f32: 1e-6 relative.  The step itself keeps the
tolerances of tests/test_gpu_ddpg.py (1e-4 x max(1, max|want|) on q, dq and gradients, 1e-5 on both nets afterwards), and as
there the ring holds only rows whose relu units all keep 1e-4 away from zero in the oracle, so that f32 cannot land on the
other side.  Which slots a step draws depends on the priorities alone, so the oracle's draw is known before the ring is
filled, and the rows are chosen so that the drawn batch also keeps that margin where step 4 evaluates the updated critic
(_ring_for_batch, the counterpart of test_gpu_ddpg._select)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import ddpg_oracle as o
import per_oracle as per
from test_gpu_ddpg import LR, PKG, ROOT, WTOL, _candidates, _cfg_kw, _check, _f64, _load, _net, _same, _snapshot

pytestmark = pytest.mark.gpu

S, A = 3, 1
ALPHA, EPS, SEED = 0.6, 0.01, 12345
EINVAL, ESTATE = -1, -4
RINGS = [(1, 1), (1023, 1023), (1024, 1024), (1025, 1025), (2049, 1500), (5000, 7300)]
SIZES = [1, 15, 16, 17, 64, 300]
PTOL = 1e-6


def _per_net(capacity, max_batch=320, prioritized=True, alpha=ALPHA, **kw):
    kw.setdefault("DDPG_CRITIC_LOSS", "paired")
    return _net(S, A, max_batch=max_batch, capacity=capacity, PRIORITIZED_REPLAY=prioritized, PRIORITIZED_REPLAY_ALPHA=alpha,
                PRIORITIZED_REPLAY_EPS=EPS, REPLAY_BUFFER_RANDOM_SEED=SEED, **kw)


def _rows(n, rng):
    return (rng.uniform(-1.5, 1.5, (n, S)).astype(np.float32), rng.uniform(-1, 1, (n, A)).astype(np.float32),
            rng.uniform(-1, 0, n).astype(np.float32), (rng.uniform(size=n) < 0.25).astype(np.float32),
            rng.uniform(-1.5, 1.5, (n, S)).astype(np.float32))


def _add(net, rows, step=None):
    """Appends the rows in calls of at most max_batch -> (size, total)."""
    n = len(rows[2])
    step = step or min(net.max_batch, net.replay_capacity)
    out = None
    for lo in range(0, n, step):
        out = net.replay_add(*(t[lo:lo + step] for t in rows))
    return out


def _random_priorities(capacity, size, rng):
    pa = np.zeros(capacity, np.float32)
    pa[:size] = rng.uniform(0.01, 2, size).astype(np.float32) ** np.float32(0.6)
    return pa


def _rel(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(np.max(np.abs(got - want) / np.abs(want)))


# ---- the draw

@pytest.mark.parametrize("capacity,added", RINGS)
def test_draw_equals_the_oracle_slot_for_slot(capacity, added):
    rng = np.random.default_rng(capacity)
    size = min(capacity, added)
    net = _per_net(capacity)
    try:
        assert _add(net, _rows(added, rng)) == (size, added)
        net.set_priorities(_random_priorities(capacity, size, rng), 2.0)
        pa, top = net.priorities()
        assert top == np.float32(2.0)
        net.replay_beta = 0.4
        for number, B in enumerate(SIZES):
            slots, w = net.sample_prioritized(B)
            want, total, clamped = per.draw(pa, size, B, SEED, number)
            print("ring %d/%d B %d: clamped %d, duplicates %d" % (capacity, size, B, clamped, B - len(set(want.tolist()))))
            assert slots.dtype == np.int32 and np.array_equal(slots, want), (B, slots, want)
            assert _rel(w, per.weights(pa, size, want, total, 0.4)) <= PTOL and w.max() == 1.0
            assert np.array_equal(net.fetch("per_w", B), w)
        # the draw changed nothing
        again, top2 = net.priorities()
        assert np.array_equal(again, pa) and top2 == top and net.get_global_step() == 0
    finally:
        net.close()


def test_draw_from_a_million_rows():
    capacity, B = 1048576, 64
    rng = np.random.default_rng(7)
    net = _per_net(capacity, max_batch=4096)
    try:
        zeros = (np.zeros((4096, S), np.float32), np.zeros((4096, A), np.float32), np.zeros(4096, np.float32),
                 np.zeros(4096, np.float32), np.zeros((4096, S), np.float32))
        for _ in range(capacity // 4096):
            got = net.replay_add(*zeros)
        assert got == (capacity, capacity)
        pa, top = net.priorities()
        assert top == 1.0 and np.all(pa == 1.0)             # every row added got max_pa
        net.set_priorities(_random_priorities(capacity, capacity, rng), 2.0)
        pa, _ = net.priorities()
        net.replay_beta = 1.0
        for number in range(2):
            slots, w = net.sample_prioritized(B)
            want, total, clamped = per.draw(pa, capacity, B, SEED, number)
            print("sample %d: clamped %d, largest slot %d" % (number, clamped, want.max()))
            assert np.array_equal(slots, want)
            assert _rel(w, per.weights(pa, capacity, want, total, 1.0)) <= PTOL
        assert want.max() > capacity - 2 * capacity // B       # the last stratum lies in the last chunks
    finally:
        net.close()


def test_heavy_tail_duplicates_the_sample_counter_and_the_seed():
    capacity = size = 2049
    pa = np.full(capacity, 1e-3, np.float32)
    pa[700] = 50.0
    rng = np.random.default_rng(1)
    rows = _rows(size, rng)
    drawn = []
    for _ in range(2):
        net = _per_net(capacity)
        try:
            _add(net, rows)
            net.set_priorities(pa, 50.0)
            net.replay_beta = 1.0
            batches = [net.sample_prioritized(64) for _ in range(3)]
            drawn.append(batches)
        finally:
            net.close()
    for number, (slots, w) in enumerate(drawn[0]):
        want, total, _ = per.draw(pa, size, 64, SEED, number)
        assert np.array_equal(slots, want)
        assert 60 <= int((slots == 700).sum()) <= 63         # 96 % of the mass: 61.5 of 64 strata
        assert _rel(w, per.weights(pa, size, want, total, 1.0)) <= PTOL
    assert not np.array_equal(drawn[0][0][0], drawn[0][1][0]) and not np.array_equal(drawn[0][1][0], drawn[0][2][0])
    for a, b in zip(drawn[0], drawn[1]):                     # a fresh handle with the same seed
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


# ---- new rows

def test_added_rows_get_max_pa_and_no_other_slot_changes():
    capacity, row_bytes = 50, 32
    rng = np.random.default_rng(2)
    net = _per_net(capacity, max_batch=64)
    seg = np.zeros((64, row_bytes // 4), np.float32)
    try:
        class Seg:
            base, nbytes = seg.ctypes.data, seg.nbytes
        net.register_transport(Seg)
        assert _add(net, _rows(30, rng)) == (30, 30)
        pa, top = net.priorities()
        assert top == 1.0 and np.all(pa[:30] == 1.0) and np.all(pa[30:] == 0.0)
        want = np.zeros(capacity, np.float32)
        want[:30] = rng.uniform(0.01, 2, 30).astype(np.float32)
        net.set_priorities(want, 3.5)
        total = 30
        # replay_add, then replay_add_gather across the ring's end, then replay_add across it again
        for how, n in (("add", 7), ("gather", 20), ("add", 45), ("gather", 1)):
            if how == "add":
                got = net.replay_add(*_rows(n, rng))
            else:
                got = net.replay_add_offsets(np.arange(n, dtype=np.int64) * row_bytes, np.zeros(n, np.float32),
                                             np.zeros((n, A), np.float32))
            per.fill(want, 3.5, total, n)
            total += n
            assert got == (min(total, capacity), total)
            pa, top = net.priorities()
            assert top == np.float32(3.5) and np.array_equal(pa, want), (how, n)
        net.unregister_transport()
    finally:
        net.close()


def test_create_on_a_ring_that_holds_rows_gives_them_one():
    rng = np.random.default_rng(3)
    net = _per_net(100, max_batch=64, prioritized=False)
    try:
        _add(net, _rows(40, rng))
        assert net._lib.ga3c_ddpg_priorities_create(net._h, ALPHA, EPS, SEED) == 0
        pa, top = net.priorities()
        assert top == 1.0 and np.all(pa[:40] == 1.0) and np.all(pa[40:] == 0.0)
    finally:
        net.close()


# ---- the step

def _ring_case(n, seed):
    """-> (online, target, rows): U(-0.3, 0.3) weights and n ring rows, for the tests that compare two handles or the
    device with itself (no margin is needed where no oracle step is compared)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    return o.random_params(S, A, rng), o.random_params(S, A, rng), _rows(n, rng)


def _ring_for_batch(n, seed, slots, w, noise, **kw):
    """-> (online, target, rows): weights and n ring rows out of 3 n candidates.  Every row keeps the margin of
    ddpg_oracle.relu_margin under the initial weights; the batch rows[slots], trained with the weights w, keeps it where
    step 4 evaluates the updated critic at the actor's output as well.  The choice is repeated until it holds."""
    rng = np.random.Generator(np.random.PCG64(seed))
    online, target = o.random_params(S, A, rng), o.random_params(S, A, rng)
    cand = _candidates(S, A, 3 * n, rng)
    ok = o.relu_margin(online, target, cand[0], cand[1], cand[4]) > 1e-4
    for _ in range(50):
        keep = np.flatnonzero(ok)[:n]
        assert keep.size == n, "only %d of %d candidate rows qualify" % (keep.size, ok.size)
        rows = tuple(t[keep] for t in cand)
        batch = _f64(tuple(t[slots] for t in rows))
        trial = o.new_state(online, target, critic_rmsprop=kw.get("critic_rmsprop", True))
        out = per.train_step(trial, *batch, np.asarray(w, np.float64), LR, np.asarray(noise, np.float64), **kw)
        t4 = o.critic_forward(trial["online"], batch[0], out["a_out"])["t"]
        bad = np.abs(t4).min(axis=1) <= 1e-4
        if not bad.any():
            return online, target, rows
        ok[keep[slots[bad]]] = False
    raise AssertionError("the choice of rows did not settle")


def _twin(online, target, rows, pa, max_pa, prioritized, **cfg):
    net = _per_net(len(rows[2]), prioritized=prioritized, **cfg)
    _load(net, online, target)
    _add(net, rows)
    if prioritized:
        net.set_priorities(pa, max_pa)
    return net


@pytest.mark.parametrize("cfg", [dict(), dict(USE_GRAD_CLIP=True)], ids=["rmsprop", "clip"])
@pytest.mark.parametrize("B", [17, 64])
def test_beta_zero_is_train_replay_on_the_same_slots_bit_for_bit(B, cfg):
    """A weight of exactly 1 changes no product: arenas 0..3 and the step counter equal those of a plain handle that is given
    the drawn slots, over two steps (the second draws from updated priorities)."""
    n = 128
    online, target, rows = _ring_case(n, 61)
    pa = _random_priorities(n, n, np.random.default_rng(4))
    net = _twin(online, target, rows, pa, 2.0, True, **cfg)
    plain = _twin(online, target, rows, pa, 2.0, False, **cfg)
    try:
        net.replay_beta = 0.0
        for step in range(2):
            q = net.train_prioritized(B, noise=[0.1])
            assert np.all(net.fetch("per_w", B) == 1.0)
            assert plain.train_replay(net.last_slots, noise=[0.1]) == q
            assert _same(_snapshot(net), _snapshot(plain)), "step %d" % step
            for name in ("y", "q", "dq"):
                assert np.array_equal(net.fetch(name, B), plain.fetch(name, B)), name
        assert net.get_global_step() == plain.get_global_step() == 2
    finally:
        net.close()
        plain.close()


def _check_update(net, before, top_before, slots, B):
    """pa after a prioritised step: (per_td + eps)^alpha at the batch's slots from the fetched y and q, the last row's where a
    slot occurs twice; every other slot as it was; max_pa the larger of old and new."""
    y, q, td = net.fetch("y", B), net.fetch("q", B), net.fetch("per_td", B)
    assert np.array_equal(td, np.abs(y - q))
    _, new = per.new_priorities(y, q, EPS, ALPHA)
    after, top = net.priorities()
    last = {int(s): i for i, s in enumerate(slots)}
    rows = np.array(sorted(last.values()))
    print("priority update: %d rows, %d slots, largest relative error %.2e" % (B, len(last), _rel(after[slots[rows]], new[rows])))
    assert _rel(after[slots[rows]], new[rows]) <= PTOL
    untouched = np.setdiff1d(np.arange(after.size), slots)
    assert np.array_equal(after[untouched], before[untouched])
    want_top = max(float(top_before), float(new.max()))
    assert abs(float(top) - want_top) <= PTOL * want_top
    if float(new.max()) <= float(top_before):
        assert top == top_before
    return after, top


@pytest.mark.parametrize("cfg", [dict(), dict(RMSPROP=False), dict(USE_GRAD_CLIP=True, RMSPROP_MOMENTUM=0.9)],
                         ids=["rmsprop", "adam", "clip-momentum"])
@pytest.mark.parametrize("beta", [0.4, 1.0])
def test_weighted_step_matches_the_oracle(beta, cfg):
    n, B = 128, 64
    noise = np.full(A, 0.05, np.float32)
    okw = {k: v for k, v in _cfg_kw(cfg).items() if k != "form"}
    pa = _random_priorities(n, n, np.random.default_rng(5))
    want_slots, want_w = per.sample(pa, n, B, SEED, 0, beta)
    online, target, rows = _ring_for_batch(n, 71, want_slots, want_w, noise, **okw)
    net = _twin(online, target, rows, pa, 0.05, True, **cfg)
    try:
        net.replay_beta = beta
        q_max, q_avg = net.train_prioritized(B, noise=noise)
        slots, w = net.last_slots, net.fetch("per_w", B)
        assert np.array_equal(slots, want_slots) and _rel(w, want_w) <= PTOL
        assert len(np.unique(w)) > B // 2, "the weights do not vary"
        st = o.new_state(online, target, critic_rmsprop=cfg.get("RMSPROP", True))
        batch = _f64(tuple(t[slots] for t in rows))
        out = per.train_step(st, *batch, w.astype(np.float64), LR, noise.astype(np.float64), **okw)
        t4 = o.critic_forward(st["online"], batch[0], out["a_out"])["t"]
        assert np.abs(t4).min() > 9e-5, "the fetched weights moved a row of the batch onto a relu's edge"
        _check("q_max", [q_max], [out["q"].max()])
        _check("q_avg", [q_avg], [out["q"].mean()])
        for name in ("y", "q", "dq"):
            _check(name, net.fetch(name, B), out[name])
        unweighted = (2.0 / B) * (out["q"] - out["y"])
        assert np.max(np.abs(out["dq"] - unweighted)) > 1e-3, "the weights did not reach the oracle's loss"
        for k in o.CRITIC_TRAINABLE:
            _check("grad " + k, net.get_variable_value(k, 4), out["critic_grads"][k])
        for k in o.ACTOR_TRAINABLE:
            _check("grad " + k, net.get_variable_value(k, 4), out["actor_grads"][k])
        for k in o.TRAINABLE:
            _check("online " + k, net.get_variable_value(k, 0), st["online"][k], WTOL)
            _check("target " + k, net.get_variable_value(k, 1), st["target"][k], WTOL)
            _check("slot a " + k, net.get_variable_value(k, 2), st["slot_a"][k], WTOL)
            _check("slot b " + k, net.get_variable_value(k, 3), st["slot_b"][k], WTOL)
        assert net.get_global_step() == 1
        _check_update(net, pa, np.float32(0.05), slots, B)      # max_pa was small: the new priorities raise it
    finally:
        net.close()


def test_update_with_duplicates_keeps_the_last_row_and_max_pa_never_decreases():
    n, B = 128, 64
    online, target, rows = _ring_case(n, 81)
    pa = np.full(n, 1e-3, np.float32)
    pa[[5, 77]] = 4.0, 2.0                                    # two slots carry nearly all the mass
    net = _twin(online, target, rows, pa, 40.0, True)
    try:
        net.replay_beta = 0.4
        before, top = pa, np.float32(40.0)
        for step in range(2):
            net.train_prioritized(B, noise=False)
            slots = net.last_slots
            if step == 0:
                assert np.array_equal(slots, per.draw(pa, n, B, SEED, 0)[0])
                assert (slots == 5).sum() > 20 and (slots == 77).sum() > 10
            before, top = _check_update(net, before, top, slots, B)
            assert top == np.float32(40.0)
    finally:
        net.close()


def test_time_prioritized_runs_whole_steps():
    n = 128
    online, target, rows = _ring_case(n, 91)
    net = _twin(online, target, rows, _random_priorities(n, n, np.random.default_rng(6)), 2.0, True)
    try:
        before = _snapshot(net)
        ms = net.time_prioritized(64, 3)
        assert ms > 0 and net.get_global_step() == 3 and not _same(before, _snapshot(net))
        slots, _ = net.sample_prioritized(64)                # three draws were taken: this one is number 3
        assert np.array_equal(slots, per.draw(net.priorities()[0], n, 64, SEED, 3)[0])
    finally:
        net.close()


# ---- return codes

def _codes(net):
    lib, h = net._lib, net._h
    B = 16
    slots, w, q, ms = (C.c_int32 * B)(), (C.c_float * B)(), (C.c_float * 2)(), C.c_float()
    pa = (C.c_float * net.replay_capacity)()
    top = C.c_float()
    return {"destroy": lambda: lib.ga3c_ddpg_priorities_destroy(h),
            "get": lambda: lib.ga3c_ddpg_priorities_get(h, pa, C.byref(top)),
            "set": lambda: lib.ga3c_ddpg_priorities_set(h, pa, 1.0),
            "sample": lambda: lib.ga3c_ddpg_sample_prioritized(h, B, 0.4, slots, w),
            "train": lambda: lib.ga3c_ddpg_train_prioritized(h, B, 0.4, LR, 2, None, q, slots),
            "time": lambda: lib.ga3c_ddpg_time_prioritized(h, B, 1, 0.4, LR, C.byref(ms)),
            "fetch per_w": lambda: lib.ga3c_ddpg_fetch(h, b"per_w", w, B),
            "fetch per_td": lambda: lib.ga3c_ddpg_fetch(h, b"per_td", w, B)}


def test_a_handle_without_priorities_refuses_the_entries_and_trains_as_before():
    n, B = 64, 16
    online, target, rows = _ring_case(n, 101)
    nets = [_twin(online, target, rows, None, None, False) for _ in range(2)]
    try:
        for name, call in _codes(nets[0]).items():
            assert call() == ESTATE, name
        slots = np.arange(B, dtype=np.int32) * 3
        for net in nets:
            net.train_replay(slots, noise=False)
        assert _same(_snapshot(nets[0]), _snapshot(nets[1]))
        # attached and taken away again: refused as before, and the ring is still there
        lib, h = nets[0]._lib, nets[0]._h
        assert lib.ga3c_ddpg_priorities_create(h, ALPHA, EPS, SEED) == 0
        assert lib.ga3c_ddpg_priorities_create(h, ALPHA, EPS, SEED) == ESTATE        # a second create
        assert _codes(nets[0])["sample"]() == 0
        assert lib.ga3c_ddpg_priorities_destroy(h) == 0
        assert _codes(nets[0])["sample"]() == ESTATE and nets[0].replay_size() == (n, n)
    finally:
        for net in nets:
            net.close()


def test_create_refusals():
    net = _per_net(64, max_batch=32, prioritized=False)
    fork = _per_net(64, max_batch=32, prioritized=False, DDPG_CRITIC_LOSS="fork")
    large = _per_net(1048577, max_batch=32, prioritized=False)
    try:
        create = net._lib.ga3c_ddpg_priorities_create
        nan = float("nan")
        for alpha, eps in ((-0.1, EPS), (1.1, EPS), (nan, EPS), (ALPHA, 0.0), (ALPHA, -1.0), (ALPHA, nan)):
            assert create(net._h, alpha, eps, SEED) == EINVAL, (alpha, eps)
        assert create(large._h, ALPHA, EPS, SEED) == EINVAL
        assert create(fork._h, ALPHA, EPS, SEED) == ESTATE
        assert create(None, ALPHA, EPS, SEED) == EINVAL
        for alpha in (0.0, 1.0):                                # the ends of the range are in it
            assert create(net._h, alpha, EPS, SEED) == 0
            assert net._lib.ga3c_ddpg_priorities_destroy(net._h) == 0
    finally:
        for m in (net, fork, large):
            m.close()
    with pytest.raises(RuntimeError):                           # NetworkDDPG attaches at construction: the same refusal
        _per_net(64, max_batch=32, prioritized=True, DDPG_CRITIC_LOSS="fork")


def test_sample_train_and_set_refusals():
    B = 16
    rng = np.random.default_rng(8)
    net = _per_net(64, max_batch=32)
    try:
        lib, h = net._lib, net._h
        codes = _codes(net)
        assert codes["sample"]() == ESTATE and codes["train"]() == ESTATE          # an empty ring
        _add(net, _rows(B, rng))
        assert codes["sample"]() == 0
        assert codes["train"]() == ESTATE and codes["time"]() == ESTATE            # exactly a batch: not MORE than one
        assert net.get_global_step() == 0
        _add(net, _rows(1, rng))
        assert codes["train"]() == 0 and net.get_global_step() == 1
        slots, w = (C.c_int32 * 64)(), (C.c_float * 64)()
        for batch in (0, -1, 33):
            assert lib.ga3c_ddpg_sample_prioritized(h, batch, 0.4, slots, w) == EINVAL
            assert lib.ga3c_ddpg_train_prioritized(h, batch, 0.4, LR, 2, None, None, None) == EINVAL
        assert lib.ga3c_ddpg_sample_prioritized(h, B, -0.5, slots, w) == EINVAL
        assert lib.ga3c_ddpg_sample_prioritized(h, B, float("nan"), slots, w) == EINVAL
        assert lib.ga3c_ddpg_sample_prioritized(h, B, 0.4, None, w) == EINVAL
        assert lib.ga3c_ddpg_train_prioritized(h, B, 0.4, LR, 2, None, None, None) == 0    # q_stats and out_slots may be null
        assert lib.ga3c_ddpg_fetch(h, b"per_w", w, B + 1) == EINVAL
        # priorities_set: 17 rows held
        good = np.zeros(64, np.float32)
        good[:17] = 0.5
        net.set_priorities(good, 1.0)
        for slot, value in ((3, -0.5), (40, -0.5), (3, float("nan")), (40, float("nan")), (16, 0.0)):
            bad = good.copy()
            bad[slot] = value
            assert lib.ga3c_ddpg_priorities_set(h, bad.ctypes.data_as(C.POINTER(C.c_float)), 1.0) == EINVAL, (slot, value)
        for top in (0.0, -1.0, float("nan")):
            assert lib.ga3c_ddpg_priorities_set(h, good.ctypes.data_as(C.POINTER(C.c_float)), top) == EINVAL
        ok = good.copy()
        ok[17], ok[40] = 0.0, 0.25                              # beyond the rows held anything that is a priority goes
        net.set_priorities(ok, 1.0)
        got, _ = net.priorities()
        assert np.array_equal(got, ok)
        with pytest.raises(ValueError):
            net.set_priorities(good[:10], 1.0)
    finally:
        net.close()


# ---- the product

@pytest.mark.timeout(300)
def test_train_sh_runs_ddpg_with_prioritized_replay(tmp_path):
    env = dict(os.environ, PYTHONPATH=ROOT)
    cmd = ["sh", os.path.join(PKG, "_train.sh"), "GAME=Pendulum-v0", "USE_DDPG=True", "PRIORITIZED_REPLAY=True",
           "DDPG_CRITIC_LOSS=paired", "TRAINING_MIN_BATCH_SIZE=64", "MAX_SECONDS=20", "AGENTS=8", "PREDICTORS=1", "TRAINERS=1",
           "DYNAMIC_SETTINGS="]
    run = subprocess.run(cmd, cwd=str(tmp_path), env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=240)
    text = run.stdout.decode(errors="replace")
    sys.stdout.write(text[-3000:])
    assert run.returncode == 0
    assert "[replay]" not in text
    lines = open(str(tmp_path / "results.txt")).read().splitlines()
    assert len(lines) >= 5, "fewer than five episodes logged"
    status = [t for t in text.splitlines() if "TPS:" in t and "[RSize:" in t]
    assert status and max(int(t.split("TPS:")[1].split("]")[0]) for t in status) > 0, "no train step was counted"
    assert int(status[-1].split("[RSize:")[1].split("]")[0]) > 64
