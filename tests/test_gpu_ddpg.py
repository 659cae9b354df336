"""-m gpu: the DDPG handle (ga3c_ddpg_*) against its f64 statement (tests/ddpg_oracle.py).

Tolerance: 1e-4 x max(1, max|want|) on activations, targets and gradients, 1e-5 on weights and optimizer slots after steps,
as tests/test_gpu_vector_net.py.  Test weights are U(-0.3, 0.3) so that pre-activations are O(1).  A relu unit within 1e-4
of zero in the oracle could land on the other side in f32, so rows with such a unit in any of the four nets are left out:
2 B candidate rows are drawn, the first B that qualify are kept, and the test asserts it found B."""
import collections
import contextlib
import os
import subprocess
import sys

import numpy as np
import pytest

import ddpg_oracle as o

pytestmark = pytest.mark.gpu

TOL = 1e-4
WTOL = 1e-5
LR = 3e-4
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "ga3c_amd")
SHAPES = [(3, 1), (7, 3)]
SIZES = [1, 16, 17, 64, 128, 300]


def _err(got, want):
    got, want = np.asarray(got, np.float64).reshape(-1), np.asarray(want, np.float64).reshape(-1)
    assert got.shape == want.shape
    return float(np.max(np.abs(got - want))), max(1.0, float(np.max(np.abs(want))))


def _check(label, got, want, tol=TOL):
    """The project's closeness (tests/test_gpu_vector_net.py:20-23): max|got - want| <= tol x max(1, max|want|)."""
    err, scale = _err(got, want)
    bound = tol * scale
    print("%-28s err %.3e bound %.3e" % (label, err, bound))
    assert err <= bound, "%s: %.3e > %.3e" % (label, err, bound)


@contextlib.contextmanager
def _config(**kw):
    import ga3c_amd  # noqa: F401
    from Config import Config
    saved = {k: getattr(Config, k) for k in kw}
    for k, v in kw.items():
        setattr(Config, k, v)
    try:
        yield Config
    finally:
        for k, v in saved.items():
            setattr(Config, k, v)


def _net(S, A, max_batch=320, capacity=1024, **kw):
    import ga3c_amd  # noqa: F401
    from NetworkDDPG import Network
    kw.setdefault("add_OUnoise", True)
    with _config(**kw):
        net = Network("gpu:0", "ddpg", A, (S,), max_batch=max_batch, replay_capacity=capacity)
    net.learning_rate = LR
    return net


def _cfg_kw(cfg):
    """Config settings -> the oracle's keyword arguments."""
    return dict(form=cfg.get("DDPG_CRITIC_LOSS", "fork"), critic_rmsprop=cfg.get("RMSPROP", True),
                momentum=cfg.get("RMSPROP_MOMENTUM", 0.0), clip=40.0 if cfg.get("USE_GRAD_CLIP") else None,
                future=cfg.get("DDPG_FUTURE_REWARD_CALC", True))


def _load(net, online, target):
    for k in o.ALL_VARS:
        net.set_variable_value(k, online[k], 0)
        net.set_variable_value(k, target[k], 1)


def _candidates(S, A, n, rng):
    return (rng.uniform(-1.5, 1.5, (n, S)).astype(np.float32), rng.uniform(-1, 1, (n, A)).astype(np.float32),
            rng.uniform(-1, 0, n).astype(np.float32), (rng.uniform(size=n) < 0.25).astype(np.float32),
            rng.uniform(-1.5, 1.5, (n, S)).astype(np.float32))


def _select(st, cand, B, noise=None, **kw):
    """The first B candidate rows whose relu units all keep 1e-4 away from zero in the oracle, in each of the four nets.
    Step 4 evaluates the critic once more, AFTER step 3 on the chosen rows and at the actor's output; there only the units
    of its second layer are differentiated through (g = dq/da; the first layer enters continuously), so those are held to
    the same margin, and the choice is repeated until it holds."""
    s, a, r, done, s2 = cand
    ok = o.relu_margin(st["online"], st["target"], s, a, s2) > 1e-4
    nz = 0.0 if noise is None else np.asarray(noise, np.float64)[None, :]
    for _ in range(20):
        keep = np.flatnonzero(ok)[:B]
        assert keep.size == B, "only %d of %d candidate rows qualify" % (keep.size, ok.size)
        trial = dict(st, online={k: v.copy() for k, v in st["online"].items()},
                     slot_a={k: v.copy() for k, v in st["slot_a"].items()}, slot_b={k: v.copy() for k, v in st["slot_b"].items()})
        rows = tuple(np.asarray(t[keep], np.float64) for t in cand)
        o.train_step(trial, *rows, LR, None, stop_after=3, **kw)
        a_out = o.actor_forward(trial["online"], rows[0])["out"] + nz
        f = o.critic_forward(trial["online"], rows[0], a_out)
        bad = np.abs(f["t"]).min(axis=1) <= 1e-4
        if not bad.any():
            return tuple(t[keep] for t in cand)
        ok[keep[bad]] = False
    raise AssertionError("the choice of rows did not settle")


def _case(S, A, B, seed, stats=False, noise=None, **kw):
    """-> (online, target, batch): U(-0.3, 0.3) weights and B rows out of 2 B candidates (_select)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    online, target = o.random_params(S, A, rng, stats=stats), o.random_params(S, A, rng, stats=stats)
    st = o.new_state(online, target, critic_rmsprop=kw.get("critic_rmsprop", True))
    return online, target, _select(st, _candidates(S, A, 2 * B, rng), B, noise, **kw)


def _f64(batch):
    return tuple(np.asarray(t, np.float64) for t in batch)


def _compare_step4(net, out, S, A, B):
    fc, fa = out["critic_fwd"], out["actor_fwd"]
    for name, want in (("y", out["y"]), ("q", out["q"]), ("dq", out["dq"]), ("c_xh1", fc["xh1"]), ("c_c1", fc["c1"]),
                       ("c_c2", fc["c2"]), ("c_dt", fc["dt"]), ("c_dn1", fc["dn1"]), ("a_xh1", fa["xh1"]), ("a_a1", fa["a1"]),
                       ("a_xh2", fa["xh2"]), ("a_a2", fa["a2"]), ("a_out", fa["out"]), ("a_noisy", out["a_out"]),
                       ("g", out["g"]), ("do", fa["do"]), ("a_dn2", fa["dn2"]), ("a_dn1", fa["dn1"])):
        _check(name, net.fetch(name, np.size(want)), want)
    if out["qt"] is not None:
        _check("qt", net.fetch("qt", B), out["qt"])
    for k in o.CRITIC_TRAINABLE:
        _check("grad " + k, net.get_variable_value(k, 4), out["critic_grads"][k])
    for k in o.ACTOR_TRAINABLE:
        _check("grad " + k, net.get_variable_value(k, 4), out["actor_grads"][k])


@pytest.mark.parametrize("S,A", SHAPES)
@pytest.mark.parametrize("B", SIZES)
def test_every_intermediate_and_gradient(S, A, B):
    """Steps 1-4 with a given noise vector: every activation, y, q, g and every gradient of both nets, with non-default
    moving statistics and done rows mixed in; the critic's weights after its step."""
    noise = np.linspace(-0.2, 0.3, A).astype(np.float32)
    online, target, batch = _case(S, A, B, 100 + B + S, stats=True, noise=noise)
    net = _net(S, A)
    try:
        _load(net, online, target)
        st = o.new_state(online, target)
        out = o.train_step(st, *_f64(batch), LR, noise.astype(np.float64), stop_after=4)
        q_max, q_avg = net.compute(batch[0], batch[2], batch[1], batch[4], batch[3], 4, noise=noise)
        _check("q_max", [q_max], [out["q_max"]])
        _check("q_avg", [q_avg], [out["q_avg"]])
        _compare_step4(net, out, S, A, B)
        for k in o.CRITIC_TRAINABLE:
            _check("after step 3 " + k, net.get_variable_value(k, 0), st["online"][k], WTOL)
        assert net.get_global_step() == 0
    finally:
        net.close()


@pytest.mark.parametrize("S,A", SHAPES)
@pytest.mark.parametrize("B", SIZES)
def test_backward_tensors_relative_to_their_largest_entry(S, A, B):
    """TOL x max(1, max|want|) is absolute below 1, and the critic's deltas shrink with 2 / B: dq, c_dt and c_dn1 are below 0.1
    from 128 rows on, a_dn2 at most sizes (tests/README.md, "how large the tensors are").  Every delta and gradient of steps
    3-4 once more with tests/closeness.py: max|got - want| / max|want| against max(16 x e32, 2^-20), e32 from the oracle run
    in float32 on the same rows (the rows keep every relu unit 1e-4 away from zero: _select)."""
    import closeness as c
    noise = np.linspace(-0.2, 0.3, A).astype(np.float32)
    online, target, batch = _case(S, A, B, 100 + B + S, stats=True, noise=noise)

    def tensors(out):
        fc, fa = out["critic_fwd"], out["actor_fwd"]
        t = {"dq": out["dq"], "c_dt": fc["dt"], "c_dn1": fc["dn1"], "g": out["g"], "do": fa["do"], "a_dn2": fa["dn2"],
             "a_dn1": fa["dn1"]}
        t.update({"grad " + k: out["critic_grads"][k] for k in o.CRITIC_TRAINABLE if k != o.DEAD})
        t.update({"grad " + k: out["actor_grads"][k] for k in o.ACTOR_TRAINABLE})
        return t

    want = tensors(o.train_step(o.new_state(online, target), *_f64(batch), LR, noise.astype(np.float64), stop_after=4))
    f32 = lambda P: {k: v.astype(np.float32) for k, v in P.items()}     # noqa: E731
    w32 = tensors(o.train_step(o.new_state(f32(online), f32(target)), *batch, LR, noise, stop_after=4))
    net = _net(S, A)
    try:
        _load(net, online, target)
        net.compute(batch[0], batch[2], batch[1], batch[4], batch[3], 4, noise=noise)
        failed = []
        for name, ref in want.items():
            assert np.asarray(w32[name]).dtype == np.float32, name
            got = net.get_variable_value(name[5:], 4) if name.startswith("grad ") else net.fetch(name, np.size(ref))
            e32 = c.rel_err(w32[name], ref)
            err = c.report("ddpg S=%d A=%d B=%d" % (S, A, B), name, got, ref, e32, c.bound(e32))
            if not err <= c.bound(e32):
                failed.append((name, err, c.bound(e32)))
        assert not failed, failed
    finally:
        net.close()


@pytest.mark.parametrize("cfg", [dict(DDPG_CRITIC_LOSS="paired"), dict(DDPG_FUTURE_REWARD_CALC=False), dict(USE_GRAD_CLIP=True),
                                 dict(RMSPROP=False)], ids=lambda c: "-".join("%s=%s" % kv for kv in c.items()))
def test_loss_forms_and_flags_without_noise(cfg):
    """'paired' loss, y = r, clipping and the Adam critic, each with no noise at all (the wrap is the identity on tanh)."""
    S, A, B = 3, 1, 64
    online, target, batch = _case(S, A, B, 7, **_cfg_kw(cfg))
    net = _net(S, A, **cfg)
    try:
        _load(net, online, target)
        st = o.new_state(online, target, critic_rmsprop=cfg.get("RMSPROP", True))
        out = o.train_step(st, *_f64(batch), LR, None, stop_after=4, **_cfg_kw(cfg))
        net.compute(batch[0], batch[2], batch[1], batch[4], batch[3], 4, noise=False)
        _compare_step4(net, out, S, A, B)
        for k in o.CRITIC_TRAINABLE:
            _check("after step 3 " + k, net.get_variable_value(k, 0), st["online"][k], WTOL)
    finally:
        net.close()


def test_fork_and_paired_losses_differ():
    S, A, B = 3, 1, 64
    online, target, batch = _case(S, A, B, 7)
    dqs = []
    for form in ("fork", "paired"):
        net = _net(S, A, DDPG_CRITIC_LOSS=form)
        try:
            _load(net, online, target)
            net.compute(batch[0], batch[2], batch[1], batch[4], batch[3], 3, noise=False)
            dqs.append(net.fetch("dq", B))
        finally:
            net.close()
    assert np.max(np.abs(dqs[0] - dqs[1])) > 1e-4


@pytest.mark.parametrize("cfg", [dict(), dict(RMSPROP=False), dict(USE_GRAD_CLIP=True, RMSPROP_MOMENTUM=0.9)],
                         ids=["rmsprop", "adam", "clip-momentum"])
@pytest.mark.parametrize("S,A", SHAPES)
def test_two_full_steps(S, A, cfg):
    """Online weights, targets, both optimizer slots and the step counter after two steps of train()."""
    B = 64
    noise = np.full(A, 0.05, np.float32)
    online, target, batch = _case(S, A, B, 31 + S, noise=noise, **_cfg_kw(cfg))
    rng = np.random.Generator(np.random.PCG64(32 + S))
    net = _net(S, A, **cfg)
    try:
        _load(net, online, target)
        st = o.new_state(online, target, critic_rmsprop=cfg.get("RMSPROP", True))
        for i in range(2):
            b = batch if i == 0 else _select(st, _candidates(S, A, 2 * B, rng), B, noise, **_cfg_kw(cfg))
            out = o.train_step(st, *_f64(b), LR, noise.astype(np.float64), **_cfg_kw(cfg))
            q_max, q_avg = net.train(b[0], b[2], b[1], b[4], b[3], noise=noise)
            _check("step %d q_max" % i, [q_max], [out["q_max"]])
            _check("step %d q_avg" % i, [q_avg], [out["q_avg"]])
            if i == 0:
                for k in o.TRAINABLE:          # targets after step 0: the one-soft-update rule on the loaded targets
                    want = 0.001 * st["online"][k] + 0.999 * target[k]
                    _check("target rule " + k, net.get_variable_value(k, 1), want, WTOL)
        assert net.get_global_step() == 2
        for k in o.TRAINABLE:
            _check("online " + k, net.get_variable_value(k, 0), st["online"][k], WTOL)
            _check("target " + k, net.get_variable_value(k, 1), st["target"][k], WTOL)
            _check("slot a " + k, net.get_variable_value(k, 2), st["slot_a"][k], WTOL)
            _check("slot b " + k, net.get_variable_value(k, 3), st["slot_b"][k], WTOL)
        dead = net.get_variable_value(o.DEAD, 0)
        assert np.array_equal(dead, online[o.DEAD].astype(np.float32)), "critic_fc2/b moved"
    finally:
        net.close()


def _snapshot(net):
    return {(k, w): net.get_variable_value(k, w) for k in o.TRAINABLE for w in (0, 1, 2, 3)}


def _same(a, b):
    return all(np.array_equal(a[k], b[k]) for k in a)


def test_train_replay_is_train_on_the_same_rows_and_the_same_call_gives_the_same_bits():
    S, A, B = 3, 1, 64
    online, target, batch = _case(S, A, 128, 11)
    s, a, r, done, s2 = batch
    rng = np.random.default_rng(3)
    slots = rng.choice(128, B, replace=False).astype(np.int32)
    snaps = []
    for how in ("replay", "train", "replay"):
        net = _net(S, A)
        try:
            _load(net, online, target)
            size, total = net.replay_add(s, a, r, done, s2)
            assert (size, total) == (128, 128)
            for step in range(2):
                if how == "replay":
                    net.train_replay(slots, stamp=total, noise=[0.1])
                else:
                    rows = [net.replay_get(i) for i in slots]
                    cols = [np.stack([row[c] for row in rows]) for c in range(5)]
                    net.train(cols[0], cols[2], cols[1], cols[4], cols[3], noise=[0.1])
            snaps.append(_snapshot(net))
        finally:
            net.close()
    assert _same(snaps[0], snaps[1]), "train_replay differs from train on the rows replay_get returns"
    assert _same(snaps[0], snaps[2]), "the same calls on a fresh handle gave other bits"


def test_ring_wraps_and_evicts_like_a_deque_and_refuses_overwritten_slots():
    import _native as nat
    S, A, cap = 3, 2, 50
    net = _net(S, A, max_batch=64, capacity=cap)
    try:
        rng = np.random.default_rng(0)
        dq, ring = collections.deque(), o.Ring(cap)
        for n in (7, 30, 13, 20, 50, 1):
            rows = [rng.normal(size=(n, S)).astype(np.float32), rng.normal(size=(n, A)).astype(np.float32),
                    rng.normal(size=n).astype(np.float32), (rng.uniform(size=n) < 0.3).astype(np.float32),
                    rng.normal(size=(n, S)).astype(np.float32)]
            size, total = net.replay_add(*rows)
            ring.add(n)
            for i in range(n):
                if len(dq) == cap:
                    dq.popleft()
                dq.append(tuple(t[i] for t in rows))
            assert (size, total) == (len(dq), ring.total) == (ring.size, ring.total)
            for j in (0, len(dq) // 2, len(dq) - 1):
                got = net.replay_get(ring.slot(j))
                assert all(np.array_equal(g, w) for g, w in zip(got, dq[j])), "position %d" % j
        # sampled before the last add of one row (which overwrote the oldest slot): that slot is stale, the others are not
        stamp, stale = ring.total - 1, (ring.total - 1) % cap
        fresh = np.array([s for s in range(cap) if s != stale][:16], np.int32)
        net.train_replay(fresh, stamp=stamp, noise=False)
        before = _snapshot(net)
        with pytest.raises(nat.StateLost):
            net.train_replay(np.array([stale] + list(fresh[:15]), np.int32), stamp=stamp, noise=False)
        assert _same(before, _snapshot(net)) and net.get_global_step() == 1
        with pytest.raises(RuntimeError):
            net.train_replay(np.array([cap], np.int32), noise=False)
    finally:
        net.close()


def test_replay_add_gather_equals_replay_add():
    """Rows `s | s2 | done | padding` read straight out of a registered host segment."""
    S, A, n = 3, 1, 40
    row_bytes = (8 * S + 4 + 15) // 16 * 16
    seg = np.zeros((64, row_bytes // 4), np.float32)                # plain host memory: register_host pins it
    rng = np.random.default_rng(5)
    s, s2 = rng.normal(size=(n, S)).astype(np.float32), rng.normal(size=(n, S)).astype(np.float32)
    a, r = rng.uniform(-1, 1, (n, A)).astype(np.float32), rng.normal(size=n).astype(np.float32)
    done = (rng.uniform(size=n) < 0.3).astype(np.float32)
    seg[:] = 0
    seg[:n, :S], seg[:n, S:2 * S], seg[:n, 2 * S] = s, s2, done
    nets = [_net(S, A, max_batch=64, capacity=32) for _ in range(2)]
    try:
        class Seg:
            base, nbytes = seg.ctypes.data, seg.nbytes
        nets[0].register_transport(Seg)
        offsets = np.arange(n, dtype=np.int64) * row_bytes
        for lo, hi in ((0, 24), (24, 40)):                            # the second call wraps round the ring's end
            got = nets[0].replay_add_offsets(offsets[lo:hi], r[lo:hi], a[lo:hi])
            assert got == nets[1].replay_add(s[lo:hi], a[lo:hi], r[lo:hi], done[lo:hi], s2[lo:hi]) == (min(hi, 32), hi)
        for slot in range(32):
            assert all(np.array_equal(g, w) for g, w in zip(nets[0].replay_get(slot), nets[1].replay_get(slot)))
        with pytest.raises(RuntimeError):
            nets[0].replay_add_offsets(np.array([seg.nbytes - 8], np.int64), r[:1], a[:1])
        nets[0].unregister_transport()
    finally:
        for net in nets:
            net.close()


def test_ou_process_of_the_handle():
    S, A = 3, 2
    net, twin = _net(S, A), _net(S, A)
    try:
        x = np.zeros(A)
        draws = []
        for i in range(100000 // A):
            xn, n = net.noise_step()
            want = o.ou_step(x, n.astype(np.float64))
            assert np.max(np.abs(xn - want)) <= 2.0 ** -23 * max(1.0, np.max(np.abs(want))), "recurrence at step %d" % i
            x = xn.astype(np.float64)
            draws.append(n)
            if i < 1000:
                assert np.array_equal(twin.noise_step()[1], n), "same seed, other stream"
        draws = np.concatenate(draws).astype(np.float64)
        print("normal draws: mean %.5f variance %.5f" % (draws.mean(), draws.var()))
        assert abs(draws.mean()) <= 0.02 and abs(draws.var() - 1.0) <= 0.02
        # one step per predict call whatever the batch: predict (own noise) - predict (none) is the state after one step
        xs = np.random.default_rng(1).uniform(-1, 1, (37, S)).astype(np.float32)
        twin2 = _net(S, A)
        try:
            for _ in range(100000 // A):
                twin2.noise_step()
            for rows in (1, 37):
                noisy, clean = net.predict(xs[:rows]), net.predict(xs[:rows], noise=False)
                step, _ = twin2.noise_step()
                assert np.max(np.abs((noisy - clean) - step[None, :])) <= 1e-6
        finally:
            twin2.close()
        given = net.predict(xs, noise=[0.5, -0.25]) - net.predict(xs, noise=False)
        assert np.max(np.abs(given - np.array([0.5, -0.25]))) <= 1e-6
    finally:
        net.close()
        twin.close()
    quiet = _net(S, A, add_OUnoise=False)
    try:
        a = quiet.predict(xs)
        assert np.array_equal(a, quiet.predict(xs, noise=False)) and np.max(np.abs(a)) <= 1.0
        far = quiet.predict(xs, noise=[0.0, 0.0])
        assert np.array_equal(far, a)
    finally:
        quiet.close()
    assert np.allclose(o.wrap([1.5, -1.5, 0.3, 3.25]), [-0.5, 0.5, 0.3, -0.75])


def test_predict_matches_the_oracle_and_sees_whole_steps():
    """Predictions issued from another thread while steps run equal the actor before some whole number of steps."""
    import threading
    S, A, B = 3, 1, 64
    online, target, batch = _case(S, A, B, 41)
    xs = batch[0]
    net = _net(S, A)
    try:
        _load(net, online, target)
        _check("predict", net.predict(xs, noise=False), o.actor_forward(online, xs)["out"])
        steps, seen, stop = 6, [], threading.Event()

        def predictor():
            while not stop.is_set():
                seen.append(net.predict(xs, noise=False))

        th = threading.Thread(target=predictor)
        th.start()
        for _ in range(steps):
            net.train(batch[0], batch[2], batch[1], batch[4], batch[3], noise=False)
        stop.set()
        th.join()
    finally:
        net.close()
    ref = _net(S, A)
    try:
        _load(ref, online, target)
        whole = [ref.predict(xs, noise=False)]
        for _ in range(steps):
            ref.train(batch[0], batch[2], batch[1], batch[4], batch[3], noise=False)
            whole.append(ref.predict(xs, noise=False))
    finally:
        ref.close()
    assert seen and all(any(np.array_equal(p, w) for w in whole) for p in seen), "a prediction saw a mix of weights"


def test_checkpoint_round_trip_refusals_and_resume(tmp_path):
    S, A, B = 3, 1, 32
    online, target, batch = _case(S, A, B, 51)
    args = (batch[0], batch[2], batch[1], batch[4], batch[3])
    path, path3 = str(tmp_path / "ddpg.npz"), str(tmp_path / "ddpg3.npz")
    net = _net(S, A)
    try:
        _load(net, online, target)
        net.train(*args, noise=False)
        net.train(*args, noise=False)
        net._lib.ga3c_ddpg_save(net._h, path.encode())
        two = _snapshot(net)
        net.train(*args, noise=False)
        three = _snapshot(net)
        with np.load(path) as z:
            assert int(z["step"]) == 2
            names = set(z.files)
            for k, t in zip(net.get_variables_names(), net.get_target_names()):
                assert k in names and t in names
                assert np.array_equal(z[k], net.get_variable_value(k, 0)) or k[:-2] in o.TRAINABLE
            assert "actor_fc1_1/W:0" in names and "actor_fc1/W/Adam_1:0" in names and "critic_fc1/W/RMSProp:0" in names
            assert "actor_norm1/moving_variance:0" in names and "critic_norm1_1/moving_mean:0" in names
            assert np.array_equal(z["critic_fc2/W:0"], two[("critic_fc2/W", 0)])
            np.savez(path3, **{k: z[k] for k in z.files})            # through numpy and back
    finally:
        net.close()
    fresh = _net(S, A)
    try:
        fresh.load_file(path3)
        assert fresh.get_global_step() == 2 and _same(two, _snapshot(fresh))
        fresh.train(*args, noise=False)                              # Adam's bias correction continues at t = 3
        assert _same(three, _snapshot(fresh))
        # cross-refusals, networks untouched
        import ga3c_amd  # noqa: F401
        from NetworkVP_vector import Network as Vec
        vec = Vec("gpu:0", "vec", A, (S,), max_batch=16)
        try:
            vpath = str(tmp_path / "vec.npz")
            vec._lib.ga3c_mlp_save(vec._h, vpath.encode())
            before = _snapshot(fresh)
            with pytest.raises(RuntimeError):
                fresh.load_file(vpath)
            assert _same(before, _snapshot(fresh)) and fresh.get_global_step() == 3
            arena = vec.get_arena(0)
            assert vec._lib.ga3c_mlp_load(vec._h, path.encode()) == -4
            assert np.array_equal(arena, vec.get_arena(0))
        finally:
            vec.close()
    finally:
        fresh.close()


@pytest.mark.timeout(120)
def test_server_drives_ddpg_with_the_native_loops_and_the_replay_thread(tmp_path, monkeypatch):
    import ga3c_amd  # noqa: F401
    from Config import Config
    monkeypatch.chdir(tmp_path)
    for k, v in (("GAME", "Pendulum-v0"), ("USE_DDPG", True), ("AGENTS", 8), ("PREDICTORS", 2), ("TRAINERS", 2), ("TIME_MAX", 5),
                 ("DYNAMIC_SETTINGS", False), ("SAVE_MODELS", False), ("TRAINING_MIN_BATCH_SIZE", 64),
                 ("REPLAY_BUFFER_SIZE", 2000), ("CONTINUOUS_INPUT", Config.CONTINUOUS_INPUT),
                 ("DISCRATE_INPUT", Config.DISCRATE_INPUT), ("DISCOUNTING", Config.DISCOUNTING),
                 ("USE_REPLAY_MEMORY", Config.USE_REPLAY_MEMORY)):
        monkeypatch.setattr(Config, k, v)
    from Server import Server
    import NetworkDDPG
    srv = Server(max_agents=16)
    assert isinstance(srv.model, NetworkDDPG.Network) and srv.zero_copy and not srv.state_cache and srv.ddpg
    assert srv.transport.row_bytes == 32
    srv.main(max_seconds=8)
    assert srv.failure is None and srv.training_step > 20 and srv.predictions_served > 1000
    assert srv.model.get_global_step() == srv.training_step
    size, total = srv.model.replay_size()
    # the small ring wrapped many times; whatever was refused as overwritten was dropped and counted, not trained
    assert size == 2000 and total > 2000 and srv.stats.replay_memory_size.value == 2000
    assert open("results.txt").read().strip()
    # a row of the ring as the agents shipped it: Pendulum's state (cos, sin, velocity), a raw reward, a 0 / 1 flag
    s, a, r, done, s2 = srv.model.replay_get(17)
    assert abs(float(s[0]) ** 2 + float(s[1]) ** 2 - 1.0) < 1e-3 and abs(float(s2[0]) ** 2 + float(s2[1]) ** 2 - 1.0) < 1e-3
    assert -1.1 <= float(r) <= -1.0 + 1e-6 and float(done) in (0.0, 1.0) and abs(float(a[0])) < 3.0
    srv.model.close()


@pytest.mark.timeout(300)
def test_train_sh_runs_ddpg_on_pendulum(tmp_path):
    """sh _train.sh GAME=Pendulum-v0 USE_DDPG=True TRAINING_MIN_BATCH_SIZE=64 MAX_SECONDS=20: trains, logs episodes, the replay
    memory grows, a checkpoint appears and reloads."""
    env = dict(os.environ, PYTHONPATH=ROOT)
    cmd = ["sh", os.path.join(PKG, "_train.sh"), "GAME=Pendulum-v0", "USE_DDPG=True", "TRAINING_MIN_BATCH_SIZE=64",
           "MAX_SECONDS=20", "AGENTS=8", "PREDICTORS=1", "TRAINERS=1", "DYNAMIC_SETTINGS=", "SAVE_FREQUENCY=5",
           "REPLAY_BUFFER_SIZE=100000", "TENSORBOARD=True", "TENSORBOARD_UPDATE_FREQUENCY=50"]
    run = subprocess.run(cmd, cwd=str(tmp_path), env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=240)
    text = run.stdout.decode(errors="replace")
    sys.stdout.write(text[-3000:])
    assert run.returncode == 0
    lines = open(str(tmp_path / "results.txt")).read().splitlines()
    assert len(lines) >= 5, "fewer than five episodes logged"
    scalars = np.loadtxt(str(tmp_path / "logs" / "network" / "scalars.csv"), delimiter=",", ndmin=2)
    assert scalars.shape[1] == 4 and scalars[-1, 0] > scalars[0, 0] and np.all(np.isfinite(scalars))
    sizes = [int(t.split("[RSize:")[1].split("]")[0]) for t in text.splitlines() if "[RSize:" in t]     # the status line
    assert sizes and sizes[-1] > 64
    found = sorted(os.listdir(str(tmp_path / "checkpoints")))
    assert found
    import ga3c_amd  # noqa: F401
    net = _net(3, 1)
    try:
        net.load_file(str(tmp_path / "checkpoints" / found[-1]))
        assert net.get_global_step() > 0
    finally:
        net.close()
