"""-m gpu: the discrete-action vector-state network of GAME = 'CartPole-v0' (ga3c_dmlp_*) against its f64
statement (tests/dmlp_oracle.py), in both wirings and both softmax branches.  Tolerance: 1e-4 x max(1, max|want|), the
project's rule, and every delta and gradient once more through tests/closeness.py.  The variables nothing reads
(DENSE_STACK = 'fork', layers 1..L-1) are held to exact zeros and unchanged bits, not to a tolerance."""
import contextlib
import glob
import os
import re
import subprocess

import numpy as np
import pytest

import dmlp_oracle as m

pytestmark = pytest.mark.gpu

TOL = 1e-4
SIZES = [1, 15, 16, 17, 128, 132, 201, 1024]
# (S, A, layers, wiring)
SHAPES = [(4, 2, (10, 10, 10, 10), "fork"), (4, 2, (10, 10, 10, 10), "chained"), (7, 5, (32, 16), "chained"),
          (3, 1, (10,), "fork")]
SHAPE_IDS = ["fork4x10", "chained4x10", "chained32_16", "one_action"]
# the backward pass shares a row of W among P = 1, 1, 2, 64 and 256 threads at these widths (the shapes above reach 8 and 16)
SPLIT_EDGES = (64, 32, (256, 129, 128, 3, 1), "chained")
# all eight layers ga3c_dmlp_create admits (GA3C_DMLP_MAX_LAYERS) at the largest S and A, in both wirings: chained, every layer
# is live; fork, only layer 8 is and 14 variables are dead.  256, 129 and small odd widths, a width of 1 in last place only (as
# above); no compared tensor of the oracle is all zero (through eight sigmoid layers dh1 is down to 4e-7 .. 7e-7, which the
# relative test holds to its own largest entry).  These two run at EIGHT_SIZES.
EIGHT_WIDTHS = (256, 129, 7, 33, 5, 128, 3, 1)
EIGHT = [(64, 32, EIGHT_WIDTHS, "chained"), (64, 32, EIGHT_WIDTHS, "fork")]
EIGHT_IDS = ["chained8", "fork8"]
EIGHT_SIZES = [1, 17, 132]
HEADS = {"plain": dict(use_log_softmax=False, min_policy=0.0), "log_softmax": dict(use_log_softmax=True, min_policy=0.0),
         "min_policy": dict(use_log_softmax=False, min_policy=0.01)}
PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ga3c_amd")


def _close(got, want, tol=TOL):
    got, want = np.asarray(got, np.float64).reshape(-1), np.asarray(want, np.float64).reshape(-1)
    return np.max(np.abs(got - want)) <= tol * max(1.0, np.max(np.abs(want)))


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


def _net(state_dim, num_actions, layers, stack, max_batch=1024, head=None, **kw):
    import ga3c_amd  # noqa: F401  (puts the flat modules on sys.path)
    from NetworkVP_discrate import Network
    head = head or HEADS["plain"]
    with _config(DENSE_LAYERS=tuple(layers), DENSE_STACK=stack, USE_LOG_SOFTMAX=head["use_log_softmax"],
                 MIN_POLICY=head["min_policy"], DUAL_RMSPROP=False, **kw):
        return Network("gpu:0", "dvec", num_actions, (state_dim,), max_batch=max_batch)


def _params(state_dim, num_actions, layers, stack):
    p = m.init_params(state_dim, num_actions, layers, stack, seed=777)
    p["logits_p/w"] = (p["logits_p/w"] * 4.0).astype(np.float32).astype(np.float64)      # a policy that is not nearly uniform
    return p


def _batch(bsz, state_dim, num_actions, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    x = rng.uniform(-1.5, 1.5, size=(bsz, state_dim)).astype(np.float32)
    a = np.eye(num_actions, dtype=np.float32)[rng.integers(0, num_actions, bsz)]
    y = rng.uniform(-1, 1, size=bsz).astype(np.float32)
    return x, y, a


def _reset(net, params):
    net.set_arena(0, m.flat(params))
    net.set_arena(1, np.ones(net.param_count, np.float32))
    net.set_arena(2, np.zeros(net.param_count, np.float32))


def _sizes(shape):
    return EIGHT_SIZES if shape in EIGHT else SIZES


def _live_layers(layers, stack):
    return list(range(1, len(layers) + 1)) if stack == "chained" else [len(layers)]


def _var(net, flat, name):
    off, size = net._offsets[name]
    return flat[off:off + size]


def _f64(*arrays):
    return [np.asarray(t, np.float64) for t in arrays]


@pytest.mark.parametrize("head", list(HEADS))
@pytest.mark.parametrize("shape", SHAPES + [SPLIT_EDGES] + EIGHT, ids=SHAPE_IDS + ["split_edges"] + EIGHT_IDS)
def test_forward_losses_and_gradients_against_the_oracle(shape, head):
    S, A, layers, stack = shape
    kw = HEADS[head]
    params = _params(S, A, layers, stack)
    net = _net(S, A, layers, stack, head=kw)
    try:
        _reset(net, params)
        assert net.param_count == m.param_count(S, A, layers, stack)
        assert [n[:-2] for n in net.get_variables_names()] == list(m.param_order(layers))
        for bsz in _sizes(shape):
            x, y, a = _batch(bsz, S, A, 100 + bsz)
            x64, y64, a64 = _f64(x, y, a)
            f = m.forward(params, x64, stack, **kw)
            p, v, z = net.predict_p_v_logits(x)
            assert _close(p, f["p"]) and _close(v, f["v"]) and _close(z, f["z"]), bsz
            assert np.all(np.abs(p.sum(axis=1) - 1.0) < 1e-5)
            net.beta = 0.01
            losses = net.compute_grads(x, y, a)
            want, g = m.loss_and_grads(params, x64, y64, a64, 0.01, stack=stack, **kw)
            for got, key in zip(losses, ("cost_p_1_agg", "cost_p_2_agg", "cost_v")):
                assert abs(got - want[key]) <= TOL * max(1.0, abs(want[key])), (bsz, key, got, want[key])
            acts = [("x", S, f["x"]), ("v", 1, f["v"]), ("p", A, f["p"]), ("z", A, f["z"]), ("dv", 1, g["dv"]), ("dz", A, g["dz"])]
            for i in _live_layers(layers, stack):
                acts += [("h%d" % i, layers[i - 1], f["h%d" % i]), ("dh%d" % i, layers[i - 1], g["dh%d" % i])]
            for name, width, ref in acts:
                assert _close(net.fetch(name, bsz * width), ref), (bsz, name)
            grad = net.get_arena(3)
            for k in m.param_order(layers):
                if k in net.dead:
                    assert not np.any(_var(net, grad, k)) and not np.any(g[k]), (bsz, k)      # exactly zero, no tolerance
                else:
                    assert _close(_var(net, grad, k), g[k]), (bsz, k)
            if A == 1:                                                                           # the softmax over one action is 1
                assert np.all(p == 1.0) and not np.any(net.fetch("dz", bsz)) and not np.any(_var(net, grad, "logits_p/w"))
        assert set(net.dead) == set(m.dead_params(layers, stack))
        if net.dead:
            with pytest.raises(RuntimeError):
                net.fetch("h1", _sizes(shape)[-1] * layers[0])              # a layer nothing reads has no rows
    finally:
        net.close()


@pytest.mark.parametrize("head", list(HEADS))
@pytest.mark.parametrize("shape", SHAPES + EIGHT, ids=SHAPE_IDS + EIGHT_IDS)
def test_backward_tensors_relative_to_their_largest_entry(shape, head):
    """Every delta and gradient once more with tests/closeness.py: max|got - want| / max|want| against max(16 x e32, 2^-20),
    e32 from the oracle run in float32 on the same rows.  A bias gradient of ONE element (logits_v/b) takes the larger of that
    single draw and what the float32 error of the delta it sums implies (closeness.e32_of_row_sum, where the reason is
    written), as the vector net's test does.  At A = 1 the softmax is 1: dz, logits_p/w and logits_p/b are exactly zero and are
    asserted zero (rel_err refuses an all-zero tensor), as are the variables nothing reads."""
    import closeness as c
    S, A, layers, stack = shape
    kw = HEADS[head]
    params = _params(S, A, layers, stack)
    p32 = {k: v.astype(np.float32) for k, v in params.items()}
    net = _net(S, A, layers, stack, head=kw)
    try:
        _reset(net, params)
        net.beta = 0.01
        failed = []
        for bsz in _sizes(shape):
            x, y, a = _batch(bsz, S, A, 100 + bsz)
            net.compute_grads(x, y, a)
            _, g = m.loss_and_grads(params, *_f64(x, y, a), 0.01, stack=stack, **kw)
            _, g32 = m.loss_and_grads(p32, x, y, a, 0.01, stack=stack, **kw)
            grad = net.get_arena(3)
            got = {"dv": net.fetch("dv", bsz), "dz": net.fetch("dz", bsz * A)}
            for i in _live_layers(layers, stack):
                got["dh%d" % i] = net.fetch("dh%d" % i, bsz * layers[i - 1])
            got.update({k: _var(net, grad, k) for k in m.param_order(layers)})
            zero = set(net.dead) | ({"dz", "logits_p/w", "logits_p/b"} if A == 1 else set())
            for name in got:
                assert np.asarray(g32[name]).dtype == np.float32, name
                if name in zero:
                    assert not np.any(got[name]) and not np.any(g[name]) and not np.any(g32[name]), (bsz, name)
                    continue
                e32 = c.rel_err(g32[name], g[name])
                if name == "logits_v/b":
                    e32 = max(e32, c.e32_of_row_sum(g32["dv"], g["dv"]))
                shape_id = (SHAPE_IDS + EIGHT_IDS)[(SHAPES + EIGHT).index(shape)]
                err = c.report("dmlp %s %s B=%d" % (shape_id, head, bsz), name, got[name], g[name], e32, c.bound(e32))
                if not err <= c.bound(e32):
                    failed.append((bsz, name, err, c.bound(e32)))
        assert not failed, failed
    finally:
        net.close()


@pytest.mark.parametrize("kind", ["plain", "clip", "momentum"])
@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[2]], ids=[SHAPE_IDS[0], SHAPE_IDS[2]])
def test_two_train_steps_against_the_oracle(shape, kind):
    S, A, layers, stack = shape
    clip = 2e-4 if kind == "clip" else None             # a norm that bites: ||g|| / n is far above it for every variable
    momentum = 0.9 if kind == "momentum" else 0.0
    params = _params(S, A, layers, stack)
    net = _net(S, A, layers, stack, USE_GRAD_CLIP=kind == "clip", GRAD_CLIP_NORM=clip or 40.0, RMSPROP_MOMENTUM=momentum)
    try:
        rng = np.random.default_rng(3)
        ms0 = rng.uniform(0.5, 1.5, net.param_count).astype(np.float32)
        mom0 = rng.uniform(-1e-3, 1e-3, net.param_count).astype(np.float32)
        theta0 = m.flat(params).astype(np.float32)
        net.set_arena(0, theta0)
        net.set_arena(1, ms0)
        net.set_arena(2, mom0)
        net.learning_rate, net.beta = 1e-3, 0.01
        ref = {k: v.copy() for k, v in params.items()}
        ms = {k: _var(net, ms0, k).astype(np.float64).reshape(params[k].shape) for k in params}
        mom = {k: _var(net, mom0, k).astype(np.float64).reshape(params[k].shape) for k in params}
        for step, bsz in enumerate((132, 201)):
            x, y, a = _batch(bsz, S, A, 7 + step)
            net.train(x, y, a)
            _, g = m.train_step(ref, ms, mom, *_f64(x, y, a), 1e-3, 0.01, stack=stack, momentum=momentum, clip=clip)
            if kind == "clip":
                live = [k for k in m.param_order(layers) if k not in net.dead]
                assert all(np.sqrt(np.sum(g[k] ** 2)) / g[k].size > clip for k in live)
        assert net.get_global_step() == 2
        theta, ms_got, mom_got = net.get_arena(0), net.get_arena(1), net.get_arena(2)
        assert _close(theta, m.flat(ref), 1e-5)
        assert _close(ms_got, m.flat(ms), 1e-5)
        if kind == "momentum":
            assert _close(mom_got, m.flat(mom), 1e-5)
        else:
            assert np.array_equal(mom_got, mom0)                     # momentum 0 never touches the slot
        assert not np.array_equal(theta, theta0)
        for k in net.dead:                                           # skipped, not stepped with zero: every bit as it was
            assert np.array_equal(_var(net, theta, k), _var(net, theta0, k)), k
            assert np.array_equal(_var(net, ms_got, k), _var(net, ms0, k)), k
            assert np.array_equal(_var(net, mom_got, k), _var(net, mom0, k)), k
        assert (len(net.dead) == 6) == (stack == "fork")
    finally:
        net.close()


@pytest.mark.parametrize("clip", [False, True])
@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[2]], ids=[SHAPE_IDS[0], SHAPE_IDS[2]])
def test_split_step_and_repeated_calls_are_bit_identical(shape, clip):
    S, A, layers, stack = shape
    params = _params(S, A, layers, stack)
    kw = {"USE_GRAD_CLIP": clip, "GRAD_CLIP_NORM": 2e-4}
    a_net, b_net = _net(S, A, layers, stack, **kw), _net(S, A, layers, stack, **kw)
    try:
        x, y, a = _batch(201, S, A, 99)
        for n in (a_net, b_net):
            _reset(n, params)
            n.learning_rate, n.beta = 1e-3, 0.01
        g1 = (b_net.compute_grads(x, y, a), b_net.get_arena(3))
        g2 = (b_net.compute_grads(x, y, a), b_net.get_arena(3))
        assert np.array_equal(g1[0], g2[0]) and np.array_equal(g1[1], g2[1])      # no float atomics anywhere
        b_net.apply_grads()
        a_net.train(x, y, a)
        for w in (0, 1, 2, 3):
            assert np.array_equal(a_net.get_arena(w), b_net.get_arena(w)), w
        assert a_net.get_global_step() == b_net.get_global_step() == 1
        for k in a_net.dead:
            assert np.array_equal(_var(a_net, a_net.get_arena(1), k), np.ones(a_net._offsets[k][1], np.float32))
    finally:
        a_net.close()
        b_net.close()


def test_gather_entries_are_bit_equal_to_host_buffers():
    """Rows read out of the registered transport -- agent slots, and rollout rows of 28 bytes (S = 7) that are 4-byte and not
    16-byte aligned -- give the bits the host-buffer entry points give."""
    import ga3c_amd  # noqa: F401
    import Transport as tp
    S, A, layers, stack = SHAPES[2]
    params = _params(S, A, layers, stack)
    t = tp.Transport.create(tp.unique_name("t_dvec"), 40, A, 4 * S, 8, 40)
    n1, n2 = _net(S, A, layers, stack), _net(S, A, layers, stack)
    try:
        for n in (n1, n2):
            _reset(n, params)
            n.learning_rate, n.beta = 1e-3, 0.01
        x, y, a = _batch(37, S, A, 5)
        ids = np.arange(37, dtype=np.uint32)[::-1].copy()
        for i, agent in enumerate(ids):
            t.state_view(int(agent), np.float32)[:] = x[i]
        n1.register_transport(t)
        p1, v1 = n1.predict_offsets(t.state_offsets(ids))
        p2, v2 = n2.predict_p_and_v(x)
        assert np.array_equal(p1, p2) and np.array_equal(v1, v2)
        slot = t.acquire(1000)
        states, returns, actions = t.rollout_views(slot)
        for i in range(37):
            states[i] = x[i].view(np.uint8)
        t.commit(slot, 37)
        got = t.pop_rollout(1000)
        offs = t.rollout_row_offsets(got, 37)
        assert np.all(offs % 4 == 0) and np.any(offs % 16 != 0)
        loss1 = n1.evaluate(None, y, a, offsets=offs)
        loss2 = n2.evaluate(x, y, a)
        assert all(np.array_equal(u, w) for u, w in zip(loss1, loss2))
        n1.train_offsets(offs, y, a)
        n2.train(x, y, a)
        assert np.array_equal(n1.last_losses, n2.last_losses)
        assert np.array_equal(n1.get_arena(0), n2.get_arena(0))
        t.release(got)
        # the pipelined halves through their C entry points, two in flight at once
        import ctypes as C
        import _native as nat
        lib = n1._lib
        tk = [C.c_int32(-1), C.c_int32(-1)]
        o1 = np.ascontiguousarray(t.state_offsets(ids[:20]))
        o2 = np.ascontiguousarray(t.state_offsets(ids[20:]))
        nat.check(lib.ga3c_dmlp_predict_gather_begin(n1._h, nat.ptr(o1, nat.i64p), 20, 0, C.byref(tk[0])))
        nat.check(lib.ga3c_dmlp_predict_gather_begin(n1._h, nat.ptr(o2, nat.i64p), 17, 0, C.byref(tk[1])))
        pb, vb = np.empty((17, A), np.float32), np.empty(17, np.float32)
        pa, va = np.empty((20, A), np.float32), np.empty(20, np.float32)
        nat.check(lib.ga3c_dmlp_predict_gather_end(n1._h, tk[1], 17, nat.ptr(pb), nat.ptr(vb)))
        nat.check(lib.ga3c_dmlp_predict_gather_end(n1._h, tk[0], 20, nat.ptr(pa), nat.ptr(va)))
        p3, v3 = n1.predict_p_and_v(x)
        assert np.array_equal(np.concatenate([pa, pb]), p3) and np.array_equal(np.concatenate([va, vb]), v3)
        assert lib.ga3c_dmlp_predict_gather_end(n1._h, tk[0], 20, nat.ptr(pa), nat.ptr(va)) == -4    # nothing begun: ESTATE
        for bad in (t.nbytes - 8, 2, -4):
            with pytest.raises(RuntimeError):
                n1.predict_offsets(np.array([bad], np.int64))         # past the segment, misaligned, before it
        before = n1.get_arena(0)
        with pytest.raises(RuntimeError):
            n1.train_offsets(np.array([t.nbytes - 8], np.int64), y[:1], a[:1])
        assert np.array_equal(n1.get_arena(0), before)
        n1.unregister_transport()
    finally:
        n1.close()
        n2.close()
        t.shutdown()
        t.close()


def test_create_refuses_what_the_handle_does_not_do():
    import ctypes as C
    import ga3c_amd  # noqa: F401
    import _native as nat
    lib = nat.hip_lib()

    def rc(**kw):
        cfg = nat.DmlpConfig()
        cfg.device, cfg.state_dim, cfg.num_actions, cfg.max_batch, cfg.num_layers, cfg.chained = 0, 4, 2, 16, 2, 0
        cfg.widths[0] = cfg.widths[1] = 10
        cfg.rmsprop_decay, cfg.rmsprop_epsilon, cfg.log_epsilon = 0.99, 0.1, 1e-6
        for k, v in kw.items():
            if k == "widths":
                for i, w in enumerate(v):
                    cfg.widths[i] = w
            else:
                setattr(cfg, k, v)
        h = C.c_void_p()
        r = lib.ga3c_dmlp_create(C.byref(cfg), C.byref(h))
        if r == 0:
            lib.ga3c_dmlp_destroy(h)
        return r

    assert rc() == 0 and rc(flags=nat.FLAG_LOG_SOFTMAX | nat.FLAG_GRAD_CLIP) == 0 and rc(chained=1) == 0
    for bad in (dict(flags=nat.FLAG_CONTINUOUS), dict(flags=nat.FLAG_DUAL_RMSPROP), dict(flags=64), dict(state_dim=0),
                dict(state_dim=65), dict(num_actions=0), dict(num_actions=33), dict(num_layers=0), dict(num_layers=9),
                dict(widths=(10, 0)), dict(widths=(257, 10)), dict(chained=2), dict(max_batch=0)):
        assert rc(**bad) == -1, bad                                   # GA3C_EINVAL


def test_checkpoint_round_trip_and_refusals(tmp_path):
    import ga3c_amd  # noqa: F401
    from NetworkVP import Network as ImageNet
    from NetworkVP_vector import Network as VectorNet
    S, A, layers, stack = SHAPES[0]
    params = _params(S, A, layers, stack)
    net, other = _net(S, A, layers, stack), _net(S, A, layers, stack)
    img = vec = None
    others = []
    try:
        _reset(net, params)
        net.learning_rate, net.beta = 1e-3, 0.01
        x, y, a = _batch(40, S, A, 3)
        net.train(x, y, a)
        path = str(tmp_path / "dvec.npz")
        assert net._lib.ga3c_dmlp_save(net._h, path.encode()) == 0
        z = np.load(path)
        assert int(z["step"]) == 1 and z["dense1_2_p/w:0"].shape == (4, 10) and z["logits_p/w:0"].shape == (10, 2)
        assert sorted(z.files) == sorted(["step"] + [k + s for k in m.param_order(layers)
                                                     for s in (":0", "/RMSProp:0", "/RMSProp_1:0")])
        assert np.array_equal(z["dense1_1_p/w:0"].ravel(), _var(net, net.get_arena(0), "dense1_1_p/w"))      # dead ones are saved
        assert other._lib.ga3c_dmlp_load(other._h, path.encode()) == 0
        for w in (0, 1, 2):
            assert np.array_equal(other.get_arena(w), net.get_arena(w))
        assert other.get_global_step() == 1
        # the other two kinds of network, both ways
        with _config(CONTINUOUS_INPUT=False):
            img = ImageNet("gpu:0", "img", 2, (84, 84, 4), max_batch=8, predict_lanes=1)
        vec = VectorNet("gpu:0", "vec", 1, (3,), max_batch=8)
        ipath, vpath = str(tmp_path / "img.npz"), str(tmp_path / "vec.npz")
        assert img._lib.ga3c_net_save(img._h, ipath.encode()) == 0
        assert vec._lib.ga3c_mlp_save(vec._h, vpath.encode()) == 0
        before = [other.get_arena(w) for w in (0, 1, 2)]
        for foreign in (ipath, vpath):
            assert other._lib.ga3c_dmlp_load(other._h, foreign.encode()) == -4
        ibefore, vbefore = img.get_arena(0), vec.get_arena(0)
        assert img._lib.ga3c_net_load(img._h, path.encode()) == -4
        assert vec._lib.ga3c_mlp_load(vec._h, path.encode()) == -4
        assert np.array_equal(img.get_arena(0), ibefore) and np.array_equal(vec.get_arena(0), vbefore)
        # this kind with another layer count, other widths, the other wiring, another A, another S
        for s2, a2, l2, st2 in ((S, A, (10, 10, 10), stack), (S, A, (10,) * 5, stack), (S, A, (10, 10, 10, 12), stack),
                                (S, A, layers, "chained"), (S, 3, layers, stack), (5, A, layers, stack)):
            n = _net(s2, a2, l2, st2, max_batch=8)
            others.append(n)
            was = n.get_arena(0)
            assert n._lib.ga3c_dmlp_load(n._h, path.encode()) == -4, (s2, a2, l2, st2)
            assert np.array_equal(n.get_arena(0), was) and n.get_global_step() == 0
        assert all(np.array_equal(other.get_arena(w), before[w]) for w in (0, 1, 2)) and other.get_global_step() == 1
        # two wirings whose shapes coincide (every width equal to S) load into each other: the file carries variables
        f4, c4 = _net(4, 2, (4, 4), "fork", max_batch=8), _net(4, 2, (4, 4), "chained", max_batch=8)
        others += [f4, c4]
        c4.set_arena(0, np.zeros(c4.param_count, np.float32))
        p4 = str(tmp_path / "f4.npz")
        assert f4._lib.ga3c_dmlp_save(f4._h, p4.encode()) == 0 and c4._lib.ga3c_dmlp_load(c4._h, p4.encode()) == 0
        assert np.array_equal(c4.get_arena(0), f4.get_arena(0))
    finally:
        for n in [net, other, img, vec] + others:
            if n is not None:
                n.close()


def test_log_writes_scalars_and_histograms(tmp_path, monkeypatch):
    import ga3c_amd  # noqa: F401
    from NetworkVP import histogram_proto
    monkeypatch.chdir(tmp_path)
    S, A, layers, stack = SHAPES[0]
    params = _params(S, A, layers, stack)
    net = _net(S, A, layers, stack)
    try:
        _reset(net, params)
        net.beta = 0.01
        x, y, a = _batch(50, S, A, 8)
        losses = net.log(x, y, a, 7)
        want, _ = m.loss_and_grads(params, *_f64(x, y, a), 0.01, stack=stack)
        f = m.forward(params, x.astype(np.float64), stack)
        row = open("logs/dvec/scalars.csv").read().strip().split(",")
        assert row[0] == "7" and len(row) == 7
        assert abs(float(row[1]) - want["cost_p_1_agg"]) <= TOL * max(1.0, abs(want["cost_p_1_agg"]))
        assert abs(float(row[4]) - want["cost_v"]) <= TOL * max(1.0, want["cost_v"])
        h = np.load("logs/dvec/histograms_00000007.npz")
        assert sorted(k[:-4] for k in h.files if k.startswith("weights_") and k.endswith("/num")) == \
            sorted("weights_%s:0" % k for k in m.param_order(layers))                # the dead variables too
        for tag, ref in (("activation_lastdense", f["h4"]), ("activation_v", f["v"]), ("activation_p", f["p"])):
            want_h = histogram_proto(ref)
            assert h[tag + "/num"] == want_h["num"]
            assert abs(h[tag + "/sum"] - want_h["sum"]) <= TOL * max(1.0, abs(want_h["sum"]), want_h["num"])
            assert abs(h[tag + "/max"] - want_h["max"]) <= TOL * max(1.0, abs(want_h["max"]))
        assert abs(losses[2] - want["cost_v"]) <= TOL * max(1.0, want["cost_v"])
    finally:
        net.close()


@pytest.mark.parametrize("head", ["plain", "log_softmax"])
def test_saturated_policy_against_the_oracle(head):
    """logits_p/w x 200, as the image net's saturation test has it: probabilities below LOG_EPSILON and next to 1, clamped
    selected actions; forward, gradients and two production steps against the oracle."""
    S, A, layers, stack = SHAPES[2]
    kw = HEADS[head]
    params = _params(S, A, layers, stack)
    params["logits_p/w"] = (m.init_params(S, A, layers, stack, seed=777)["logits_p/w"] * 200.0).astype(np.float32).astype(np.float64)
    net = _net(S, A, layers, stack, head=kw)
    try:
        _reset(net, params)
        net.learning_rate, net.beta = 1e-3, 0.01
        x, y, a = _batch(132, S, A, 21)
        f = m.forward(params, x.astype(np.float64), stack, **kw)
        assert f["p"].min() < 1e-9 and f["p"].max() > 0.9999
        assert np.any((f["p"] * a).sum(axis=1) < 1e-6)                # selected actions under the clamp
        p, v, _ = net.predict_p_v_logits(x)
        assert _close(p, f["p"]) and _close(v, f["v"]) and np.all(np.isfinite(p))
        losses = net.compute_grads(x, y, a)
        want, g = m.loss_and_grads(params, *_f64(x, y, a), 0.01, stack=stack, **kw)
        for got, key in zip(losses, ("cost_p_1_agg", "cost_p_2_agg", "cost_v")):
            assert abs(got - want[key]) <= TOL * max(1.0, abs(want[key])), (key, got, want[key])
        grad = net.get_arena(3)
        assert np.all(np.isfinite(grad))
        for k in m.param_order(layers):
            assert _close(_var(net, grad, k), g[k]), k
        ref = {k: t.copy() for k, t in params.items()}
        ms = {k: np.ones_like(t) for k, t in params.items()}
        mom = {k: np.zeros_like(t) for k, t in params.items()}
        for step in range(2):
            xb, yb, ab = _batch(132, S, A, 30 + step)
            net.train(xb, yb, ab)
            m.train_step(ref, ms, mom, *_f64(xb, yb, ab), 1e-3, 0.01, stack=stack, **kw)
        assert _close(net.get_arena(0), m.flat(ref), 1e-5) and _close(net.get_arena(1), m.flat(ms), 1e-5)
    finally:
        net.close()


@pytest.mark.timeout(180)
def test_server_drives_the_net_with_the_native_loops(tmp_path, monkeypatch):
    import ga3c_amd  # noqa: F401
    from Config import Config
    monkeypatch.chdir(tmp_path)
    for k, v in (("GAME", "CartPole-v0"), ("AGENTS", 8), ("PREDICTORS", 2), ("TRAINERS", 2), ("TIME_MAX", 5),
                 ("DYNAMIC_SETTINGS", False), ("SAVE_MODELS", False), ("TRAINING_MIN_BATCH_SIZE", 0),
                 ("CONTINUOUS_INPUT", Config.CONTINUOUS_INPUT), ("DISCRATE_INPUT", Config.DISCRATE_INPUT),
                 ("DENSE_LAYERS", Config.DENSE_LAYERS), ("DENSE_STACK", Config.DENSE_STACK)):
        monkeypatch.setattr(Config, k, v)
    from Server import Server
    import NetworkVP_discrate
    srv = Server(max_agents=16)
    assert isinstance(srv.model, NetworkVP_discrate.Network) and srv.zero_copy and not srv.state_cache
    assert not srv.transport.float_actions and srv.transport.state_bytes == 16 and srv.num_actions == 2
    seen = set()
    inner = srv.model.train_offsets

    def spy(offsets, y_r, a):
        assert a.dtype == np.float32 and a.shape == (len(offsets), 2) and np.all(a.sum(axis=1) == 1.0)
        seen.update(np.argmax(a, axis=1).tolist())
        inner(offsets, y_r, a)

    monkeypatch.setattr(srv.model, "train_offsets", spy)
    srv.main(max_seconds=8)
    assert srv.failure is None and srv.training_step > 20 and srv.predictions_served > 1000
    assert srv.model.get_global_step() == srv.training_step
    assert seen and seen <= {0, 1}
    assert open("results.txt").read().strip()


@pytest.mark.timeout(300)
def test_train_script_runs_cartpole_and_play_loads_its_checkpoint(tmp_path):
    env = dict(os.environ, PYTHONUNBUFFERED="1")
    cwd = str(tmp_path)
    run = subprocess.run(["sh", os.path.join(PKG, "_train.sh"), "GAME=CartPole-v0", "MAX_SECONDS=20", "AGENTS=16",
                          "PREDICTORS=2", "TRAINERS=2", "TIME_MAX=20", "SAVE_FREQUENCY=2000", "DYNAMIC_SETTINGS="],
                         cwd=cwd, env=env, capture_output=True, text=True, timeout=200)
    assert run.returncode == 0, run.stdout[-3000:] + run.stderr[-3000:]
    assert "died" not in run.stdout + run.stderr
    tps = [int(t) for t in re.findall(r"TPS:\s*(\d+)\]", run.stdout)]
    pps = [int(t) for t in re.findall(r"PPS:\s*(\d+)", run.stdout)]
    assert tps and max(tps) > 0 and pps and max(pps) > 0, run.stdout[-2000:]
    print("CartPole-v0, 20 s: last status line %s" % [ln for ln in run.stdout.splitlines() if "TPS:" in ln][-1])
    lines = open(os.path.join(cwd, "results.txt")).read().strip().splitlines()
    # an episode is at most 200 steps; the frame accounting of ProcessAgent.py:174 counts len(rollout) + 1 per rollout, and a
    # rollout of TIME_MAX = 20 new steps carries the previous rollout's last row as well: two extra per rollout
    assert lines and all(1 <= int(ln.split(",")[2]) <= 200 + 2 * (200 // 20 + 1) for ln in lines)
    found = sorted(glob.glob(os.path.join(cwd, "checkpoints", "network_????????.npz")))
    assert found
    z = np.load(found[-1])
    assert z["dense1_4_p/w:0"].shape == (4, 10) and z["logits_p/w:0"].shape == (10, 2) and int(z["step"]) > 0
    before = open(found[-1], "rb").read()
    play = subprocess.run(["sh", os.path.join(PKG, "_play.sh"), "GAME=CartPole-v0", "MAX_SECONDS=6", "PRINT_STATS_FREQUENCY=1"],
                          cwd=cwd, env=env, capture_output=True, text=True, timeout=200)
    assert play.returncode == 0, play.stdout[-3000:] + play.stderr[-3000:]
    assert "checkpoint not loaded" not in play.stdout and "died" not in play.stdout + play.stderr
    assert re.findall(r"TPS:\s*(\d+)\]", play.stdout) and all(int(t) == 0 for t in re.findall(r"TPS:\s*(\d+)\]", play.stdout))
    assert sorted(glob.glob(os.path.join(cwd, "checkpoints", "network_????????.npz"))) == found
    assert open(found[-1], "rb").read() == before
    assert len(open(os.path.join(cwd, "results.txt")).read().strip().splitlines()) > len(lines)
