"""-m gpu: the host half of the DDPG handle (ga3c_ddpg_*) -- what it refuses and with which return code, its
variable table and arena selectors, its prediction tickets and what a refused checkpoint leaves behind.  Arithmetic is
tests/test_gpu_ddpg.py's; nothing here has a tolerance: a return code is equal or not, and results are compared bit for bit.

One small handle: S = 3, A = 2, max_batch 16, a ring of 32 rows, two prediction lanes, add_OUnoise off, so that the gather
entries' GA3C_DDPG_NOISE_OWN adds nothing and only wraps, like predict(noise=False)."""
import contextlib
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

OK, EINVAL, ESTATE = 0, -1, -4
S, A, MAXB, CAP, LANES = 3, 2, 16, 32, 2
H1, H2 = 400, 300
MOVING = {"actor_norm1/moving_mean": H1, "actor_norm1/moving_variance": H1, "actor_norm2/moving_mean": H2,
          "actor_norm2/moving_variance": H2, "critic_norm1/moving_mean": H1, "critic_norm1/moving_variance": H1}


@contextlib.contextmanager
def _handle(**kw):
    import ga3c_amd  # noqa: F401
    from Config import Config
    from NetworkDDPG import Network
    kw.setdefault("add_OUnoise", False)
    saved = {k: getattr(Config, k) for k in kw}
    for k, v in kw.items():
        setattr(Config, k, v)
    try:
        net = Network("gpu:0", "ddpg_host", A, (S,), max_batch=MAXB, predict_lanes=LANES, replay_capacity=CAP)
    finally:
        for k, v in saved.items():
            setattr(Config, k, v)
    net.learning_rate = 3e-4
    try:
        yield net
    finally:
        net.close()


def _valid_config():
    import ga3c_amd  # noqa: F401
    import _native as nat
    return nat.DdpgConfig(device=0, state_dim=S, num_actions=A, max_batch=MAXB, replay_capacity=CAP, predict_lanes=LANES,
                          flags=nat.DDPG_FUTURE_REWARD, tau=0.001, gamma=0.99, actor_lr=1.0, critic_lr=1.0, rmsprop_decay=0.99,
                          rmsprop_momentum=0.0, rmsprop_epsilon=0.1, grad_clip_norm=40.0, ou_sigma=0.3, ou_theta=0.15, ou_dt=0.01,
                          seed=1)


def _rows(n, seed=0):
    rng = np.random.default_rng(seed)
    return (rng.normal(size=(n, S)).astype(np.float32), rng.uniform(-1, 1, (n, A)).astype(np.float32),
            rng.normal(size=n).astype(np.float32), (rng.uniform(size=n) < 0.3).astype(np.float32),
            rng.normal(size=(n, S)).astype(np.float32))


def _snapshot(net):
    """Every variable in arenas 0..3, and the step."""
    out = {(k, w): net.get_variable_value(k, w) for k in net.get_variables_names() for w in range(4)}
    out["step"] = net.get_global_step()
    return out


def _same(a, b):
    return a.keys() == b.keys() and all(np.array_equal(a[k], b[k]) for k in a)


def test_create_refuses_each_bad_field_on_its_own():
    import ga3c_amd  # noqa: F401
    import _native as nat
    lib = nat.hip_lib()
    ndev = C.c_int32()
    assert lib.ga3c_device_count(C.byref(ndev)) == OK
    cases = [("state_dim", 0), ("state_dim", 65), ("num_actions", 0), ("num_actions", 33), ("max_batch", 0), ("max_batch", 4097),
             ("replay_capacity", 0), ("flags", 1 << 5), ("predict_lanes", -1), ("predict_lanes", 65), ("tau", -0.1), ("tau", 1.5),
             ("tau", float("nan")), ("device", ndev.value)]
    for field, value in cases:
        cfg = _valid_config()
        setattr(cfg, field, value)
        handle = C.c_void_p(1)
        assert lib.ga3c_ddpg_create(C.byref(cfg), C.byref(handle)) == EINVAL, (field, value)
        assert not handle.value, (field, value)
    handle = C.c_void_p()                                       # ... and the config they were all made from is a good one
    assert lib.ga3c_ddpg_create(C.byref(_valid_config()), C.byref(handle)) == OK and handle.value
    assert lib.ga3c_ddpg_destroy(handle) == OK


def test_variable_table_and_arena_selectors():
    import NetworkDDPG as nd
    import _native as nat
    with _handle() as net:
        lib, h = net._lib, net._h
        shapes = dict(nd.param_shapes(S, A), **{k: (n,) for k, n in MOVING.items()})
        names = [lib.ga3c_ddpg_param_name(h, i).decode() for i in range(lib.ga3c_ddpg_num_params(h))]
        assert names == list(nd.TRAINABLE) + list(MOVING)
        for name in names:
            for spelled in (name, name + ":0"):
                count, ndim, trainable = C.c_int64(), C.c_int32(), C.c_int32(-1)
                shape = (C.c_int64 * 4)()
                assert lib.ga3c_ddpg_param_info(h, spelled.encode(), C.byref(count), C.byref(ndim), shape, C.byref(trainable)) == OK
                assert tuple(shape[:ndim.value]) == shapes[name] and count.value == int(np.prod(shapes[name]))
                assert trainable.value == (0 if name in MOVING else 1)
                buf = np.empty(count.value, np.float32)
                assert lib.ga3c_ddpg_get_param(h, spelled.encode(), 0, nat.ptr(buf), buf.size) == OK
                assert lib.ga3c_ddpg_set_param(h, spelled.encode(), 0, nat.ptr(buf), buf.size) == OK
        buf = np.zeros(H1, np.float32)
        count = C.c_int64()
        assert lib.ga3c_ddpg_param_info(h, b"actor_fc3/b", C.byref(count), None, None, None) == EINVAL
        assert lib.ga3c_ddpg_get_param(h, b"actor_fc3/b", 0, nat.ptr(buf), H1) == EINVAL
        assert lib.ga3c_ddpg_set_param(h, b"actor_fc3/b", 0, nat.ptr(buf), H1) == EINVAL
        assert lib.ga3c_ddpg_get_param(h, b"actor_fc1/b", 0, nat.ptr(buf), H1 - 1) == EINVAL
        assert lib.ga3c_ddpg_set_param(h, b"actor_fc1/b", 0, nat.ptr(buf), H1 - 1) == EINVAL
        assert lib.ga3c_ddpg_get_param(h, b"actor_fc1/b", 4, nat.ptr(buf), H1) == OK
        for which in (5, -1):
            assert lib.ga3c_ddpg_get_param(h, b"actor_fc1/b", which, nat.ptr(buf), H1) == EINVAL
            assert lib.ga3c_ddpg_set_param(h, b"actor_fc1/b", which, nat.ptr(buf), H1) == EINVAL
        before = net.get_variable_value("actor_fc1/b", 4)
        ones = buf + 1
        assert lib.ga3c_ddpg_set_param(h, b"actor_fc1/b", 4, nat.ptr(ones), H1) == EINVAL          # the gradient is read-only
        assert np.array_equal(net.get_variable_value("actor_fc1/b", 4), before)
        for which in range(4):
            value = buf + which
            assert lib.ga3c_ddpg_set_param(h, b"actor_fc1/b", which, nat.ptr(value), H1) == OK
            assert np.array_equal(net.get_variable_value("actor_fc1/b", which), value)


def test_step_is_set_and_a_negative_one_refused():
    with _handle() as net:
        lib, h = net._lib, net._h
        assert lib.ga3c_ddpg_set_step(h, 7) == OK
        assert net.get_global_step() == 7
        assert lib.ga3c_ddpg_set_step(h, -1) == EINVAL
        assert net.get_global_step() == 7


def test_batch_bounds_of_predict_train_and_train_replay():
    import _native as nat
    with _handle() as net:
        lib, h = net._lib, net._h
        s, a, r, done, s2 = _rows(MAXB + 1)
        out, q = np.empty((MAXB + 1, A), np.float32), np.empty(2, np.float32)
        slots = np.arange(MAXB + 1, dtype=np.int32)
        assert net.replay_add(s[:MAXB], a[:MAXB], r[:MAXB], done[:MAXB], s2[:MAXB]) == (MAXB, MAXB)
        assert net.replay_add(s[:MAXB], a[:MAXB], r[:MAXB], done[:MAXB], s2[:MAXB]) == (CAP, CAP)
        for b, want in ((0, EINVAL), (MAXB + 1, EINVAL), (MAXB, OK)):
            assert lib.ga3c_ddpg_predict(h, nat.ptr(s), b, nat.DDPG_NOISE_NONE, None, nat.ptr(out)) == want
            assert lib.ga3c_ddpg_train(h, nat.ptr(s), nat.ptr(a), nat.ptr(r), nat.ptr(done), nat.ptr(s2), b, 3e-4,
                                       nat.DDPG_NOISE_NONE, None, nat.ptr(q)) == want
            assert lib.ga3c_ddpg_train_replay(h, nat.ptr(slots, nat.i32p), b, -1, 3e-4, nat.DDPG_NOISE_NONE, None, nat.ptr(q)) == want
        assert net.get_global_step() == 2


def test_segment_registration_and_offsets():
    import _native as nat
    with _handle() as net:
        lib, h = net._lib, net._h
        seg = np.random.default_rng(1).normal(size=(64, S)).astype(np.float32)
        base, nbytes = C.c_void_p(seg.ctypes.data), seg.nbytes
        p, v = np.empty((1, A), np.float32), np.empty(1, np.float32)

        def gather(offset, u8=0):
            off = np.array([offset], np.int64)
            return lib.ga3c_ddpg_predict_gather(h, nat.ptr(off, nat.i64p), 1, u8, nat.ptr(p), nat.ptr(v), None)

        assert gather(0) == ESTATE                                  # nothing registered
        assert lib.ga3c_ddpg_register_host(h, base, nbytes) == OK
        assert lib.ga3c_ddpg_register_host(h, base, nbytes) == ESTATE
        assert gather(0) == OK
        assert gather(nbytes - 4 * S) == OK                         # the last whole row
        assert np.array_equal(p, net.predict(seg[-1:], noise=False))
        for bad in (2, -4, nbytes - 4 * S + 4):
            assert gather(bad) == EINVAL, bad
        assert gather(0, u8=1) == EINVAL
        ticket = C.c_int32(-1)
        off = np.zeros(1, np.int64)
        assert lib.ga3c_ddpg_predict_gather_begin(h, nat.ptr(off, nat.i64p), 1, 1, C.byref(ticket)) == EINVAL
        assert lib.ga3c_ddpg_unregister_host(h) == OK
        assert lib.ga3c_ddpg_unregister_host(h) == OK
        assert gather(0) == ESTATE


def test_tickets_out_of_order_and_misused():
    import _native as nat
    with _handle() as net:
        lib, h = net._lib, net._h
        seg = np.random.default_rng(2).normal(size=(8, S)).astype(np.float32)
        assert lib.ga3c_ddpg_register_host(h, C.c_void_p(seg.ctypes.data), seg.nbytes) == OK
        offs = np.arange(8, dtype=np.int64) * 4 * S

        def begin(lo, hi):
            ticket = C.c_int32(-1)
            part = np.ascontiguousarray(offs[lo:hi])
            assert lib.ga3c_ddpg_predict_gather_begin(h, nat.ptr(part, nat.i64p), hi - lo, 0, C.byref(ticket)) == OK
            return ticket.value

        def end(ticket, b):
            p, v = np.full((b, A), np.nan, np.float32), np.full(b, np.nan, np.float32)
            return lib.ga3c_ddpg_predict_gather_end(h, ticket, b, nat.ptr(p), nat.ptr(v)), p, v

        t5, t3 = begin(0, 5), begin(5, 8)
        assert sorted((t5, t3)) == [0, 1]
        rc3, p3, v3 = end(t3, 3)
        rc5, p5, v5 = end(t5, 5)
        assert rc3 == OK and rc5 == OK
        want = net.predict(seg, noise=False)
        assert np.array_equal(p5, want[:5]) and np.array_equal(p3, want[5:])
        assert np.array_equal(v5, want[:5, 0]) and np.array_equal(v3, want[5:, 0])
        assert end(t5, 5)[0] == ESTATE                              # ended already
        assert end(-1, 5)[0] == ESTATE and end(LANES, 5)[0] == ESTATE
        t = begin(0, 5)
        assert end(t, 4)[0] == EINVAL                               # the wrong batch: refused, and the lane is free again
        assert end(t, 5)[0] == ESTATE
        for _ in range(2):
            ta, tb = begin(0, 5), begin(5, 8)
            assert sorted((ta, tb)) == [0, 1]
            rca, pa, _ = end(ta, 5)
            rcb, pb, _ = end(tb, 3)
            assert rca == OK and rcb == OK and np.array_equal(pa, want[:5]) and np.array_equal(pb, want[5:])
        assert lib.ga3c_ddpg_unregister_host(h) == OK


def test_fetch_refuses_an_unknown_name_and_a_wrong_count():
    import _native as nat
    with _handle() as net:
        lib, h = net._lib, net._h
        s, a, r, done, s2 = _rows(4)
        net.train(s, r, a, s2, done, noise=False)
        out = np.empty(8, np.float32)
        assert lib.ga3c_ddpg_fetch(h, b"q", nat.ptr(out), 4) == OK
        assert lib.ga3c_ddpg_fetch(h, b"a_out", nat.ptr(out), 4 * A) == OK
        assert lib.ga3c_ddpg_fetch(h, b"q", nat.ptr(out), 5) == EINVAL
        assert lib.ga3c_ddpg_fetch(h, b"a_out", nat.ptr(out), 4) == EINVAL
        assert lib.ga3c_ddpg_fetch(h, b"no_such_buffer", nat.ptr(out), 4) == EINVAL


def test_a_refused_checkpoint_writes_nothing_and_unnamed_slots_survive_a_load(tmp_path):
    good, bad = str(tmp_path / "good.npz"), str(tmp_path / "bad.npz")
    s, a, r, done, s2 = _rows(8)
    with _handle() as net, _handle(RMSPROP=False) as adam:
        lib = net._lib
        net.train(s, r, a, s2, done, noise=False)
        assert lib.ga3c_ddpg_save(net._h, good.encode()) == OK
        with np.load(good) as z:
            members = {k: z[k] for k in z.files}
        assert members["step"].dtype == np.int64 and int(members["step"]) == 1
        net.train(s, r, a, s2, done, noise=False)                    # the handle now differs from the file everywhere
        net.set_global_step(7)

        def rewritten(change):
            out = dict(members)
            change(out)
            np.savez(bad, **out)
            return bad.encode()

        def remove(m):
            del m["actor_norm1/moving_mean:0"]

        def reshape(m):
            m["actor_fc2/W:0"] = m["actor_fc2/W:0"].T.copy()

        def negative(m):
            m["step"] = np.int64(-1)

        def narrow(m):
            m["step"] = np.int32(1)

        before = _snapshot(net)
        for change in (remove, reshape, negative, narrow):
            assert lib.ga3c_ddpg_load(net._h, rewritten(change)) == ESTATE, change.__name__
            assert _same(before, _snapshot(net)), change.__name__
        # RMSProp slots of the critic where this handle keeps Adam's
        adam.train(s, r, a, s2, done, noise=False)
        before_adam = _snapshot(adam)
        assert lib.ga3c_ddpg_load(adam._h, good.encode()) == ESTATE
        assert _same(before_adam, _snapshot(adam))
        # no member names slot 2 of a moving statistic: a load leaves it alone
        sentinel = np.arange(H1, dtype=np.float32) + 0.5
        net.set_variable_value("actor_norm1/moving_mean", sentinel, 2)
        assert lib.ga3c_ddpg_load(net._h, rewritten(lambda m: None)) == OK
        assert net.get_global_step() == 1
        assert np.array_equal(net.get_variable_value("actor_norm1/moving_mean", 2), sentinel)
        assert np.array_equal(net.get_variable_value("critic_fc2/W", 0), members["critic_fc2/W:0"])
        assert np.array_equal(net.get_variable_value("critic_fc2/W", 2), members["critic_fc2/W/RMSProp:0"])
