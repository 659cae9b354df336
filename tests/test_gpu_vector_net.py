"""-m gpu: the vector-state network of GAME = 'Pendulum-v0' (ga3c_mlp_*) against its f64 statement
(tests/mlp_oracle.py).  Tolerance: 1e-4 x max(1, max|want|), as in tests/test_gpu_continuous.py.  Every batch keeps away from
the atan2 branch cut, where o jumps from 1 to -1 and f32 and f64 may fall on either side."""
import contextlib
import os
import re
import subprocess

import numpy as np
import pytest

import mlp_oracle as m
from vector_limit_cases import batch as _batch, params as _params      # shared with tests/test_gpu_vector_limits.py

pytestmark = pytest.mark.gpu

TOL = 1e-4
SIZES = [1, 15, 16, 17, 128, 132, 201, 1024]
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


def _net(state_dim, num_actions, max_batch=1024, **kw):
    import ga3c_amd  # noqa: F401  (puts the flat modules on sys.path)
    from NetworkVP_vector import Network
    with _config(**kw):
        return Network("gpu:0", "vec", num_actions, (state_dim,), max_batch=max_batch)


def _reset(net, params):
    net.set_arena(0, m.flat(params))
    net.set_arena(1, np.ones(net.param_count, np.float32))
    net.set_arena(2, np.zeros(net.param_count, np.float32))


@pytest.mark.parametrize("state_dim", [3, 7])
def test_forward_losses_and_gradients_against_the_oracle(state_dim):
    A = 1 if state_dim == 3 else 3
    params = _params(state_dim, A)
    net = _net(state_dim, A)
    try:
        _reset(net, params)
        for bsz in SIZES:
            x, y, a = _batch(params, bsz, state_dim, A, 100 + bsz)
            f = m.forward(params, x.astype(np.float64))
            p, v, z = net.predict_p_v_logits(x)
            assert _close(p, f["o"]) and _close(v, f["v"]) and _close(z, f["z"]), bsz
            net.beta = 0.01
            losses = net.compute_grads(x, y, a)
            want, g = m.loss_and_grads(params, x.astype(np.float64), y.astype(np.float64), a.astype(np.float64), 0.01)
            for got, key in zip(losses, ("cost_p_1_agg", "cost_p_2_agg", "cost_v")):
                assert abs(got - want[key]) <= TOL * max(1.0, abs(want[key])), (bsz, key, got, want[key])
            for name, width in (("x", state_dim), ("pd1", 4), ("pd2", 256), ("pd3", 256), ("pd4", 100), ("d1", 64),
                                ("v", 1), ("p", A), ("z", 2 * A)):
                ref = f["o"] if name == "p" else f[name]
                assert _close(net.fetch(name, bsz * width), ref), (bsz, name)
            for name, width in (("dv", 1), ("dz", 2 * A), ("dd1", 64), ("dpd4", 100), ("dpd3", 256), ("dpd2", 256),
                                ("dpd1", 4)):
                assert _close(net.fetch(name, bsz * width), g[name]), (bsz, name)
            grad = net.get_arena(3)
            for k in m.PARAM_ORDER:
                off, size = net._offsets[k]
                assert _close(grad[off:off + size], g[k]), (bsz, k)
    finally:
        net.close()


@pytest.mark.parametrize("state_dim", [3, 7])
def test_backward_tensors_relative_to_their_largest_entry(state_dim):
    """TOL x max(1, max|want|) is absolute below 1, and here dpd3 / dpd4 stay below 0.1 at every size and every gradient at
    B = 1 (tests/README.md, "how large the tensors are").  Every delta and gradient once more with tests/closeness.py:
    max|got - want| / max|want| against max(16 x e32, 2^-20), e32 from the oracle run in float32 on the same rows.  A bias
    gradient of ONE element (logits_v/b; out_x/b and out_y/b when A = 1) takes the larger of that single draw and what the
    float32 error of the delta it sums implies (closeness.e32_of_row_sum, where the reason is written): out_y/b at
    B = 15, A = 1 came out at rel_err 2.5e-6 with a single draw of 3e-8, while out_y/w -- the same delta summed with weights in
    (0, 1) -- has e32 2.3e-7 and rel_err 2.5e-6 as well; the delta's own error gives 1.1e-6 for the bias."""
    import closeness as c
    A = 1 if state_dim == 3 else 3
    params = _params(state_dim, A)
    p32 = {k: v.astype(np.float32) for k, v in params.items()}
    net = _net(state_dim, A)
    try:
        _reset(net, params)
        net.beta = 0.01
        failed = []
        for bsz in SIZES:
            x, y, a = _batch(params, bsz, state_dim, A, 100 + bsz)
            net.compute_grads(x, y, a)
            _, g = m.loss_and_grads(params, x.astype(np.float64), y.astype(np.float64), a.astype(np.float64), 0.01)
            _, g32 = m.loss_and_grads(p32, x, y, a, 0.01)
            grad = net.get_arena(3)
            got = {name: net.fetch(name, bsz * width) for name, width in (("dv", 1), ("dz", 2 * A), ("dd1", 64), ("dpd4", 100),
                                                                          ("dpd3", 256), ("dpd2", 256), ("dpd1", 4))}
            got.update({k: grad[net._offsets[k][0]:net._offsets[k][0] + net._offsets[k][1]] for k in m.PARAM_ORDER})
            for name in got:
                assert np.asarray(g32[name]).dtype == np.float32, name
                e32 = c.rel_err(g32[name], g[name])
                sums = {"logits_v/b": ("dv", slice(None)), "logits_p/out_x/b": ("dz", (slice(None), slice(0, A))),
                        "logits_p/out_y/b": ("dz", (slice(None), slice(A, 2 * A)))}
                if name in sums and np.size(g[name]) == 1:
                    col = sums[name]
                    e32 = max(e32, c.e32_of_row_sum(np.asarray(g32[col[0]])[col[1]], np.asarray(g[col[0]])[col[1]]))
                err = c.report("vector S=%d B=%d" % (state_dim, bsz), name, got[name], g[name], e32, c.bound(e32))
                if not err <= c.bound(e32):
                    failed.append((bsz, name, err, c.bound(e32)))
        assert not failed, failed
    finally:
        net.close()


@pytest.mark.parametrize("kind", ["plain", "clip", "momentum"])
def test_two_train_steps_against_the_oracle(kind):
    kw = {"USE_GRAD_CLIP": kind == "clip", "GRAD_CLIP_NORM": 2e-4 if kind == "clip" else 40.0,
          "RMSPROP_MOMENTUM": 0.9 if kind == "momentum" else 0.0}
    params = _params(3, 1)
    net = _net(3, 1, **kw)
    try:
        _reset(net, params)
        net.learning_rate, net.beta = 1e-3, 0.01
        ref = {k: v.copy() for k, v in params.items()}
        ms = {k: np.ones_like(v) for k, v in params.items()}
        mom = {k: np.zeros_like(v) for k, v in params.items()}
        for step, bsz in enumerate((132, 201)):
            x, y, a = _batch(params, bsz, 3, 1, 7 + step)
            net.train(x, y, a)
            _, g = m.loss_and_grads(ref, x.astype(np.float64), y.astype(np.float64), a.astype(np.float64), 0.01)
            m.rmsprop_update(ref, ms, g, 1e-3, momentum=kw["RMSPROP_MOMENTUM"], mom=mom,
                             clip=kw["GRAD_CLIP_NORM"] if kind == "clip" else None)
        assert net.get_global_step() == 2
        assert _close(net.get_arena(0), m.flat(ref), 1e-5)
        assert _close(net.get_arena(1), m.flat(ms), 1e-5)
        if kind == "momentum":
            assert _close(net.get_arena(2), m.flat(mom), 1e-5)
    finally:
        net.close()


@pytest.mark.parametrize("clip", [False, True])
def test_split_step_and_repeated_calls_are_bit_identical(clip):
    params = _params(3, 1)
    kw = {"USE_GRAD_CLIP": clip, "GRAD_CLIP_NORM": 2e-4}
    a_net, b_net = _net(3, 1, **kw), _net(3, 1, **kw)
    try:
        x, y, a = _batch(params, 201, 3, 1, 99)
        for n in (a_net, b_net):
            _reset(n, params)
            n.learning_rate, n.beta = 1e-3, 0.01
        g1 = (b_net.compute_grads(x, y, a), b_net.get_arena(3))
        g2 = (b_net.compute_grads(x, y, a), b_net.get_arena(3))
        assert np.array_equal(g1[0], g2[0]) and np.array_equal(g1[1], g2[1])      # no float atomics anywhere
        b_net.apply_grads()
        a_net.train(x, y, a)
        for w in (0, 1, 3):
            assert np.array_equal(a_net.get_arena(w), b_net.get_arena(w)), w
        assert a_net.get_global_step() == b_net.get_global_step() == 1
    finally:
        a_net.close()
        b_net.close()


def test_gather_entries_are_bit_equal_to_host_buffers():
    """Rows read out of the registered transport -- agent slots, and rollout rows of 12 bytes that are not 16-byte
    aligned -- give the bits the host-buffer entry points give."""
    import ga3c_amd  # noqa: F401
    import Transport as tp
    params = _params(3, 1)
    t = tp.Transport.create(tp.unique_name("t_vec"), 40, 1, 12, 8, 40, float_actions=True)
    n1, n2 = _net(3, 1), _net(3, 1)
    try:
        for n in (n1, n2):
            _reset(n, params)
            n.learning_rate, n.beta = 1e-3, 0.01
        x, y, a = _batch(params, 37, 3, 1, 5)
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
        assert np.any(offs % 16 != 0)
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
        lib = n1._lib
        tk = [C.c_int32(-1), C.c_int32(-1)]
        o1 = np.ascontiguousarray(t.state_offsets(ids[:20]))
        o2 = np.ascontiguousarray(t.state_offsets(ids[20:]))
        import _native as nat
        nat.check(lib.ga3c_mlp_predict_gather_begin(n1._h, nat.ptr(o1, nat.i64p), 20, 0, C.byref(tk[0])))
        nat.check(lib.ga3c_mlp_predict_gather_begin(n1._h, nat.ptr(o2, nat.i64p), 17, 0, C.byref(tk[1])))
        pb, vb = np.empty((17, 1), np.float32), np.empty(17, np.float32)
        pa, va = np.empty((20, 1), np.float32), np.empty(20, np.float32)
        nat.check(lib.ga3c_mlp_predict_gather_end(n1._h, tk[1], 17, nat.ptr(pb), nat.ptr(vb)))
        nat.check(lib.ga3c_mlp_predict_gather_end(n1._h, tk[0], 20, nat.ptr(pa), nat.ptr(va)))
        p3, v3 = n1.predict_p_and_v(x)
        assert np.array_equal(np.concatenate([pa, pb]), p3) and np.array_equal(np.concatenate([va, vb]), v3)
        assert lib.ga3c_mlp_predict_gather_end(n1._h, tk[0], 20, nat.ptr(pa), nat.ptr(va)) == -4    # nothing begun: ESTATE
        bad = np.array([t.nbytes - 8], np.int64)
        with pytest.raises(RuntimeError):
            n1.predict_offsets(bad)                                                          # a row past the segment
        n1.unregister_transport()
    finally:
        n1.close()
        n2.close()
        t.shutdown()
        t.close()


def test_checkpoint_round_trip_and_refusals(tmp_path):
    import ga3c_amd  # noqa: F401
    from NetworkVP import Network as ImageNet
    params = _params(3, 1)
    net = _net(3, 1)
    other = _net(3, 1)
    img = None
    try:
        _reset(net, params)
        net.learning_rate, net.beta = 1e-3, 0.01
        x, y, a = _batch(params, 40, 3, 1, 3)
        net.train(x, y, a)
        path = str(tmp_path / "vec.npz")
        assert net._lib.ga3c_mlp_save(net._h, path.encode()) == 0
        z = np.load(path)
        assert int(z["step"]) == 1 and z["dense13_p/w:0"].shape == (256, 256) and "logits_p/out_y/b/RMSProp_1:0" in z
        assert other._lib.ga3c_mlp_load(other._h, path.encode()) == 0
        for w in (0, 1, 2):
            assert np.array_equal(other.get_arena(w), net.get_arena(w))
        assert other.get_global_step() == 1
        with _config(CONTINUOUS_INPUT=True):
            img = ImageNet("gpu:0", "img", 1, (84, 84, 4), max_batch=8, predict_lanes=1)
        ipath = str(tmp_path / "img.npz")
        assert img._lib.ga3c_net_save(img._h, ipath.encode()) == 0
        before = other.get_arena(0)
        assert other._lib.ga3c_mlp_load(other._h, ipath.encode()) == -4                 # image file into the vector net
        assert np.array_equal(other.get_arena(0), before)
        ibefore = img.get_arena(0)
        assert img._lib.ga3c_net_load(img._h, path.encode()) == -4                      # vector file into the image net
        assert np.array_equal(img.get_arena(0), ibefore)
        n7 = _net(7, 1)
        try:
            assert n7._lib.ga3c_mlp_load(n7._h, path.encode()) == -4                    # another state size
        finally:
            n7.close()
    finally:
        net.close()
        other.close()
        if img is not None:
            img.close()


def test_log_writes_scalars_and_histograms(tmp_path, monkeypatch):
    import ga3c_amd  # noqa: F401
    from NetworkVP import histogram_proto
    monkeypatch.chdir(tmp_path)
    params = _params(3, 1)
    net = _net(3, 1)
    try:
        _reset(net, params)
        net.beta = 0.01
        x, y, a = _batch(params, 50, 3, 1, 8)
        losses = net.log(x, y, a, 7)
        want, _ = m.loss_and_grads(params, x.astype(np.float64), y.astype(np.float64), a.astype(np.float64), 0.01)
        f = m.forward(params, x.astype(np.float64))
        row = open("logs/vec/scalars.csv").read().strip().split(",")
        assert row[0] == "7" and len(row) == 7
        assert abs(float(row[4]) - want["cost_v"]) <= TOL * max(1.0, want["cost_v"])
        h = np.load("logs/vec/histograms_00000007.npz")
        assert len([k for k in h.files if k.startswith("weights_") and k.endswith("/num")]) == 16
        for tag, ref in (("activation_pd1", f["pd1"]), ("activation_pd2", f["pd2"]), ("activation_d2", f["d1"]),
                         ("activation_v", f["v"]), ("activation_p", f["o"])):
            want_h = histogram_proto(ref)
            assert h[tag + "/num"] == want_h["num"]
            assert abs(h[tag + "/sum"] - want_h["sum"]) <= TOL * max(1.0, abs(want_h["sum"]), want_h["num"])
            assert abs(h[tag + "/max"] - want_h["max"]) <= TOL * max(1.0, abs(want_h["max"]))
        assert abs(losses[2] - want["cost_v"]) <= TOL * max(1.0, want["cost_v"])
    finally:
        net.close()


@pytest.mark.timeout(180)
def test_server_drives_the_net_with_the_native_loops(tmp_path, monkeypatch):
    import ga3c_amd  # noqa: F401
    from Config import Config
    monkeypatch.chdir(tmp_path)
    for k, v in (("GAME", "Pendulum-v0"), ("AGENTS", 8), ("PREDICTORS", 2), ("TRAINERS", 2), ("TIME_MAX", 5),
                 ("DYNAMIC_SETTINGS", False), ("SAVE_MODELS", False), ("TRAINING_MIN_BATCH_SIZE", 0),
                 ("CONTINUOUS_INPUT", Config.CONTINUOUS_INPUT), ("DISCRATE_INPUT", Config.DISCRATE_INPUT)):
        monkeypatch.setattr(Config, k, v)
    from Server import Server
    import NetworkVP_vector
    srv = Server(max_agents=16)
    assert isinstance(srv.model, NetworkVP_vector.Network) and srv.zero_copy and not srv.state_cache
    srv.main(max_seconds=8)
    assert srv.failure is None and srv.training_step > 20 and srv.predictions_served > 1000
    assert srv.model.get_global_step() == srv.training_step
    assert open("results.txt").read().strip()


@pytest.mark.timeout(240)
def test_train_script_runs_pendulum(tmp_path):
    env = dict(os.environ, PYTHONUNBUFFERED="1")
    run = subprocess.run(["sh", os.path.join(PKG, "_train.sh"), "GAME=Pendulum-v0", "MAX_SECONDS=20", "AGENTS=16",
                          "PREDICTORS=2", "TRAINERS=2", "TIME_MAX=20", "SAVE_MODELS=", "DYNAMIC_SETTINGS="],
                         cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=200)
    assert run.returncode == 0, run.stdout[-3000:] + run.stderr[-3000:]
    assert "died" not in run.stdout + run.stderr
    tps = [int(t) for t in re.findall(r"TPS:\s*(\d+)\]", run.stdout)]
    assert tps and max(tps) > 0, run.stdout[-2000:]
    lines = open(os.path.join(str(tmp_path), "results.txt")).read().strip().splitlines()
    assert lines and all(int(ln.split(",")[2]) > 0 for ln in lines)
