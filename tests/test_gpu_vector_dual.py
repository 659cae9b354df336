"""-m gpu: Config.DUAL_RMSPROP on the vector-state network of GAME = 'Pendulum-v0' (ga3c_mlp_* with GA3C_FLAG_DUAL_RMSPROP,
DESIGN.md 8h) against its f64 statement (tests/mlp_dual_oracle.py), and bit for bit against the single-optimizer network
where the two must agree.  Parameters and batches are built as tests/test_gpu_vector_net.py builds them: init_params(seed =
777), widened head biases, and every batch away from the atan2 branch cut.  Absolute tolerance: 1e-4 x max(1, max|want|), as
there; every per-cost tensor is also held relative to its own largest entry (tests/closeness.py), because the policy cost's
tensors are small (norms 0.016 .. 0.45 at S = 3, B = 132 against 4.7 .. 214 for the value cost)."""
import ctypes as C
import functools

import numpy as np
import pytest

import closeness as c
import mlp_oracle as m
import mlp_dual_oracle as d
import vector_limit_cases as vc
from vector_limit_cases import close as _close, config as _config, e32 as _e32, mask as _mask, reset as _reset

pytestmark = pytest.mark.gpu

TOL = 1e-4
SIZES = [1, 15, 16, 17, 33, 132]        # the tile is 16 rows: one row, a tile short by one, full, plus one, 2 + 1, 8 tiles + 4
SHAPES = [(3, 1), (7, 3)]
MAX_BATCH = 256
BETA = 0.01
DELTAS = ("dd1", "dpd4", "dpd3", "dpd2", "dpd1")
WIDTHS = {"dd1": 64, "dpd4": 100, "dpd3": 256, "dpd2": 256, "dpd1": 4}
# A tensor whose kernel needs more than closeness.FACTOR would get its factor here, with the reason from its summation
# length beside it.  None does.
TENSOR_FACTOR = {}


def _net(state_dim, num_actions, dual=True, **kw):
    import ga3c_amd  # noqa: F401  (puts the flat modules on sys.path)
    from NetworkVP_vector import Network
    with _config(DUAL_RMSPROP=dual, **kw):
        return Network("gpu:0", "vecdual", num_actions, (state_dim,), max_batch=MAX_BATCH)


@functools.lru_cache(maxsize=None)
def _params(state_dim, num_actions):
    return vc.params(state_dim, num_actions)


@functools.lru_cache(maxsize=None)
def _batch(bsz, state_dim, num_actions, seed):
    return vc.batch(_params(state_dim, num_actions), bsz, state_dim, num_actions, seed)


def _f64(x, y, a):
    return x.astype(np.float64), y.astype(np.float64), a.astype(np.float64)


def _no_slot_regions_untouched(net):
    """The policy optimizer has no slot on logits_v/*, the value optimizer none on logits_p/*: ms = 1, mom = 0, bit for bit."""
    head_v, head_p = _mask(net, d.HEAD_V), _mask(net, d.HEAD_P)
    for which, mask, want in ((1, head_v, 1.0), (2, head_v, 0.0), (4, head_p, 1.0), (5, head_p, 0.0)):
        assert np.array_equal(net.get_arena(which)[mask], np.full(int(mask.sum()), want, np.float32)), which


# ---- gradients against the dual oracle
@pytest.mark.parametrize("state_dim,num_actions", SHAPES)
def test_both_costs_deltas_and_gradients_against_the_oracle(state_dim, num_actions):
    S, A = state_dim, num_actions
    params = _params(S, A)
    p32 = {k: v.astype(np.float32) for k, v in params.items()}
    net = _net(S, A)
    try:
        _reset(net, params)
        net.beta = BETA
        failed = []
        for bsz in SIZES:
            x, y, a = _batch(bsz, S, A, 100 + bsz)
            losses = net.compute_grads(x, y, a)
            want, gp, gv = d.dual_grads(params, *_f64(x, y, a), BETA)
            _, gp32, gv32 = d.dual_grads(p32, x, y, a, BETA)
            for got, key in zip(losses, ("cost_p_1_agg", "cost_p_2_agg", "cost_v")):
                assert abs(got - want[key]) <= TOL * max(1.0, abs(want[key])), (bsz, key, got, want[key])
            arena = {"p": net.get_arena(3), "v": net.get_arena(6)}
            for cost, g, g32, suffix in (("p", gp, gp32, ""), ("v", gv, gv32, "_v")):
                got = {name: net.fetch(name + suffix, bsz * WIDTHS[name]) for name in DELTAS}
                got["dz" if cost == "p" else "dv"] = net.fetch("dz", bsz * 2 * A) if cost == "p" else net.fetch("dv", bsz)
                for k in m.PARAM_ORDER:
                    off, size = net._offsets[k]
                    got[k] = arena[cost][off:off + size]
                for name, val in got.items():
                    if name in (d.HEAD_V if cost == "p" else d.HEAD_P):
                        assert not np.any(g[name]) and np.array_equal(val, np.zeros(val.size, np.float32)), (bsz, cost, name)
                        continue
                    assert _close(val, g[name]), (bsz, cost, name)
                    assert np.asarray(g32[name]).dtype == np.float32, name
                    e32 = _e32(name, g32, g, gv32 if cost == "v" else gp32, gv if cost == "v" else gp, A)
                    bound = max(TENSOR_FACTOR.get(name, c.FACTOR) * e32, c.FLOOR)
                    err = c.report("dual S=%d B=%d cost_%s" % (S, bsz, cost), name, val, g[name], e32, bound)
                    if not err <= bound:
                        failed.append((bsz, cost, name, err, bound))
        assert not failed, failed
    finally:
        net.close()


# ---- bit facts against the single-optimizer network
def test_forward_losses_head_deltas_and_head_gradients_are_the_single_networks_bits():
    S, A = 3, 1
    params = _params(S, A)
    dual, single = _net(S, A), _net(S, A, dual=False)
    try:
        _reset(dual, params)
        _reset(single, params, dual=False)
        dual.beta = single.beta = BETA
        head_v, head_p = _mask(dual, d.HEAD_V), _mask(dual, d.HEAD_P)
        for bsz in (33, 132):
            x, y, a = _batch(bsz, S, A, 100 + bsz)
            for u, w in zip(dual.predict_p_v_logits(x), single.predict_p_v_logits(x)):
                assert np.array_equal(u, w), bsz
            assert np.array_equal(dual.compute_grads(x, y, a), single.compute_grads(x, y, a)), bsz
            for name, width in (("dv", 1), ("dz", 2 * A), ("pd3", 256), ("d1", 64), ("lossrow", 3)):
                assert np.array_equal(dual.fetch(name, bsz * width), single.fetch(name, bsz * width)), (bsz, name)
            g_single, g_p, g_v = single.get_arena(3), dual.get_arena(3), dual.get_arena(6)
            assert np.array_equal(g_v[head_v], g_single[head_v]) and np.any(g_v[head_v]), bsz
            assert np.array_equal(g_p[head_p], g_single[head_p]) and np.any(g_p[head_p]), bsz
            assert np.array_equal(g_p[head_v], np.zeros(int(head_v.sum()), np.float32)), bsz
            assert np.array_equal(g_v[head_p], np.zeros(int(head_p.sum()), np.float32)), bsz
    finally:
        dual.close()
        single.close()


# ---- two production steps
KINDS = {"plain": {}, "momentum": {"RMSPROP_MOMENTUM": 0.9},
         "clip_all": {"USE_GRAD_CLIP": True, "GRAD_CLIP_NORM": 1e-3},
         "clip_none": {"USE_GRAD_CLIP": True, "GRAD_CLIP_NORM": 1e4},
         "clip_value_only": {"USE_GRAD_CLIP": True, "GRAD_CLIP_NORM": 1.0}}


@pytest.mark.parametrize("kind", list(KINDS))
def test_two_train_steps_against_the_oracle(kind):
    """B = 132, then 33.  The clip norms come from the oracle's own per-cost norms at S = 3, A = 1 (smallest 1.2e-2, largest
    3.5e2 over B = 1 .. 201): 1e-3 bites on every tensor of both costs, 1e4 on none, and 1.0 at B = 132 on every value
    tensor (norms >= 4.7) and on no policy tensor (<= 0.45).  Which tensors a norm bit is asserted from the oracle's norms,
    so a drifting fixture fails here instead of testing nothing.  (At the second step, B = 33, the value norms reach down
    to 0.71: there 1.0 is only asserted to bite on some value tensor and on no policy tensor.)"""
    S, A = 3, 1
    kw = dict({"USE_GRAD_CLIP": False, "GRAD_CLIP_NORM": 40.0, "RMSPROP_MOMENTUM": 0.0}, **KINDS[kind])
    clip = kw["GRAD_CLIP_NORM"] if kw["USE_GRAD_CLIP"] else None
    params = _params(S, A)
    net = _net(S, A, **kw)
    try:
        _reset(net, params)
        net.learning_rate, net.beta = 1e-3, BETA
        ref = {k: v.copy() for k, v in params.items()}
        slots = d.init_slots(ref)
        for step, bsz in enumerate((132, 33)):
            x, y, a = _batch(bsz, S, A, 7 + step)
            net.train(x, y, a)
            _, gp, gv = d.dual_grads(ref, *_f64(x, y, a), BETA)
            norm_p = [n for k, n in d.norms(gp).items() if k not in d.HEAD_V]
            norm_v = [n for k, n in d.norms(gv).items() if k not in d.HEAD_P]
            assert len(norm_p) == 14 and len(norm_v) == 12
            if kind == "clip_all":
                assert min(norm_p + norm_v) > 10 * clip, (step, min(norm_p + norm_v))
            elif kind == "clip_none":
                assert max(norm_p + norm_v) < 0.1 * clip, (step, max(norm_p + norm_v))
            elif kind == "clip_value_only":
                assert max(norm_p) < 0.7 * clip, (step, max(norm_p))
                if step == 0:
                    assert min(norm_v) > 4 * clip, min(norm_v)
                else:
                    assert max(norm_v) > 4 * clip, max(norm_v)
            d.dual_rmsprop_update(ref, slots, gp, gv, 1e-3, momentum=kw["RMSPROP_MOMENTUM"], clip=clip)
        assert net.get_global_step() == 2
        assert _close(net.get_arena(0), m.flat(ref), 1e-5)
        assert _close(net.get_arena(1), m.flat(slots["ms_p"]), 1e-5)
        assert _close(net.get_arena(4), m.flat(slots["ms_v"]), 1e-5)
        if kind == "momentum":
            assert _close(net.get_arena(2), m.flat(slots["mom_p"]), 1e-5)
            assert _close(net.get_arena(5), m.flat(slots["mom_v"]), 1e-5)
            assert np.any(net.get_arena(2)) and np.any(net.get_arena(5))
        _no_slot_regions_untouched(net)
        trunk = _mask(net, d.TRUNK_VARS)
        assert np.any(net.get_arena(1)[trunk] != 1.0) and np.any(net.get_arena(4)[trunk] != 1.0)
    finally:
        net.close()


# ---- bit-reproducibility
@pytest.mark.parametrize("clip", [False, True])
def test_split_step_and_repeated_calls_are_bit_identical(clip):
    S, A = 3, 1
    params = _params(S, A)
    kw = {"USE_GRAD_CLIP": clip, "GRAD_CLIP_NORM": 1.0}
    a_net, b_net = _net(S, A, **kw), _net(S, A, **kw)
    try:
        x, y, a = _batch(132, S, A, 99)
        for n in (a_net, b_net):
            _reset(n, params)
            n.learning_rate, n.beta = 1e-3, BETA
        g1 = (b_net.compute_grads(x, y, a), b_net.get_arena(3), b_net.get_arena(6))
        g2 = (b_net.compute_grads(x, y, a), b_net.get_arena(3), b_net.get_arena(6))
        assert all(np.array_equal(u, w) for u, w in zip(g1, g2))           # no float atomics anywhere
        assert b_net.get_global_step() == 0
        b_net.apply_grads()
        a_net.train(x, y, a)
        for w in (0, 1, 2, 3, 4, 5, 6):
            assert np.array_equal(a_net.get_arena(w), b_net.get_arena(w)), w
        assert not np.array_equal(a_net.get_arena(0), m.flat(params).astype(np.float32))
        assert a_net.get_global_step() == b_net.get_global_step() == 1
    finally:
        a_net.close()
        b_net.close()


# ---- transport
def test_train_offsets_on_unaligned_transport_rows_is_bit_equal_to_host_rows():
    import ga3c_amd  # noqa: F401
    import Transport as tp
    S, A = 3, 1
    params = _params(S, A)
    t = tp.Transport.create(tp.unique_name("t_vecdual"), 40, 1, 12, 8, 40, float_actions=True)
    n1, n2 = _net(S, A), _net(S, A)
    try:
        for n in (n1, n2):
            _reset(n, params)
            n.learning_rate, n.beta = 1e-3, BETA
        x, y, a = _batch(37, S, A, 5)
        n1.register_transport(t)
        slot = t.acquire(1000)
        states, _, _ = t.rollout_views(slot)
        for i in range(37):
            states[i] = x[i].view(np.uint8)
        t.commit(slot, 37)
        got = t.pop_rollout(1000)
        offs = t.rollout_row_offsets(got, 37)
        assert np.any(offs % 16 != 0)
        n1.train_offsets(offs, y, a)
        n2.train(x, y, a)
        assert np.array_equal(n1.last_losses, n2.last_losses)
        for w in (0, 1, 3, 4, 6):
            assert np.array_equal(n1.get_arena(w), n2.get_arena(w)), w
        assert n1.get_global_step() == n2.get_global_step() == 1
        t.release(got)
        n1.unregister_transport()
    finally:
        n1.close()
        n2.close()
        t.shutdown()
        t.close()


# ---- arenas and create
def test_arena_selectors_fetch_names_and_create_flags():
    import ga3c_amd  # noqa: F401
    import _native as nat
    S, A = 3, 1
    dual, single = _net(S, A), _net(S, A, dual=False)
    try:
        n = dual.param_count
        for which in (4, 5, 6):
            with pytest.raises(RuntimeError):
                single.get_arena(which)
            assert dual.get_arena(which).size == n
        for which in (3, 6, 7):
            with pytest.raises(RuntimeError):
                dual.set_arena(which, np.zeros(n, np.float32))
        with pytest.raises(RuntimeError):
            single.set_arena(4, np.ones(n, np.float32))
        assert np.array_equal(dual.get_arena(4), np.ones(n, np.float32)) and not np.any(dual.get_arena(5))
        dual.set_variable_value("dense1/b", np.full(64, 2.0, np.float32), which=4)
        assert np.array_equal(dual.get_variable_value("dense1/b", which=4), np.full(64, 2.0, np.float32))
        with pytest.raises(RuntimeError):
            dual.set_variable_value("dense1/b", np.zeros(64, np.float32), which=6)
        x, y, a = _batch(17, S, A, 117)
        for net in (dual, single):
            net.set_arena(0, m.flat(_params(S, A)))
            net.compute_grads(x, y, a)
        assert dual.fetch("dd1_v", 17 * 64).size == 17 * 64 and dual.fetch("dpd1_v", 17 * 4).size == 17 * 4
        for name, count in (("dd1_v", 17 * 64), ("dpd4_v", 17 * 100), ("dpd1_v", 17 * 4)):
            with pytest.raises(RuntimeError):
                single.fetch(name, count)
        for name in ("dv_v", "dz_v", "d1_v", "x_v"):
            with pytest.raises(RuntimeError):
                dual.fetch(name, 17)

        def rc(flags):
            cfg = nat.MlpConfig()
            cfg.device, cfg.state_dim, cfg.num_actions, cfg.max_batch, cfg.flags = 0, S, A, 16, flags
            cfg.rmsprop_decay, cfg.rmsprop_momentum, cfg.rmsprop_epsilon, cfg.grad_clip_norm = 0.99, 0.0, 0.1, 40.0
            cfg.predict_lanes = 1
            h = C.c_void_p()
            r = dual._lib.ga3c_mlp_create(C.byref(cfg), C.byref(h))
            if r == 0:
                dual._lib.ga3c_mlp_destroy(h)
            return r

        ok = nat.FLAG_CONTINUOUS | nat.FLAG_DUAL_RMSPROP
        assert rc(ok) == 0 and rc(ok | nat.FLAG_GRAD_CLIP) == 0
        assert rc(ok | 64) == -1 and rc(ok | nat.FLAG_LOG_SOFTMAX) == -1 and rc(nat.FLAG_DUAL_RMSPROP) == -1      # GA3C_EINVAL
    finally:
        dual.close()
        single.close()


# ---- checkpoint
def _member_names():
    names = {"step"}
    for k in m.PARAM_ORDER:
        names.add(k + ":0")
        if k in d.TRUNK_VARS:
            names.update(k + s for s in ("/RMSProp:0", "/RMSProp_1:0", "/RMSProp_2:0", "/RMSProp_3:0"))
        else:
            names.update(k + s for s in ("/RMSProp:0", "/RMSProp_1:0"))
    return names


def test_checkpoint_member_names_round_trip_and_refusals(tmp_path):
    S, A = 3, 1
    params = _params(S, A)
    net, other, single = _net(S, A, RMSPROP_MOMENTUM=0.9), _net(S, A, RMSPROP_MOMENTUM=0.9), _net(S, A, dual=False)
    try:
        _reset(net, params)
        _reset(single, params, dual=False)
        for n in (net, single):
            n.learning_rate, n.beta = 1e-3, BETA
            n.train(*_batch(33, S, A, 3))
        path, spath = str(tmp_path / "dual.npz"), str(tmp_path / "single.npz")
        assert net._lib.ga3c_mlp_save(net._h, path.encode()) == 0
        assert single._lib.ga3c_mlp_save(single._h, spath.encode()) == 0
        z = np.load(path)
        assert set(z.files) == _member_names()
        assert "logits_v/w/RMSProp_2:0" not in z.files and "logits_p/out_x/w/RMSProp_2:0" not in z.files
        assert int(z["step"]) == 1 and z["dense13_p/w/RMSProp_3:0"].shape == (256, 256)
        arenas = {w: net.get_arena(w) for w in (0, 1, 2, 4, 5)}
        for k in m.PARAM_ORDER:                          # which arena each member holds
            off, size = net._offsets[k]
            sl = slice(off, off + size)
            assert np.array_equal(z[k + ":0"].ravel(), arenas[0][sl]), k
            if k in d.TRUNK_VARS:
                pairs = ((4, "/RMSProp:0"), (5, "/RMSProp_1:0"), (1, "/RMSProp_2:0"), (2, "/RMSProp_3:0"))
            elif k in d.HEAD_V:
                pairs = ((4, "/RMSProp:0"), (5, "/RMSProp_1:0"))
            else:
                pairs = ((1, "/RMSProp:0"), (2, "/RMSProp_1:0"))
            for w, suffix in pairs:
                assert np.array_equal(z[k + suffix].ravel(), arenas[w][sl]), (k, suffix)
        assert np.any(arenas[2]) and np.any(arenas[5]) and not np.array_equal(arenas[1], arenas[4])
        assert other._lib.ga3c_mlp_load(other._h, path.encode()) == 0
        for w in (0, 1, 2, 4, 5):
            assert np.array_equal(other.get_arena(w), arenas[w]), w
        assert other.get_global_step() == 1
        # files of the other kind, both ways; the refused network keeps every arena and its step
        before = {w: other.get_arena(w) for w in (0, 1, 2, 4, 5)}
        assert other._lib.ga3c_mlp_load(other._h, spath.encode()) == -4            # GA3C_ESTATE: a single-optimizer file
        for w in before:
            assert np.array_equal(other.get_arena(w), before[w]), w
        sbefore = {w: single.get_arena(w) for w in (0, 1, 2)}
        assert single._lib.ga3c_mlp_load(single._h, path.encode()) == -4           # a dual file into one optimizer
        for w in sbefore:
            assert np.array_equal(single.get_arena(w), sbefore[w]), w
        assert other.get_global_step() == 1 and single.get_global_step() == 1
        assert set(np.load(spath).files) == {"step"} | {k + s for k in m.PARAM_ORDER for s in (":0", "/RMSProp:0", "/RMSProp_1:0")}
    finally:
        net.close()
        other.close()
        single.close()


# ---- Server
@pytest.mark.timeout(120)
def test_server_trains_pendulum_with_two_optimizers(tmp_path, monkeypatch):
    import ga3c_amd  # noqa: F401
    from Config import Config
    monkeypatch.chdir(tmp_path)
    for k, v in (("GAME", "Pendulum-v0"), ("DUAL_RMSPROP", True), ("AGENTS", 8), ("PREDICTORS", 2), ("TRAINERS", 2),
                 ("TIME_MAX", 5), ("DYNAMIC_SETTINGS", False), ("SAVE_MODELS", False), ("TRAINING_MIN_BATCH_SIZE", 0),
                 ("CONTINUOUS_INPUT", True), ("DISCRATE_INPUT", False)):
        monkeypatch.setattr(Config, k, v)
    from Server import Server
    import NetworkVP_vector
    srv = Server(max_agents=16)
    assert isinstance(srv.model, NetworkVP_vector.Network)
    srv.main(max_seconds=5)
    assert srv.failure is None and srv.training_step > 20
    net = srv.model
    assert net.get_global_step() == srv.training_step
    trunk, head_v = _mask(net, d.TRUNK_VARS), _mask(net, d.HEAD_V)
    assert np.mean(net.get_arena(4)[trunk] != 1.0) > 0.999
    assert np.array_equal(net.get_arena(1)[head_v], np.ones(int(head_v.sum()), np.float32))
    assert np.all(np.isfinite(net.get_arena(0)))
