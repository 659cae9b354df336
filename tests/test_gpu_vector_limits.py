"""-m gpu: the vector-state network of GAME = 'Pendulum-v0' (ga3c_mlp_*) at the limits of the shapes
ga3c_mlp_create admits and with a saturated angle head, against its f64 statements (tests/mlp_oracle.py,
tests/mlp_dual_oracle.py).  tests/test_gpu_vector_net.py and tests/test_gpu_vector_dual.py run (S, A) = (3, 1) and (7, 3); here
the three heads' [64, 1 + 2A] layer has up to 65 columns (a second wave, dense_bwd_split slices of 17 / 16 / 16 / 16 terms, the
dense14 delta 1040 floats into bufB), load_input_tile fills one float per row and all of xin, and the sigmoids of the head
reach exactly 0 and exactly 1.  The cases and the conditions that make them worth running are tests/vector_limit_cases.py's
(tests/test_vector_limits_cpu.py asserts them without a GPU; each test here asserts them again before it looks at the device).

Tolerances: 1e-4 x max(1, max|want|) (1e-5 after two steps), the project's rule, and every delta and gradient once more
through tests/closeness.py: rel_err against max(16 x e32, 2^-20), e32 from the oracle run in float32 on the same rows."""
import contextlib
import functools

import numpy as np
import pytest

import closeness as c
import mlp_dual_oracle as d
import mlp_oracle as m
import vector_limit_cases as vc
from vector_limit_cases import close as _close, config as _config, e32 as _e32, mask as _mask, reset as _reset

pytestmark = pytest.mark.gpu

TOL = 1e-4
BETA = vc.BETA
ACTS = (("x", None), ("pd1", 4), ("pd2", 256), ("pd3", 256), ("pd4", 100), ("d1", 64), ("v", 1), ("p", "A"), ("z", "2A"))
DELTAS = (("dv", 1), ("dz", "2A"), ("dd1", 64), ("dpd4", 100), ("dpd3", 256), ("dpd2", 256), ("dpd1", 4))
TRUNK_DELTAS = tuple(t for t in DELTAS if t[0] not in ("dv", "dz"))
DUAL_SHAPES = [(64, 32), (1, 32), (64, 1)]
DUAL_SIZES = [1, 17, 132]
STEP_SHAPES = [(64, 32), (1, 1)]
STEP_SIZES = (132, 17)
# tf.clip_by_average_norm: ||g|| / n is above CLIP for every variable, asserted from the oracle's gradients at every step (its
# smallest is 1.7e-4, dense13_p/w at S = 64, A = 32, B = 17; tests/test_gpu_vector_net.py's 2e-4 would leave that one unclipped).
# A clipped variable of n entries moves by about lr x CLIP x sqrt(n): 2.4e-5 for dense13_p/w, so 1e-5 sees the wide trunk
# layers' steps and not the heads'; a smaller norm would leave nothing to see.
CLIP = 1e-4
# A tensor whose kernel needs more than closeness.FACTOR has its factor here, with the reason from its summation length.
# dv and logits_v/b on a batch of ONE row, and only there: both are then ONE element, dv = v - y_r with v = b + sum_k d1_k Wv_k
# over K = 64 products, and logits_v/b the "sum" of that one element, so closeness.e32_of_row_sum hands the same single draw
# back.  A single draw of the float32 oracle can come out at one rounding of the result (seen over the six shapes: 3e-9 ..
# 1e-6), while another order of the same K terms has the typical error of the sum, about sqrt(K) roundings: sqrt(64) = 8 on top
# of the 16 that every tensor has.  Needed: 21.2 (S = 1, A = 32: dv at rel_err 1.52e-6 = 3.8 ulp of v = 1.23, e32 7.2e-8).
ONE_ROW_FACTOR = {"dv": c.FACTOR * 8.0, "logits_v/b": c.FACTOR * 8.0}
TENSOR_FACTOR = {}          # at every other size: none needed


def _width(w, S, A):
    return {None: S, "A": A, "2A": 2 * A}.get(w, w)


def _net(state_dim, num_actions, dual=False, **kw):
    import ga3c_amd  # noqa: F401  (puts the flat modules on sys.path)
    from NetworkVP_vector import Network
    with _config(DUAL_RMSPROP=dual, **kw):
        return Network("gpu:0", "veclim", num_actions, (state_dim,), max_batch=vc.MAX_BATCH)


@contextlib.contextmanager
def _nets(*makers):
    """The handles that `makers` (calls of _net, not yet made) create, every one that came to exist closed at the end."""
    nets = []
    try:
        for make in makers:
            nets.append(make())
        yield nets
    finally:
        for n in nets:
            n.close()


def _make(*args, **kw):
    return functools.partial(_net, *args, **kw)


def _vars(net, arena):
    return {k: arena[net._offsets[k][0]:net._offsets[k][0] + net._offsets[k][1]] for k in m.PARAM_ORDER}


def _grads32(fn, params, x, y, a):
    """The oracle `fn` in float32 on the same rows (expf overflows where the sigmoid is exactly 0: that is the case)."""
    with np.errstate(over="ignore"):
        return fn(vc.f32_params(params), x, y, a, BETA)


@functools.lru_cache(maxsize=None)
def _oracle(S, A, bsz):
    """(forward, losses, g, g32) of the single-optimizer network on limit_batch(S, A, bsz); shared, never written to."""
    params = vc.limit_params(S, A)
    x, y, a = vc.limit_batch(S, A, bsz)
    f = m.forward(params, x.astype(np.float64))
    want, g = m.loss_and_grads(params, *vc.f64(x, y, a), BETA)
    return f, want, g, _grads32(m.loss_and_grads, params, x, y, a)[1]


@functools.lru_cache(maxsize=None)
def _dual_oracle(S, A, bsz):
    params = vc.limit_params(S, A)
    x, y, a = vc.limit_batch(S, A, bsz)
    want, gp, gv = d.dual_grads(params, *vc.f64(x, y, a), BETA)
    _, gp32, gv32 = _grads32(d.dual_grads, params, x, y, a)
    return want, gp, gv, gp32, gv32


def _check_losses(losses, want, where):
    for got, key in zip(losses, ("cost_p_1_agg", "cost_p_2_agg", "cost_v")):
        assert np.isfinite(got) and abs(got - want[key]) <= TOL * max(1.0, abs(want[key])), (where, key, got, want[key])


def _relative(case, got, g, g32, A, failed, bsz):
    """Every tensor of `got` through closeness: one printed line each, the misses appended to `failed`.  e32 is
    vector_limit_cases.e32 (a bias gradient of ONE element: the larger of its single draw and closeness.e32_of_row_sum of the
    delta it sums); the factor is closeness.FACTOR but for ONE_ROW_FACTOR at bsz = 1."""
    for name, val in got.items():
        assert np.asarray(g32[name]).dtype == np.float32, name
        e32 = _e32(name, g32, g, g32, g, A)
        factor = ONE_ROW_FACTOR.get(name, c.FACTOR) if bsz == 1 else TENSOR_FACTOR.get(name, c.FACTOR)
        assert bsz != 1 or name not in ONE_ROW_FACTOR or np.size(g[name]) == 1
        bound = max(factor * e32, c.FLOOR)
        err = c.report(case, name, val, g[name], e32, bound)
        if not err <= bound:
            failed.append((case, name, err, bound))


def _fetch(net, names, bsz, S, A, suffix=""):
    return {name: net.fetch(name + suffix, bsz * _width(w, S, A)) for name, w in names}


# ---- 1, 2: the single-optimizer network at every (shape, size)
@pytest.mark.parametrize("state_dim,num_actions", vc.SHAPES)
def test_forward_losses_and_gradients_against_the_oracle(state_dim, num_actions):
    S, A = state_dim, num_actions
    params = vc.limit_params(S, A)
    for bsz in vc.SIZES:
        vc.check_kept(S, A, bsz)
    with _nets(_make(S, A)) as (net,):
        _reset(net, params, dual=False)
        assert net.param_count == m.param_count(S, A)
        net.beta = BETA
        for bsz in vc.SIZES:
            x, y, a = vc.limit_batch(S, A, bsz)
            f, want, g, _ = _oracle(S, A, bsz)
            p, v, z = net.predict_p_v_logits(x)
            assert p.shape == (bsz, A) and z.shape == (bsz, 2 * A)
            assert _close(p, f["o"]) and _close(v, f["v"]) and _close(z, f["z"]), bsz
            _check_losses(net.compute_grads(x, y, a), want, bsz)
            for name, val in _fetch(net, ACTS, bsz, S, A).items():
                assert _close(val, f["o"] if name == "p" else f[name]), (bsz, name)
            for name, val in _fetch(net, DELTAS, bsz, S, A).items():
                assert _close(val, g[name]), (bsz, name)
            grad = net.get_arena(3)
            assert np.all(np.isfinite(grad))
            for k, val in _vars(net, grad).items():
                assert _close(val, g[k]), (bsz, k)


@pytest.mark.parametrize("state_dim,num_actions", vc.SHAPES)
def test_backward_tensors_relative_to_their_largest_entry(state_dim, num_actions):
    """Every delta and gradient with tests/closeness.py.  A bias gradient of ONE element (logits_v/b; out_x/b and out_y/b
    when A = 1) takes the larger of its single draw and what the float32 error of the delta it sums implies
    (closeness.e32_of_row_sum), as in tests/test_gpu_vector_net.py."""
    S, A = state_dim, num_actions
    params = vc.limit_params(S, A)
    for bsz in vc.SIZES:
        vc.check_kept(S, A, bsz)
        vc.no_zero_tensor(_oracle(S, A, bsz)[2], tuple(n for n, _ in DELTAS) + m.PARAM_ORDER, (S, A, bsz))
    with _nets(_make(S, A)) as (net,):
        _reset(net, params, dual=False)
        net.beta = BETA
        failed = []
        for bsz in vc.SIZES:
            x, y, a = vc.limit_batch(S, A, bsz)
            _, _, g, g32 = _oracle(S, A, bsz)
            net.compute_grads(x, y, a)
            got = _fetch(net, DELTAS, bsz, S, A)
            got.update(_vars(net, net.get_arena(3)))
            _relative("limits S=%d A=%d B=%d" % (S, A, bsz), got, g, g32, A, failed, bsz)
        assert not failed, failed


# ---- 3: two optimizers
@pytest.mark.parametrize("state_dim,num_actions", DUAL_SHAPES)
def test_dual_both_costs_against_the_oracle_and_the_single_networks_bits(state_dim, num_actions):
    """Both costs' deltas and gradients (arenas 3 and 6) against mlp_dual_oracle by both comparators, exact zeros where a cost
    has no path, and forward, losses, dv, dz and the head gradients bit-equal to a single-optimizer handle on the same rows."""
    S, A = state_dim, num_actions
    params = vc.limit_params(S, A)
    for bsz in DUAL_SIZES:
        vc.check_kept(S, A, bsz)
        _, gp, gv, _, _ = _dual_oracle(S, A, bsz)
        vc.no_zero_tensor(gp, tuple(k for k in d.DELTAS + ("dz",) + m.PARAM_ORDER if k not in d.HEAD_V), (S, A, bsz, "p"))
        vc.no_zero_tensor(gv, tuple(k for k in d.DELTAS + ("dv",) + m.PARAM_ORDER if k not in d.HEAD_P), (S, A, bsz, "v"))
    with _nets(_make(S, A, dual=True), _make(S, A)) as (dual, single):
        _reset(dual, params)
        _reset(single, params, dual=False)
        dual.beta = single.beta = BETA
        head_v, head_p = _mask(dual, d.HEAD_V), _mask(dual, d.HEAD_P)
        failed = []
        for bsz in DUAL_SIZES:
            x, y, a = vc.limit_batch(S, A, bsz)
            want, gp, gv, gp32, gv32 = _dual_oracle(S, A, bsz)
            for u, w in zip(dual.predict_p_v_logits(x), single.predict_p_v_logits(x)):
                assert np.array_equal(u, w), bsz
            losses = dual.compute_grads(x, y, a)
            assert np.array_equal(losses, single.compute_grads(x, y, a)), bsz
            _check_losses(losses, want, bsz)
            for name, width in (("dv", 1), ("dz", 2 * A), ("pd3", 256), ("d1", 64), ("lossrow", 3)):
                assert np.array_equal(dual.fetch(name, bsz * width), single.fetch(name, bsz * width)), (bsz, name)
            g_single, arena = single.get_arena(3), {"p": dual.get_arena(3), "v": dual.get_arena(6)}
            assert np.array_equal(arena["v"][head_v], g_single[head_v]) and np.any(arena["v"][head_v]), bsz
            assert np.array_equal(arena["p"][head_p], g_single[head_p]) and np.any(arena["p"][head_p]), bsz
            for cost, g, g32, suffix, no_path in (("p", gp, gp32, "", d.HEAD_V), ("v", gv, gv32, "_v", d.HEAD_P)):
                got = _fetch(dual, TRUNK_DELTAS, bsz, S, A, suffix)
                got["dz" if cost == "p" else "dv"] = dual.fetch("dz", bsz * 2 * A) if cost == "p" else dual.fetch("dv", bsz)
                got.update(_vars(dual, arena[cost]))
                for name in no_path:                                   # exactly zero, no tolerance
                    val = got.pop(name)
                    assert not np.any(g[name]) and np.array_equal(val, np.zeros(val.size, np.float32)), (bsz, cost, name)
                for name, val in got.items():
                    assert np.all(np.isfinite(val)) and _close(val, g[name]), (bsz, cost, name)
                _relative("limits dual S=%d A=%d B=%d cost_%s" % (S, A, bsz, cost), got, g, g32, A, failed, bsz)
        assert not failed, failed


# ---- 4: two production steps
def _random_slots(net, params, seed):
    """(ms0, mom0) arenas and the same values as the oracle's dicts."""
    rng = np.random.default_rng(seed)
    ms0 = rng.uniform(0.5, 1.5, net.param_count).astype(np.float32)
    mom0 = rng.uniform(-1e-3, 1e-3, net.param_count).astype(np.float32)
    ms, mom = ({k: v.astype(np.float64).reshape(params[k].shape) for k, v in _vars(net, flat).items()} for flat in (ms0, mom0))
    return ms0, mom0, ms, mom


@pytest.mark.parametrize("kind", ["plain", "clip", "momentum", "dual"])
@pytest.mark.parametrize("state_dim,num_actions", STEP_SHAPES)
def test_two_train_steps_against_the_oracle(state_dim, num_actions, kind):
    """B = 132, then 17, from random ms and mom (both optimizers' when there are two).

    The clipped variant also holds every variable's two steps to that variable's own largest step, because 1e-5 sees only
    the wide trunk layers there (CLIP above): max|step - want| / max|want| against
        2^-23 max|theta| / max|want|  +  2 x max(16 x e32, 2^-20).
    First term: theta is float32 and each of the two updates rounds it to within half an ulp, 2^-24 |theta|.  Second: the step
    is lr g s / sqrt(ms + eps) with s = clip n / ||g||; g and its norm are each within the relative test's bound of this
    variable's gradient, e32 the larger of the two batches'.  (Where a variable's step is below theta's ulp -- the head biases
    at A = 1 -- the first term passes 1 and the line says nothing; the float32 oracle sits at 0.6 .. 0.75 of the bound.)"""
    S, A = state_dim, num_actions
    dual = kind == "dual"
    clip = CLIP if kind == "clip" else None
    momentum = 0.9 if kind == "momentum" else 0.0
    params = vc.limit_params(S, A)
    for step, bsz in enumerate(STEP_SIZES):
        vc.check_kept(S, A, bsz, seed=7 + step)
    with _nets(_make(S, A, dual=dual, USE_GRAD_CLIP=kind == "clip", GRAD_CLIP_NORM=clip or 40.0,
                    RMSPROP_MOMENTUM=momentum)) as (net,):
        theta0 = m.flat(params).astype(np.float32)
        net.set_arena(0, theta0)
        ms0, mom0, ms, mom = _random_slots(net, params, 3)
        net.set_arena(1, ms0)
        net.set_arena(2, mom0)
        if dual:
            ms0_v, mom0_v, ms_v, mom_v = _random_slots(net, params, 4)
            net.set_arena(4, ms0_v)
            net.set_arena(5, mom0_v)
            slots = {"ms_p": ms, "mom_p": mom, "ms_v": ms_v, "mom_v": mom_v}
        net.learning_rate, net.beta = 1e-3, BETA
        ref = {k: v.copy() for k, v in params.items()}
        e32 = dict.fromkeys(m.PARAM_ORDER, 0.0)
        for step, bsz in enumerate(STEP_SIZES):
            x, y, a = vc.batch(params, bsz, S, A, 7 + step)
            net.train(x, y, a)
            if dual:
                _, gp, gv = d.dual_grads(ref, *vc.f64(x, y, a), BETA)
                d.dual_rmsprop_update(ref, slots, gp, gv, 1e-3)
            else:
                _, g = m.loss_and_grads(ref, *vc.f64(x, y, a), BETA)
                if kind == "clip":
                    assert all(np.sqrt(np.sum(g[k] ** 2)) / g[k].size > 1.5 * clip for k in m.PARAM_ORDER), (step, bsz)
                    _, g32 = _grads32(m.loss_and_grads, ref, x, y, a)
                    e32 = {k: max(e32[k], _e32(k, g32, g, g32, g, A)) for k in m.PARAM_ORDER}
                m.rmsprop_update(ref, ms, g, 1e-3, momentum=momentum, mom=mom, clip=clip)
        assert net.get_global_step() == 2
        theta = net.get_arena(0)
        assert np.all(np.isfinite(theta)) and not np.array_equal(theta, theta0)
        assert _close(theta, m.flat(ref), 1e-5)
        assert _close(net.get_arena(1), m.flat(ms), 1e-5)
        if kind == "clip":
            failed = []
            for k, got in _vars(net, theta0.astype(np.float64) - theta).items():
                want = (params[k] - ref[k]).reshape(-1)
                bound = 2.0 ** -23 * np.max(np.abs(params[k])) / np.max(np.abs(want)) + 2.0 * max(c.FACTOR * e32[k], c.FLOOR)
                err = c.rel_err(got, want)
                print("clipped steps S=%d A=%d %-18s max|step| %.2e  rel_err %.3e  bound %.3e" % (S, A, k, np.max(np.abs(want)), err,
                                                                                               bound))
                if not err <= bound:
                    failed.append((k, err, bound))
            assert not failed, failed
        if kind == "momentum":
            assert _close(net.get_arena(2), m.flat(mom), 1e-5)
        else:
            assert np.array_equal(net.get_arena(2), mom0)                # momentum 0 never touches the slot
        if dual:
            assert _close(net.get_arena(4), m.flat(ms_v), 1e-5)
            assert np.array_equal(net.get_arena(5), mom0_v)
            head_v, head_p = _mask(net, d.HEAD_V), _mask(net, d.HEAD_P)    # no slot there: every bit as it was
            assert np.array_equal(net.get_arena(1)[head_v], ms0[head_v]) and np.array_equal(net.get_arena(4)[head_p], ms0_v[head_p])
            trunk = _mask(net, d.TRUNK_VARS)
            assert np.mean(net.get_arena(1)[trunk] != ms0[trunk]) > 0.999 and np.mean(net.get_arena(4)[trunk] != ms0_v[trunk]) > 0.999


# ---- 5: bit-reproducibility
@pytest.mark.parametrize("clip", [False, True])
def test_split_step_and_repeated_calls_are_bit_identical(clip):
    S, A, bsz = 64, 32, 132
    params = vc.limit_params(S, A)
    vc.check_kept(S, A, bsz, seed=99)
    kw = {"USE_GRAD_CLIP": clip, "GRAD_CLIP_NORM": CLIP}
    with _nets(_make(S, A, **kw), _make(S, A, **kw)) as (a_net, b_net):
        x, y, a = vc.batch(params, bsz, S, A, 99)
        for n in (a_net, b_net):
            _reset(n, params, dual=False)
            n.learning_rate, n.beta = 1e-3, BETA
        g1 = (b_net.compute_grads(x, y, a), b_net.get_arena(3))
        g2 = (b_net.compute_grads(x, y, a), b_net.get_arena(3))
        assert np.array_equal(g1[0], g2[0]) and np.array_equal(g1[1], g2[1])      # no float atomics anywhere
        assert np.any(g1[1]) and b_net.get_global_step() == 0
        b_net.apply_grads()
        a_net.train(x, y, a)
        for w in (0, 1, 2, 3):
            assert np.array_equal(a_net.get_arena(w), b_net.get_arena(w)), w
        assert not np.array_equal(a_net.get_arena(0), m.flat(params).astype(np.float32))
        assert a_net.get_global_step() == b_net.get_global_step() == 1


# ---- 6: rows gathered out of the transport
@pytest.mark.parametrize("state_dim,num_actions", [(64, 32), (1, 32)])
def test_gather_entries_are_bit_equal_to_host_buffers(state_dim, num_actions):
    """Agent slots and rollout rows of 256 bytes and of 4 bytes (S = 1: four rows to a 16-byte line) read out of the registered
    transport give the bits the host-buffer entry points give on a second handle."""
    import ga3c_amd  # noqa: F401
    import Transport as tp
    S, A, bsz = state_dim, num_actions, 37
    params = vc.limit_params(S, A)
    vc.check_kept(S, A, bsz, seed=5)
    t = tp.Transport.create(tp.unique_name("t_veclim"), 40, A, 4 * S, 8, 40, float_actions=True)
    try:
        with _nets(_make(S, A), _make(S, A)) as (n1, n2):
            for n in (n1, n2):
                _reset(n, params, dual=False)
                n.learning_rate, n.beta = 1e-3, BETA
            x, y, a = vc.batch(params, bsz, S, A, 5)
            ids = np.arange(bsz, dtype=np.uint32)[::-1].copy()
            for i, agent in enumerate(ids):
                t.state_view(int(agent), np.float32)[:] = x[i]
            n1.register_transport(t)
            p1, v1 = n1.predict_offsets(t.state_offsets(ids))
            p2, v2 = n2.predict_p_and_v(x)
            assert np.array_equal(p1, p2) and np.array_equal(v1, v2) and np.any(p1)
            slot = t.acquire(1000)
            states, _, _ = t.rollout_views(slot)
            for i in range(bsz):
                states[i] = x[i].view(np.uint8)
            t.commit(slot, bsz)
            got = t.pop_rollout(1000)
            offs = t.rollout_row_offsets(got, bsz)
            assert np.all(offs % 4 == 0) and (S != 1 or np.any(offs % 16 != 0))
            loss1 = n1.evaluate(None, y, a, offsets=offs)
            loss2 = n2.evaluate(x, y, a)
            assert all(np.array_equal(u, w) for u, w in zip(loss1, loss2))
            n1.train_offsets(offs, y, a)
            n2.train(x, y, a)
            assert np.array_equal(n1.last_losses, n2.last_losses)
            for w in (0, 1, 3):
                assert np.array_equal(n1.get_arena(w), n2.get_arena(w)), w
            assert n1.get_global_step() == n2.get_global_step() == 1
            t.release(got)
            n1.unregister_transport()
    finally:
        t.shutdown()
        t.close()


# ---- 7: the saturated head
def _saturated_case(S, A):
    """-> (params, rows, forward, losses, g, g32, where the float32 sigmoids are exactly 0 or 1 [B, 2A])."""
    vc.check_saturated(S, A)
    params = vc.saturated_params(S, A)
    x, y, a = vc.saturated_batch(S, A)
    f = m.forward(params, x.astype(np.float64))
    want, g = m.loss_and_grads(params, *vc.f64(x, y, a), BETA)
    vc.no_zero_tensor(g, tuple(n for n, _ in DELTAS) + m.PARAM_ORDER, (S, A))
    with np.errstate(over="ignore"):
        f32 = m.forward(vc.f32_params(params), x)
    s32 = np.concatenate([f32["sx"], f32["sy"]], axis=1)
    flat = (s32 == 0.0) | (s32 == 1.0)
    assert np.any(s32 == 0.0) and np.any(s32 == 1.0) and not np.all(flat)
    return params, (x, y, a), f, want, g, _grads32(m.loss_and_grads, params, x, y, a)[1], flat


@pytest.mark.parametrize("state_dim,num_actions", vc.SATURATED)
def test_saturated_head_against_the_oracle(state_dim, num_actions):
    """logits_p/out_x/w and out_y/w x 100: sigm(h) is exactly 1 beyond |h| of about 17 and exactly 0 below about -88.7, where
    expf(-h) overflows; sx (1 - sx) is then exactly 0 while X or Y sit at exactly +-0.5.  Forward, every delta
    and gradient by both comparators, exact zeros of dz where the float32 sigmoid has no slope, and two production steps."""
    S, A = state_dim, num_actions
    params, (x, y, a), f, want, g, g32, flat = _saturated_case(S, A)
    with _nets(_make(S, A)) as (net,):
        _reset(net, params, dual=False)
        net.learning_rate, net.beta = 1e-3, BETA
        p, v, z = net.predict_p_v_logits(x)
        assert all(np.all(np.isfinite(t)) for t in (p, v, z))
        assert _close(p, f["o"]) and _close(v, f["v"]) and _close(z, f["z"])
        _check_losses(net.compute_grads(x, y, a), want, "saturated")
        got = _fetch(net, DELTAS, vc.SAT_B, S, A)
        got.update(_vars(net, net.get_arena(3)))
        for name, val in got.items():
            assert np.all(np.isfinite(val)) and _close(val, g[name]), name
        dz = got["dz"].reshape(vc.SAT_B, 2 * A)
        print("saturated S=%d A=%d: %d of %d float32 sigmoids are exactly 0 or 1" % (S, A, int(flat.sum()), flat.size))
        assert not np.any(dz[flat]) and np.any(dz[~flat])
        failed = []
        _relative("saturated S=%d A=%d B=%d" % (S, A, vc.SAT_B), got, g, g32, A, failed, vc.SAT_B)
        assert not failed, failed
        # two production steps from ms = 1, mom = 0
        _reset(net, params, dual=False)
        ref = {k: t.copy() for k, t in params.items()}
        ms = {k: np.ones_like(t) for k, t in params.items()}
        for step in range(2):
            vc.check_kept(S, A, vc.SAT_B, params, 30 + step)
            xb, yb, ab = vc.batch(params, vc.SAT_B, S, A, 30 + step)
            net.train(xb, yb, ab)
            _, gs = m.loss_and_grads(ref, *vc.f64(xb, yb, ab), BETA)
            m.rmsprop_update(ref, ms, gs, 1e-3)
        assert np.all(np.isfinite(net.get_arena(0))) and np.all(np.isfinite(net.get_arena(1)))
        assert _close(net.get_arena(0), m.flat(ref), 1e-5) and _close(net.get_arena(1), m.flat(ms), 1e-5)


def test_saturated_head_with_two_optimizers():
    """The saturated rows with one optimizer per cost: forward, then arenas 3 and 6 and both delta streams finite and within
    both bounds, then two production steps: theta and the value optimizer's ms to 1e-5, every arena finite.  The policy
    optimizer's ms is held to finiteness only: alone, without the value cost's large entries beside it, it is 0.99 + 0.01 g^2
    of gradients whose float32 error is 1e-5 of themselves in this regime, and the oracle run in float32 is itself 3.0e-4
    off where 1e-5 x max|want| allows 1.4e-4."""
    S, A = 64, 32
    params, (x, y, a), f, want, _, _, flat = _saturated_case(S, A)
    _, gp, gv = d.dual_grads(params, *vc.f64(x, y, a), BETA)
    _, gp32, gv32 = _grads32(d.dual_grads, params, x, y, a)
    with _nets(_make(S, A, dual=True)) as (net,):
        _reset(net, params)
        net.learning_rate, net.beta = 1e-3, BETA
        p, v, z = net.predict_p_v_logits(x)
        assert all(np.all(np.isfinite(t)) for t in (p, v, z))
        assert _close(p, f["o"]) and _close(v, f["v"]) and _close(z, f["z"])
        _check_losses(net.compute_grads(x, y, a), want, "saturated dual")
        assert not np.any(net.fetch("dz", vc.SAT_B * 2 * A).reshape(vc.SAT_B, 2 * A)[flat])
        failed = []
        for cost, g, g32, which, suffix, no_path in (("p", gp, gp32, 3, "", d.HEAD_V), ("v", gv, gv32, 6, "_v", d.HEAD_P)):
            arena = net.get_arena(which)
            assert np.all(np.isfinite(arena))
            got = _fetch(net, TRUNK_DELTAS, vc.SAT_B, S, A, suffix)
            got.update(_vars(net, arena))
            for name in no_path:
                assert not np.any(g[name]) and not np.any(got.pop(name)), (cost, name)
            for name, val in got.items():
                assert np.all(np.isfinite(val)) and _close(val, g[name]), (cost, name)
            _relative("saturated dual S=%d A=%d B=%d cost_%s" % (S, A, vc.SAT_B, cost), got, g, g32, A, failed, vc.SAT_B)
        assert not failed, failed
        ref = {k: t.copy() for k, t in params.items()}
        slots = d.init_slots(ref)
        for step in range(2):
            xb, yb, ab = vc.batch(params, vc.SAT_B, S, A, 30 + step)
            net.train(xb, yb, ab)
            _, sp, sv = d.dual_grads(ref, *vc.f64(xb, yb, ab), BETA)
            d.dual_rmsprop_update(ref, slots, sp, sv, 1e-3)
        assert net.get_global_step() == 2
        assert all(np.all(np.isfinite(net.get_arena(w))) for w in (0, 1, 2, 4, 5))
        assert _close(net.get_arena(0), m.flat(ref), 1e-5) and _close(net.get_arena(4), m.flat(slots["ms_v"]), 1e-5)
        head_v = _mask(net, d.HEAD_V)
        assert np.array_equal(net.get_arena(1)[head_v], np.ones(int(head_v.sum()), np.float32))
        assert np.mean(net.get_arena(1)[~head_v] != 1.0) > 0.99
