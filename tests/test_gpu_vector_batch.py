"""-m gpu: the two vector-state networks (ga3c_mlp_*, ga3c_dmlp_*) from 1025 to 65536 rows, the max_batch their create calls
admit, against their f64 statements (tests/mlp_oracle.py, tests/mlp_dual_oracle.py, tests/dmlp_oracle.py).  The older files stop
at 1024 rows; the batch size is the dimension along which these kernels' arithmetic changes character (one chain of B terms per
gradient element and loss sum, up to 4096 workgroups of 16 rows, about 2000 floats of workspace per row).  The cases, the heavy-row
batches and the bounds are tests/vector_batch_cases.py's; tests/test_vector_batch_cpu.py asserts without a GPU what makes them
worth running.  One handle per (network, shape, head), created with max_batch = 65536, serves all its sizes.

Tolerances: 1e-4 x max(1, max|want|) (1e-5 after two steps), the project's rule, and every delta and gradient once more through
tests/closeness.py: rel_err against max(16 x e32, 2^-20), e32 from the oracle run in float32 on the same rows.

What these tests found at 65536 rows with the float32 chains the kernels had (tests/README.md has the figures): cost_p_2_agg of
the eight-layer net 6.4e-4 off its sum, and ms after two steps at 1.1 (momentum) and 1.3 (two optimizers) of 1e-5 x max(ms)."""
import numpy as np
import pytest

import closeness as c
import mlp_dual_oracle as d
import mlp_oracle as m
import vector_batch_cases as vb
import vector_limit_cases as vc
from vector_limit_cases import close as _close

pytestmark = pytest.mark.gpu

TOL = 1e-4
EINVAL = -1
LIMIT = vb.MAX_BATCH


def _create(n, max_batch=LIMIT, dual=False, **kw):
    import ga3c_amd  # noqa: F401  (puts the flat modules on sys.path)
    if n.kind == "mlp":
        from NetworkVP_vector import Network
        with vc.config(DUAL_RMSPROP=dual, **kw):
            return Network("gpu:0", "vecbatch", n.A, (n.S,), max_batch=max_batch, predict_lanes=2)
    from NetworkVP_discrate import Network
    with vc.config(DENSE_LAYERS=tuple(n.layers), DENSE_STACK=n.stack, USE_LOG_SOFTMAX=n.kw["use_log_softmax"],
                   MIN_POLICY=n.kw["min_policy"], DUAL_RMSPROP=False, **kw):
        return Network("gpu:0", "dvecbatch", n.A, (n.S,), max_batch=max_batch, predict_lanes=2)


@pytest.fixture(scope="module")
def handles():
    """-> get(net_id, head): the one handle of that network, made at its first use and closed with the module."""
    made = {}

    def get(net_id, head):
        if (net_id, head) not in made:
            made[net_id, head] = _create(vb.net(net_id, head))
        return made[net_id, head]
    yield get
    for h in made.values():
        h.close()


def _reset(net, params, flat, dual=False):
    """theta = params, ms = 1, mom = 0 (both optimizers' slots when there are two)."""
    net.set_arena(0, flat(params))
    for w in (1, 4) if dual else (1,):
        net.set_arena(w, np.ones(net.param_count, np.float32))
    for w in (2, 5) if dual else (2,):
        net.set_arena(w, np.zeros(net.param_count, np.float32))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype == np.float32 and a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _var(net, flat, name):
    off, size = net._offsets[name]
    return flat[off:off + size]


def _fetch(net, n, names, B):
    return {k: net.fetch(k, B * n.widths[k]) for k in names}


def _check_losses(losses, want, where):
    for got, key in zip(losses, vb.LOSSES):
        assert np.isfinite(got) and abs(got - want[key]) <= TOL * max(1.0, abs(want[key])), (where, key, got, want[key])


def _held(what, got, want, tol):
    """_close, with the figure printed first: max|got - want| as a share of tol x max(1, max|want|)."""
    diff, scale = _measure(got, want)
    print("%-44s max|got - want| %.3e = %.3f of %g x max(1, %.3e)" % (what, diff, diff / (tol * max(1.0, scale)), tol, scale))
    return diff <= tol * max(1.0, scale)


def _measure(got, want):
    """-> (max|got - want|, max|want|), one pass for both comparators."""
    got, want = np.asarray(got, np.float64).reshape(-1), np.asarray(want, np.float64).reshape(-1)
    assert got.shape == want.shape and np.all(np.isfinite(got))
    return float(np.max(np.abs(got - want))), float(np.max(np.abs(want)))


# ---- 1: forward, losses, deltas, gradients at every size, on the plain and the two heavy-row batches
@pytest.mark.parametrize("net_id,head,B", vb.CASES, ids=vb.CASE_IDS)
def test_rows_losses_deltas_and_gradients_against_the_oracle(handles, net_id, head, B):
    """Both comparators on every delta and gradient; the forward tensors (the same in all three batches) on the plain one.  Per
    batch the worst tensor is printed with its rel_err / bound and rel_err / e32.  predict_p_v_logits is the host-buffer
    predict: it takes a prediction lane (predict_begin's take_lane, csrc/ga3c_vecnet.hpp), stages the rows in the lane's pinned
    h_x and reads the lane's outputs, so every size here, 1025 and 65536 among them, is a prediction on a lane."""
    cs = vb.case(net_id, head, B)
    n = cs.net
    net = handles(net_id, head)
    _reset(net, n.params, n.flat)
    net.beta = vb.BETA
    assert net.max_batch == LIMIT and net.param_count == n.flat(n.params).size
    failed = []
    for kind in vb.KINDS:
        want = cs.want[kind]
        where = "%s %s B=%d %s" % (net_id, head, B, kind)
        if kind == "plain":
            p, v, z = net.predict_p_v_logits(cs.x)
            assert p.shape == (B, n.A) and v.shape == (B,) and z.shape == (B, n.widths["z"])
            assert _close(p, want["p"]) and _close(v, want["v"]) and _close(z, want["z"]), where
        _check_losses(net.compute_grads(cs.x, cs.y[kind], cs.a), cs.losses[kind], where)
        if kind == "plain":
            for name, val in _fetch(net, n, n.acts, B).items():
                assert _close(val, want[name]), (where, name)
        got = _fetch(net, n, n.deltas, B)
        grad = net.get_arena(3)
        assert np.all(np.isfinite(grad))
        got.update({k: _var(net, grad, k) for k in n.grads})
        for k in getattr(n, "dead", ()):
            assert not np.any(_var(net, grad, k)), (where, k)                      # exactly zero, no tolerance
        worst = (0.0, None, 0.0)
        for name, val in got.items():
            diff, scale = _measure(val, want[name])
            assert diff <= TOL * max(1.0, scale), (where, name, diff, scale)
            err, bound = diff / scale, cs.bound(kind, name)
            if err / bound > worst[0]:
                worst = (err / bound, name, err / cs.e32[kind][name])
            if not err <= bound:
                failed.append((where, name, err, bound))
        print("%-40s worst %-18s rel_err / bound %.3f  rel_err / e32 %6.2f" % (where, worst[1], worst[0], worst[2]))
    assert not failed, failed


# ---- 2: a row's outputs do not depend on its place
ROW_NETS = [("mlp-3-1", "angle"), ("dmlp-chained", "plain")]


def _per_row(net, n, x, y, a):
    B = len(y)
    p, v, z = net.predict_p_v_logits(x)
    net.compute_grads(x, y, a)
    out = dict(p=p, v=v, z=z)
    out.update({k: val.reshape(B, -1) for k, val in _fetch(net, n, ("dz", "dv", n.first_delta), B).items()})
    return out


@pytest.mark.parametrize("net_id,head", ROW_NETS, ids=[t[0] for t in ROW_NETS])
def test_a_rows_outputs_do_not_depend_on_its_place_at_65536_rows(handles, net_id, head):
    """The batch against the same rows permuted: p, v, z, dz, dv and the first layer's delta of every row, bit for bit.  Then one
    state written to rows 0, 15, 16, 1024, 65520 and 65535 -- the first and last rows of the first and the last tile, and of
    tile 64 -- gives one set of bits."""
    cs = vb.case(net_id, head, LIMIT)
    n, net = cs.net, handles(net_id, head)
    _reset(net, n.params, n.flat)
    net.beta = vb.BETA
    x, y, a = cs.x, cs.y["plain"], cs.a
    perm = vb.permutation(LIMIT)
    base, moved = _per_row(net, n, x, y, a), _per_row(net, n, x[perm], y[perm], a[perm])
    for k in base:
        assert np.any(base[k]) and _same(moved[k], base[k][perm]), k
    rows = np.array(vb.SAME_ROWS)
    x2, y2, a2 = x.copy(), y.copy(), a.copy()
    x2[rows], y2[rows], a2[rows] = x[7], y[7], a[7]
    out = _per_row(net, n, x2, y2, a2)
    for k in out:
        for r in rows:
            assert _same(out[k][r], base[k][7]), (k, r)
        assert _same(out[k][1], base[k][1]) and _same(out[k][LIMIT - 2], base[k][LIMIT - 2]), k


# ---- 3: rows gathered out of a registered segment
@pytest.mark.parametrize("B", [1025, LIMIT])
@pytest.mark.parametrize("state_dim,num_actions", [(64, 32), (1, 32)], ids=["rows-of-256-bytes", "rows-of-4-bytes"])
def test_gather_entries_are_bit_equal_to_host_buffers(state_dim, num_actions, B):
    """predict_gather over B agent slots (in reverse order) and train_gather over a rollout of B rows, B = 1025 and 65536, with
    rows of 256 bytes and of 4 bytes (four to a 16-byte line), give the bits of the host-buffer entry points.  Both predictions
    run on a prediction lane of a handle of max_batch = 65536."""
    import ga3c_amd  # noqa: F401
    import Transport as tp
    from NetworkVP_vector import Network
    S, A = state_dim, num_actions
    params = vc.limit_params(S, A)
    rng = np.random.Generator(np.random.PCG64(3 + S))
    x = rng.uniform(-1.5, 1.5, size=(B, S)).astype(np.float32)
    a = rng.uniform(-1, 1, size=(B, A)).astype(np.float32)
    y = rng.uniform(-1, 1, size=B).astype(np.float32)
    t = tp.Transport.create(tp.unique_name("t_vecbatch"), B, A, 4 * S, 1, B, float_actions=True)
    with vc.config(DUAL_RMSPROP=False):
        net = Network("gpu:0", "vecbatch", A, (S,), max_batch=LIMIT, predict_lanes=2)
    try:
        _reset(net, params, m.flat)
        net.learning_rate, net.beta = vb.STEP_LR, vb.BETA
        ids = np.arange(B, dtype=np.uint32)[::-1].copy()
        t.agent_states[ids] = x.view(np.uint8).reshape(B, 4 * S)
        net.register_transport(t)
        p1, v1 = net.predict_offsets(t.state_offsets(ids))
        p2, v2 = net.predict_p_and_v(x)
        assert _same(p1, p2) and _same(v1, v2) and np.any(p1)
        slot = t.acquire(1000)
        states, _, _ = t.rollout_views(slot)
        states[:B] = x.view(np.uint8).reshape(B, 4 * S)
        t.commit(slot, B)
        got = t.pop_rollout(1000)
        offs = t.rollout_row_offsets(got, B)
        assert offs.size == B and np.all(offs % 4 == 0) and (S != 1 or np.any(offs % 16 != 0))
        net.train_offsets(offs, y, a)
        gathered = [net.last_losses.copy()] + [net.get_arena(w) for w in (0, 1, 3)]
        _reset(net, params, m.flat)
        net.train(x, y, a)
        plain = [net.last_losses.copy()] + [net.get_arena(w) for w in (0, 1, 3)]
        assert all(_same(u, w) for u, w in zip(gathered, plain))
        assert not _same(plain[1], m.flat(params).astype(np.float32)) and net.get_global_step() == 2
        t.release(got)
        net.unregister_transport()
    finally:
        net.close()
        t.shutdown()
        t.close()


# ---- 4: two production steps
def _slots(net, params, seed):
    """(ms0, mom0) arenas and the same values as the oracle's dicts."""
    rng = np.random.default_rng(seed)
    ms0 = rng.uniform(0.5, 1.5, net.param_count).astype(np.float32)
    mom0 = rng.uniform(-1e-3, 1e-3, net.param_count).astype(np.float32)
    ms, mom = ({k: _var(net, flat, k).astype(np.float64).reshape(params[k].shape) for k in params} for flat in (ms0, mom0))
    return ms0, mom0, ms, mom


@pytest.mark.parametrize("B", vb.STEP_SIZES)
@pytest.mark.parametrize("way", list(vb.STEP_WAYS))
@pytest.mark.parametrize("net_id,head", vb.STEP_NETS, ids=[t[0] for t in vb.STEP_NETS])
def test_two_train_steps_against_the_oracle(net_id, head, way, B):
    """Two steps of B rows from random ms and mom, held as tests/test_gpu_vector_limits.py holds them: theta, ms and (with
    momentum) mom to 1e-5 x max(1, max|want|) at its learning rate.  A gradient here is a sum over up to 65536 rows, so
    0.01 g^2 is far above ms0 and eps and the step is close to lr x 10 x sign(g): theta says little about g at these sizes
    (tests/README.md); ms = 0.99 ms0 + 0.01 g^2 does, and test_the_fused_step_used_the_oracles_gradient reads g itself back."""
    n = vb.net(net_id, head)
    kw = vb.STEP_WAYS[way]
    clip, momentum = (vb.STEP_CLIP if kw.get("clip") else None), kw.get("momentum", 0.0)
    net = _create(n, max_batch=B, USE_GRAD_CLIP=clip is not None, GRAD_CLIP_NORM=clip or 40.0, RMSPROP_MOMENTUM=momentum)
    try:
        theta0 = n.flat(n.params).astype(np.float32)
        net.set_arena(0, theta0)
        ms0, mom0, ms, mom = _slots(net, n.params, 3)
        net.set_arena(1, ms0)
        net.set_arena(2, mom0)
        net.learning_rate, net.beta = vb.STEP_LR, vb.BETA
        ref = {k: v.copy() for k, v in n.params.items()}
        for step in range(2):
            x, y, a = vb.step_batch(net_id, head, B, step)
            net.train(x, y, a)
            g = n.train_step(ref, ms, mom, x, y, a, vb.STEP_LR, momentum=momentum, clip=clip)
            if clip is not None:
                assert all(np.sqrt(np.sum(g[k] ** 2)) / g[k].size > 1.5 * clip for k in n.grads), step
        assert net.get_global_step() == 2
        theta, ms_got, mom_got = net.get_arena(0), net.get_arena(1), net.get_arena(2)
        assert np.all(np.isfinite(theta)) and not np.array_equal(theta, theta0)
        where = "steps %s %s B=%d " % (net_id, way, B)
        assert _held(where + "theta", theta, n.flat(ref), 1e-5)
        assert _held(where + "ms", ms_got, n.flat(ms), 1e-5)
        if momentum:
            assert _held(where + "mom", mom_got, n.flat(mom), 1e-5)
        else:
            assert np.array_equal(mom_got, mom0)                         # momentum 0 never touches the slot
        for k in getattr(n, "dead", ()):
            assert all(np.array_equal(_var(net, u, k), _var(net, w, k)) for u, w in ((theta, theta0), (ms_got, ms0), (mom_got, mom0)))
    finally:
        net.close()


@pytest.mark.parametrize("B", vb.STEP_SIZES)
def test_two_train_steps_with_two_optimizers(B):
    """DUAL_RMSPROP on ga3c_mlp: both costs' steps against mlp_dual_oracle, the slots a cost has no path to bit for bit as set."""
    net_id, head = vb.STEP_NETS[0]
    n = vb.net(net_id, head)
    net = _create(n, max_batch=B, dual=True)
    try:
        theta0 = m.flat(n.params).astype(np.float32)
        net.set_arena(0, theta0)
        ms0, mom0, ms, mom = _slots(net, n.params, 3)
        ms0_v, mom0_v, ms_v, mom_v = _slots(net, n.params, 4)
        for w, flat in ((1, ms0), (2, mom0), (4, ms0_v), (5, mom0_v)):
            net.set_arena(w, flat)
        slots = {"ms_p": ms, "mom_p": mom, "ms_v": ms_v, "mom_v": mom_v}
        net.learning_rate, net.beta = vb.STEP_LR, vb.BETA
        ref = {k: v.copy() for k, v in n.params.items()}
        head_v, head_p = vc.mask(net, d.HEAD_V), vc.mask(net, d.HEAD_P)
        for step in range(2):
            x, y, a = vb.step_batch(net_id, head, B, step)
            net.train(x, y, a)
            _, gp, gv = d.dual_grads(ref, *vc.f64(x, y, a), vb.BETA)
            if step == 1:                                                # the last gradients, exact zeros where a cost has no path
                arena = {"p": net.get_arena(3), "v": net.get_arena(6)}
                assert not np.any(arena["p"][head_v]) and not np.any(arena["v"][head_p])
                for cost, g, no_path in (("p", gp, d.HEAD_V), ("v", gv, d.HEAD_P)):
                    for k in m.PARAM_ORDER:
                        assert k in no_path or _close(_var(net, arena[cost], k), g[k]), (cost, k)
            d.dual_rmsprop_update(ref, slots, gp, gv, vb.STEP_LR)
        assert net.get_global_step() == 2
        held = [_held("steps dual B=%d %s" % (B, what), net.get_arena(w), m.flat(want), 1e-5)
                for what, w, want in (("theta", 0, ref), ("ms_p", 1, ms), ("ms_v", 4, ms_v))]
        assert all(held), held
        assert np.array_equal(net.get_arena(2), mom0) and np.array_equal(net.get_arena(5), mom0_v)
        assert np.array_equal(net.get_arena(1)[head_v], ms0[head_v]) and np.array_equal(net.get_arena(4)[head_p], ms0_v[head_p])
        trunk = vc.mask(net, d.TRUNK_VARS)
        assert np.mean(net.get_arena(1)[trunk] != ms0[trunk]) > 0.999 and np.mean(net.get_arena(4)[trunk] != ms0_v[trunk]) > 0.999
    finally:
        net.close()


@pytest.mark.parametrize("B", vb.STEP_SIZES)
@pytest.mark.parametrize("net_id,head", vb.STEP_NETS, ids=[t[0] for t in vb.STEP_NETS])
def test_the_fused_step_used_the_oracles_gradient(handles, net_id, head, B):
    """One production step from ms = 0, mom = 0 on the case's plain batch: closeness.g_eff reads every gradient element the fused
    step used back from ms' = omr g^2 and the sign of the step, whatever the weight's ulp; held per tensor to the case's bound,
    as tests/test_gpu_step_probe.py holds the image net's."""
    cs = vb.case(net_id, head, B)
    n, net = cs.net, handles(net_id, head)
    theta = n.flat(n.params).astype(np.float32)
    net.set_arena(0, theta)
    net.set_arena(1, np.zeros(net.param_count, np.float32))
    net.set_arena(2, np.zeros(net.param_count, np.float32))
    net.learning_rate, net.beta = vb.STEP_LR, vb.BETA
    net.train(cs.x, cs.y["plain"], cs.a)
    _check_losses(net.last_losses, cs.losses["plain"], "fused step")
    sign, mag = c.g_eff(theta, net.get_arena(0), net.get_arena(1))
    failed = []
    for k in n.grads:
        got, ref = c.signed_or_magnitude(_var(net, sign, k), _var(net, mag, k), cs.want["plain"][k])
        err = c.report("g_eff %s B=%d" % (net_id, B), k, got, ref, cs.e32["plain"][k], cs.bound("plain", k))
        if not err <= cs.bound("plain", k):
            failed.append((k, err, cs.bound("plain", k)))
    assert not failed, failed


@pytest.mark.parametrize("net_id,head", vb.STEP_NETS, ids=[t[0] for t in vb.STEP_NETS])
def test_split_step_and_repeated_calls_are_bit_identical_at_65536_rows(handles, net_id, head):
    cs = vb.case(net_id, head, LIMIT)
    n, net = cs.net, handles(net_id, head)
    x, y, a = cs.x, cs.y["last"], cs.a
    net.learning_rate, net.beta = vb.STEP_LR, vb.BETA
    _reset(net, n.params, n.flat)
    step0 = net.get_global_step()
    g1 = (net.compute_grads(x, y, a), net.get_arena(3))
    g2 = (net.compute_grads(x, y, a), net.get_arena(3))
    assert _same(g1[0], g2[0]) and _same(g1[1], g2[1]) and np.any(g1[1])        # no float atomics anywhere
    assert net.get_global_step() == step0
    net.apply_grads()
    split = [net.get_arena(w) for w in (0, 1, 2, 3)]
    _reset(net, n.params, n.flat)
    net.train(x, y, a)
    for w, want in enumerate(split):
        assert _same(net.get_arena(w), want), w
    assert not _same(split[0], n.flat(n.params).astype(np.float32)) and net.get_global_step() == step0 + 2


# ---- 5: the device actors at the row limit
def _actor_fields(game):
    return ("obs", "p", "action", "done", "elapsed", "draws") + (("reward",) if game == "pendulum" else ())


def _policy(n, obs):
    """-> (the network oracle's prediction rows for the observations, which rows it can be held on): ga3c_mlp's angle jumps by 2
    where a row lies on the atan2 branch cut, so only mlp_oracle.safe_rows are compared there."""
    x = obs.astype(np.float64)
    if n.kind == "mlp":
        return m.forward(n.params, x)["o"], m.safe_rows(n.params, x, 1e-3)
    import dmlp_oracle as dm
    return dm.forward(n.params, x, n.stack, **n.kw)["p"], np.ones(len(x), bool)


@pytest.mark.parametrize("game", list(vb.ACTOR_CASES))
def test_device_actors_at_the_row_limit(handles, game):
    """N = 16384 environments at TIME_MAX = 3: 16 per thread of the 1024-thread scan, and the first cut, on step 5, lays out
    N x 4 = 65536 rows -- off[row], by and ba up to row 65535, cap = N x T1 = max_batch.  As
    test_the_scan_with_several_environments_per_thread: the oracle follows the device's physics, the forced episodes
    (test_gpu_device_agents._forced) end on the cut; batch_x / batch_a / batch_y_r bit for bit, episode records and counts
    against the actors' oracle.  Every predicted step's p for all N environments is held to the network oracle on the
    observations the step began with.  Then, from a fresh set of actors, the training step of actors_run(1, train=True) on
    65536 rows: the stepped arenas against the network oracle's train_step on the fetched batch at the tolerance of the
    two-step tests, and bit-equal to a twin handle's train() on that batch."""
    from test_gpu_device_agents import _forced
    net_id, head, N, time_max = vb.ACTOR_CASES[game]
    n, net = vb.net(net_id, head), handles(net_id, head)
    _reset(net, n.params, n.flat)
    net.learning_rate, net.beta = vb.STEP_LR, vb.BETA
    ora, _, _ = vb.actors_oracle(game)
    forced, last = _forced(N), time_max + 1
    net.actors_create(N, time_max, vb.ACTOR_GAMMA, vb.ACTOR_SEED)
    try:
        obs, held = None, 0
        for step in range(last + 1):
            if step == last:
                elapsed = net.actors_get("elapsed")
                elapsed[forced] = 199
                net.actors_set("elapsed", elapsed)
                for i in forced:
                    ora.env[i].elapsed = 199
            for e, ph in zip(ora.env, net.actors_get("phys")):       # re-seeded from the device's physics before every step
                e.phys = ph.copy()
            stats = net.actors_run(1, train=False)
            g = {k: net.actors_get(k) for k in _actor_fields(game)}
            if step > 0:                                             # the first step is taken without a prediction
                want, ok = _policy(n, obs)
                assert ok.mean() > 0.98 and _close(g["p"][ok], want[ok]), step
                held += int(ok.sum())
            if game == "pendulum":
                res, batch, episodes = ora.step(g["p"], actions=g["action"], dones=g["done"], rewards=g["reward"])
            else:
                res, batch, episodes = ora.step(g["p"], actions=g["action"], dones=None if step == 0 else g["done"])
            own_done = np.array([r["own_done"] for r in res])
            assert np.array_equal(own_done, g["done"].astype(bool)), step
            assert np.array_equal([e.elapsed for e in ora.env], g["elapsed"]), step
            assert np.array_equal([e.rng.draws for e in ora.env], g["draws"].astype(np.int64)), step
            for e, ob in zip(ora.env, g["obs"]):
                e.obs = ob.copy()
            obs = g["obs"]
            rows = net.actors_get("batch_rows")
            assert stats == (N, 0, 0, len(episodes))
            got_eps = net.actors_episodes()
            assert len(got_eps) == len(episodes)
            for (gr, gl), (wr, wl) in zip(got_eps, episodes):
                assert np.float64(gr).view(np.uint64) == np.float64(wr).view(np.uint64) and gl == wl
            if step < last:
                assert rows == 0 and batch is None and not episodes
                continue
            assert rows == N * (time_max + 1) == LIMIT and len(episodes) == len(forced)
            assert np.array_equal(np.flatnonzero(g["done"]), forced)
            for name, want in zip(("batch_x", "batch_a", "batch_y_r"), batch):
                got = net.actors_get(name)
                assert got.shape == want.shape and _same(got, want), name
            assert len(np.unique(batch[0], axis=0)) > N              # the rows tell the environments apart
        assert held > 0.98 * N * last
    finally:
        net.actors_destroy()
    # the training step on the 65536 rows of the first cut
    twin = _create(n)
    try:
        _reset(net, n.params, n.flat)
        _reset(twin, n.params, n.flat)
        twin.learning_rate, twin.beta = vb.STEP_LR, vb.BETA
        step0 = net.get_global_step()
        net.actors_create(N, time_max, vb.ACTOR_GAMMA, vb.ACTOR_TRAIN_SEED)
        try:
            assert net.actors_run(last, train=True) == (last * N, 0, 0, 0)           # nothing cut yet
            assert _same(net.get_arena(0), n.flat(n.params).astype(np.float32))
            assert net.actors_run(1, train=True) == (N, 1, LIMIT, 0)
            x, y, a = (net.actors_get(k) for k in ("batch_x", "batch_y_r", "batch_a"))
        finally:
            net.actors_destroy()
        assert x.shape == (LIMIT, n.S) and y.shape == (LIMIT,) and a.shape == (LIMIT, n.A)
        twin.train(x, y, a)
        for w in (0, 1, 2, 3):
            assert _same(net.get_arena(w), twin.get_arena(w)), w
        assert net.get_global_step() == step0 + 1
        ref = {k: v.copy() for k, v in n.params.items()}
        ms = {k: np.ones_like(v) for k, v in ref.items()}
        mom = {k: np.zeros_like(v) for k, v in ref.items()}
        n.train_step(ref, ms, mom, x, y, a, vb.STEP_LR)
        where = "actors %s train " % game
        assert not _same(net.get_arena(0), n.flat(n.params).astype(np.float32))
        assert _held(where + "theta", net.get_arena(0), n.flat(ref), 1e-5)
        assert _held(where + "ms", net.get_arena(1), n.flat(ms), 1e-5)
    finally:
        twin.close()


# ---- 6: refusals
def test_refusals_by_code_and_text_leave_the_handle_usable(handles):
    """max_batch = 65537 at both creates, a batch of 65537 rows on a handle of 65536, and device actors whose rows exceed 65536.
    (65537 is prime: with TIME_MAX + 1 >= 2 rows per environment no N x T1 equals it.  The first products past the limit are
    32769 x 2 and 21846 x 3 = 65538; the limit itself, 32768 x 2, is admitted.)"""
    import ga3c_amd  # noqa: F401
    import _native as nat
    lib = nat.hip_lib()
    for net_id, head, prefix in (("mlp-3-1", "angle", "ga3c_mlp"), ("dmlp-fork", "plain", "ga3c_dmlp")):
        n = vb.net(net_id, head)
        with pytest.raises(RuntimeError, match=r"%s_create failed \(%d\): max_batch 65537 outside \[1,65536\]" % (prefix, EINVAL)):
            _create(n, max_batch=LIMIT + 1)
        net = handles(net_id, head)
        _reset(net, n.params, n.flat)
        x, y, a = n.batch(32)
        before = net.predict_p_and_v(x)
        big = np.zeros((LIMIT + 1, n.S), np.float32)
        theta, step = net.get_arena(0), net.get_global_step()
        for call in (lambda: net.predict_p_and_v(big), lambda: net.compute_grads(big, np.zeros(LIMIT + 1), np.zeros((LIMIT + 1, n.A))),
                     lambda: net.train(big, np.zeros(LIMIT + 1), np.zeros((LIMIT + 1, n.A)))):
            with pytest.raises(RuntimeError, match=r"failed \(%d\): batch 65537 outside \[1,65536\]" % EINVAL):
                call()
        create = getattr(lib, prefix + "_actors_create")
        for count, time_max in ((32769, 1), (21846, 2), (LIMIT + 1, 1)):
            assert create(net._h, count, time_max, 0.99, 1) == EINVAL, (count, time_max)
            assert b"rows exceed the network's max_batch 65536" in lib.ga3c_last_error()
        net.actors_create(32768, 1, 0.99, 1)                            # 65536 rows: admitted
        net.actors_destroy()
        after = net.predict_p_and_v(x)
        assert _same(after[0], before[0]) and _same(after[1], before[1]) and np.any(after[0])
        assert _same(net.get_arena(0), theta) and net.get_global_step() == step
