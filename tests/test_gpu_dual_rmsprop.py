"""-m gpu: Config.DUAL_RMSPROP on the HIP path against its f64 statement (tests/dual_oracle.py).

One forward pass, one backward pass per cost on the same weights, then the value optimizer's step and the policy
optimizer's step in one kernel.  Tolerance: the existing 1e-4 x max(1, max|want|) per arena.
"""
import contextlib

import numpy as np
import pytest

import dual_oracle as d
import ga3c_oracle as o

pytestmark = pytest.mark.gpu

TOL = 1e-4
SLOTS = (("ms_p", 1), ("mom_p", 2), ("ms_v", 4), ("mom_v", 5))


@contextlib.contextmanager
def _config(**kw):
    import ga3c_amd  # noqa: F401  (puts the flat modules on sys.path)
    from Config import Config
    saved = {k: getattr(Config, k) for k in kw}
    for k, v in kw.items():
        setattr(Config, k, v)
    try:
        yield Config
    finally:
        for k, v in saved.items():
            setattr(Config, k, v)


def _net(num_actions, max_batch, dual=True, train_lanes=None, **kw):
    from NetworkVP import Network
    with _config(DUAL_RMSPROP=dual, **kw):
        return Network("gpu:0", "dual" if dual else "single", num_actions, (84, 84, 4), max_batch=max_batch, predict_lanes=1,
                       train_lanes=train_lanes)


def _batch(bsz, num_actions, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    xk = rng.integers(0, 256, size=(bsz, 84, 84, 4), dtype=np.uint8)
    x = xk.astype(np.float32) / np.float32(128.0) - np.float32(1.0)
    a = np.eye(num_actions, dtype=np.float32)[rng.integers(0, num_actions, size=bsz)]
    y = rng.uniform(-1, 1, size=bsz)
    return xk, x, a, y


def _reset(net):
    """Oracle init weights and fresh slots for both optimizers (ms = 1, mom = 0)."""
    net.set_arena(0, d.flat(o.init_params(net.num_actions)))
    for _, w in SLOTS:
        net.set_arena(w, np.full(net.param_count, 1.0 if w in (1, 4) else 0.0, np.float32))


def _close_rule(got, want):
    return np.max(np.abs(got - want)) <= TOL * max(1.0, np.max(np.abs(want)))


def _oracle_steps(num_actions, x, y, a, steps, lr, beta, momentum=0.0, clip=None):
    params = o.init_params(num_actions)
    slots = d.init_slots(params)
    for _ in range(steps):
        _, gp, gv = d.dual_grads(params, x.astype(np.float64), y, a.astype(np.float64), beta)
        d.dual_rmsprop_update(params, slots, gp, gv, lr, momentum=momentum, clip=clip)
    return params, slots


@pytest.fixture(scope="module")
def dual_nets():
    import ga3c_amd  # noqa: F401
    made = {}

    def get(num_actions):
        if num_actions not in made:
            made[num_actions] = _net(num_actions, 160)
        return made[num_actions]
    yield get
    for n in made.values():
        n.close()


@pytest.mark.parametrize("num_actions", [6, 18])
@pytest.mark.parametrize("bsz", [1, 5, 96, 97, 128, 132, 145])
def test_two_dual_steps_match_oracle(dual_nets, bsz, num_actions):
    """Batch sizes cross the split / fused conv backward seam (96 / 97), the fused conv stack's limit (128 / 132) and the
    dense1_bwd_tile tail (132 / 145).  uint8 and f32 states give the same bits."""
    net = dual_nets(num_actions)
    xk, x, a, y = _batch(bsz, num_actions, 1000 + bsz)
    lr, beta = 1e-3, 0.01
    results = []
    for states in (x, xk):
        _reset(net)
        net.learning_rate, net.beta = lr, beta
        for _ in range(2):
            net.train(states, y, a)
        results.append([net.get_arena(w) for w in (0, 1, 2, 4, 5)])
    for got_f32, got_u8 in zip(*results):
        assert np.array_equal(got_f32, got_u8)
    params, slots = _oracle_steps(num_actions, x, y, a, 2, lr, beta)
    theta, ms_p, mom_p, ms_v, mom_v = results[0]
    assert _close_rule(theta, d.flat(params)), np.max(np.abs(theta - d.flat(params)))
    for got, key in ((ms_p, "ms_p"), (mom_p, "mom_p"), (ms_v, "ms_v"), (mom_v, "mom_v")):
        assert _close_rule(got, d.flat(slots[key])), key
    # the step really moved every variable, each head by its own optimizer
    init = d.flat(o.init_params(num_actions))
    assert np.all(theta[d.region_mask(num_actions, ("logits_v/b", "logits_p/b"))] !=
                  init[d.region_mask(num_actions, ("logits_v/b", "logits_p/b"))])


@pytest.mark.parametrize("momentum", [0.0, 0.5])
def test_slots_without_a_reference_slot_stay_untouched(momentum):
    num_actions = 6
    net = _net(num_actions, 32, RMSPROP_MOMENTUM=momentum)
    try:
        _, x, a, y = _batch(17, num_actions, 5)
        net.learning_rate, net.beta = 1e-3, 0.02
        for _ in range(3):
            net.train(x, y, a)
        head_p = d.region_mask(num_actions, d.HEAD_P)
        head_v = d.region_mask(num_actions, d.HEAD_V)
        assert np.all(net.get_arena(4)[head_p] == 1.0) and np.all(net.get_arena(5)[head_p] == 0.0)
        assert np.all(net.get_arena(1)[head_v] == 1.0) and np.all(net.get_arena(2)[head_v] == 0.0)
        assert np.all(net.get_arena(1)[head_p] != 1.0) and np.all(net.get_arena(4)[head_v] != 1.0)
        if momentum:
            assert np.any(net.get_arena(2)[head_p] != 0.0) and np.any(net.get_arena(5)[head_v] != 0.0)
            params, slots = _oracle_steps(num_actions, x, y, a, 3, 1e-3, 0.02, momentum=momentum)
            assert _close_rule(net.get_arena(0), d.flat(params))
            assert _close_rule(net.get_arena(2), d.flat(slots["mom_p"])) and _close_rule(net.get_arena(5), d.flat(slots["mom_v"]))
    finally:
        net.close()


@pytest.mark.parametrize("bite", ["every", "none"])
def test_grad_clip_by_norm_matches_oracle(bite):
    """USE_GRAD_CLIP under dual: tf.clip_by_norm per gradient tensor of each cost.  One clip norm below every tensor's
    norm, one above all of them."""
    num_actions, bsz = 6, 21
    _, x, a, y = _batch(bsz, num_actions, 77)
    params = o.init_params(num_actions)
    _, gp, gv = d.dual_grads(params, x.astype(np.float64), y, a.astype(np.float64), 0.02)
    norms = [np.sqrt(np.sum(np.asarray(g[k]) ** 2)) for g, heads in ((gp, d.HEAD_V), (gv, d.HEAD_P))
             for k in o.PARAM_ORDER if k not in heads]
    clip = 0.5 * min(norms) if bite == "every" else 2.0 * max(norms)
    net = _net(num_actions, 32, USE_GRAD_CLIP=True, GRAD_CLIP_NORM=float(clip))
    try:
        net.learning_rate, net.beta = 1e-3, 0.02
        for _ in range(2):
            net.train(x, y, a)
        want, slots = _oracle_steps(num_actions, x, y, a, 2, 1e-3, 0.02, clip=clip)
        init = d.flat(o.init_params(num_actions))
        got_step, want_step = net.get_arena(0) - init, d.flat(want) - init
        assert np.max(np.abs(got_step - want_step)) <= 2e-3 * np.max(np.abs(want_step))
        for key, w in SLOTS:
            assert _close_rule(net.get_arena(w), d.flat(slots[key])), key
        unclipped, _ = _oracle_steps(num_actions, x, y, a, 2, 1e-3, 0.02)
        moved = np.max(np.abs(d.flat(unclipped) - d.flat(want)))
        assert (moved > 1e-2 * np.max(np.abs(want_step))) == (bite == "every"), moved
    finally:
        net.close()


def test_compute_grads_parts_sum_to_single_gradient():
    num_actions = 6
    _, x, a, y = _batch(40, num_actions, 9)
    dual, single = _net(num_actions, 64), _net(num_actions, 64, dual=False)
    try:
        for net in (dual, single):
            net.beta = 0.01
            net.compute_grads(x, y, a)
        gp, gv, g = dual.get_arena(3), dual.get_arena(6), single.get_arena(3)
        assert _close_rule(gp + gv, g), np.max(np.abs(gp + gv - g))
        assert not np.any(gp[d.region_mask(num_actions, d.HEAD_V)]) and not np.any(gv[d.region_mask(num_actions, d.HEAD_P)])
        with pytest.raises(RuntimeError):
            single.get_arena(6)
    finally:
        dual.close()
        single.close()


def _dual_member_names():
    names = {"step"}
    for k in o.PARAM_ORDER:
        names.add(k + ":0")
        if k.startswith("logits_p/") or k.startswith("logits_v/"):
            names.update({k + "/RMSProp:0", k + "/RMSProp_1:0"})
        else:
            names.update({k + "/RMSProp:0", k + "/RMSProp_1:0", k + "/RMSProp_2:0", k + "/RMSProp_3:0"})
    return names


def test_checkpoint_members_round_trip_and_refusals(tmp_path):
    num_actions = 6
    _, x, a, y = _batch(12, num_actions, 4)
    dual = _net(num_actions, 16, RMSPROP_MOMENTUM=0.5)
    single = _net(num_actions, 16, dual=False, RMSPROP_MOMENTUM=0.5)
    try:
        for net in (dual, single):
            net.learning_rate, net.beta = 1e-3, 0.01
            for _ in range(2):
                net.train(x, y, a)
        dpath, spath = str(tmp_path / "dual.npz"), str(tmp_path / "single.npz")
        assert dual._lib.ga3c_net_save(dual._h, dpath.encode()) == 0
        assert single._lib.ga3c_net_save(single._h, spath.encode()) == 0
        with np.load(dpath) as z:
            assert set(z.files) == _dual_member_names()
            assert int(z["step"]) == 2
            # value optimizer's slots first in the trunk, policy optimizer's after them; each head its own optimizer's
            ms_v, ms_p = dual.get_arena(4), dual.get_arena(1)
            off = 0
            for k in o.PARAM_ORDER:
                size = int(np.prod(o.param_shapes(num_actions)[k]))
                if k.startswith("logits_p/"):
                    assert np.array_equal(z[k + "/RMSProp:0"].reshape(-1), ms_p[off:off + size]), k
                else:
                    assert np.array_equal(z[k + "/RMSProp:0"].reshape(-1), ms_v[off:off + size]), k
                if not k.startswith("logits_"):
                    assert np.array_equal(z[k + "/RMSProp_2:0"].reshape(-1), ms_p[off:off + size]), k
                off += size
        saved = [dual.get_arena(w) for w in (0, 1, 2, 4, 5)]
        dual.train(x, y, a)
        assert dual._lib.ga3c_net_load(dual._h, dpath.encode()) == 0
        for w, want in zip((0, 1, 2, 4, 5), saved):
            assert np.array_equal(dual.get_arena(w), want), w
        assert dual.get_global_step() == 2
        # a file of the other kind is refused and leaves the network as it was
        for net, path, ws in ((dual, spath, (0, 1, 2, 4, 5)), (single, dpath, (0, 1, 2))):
            before = [net.get_arena(w) for w in ws]
            step = net.get_global_step()
            assert net._lib.ga3c_net_load(net._h, path.encode()) == -4
            assert all(np.array_equal(net.get_arena(w), b) for w, b in zip(ws, before))
            assert net.get_global_step() == step
    finally:
        dual.close()
        single.close()


# ---- the checkpoint path all networks share (csrc/ga3c_vartable.hpp), on the smallest handle: A = 2, one row, one lane
WRITABLE = {True: (0, 1, 2, 4, 5), False: (0, 1, 2)}


def _fill(net, dual, seed, step):
    """Every writable arena to values of its own, the step to `step` -> {arena: values}."""
    rng = np.random.Generator(np.random.PCG64(seed))
    arenas = {w: rng.normal(size=net.param_count).astype(np.float32) for w in WRITABLE[dual]}
    for w, flat in arenas.items():
        net.set_arena(w, flat)
    net._call("set_step", step)
    return arenas


def _head_masks(net):
    """-> (elements of logits_v/*, elements of logits_p/*)"""
    masks = []
    for head in ("logits_v/", "logits_p/"):
        mask = np.zeros(net.param_count, bool)
        for k in net.param_order:
            if k.startswith(head):
                off, size = net._offsets[k]
                mask[off:off + size] = True
        assert mask.any()
        masks.append(mask)
    return masks


def _dual_members_in_order(parent):
    """The members of a dual file behind "step": variable-major, as every writer of the project writes them, or (parent) in
    the order the image network wrote before it shared that path: all ":0" first, then the slots variable by variable."""
    def slots(k):
        if k.startswith("logits_"):
            return [k + "/RMSProp:0", k + "/RMSProp_1:0"]
        return [k + s for s in ("/RMSProp:0", "/RMSProp_1:0", "/RMSProp_2:0", "/RMSProp_3:0")]
    if parent:
        return [k + ":0" for k in o.PARAM_ORDER] + [name for k in o.PARAM_ORDER for name in slots(k)]
    return [name for k in o.PARAM_ORDER for name in [k + ":0"] + slots(k)]


def test_a_member_of_the_right_count_and_another_shape_is_refused(tmp_path):
    num_actions = 2
    net = _net(num_actions, 1, dual=False)
    try:
        saved = _fill(net, False, 1, 5)
        good, bad = str(tmp_path / "good.npz"), str(tmp_path / "bad.npz")
        net._call("save", good.encode())
        with np.load(good) as z:
            members = {k: z[k] for k in z.files}
        assert members["logits_p/w:0"].shape == (256, num_actions)
        members["logits_p/w:0"] = members["logits_p/w:0"].reshape(num_actions, 256)      # the same 512 elements
        np.savez(bad, **members)
        before = _fill(net, False, 2, 9)
        assert net._lib.ga3c_net_load(net._h, bad.encode()) == -4                        # GA3C_ESTATE
        for w in (0, 1, 2):
            assert np.array_equal(net.get_arena(w), before[w]), w
        assert net.get_global_step() == 9
        net._call("load", good.encode())                        # the file as written still loads
        for w in (0, 1, 2):
            assert np.array_equal(net.get_arena(w), saved[w]), w
        assert net.get_global_step() == 5
    finally:
        net.close()


def test_a_dual_file_is_variable_major_and_one_in_the_earlier_member_order_loads_the_same(tmp_path):
    net = _net(2, 1)
    try:
        _fill(net, True, 3, 5)
        path, parent = str(tmp_path / "dual.npz"), str(tmp_path / "parent_order.npz")
        net._call("save", path.encode())
        with np.load(path) as z:
            assert z.files == ["step"] + _dual_members_in_order(parent=False)
            members = {k: z[k] for k in z.files}
        np.savez(parent, **{k: members[k] for k in ["step"] + _dual_members_in_order(parent=True)})
        with np.load(parent) as z:
            assert z.files == ["step"] + _dual_members_in_order(parent=True) and z.files != list(members)
        loaded = []
        for file in (path, parent):
            _fill(net, True, 4, 0)
            net._call("load", file.encode())
            loaded.append([net.get_arena(w) for w in WRITABLE[True]] + [net.get_global_step()])
        for got, want in zip(loaded[1][:-1], loaded[0][:-1]):
            assert np.array_equal(got, want)
        assert loaded[1][-1] == loaded[0][-1] == 5
    finally:
        net.close()


def test_a_load_resets_slot_regions_no_member_names_on_the_image_network_and_keeps_them_on_the_vector_network(tmp_path):
    """Where a load starts from: the image network from the slots' initial values, ms = 1 and mom = 0, the
    vector-state network from what its arenas hold.  The regions no member names are the policy optimizer's slots (arenas
    1 / 2) over logits_v/* and the value optimizer's (4 / 5) over logits_p/*."""
    from NetworkVP_vector import Network as VectorNetwork
    image = _net(2, 1)
    with _config(DUAL_RMSPROP=True):
        vector = VectorNetwork("gpu:0", "vecdual", 1, (3,), max_batch=1, predict_lanes=1)
    try:
        for net, unnamed in ((image, {1: 1.0, 2: 0.0, 4: 1.0, 5: 0.0}), (vector, {1: 7.0, 2: 7.0, 4: 7.0, 5: 7.0})):
            prefix = net.PREFIX
            saved = _fill(net, True, 6, 5)
            path = str(tmp_path / (prefix + ".npz"))
            net._call("save", path.encode())
            for w in (1, 2, 4, 5):
                net.set_arena(w, np.full(net.param_count, 7.0, np.float32))
            net._call("load", path.encode())
            head_v, head_p = _head_masks(net)
            assert np.array_equal(net.get_arena(0), saved[0]), prefix
            for w, mask in ((1, head_v), (2, head_v), (4, head_p), (5, head_p)):
                got = net.get_arena(w)
                assert np.all(got[mask] == np.float32(unnamed[w])), (prefix, w)
                assert np.array_equal(got[~mask], saved[w][~mask]), (prefix, w)
    finally:
        image.close()
        vector.close()


def test_one_rank_communicator_and_one_hogwild_lane_give_the_same_bits():
    from NetworkVP import Network
    num_actions = 6
    xk, _, a, y = _batch(24, num_actions, 8)
    plain, rccl, hog = _net(num_actions, 32), _net(num_actions, 32), _net(num_actions, 32, train_lanes=2)
    try:
        rccl.comm_init(Network.make_comm_id(), 0, 1)
        for net in (plain, rccl, hog):
            net.learning_rate, net.beta = 1e-3, 0.01
            for _ in range(3):
                net.train(xk, y, a)
        for w in (0, 1, 2, 3, 4, 5, 6):
            want = plain.get_arena(w)
            assert np.array_equal(rccl.get_arena(w), want), w
            if w not in (3, 6):        # (the Hogwild lanes each keep a gradient arena of their own)
                assert np.array_equal(hog.get_arena(w), want), w
        assert plain.get_global_step() == rccl.get_global_step() == hog.get_global_step() == 3
    finally:
        for net in (plain, rccl, hog):
            net.close()


@pytest.mark.timeout(180)
@pytest.mark.filterwarnings("error::pytest.PytestUnhandledThreadExceptionWarning")
def test_server_trains_with_dual_rmsprop(tmp_path, monkeypatch):
    """The engine end to end (agents, transport, predictor and trainer threads; zero-copy intake, state cache) with
    DUAL_RMSPROP=True: it trains, its losses stay finite, and `step` counts one per train call."""
    import ga3c_amd  # noqa: F401
    from Config import Config
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(Config, "ZERO_COPY", True)
    monkeypatch.setattr(Config, "STATE_CACHE", True)
    with _config(DUAL_RMSPROP=True, AGENTS=6, PREDICTORS=2, TRAINERS=1, SYNTHETIC_EPISODE_LENGTH=40, TIME_MAX=5,
                 DYNAMIC_SETTINGS=False, SAVE_MODELS=False, TRAINING_MIN_BATCH_SIZE=11, NUM_ACTIONS=6,
                 PREDICTION_BATCH_SIZE=32):
        from Server import Server
        srv = Server(max_agents=8)
        try:
            before = srv.model.get_arena(0)
            srv.main(max_seconds=5)
            after = srv.model.get_arena(0)
            assert srv.predictions_served > 100 and srv.training_step > 5
            assert srv.model.get_global_step() == srv.training_step
            assert np.all(np.isfinite(after)) and np.max(np.abs(after - before)) > 1e-5
            assert srv.model.last_losses is not None and np.all(np.isfinite(srv.model.last_losses))
            assert np.any(srv.model.get_arena(4) != 1.0)      # the value optimizer's slots moved
        finally:
            srv.model.close()
