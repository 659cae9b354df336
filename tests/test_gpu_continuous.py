"""-m gpu: Config.CONTINUOUS_INPUT on the HIP path against its f64 statement (tests/continuous_oracle.py).

The angle-output policy head (heads_cont_kernel), its 2A + 2 weight-gradient roles (dense1_bwd_tile_kernel<..., CONT>) and
the 12-tensor optimizer step, through the entry points that reach them.  Tolerance: 1e-4 x max(1, max|want|), as elsewhere.
Every batch keeps away from the branch cut (X < 0, Y = 0), where o jumps from 1 to -1 and f32 and f64 may fall on either side.
"""
import contextlib

import numpy as np
import pytest

import continuous_oracle as c
import ga3c_oracle as o

pytestmark = pytest.mark.gpu

TOL = 1e-4
SEAMS = [1, 5, 96, 97, 128, 129, 132, 145]


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


def _net(num_actions, max_batch, continuous=True, train_lanes=None, **kw):
    from NetworkVP import Network
    with _config(CONTINUOUS_INPUT=continuous, **kw):
        return Network("gpu:0", "cont" if continuous else "disc", num_actions, (84, 84, 4), max_batch=max_batch,
                       predict_lanes=1, train_lanes=train_lanes)


def _params(num_actions):
    return c.init_params(num_actions, seed=4321)


def _batch(bsz, num_actions, seed):
    """bsz rows (uint8 and f32) whose every action keeps |Y| >= 1e-3 where X < 0; y_r and float actions in [-1, 1]."""
    params = _params(num_actions)
    rng = np.random.Generator(np.random.PCG64(seed))
    xk = rng.integers(0, 256, size=(2 * bsz + 16, 84, 84, 4), dtype=np.uint8)
    x = xk.astype(np.float32) / np.float32(128.0) - np.float32(1.0)
    keep = c.safe_rows(params, x.astype(np.float64), 1e-3)
    xk, x = xk[keep][:bsz], x[keep][:bsz]
    assert x.shape[0] == bsz
    a = rng.uniform(-1, 1, size=(bsz, num_actions)).astype(np.float32)
    y = rng.uniform(-1, 1, size=bsz)
    return xk, x, a, y


def _reset(net):
    net.set_arena(0, c.flat(_params(net.num_actions)))
    net.set_arena(1, np.ones(net.param_count, np.float32))
    net.set_arena(2, np.zeros(net.param_count, np.float32))


def _close(got, want, tol=TOL):
    got, want = np.asarray(got, np.float64).reshape(-1), np.asarray(want, np.float64).reshape(-1)
    return np.max(np.abs(got - want)) <= tol * max(1.0, np.max(np.abs(want)))


@pytest.fixture(scope="module")
def nets():
    import ga3c_amd  # noqa: F401
    made = {}

    def get(num_actions):
        if num_actions not in made:
            made[num_actions] = _net(num_actions, 160)
        return made[num_actions]
    yield get
    for n in made.values():
        n.close()


@pytest.mark.parametrize("num_actions", [1, 3, 6])
@pytest.mark.parametrize("bsz", SEAMS)
def test_forward_matches_oracle(nets, bsz, num_actions):
    net = nets(num_actions)
    _reset(net)
    xk, x, _, _ = _batch(bsz, num_actions, 100 + bsz)
    want = c.forward(_params(num_actions), x.astype(np.float64))
    for states in (x, xk):
        p, v, z = net.predict_p_v_logits(states)
        assert p.shape == (bsz, num_actions) and z.shape == (bsz, 2 * num_actions)
        assert np.all(p > -1) and np.all(p <= 1)
        assert _close(p, want["o"]) and _close(v, want["v"]) and _close(z, want["z"]), (
            np.max(np.abs(p - want["o"])), np.max(np.abs(z - want["z"])))


@pytest.mark.parametrize("num_actions", [1, 3, 6])
@pytest.mark.parametrize("bsz", SEAMS)
def test_losses_and_gradient_match_oracle(nets, bsz, num_actions):
    net = nets(num_actions)
    _reset(net)
    _, x, a, y = _batch(bsz, num_actions, 200 + bsz)
    net.beta = 0.02
    losses = net.compute_grads(x, y, a)
    want_l, g = c.loss_and_grads(_params(num_actions), x.astype(np.float64), y, a.astype(np.float64), 0.02)
    want = np.array([want_l["cost_p_1_agg"], want_l["cost_p_2_agg"], want_l["cost_v"]])
    assert _close(losses, want), (losses, want)
    got = net.get_arena(3)
    assert _close(got, c.flat(g)), np.max(np.abs(got - c.flat(g)))
    # the head columns alone, at their own scale (they are a small part of the arena)
    heads = np.concatenate([g[k].reshape(-1) for k in c.HEADS])
    assert _close(got[-heads.size:], heads)
    assert _close(net.fetch("dz", bsz * 2 * num_actions), g["dz"])


def _oracle_steps(num_actions, x, y, a, steps, lr, beta, momentum=0.0, clip=None):
    params = _params(num_actions)
    ms = {k: np.ones_like(t) for k, t in params.items()}
    mom = {k: np.zeros_like(t) for k, t in params.items()}
    for _ in range(steps):
        _, g = c.loss_and_grads(params, x.astype(np.float64), y, a.astype(np.float64), beta)
        c.rmsprop_update(params, ms, g, lr, momentum=momentum, mom=mom, clip=clip)
    return params, ms, mom


@pytest.mark.parametrize("bsz", [128, 132])
@pytest.mark.parametrize("variant", ["plain", "clip", "momentum"])
def test_production_train_step_matches_oracle(bsz, variant):
    """The fused update (plain, momentum) and the optimizer launch with tf.clip_by_average_norm per variable (clip: one
    clip norm that bites on every tensor, out_x and out_y normed apart)."""
    num_actions = 3
    xk, x, a, y = _batch(bsz, num_actions, 300 + bsz)
    lr, beta = 1e-3, 0.01
    kw, clip, momentum = {}, None, 0.0
    if variant == "clip":
        _, g = c.loss_and_grads(_params(num_actions), x.astype(np.float64), y, a.astype(np.float64), beta)
        clip = 0.5 * min(np.sqrt(np.sum(g[k] ** 2)) / g[k].size for k in c.PARAM_ORDER)
        kw = dict(USE_GRAD_CLIP=True, GRAD_CLIP_NORM=float(clip))
    elif variant == "momentum":
        momentum = 0.5
        kw = dict(RMSPROP_MOMENTUM=momentum)
    net = _net(num_actions, 160, **kw)
    try:
        results = []
        for states in (x, xk):
            _reset(net)
            net.learning_rate, net.beta = lr, beta
            for _ in range(2):
                net.train(states, y, a)
            results.append([net.get_arena(w) for w in (0, 1, 2)])
        for got_f32, got_u8 in zip(*results):
            assert np.array_equal(got_f32, got_u8)
        params, ms, mom = _oracle_steps(num_actions, x, y, a, 2, lr, beta, momentum=momentum, clip=clip)
        theta, ms_got, mom_got = results[0]
        if clip is None:
            assert _close(theta, c.flat(params)), np.max(np.abs(theta - c.flat(params)))
        else:       # the clipped step is small: compare the step, as test_gpu_dual_rmsprop does
            init = c.flat(_params(num_actions))
            got_step, want_step = theta - init, c.flat(params) - init
            assert np.max(np.abs(got_step - want_step)) <= 2e-3 * np.max(np.abs(want_step))
        assert _close(ms_got, c.flat(ms))
        if momentum:
            assert _close(mom_got, c.flat(mom)) and np.any(mom_got != 0)
        init = c.flat(_params(num_actions))
        n = theta.size
        for lo in (n - 257 * num_actions - num_actions, n - num_actions):       # out_x/b and out_y/b moved
            assert np.all(theta[lo:lo + num_actions] != init[lo:lo + num_actions])
        assert net.get_global_step() == 4
    finally:
        net.close()


def test_gather_and_frames_entry_points_match_the_host_buffer_path():
    import Transport as tp
    num_actions = 3
    net = _net(num_actions, 64)
    t = tp.Transport.create(tp.unique_name("t_cont"), 40, num_actions, 84 * 84 * 4, 8, 6, float_actions=True)
    try:
        _reset(net)
        xk, x, a, y = _batch(33, num_actions, 17)
        net.register_transport(t)
        t.agent_states[:33] = xk.reshape(33, -1)
        ids = np.arange(33, dtype=np.uint32)
        p1, v1 = net.predict_offsets(t.state_offsets(ids))
        p2, v2, _ = net.predict_p_v_logits(xk)
        assert np.array_equal(p1, p2) and np.array_equal(v1, v2)
        want = c.forward(_params(num_actions), x.astype(np.float64))
        assert _close(p1, want["o"]) and _close(v1, want["v"])
        # frames: four frames per agent fill the device queues; the prediction is that of the stacked states
        net.frames_config(4, 210, 160, 3)
        rng = np.random.default_rng(3)
        agents = np.arange(4, dtype=np.int32)
        for i in range(4):
            net.push_frames(rng.integers(0, 256, size=(4, 210, 160, 3), dtype=np.uint8), agents,
                            reset=np.full(4, 1 if i == 0 else 0, np.uint8))
        pf, vf = net.predict_frames(agents)
        states = np.stack([net.frame_state(i)[0] for i in range(4)])
        ps, vs, _ = net.predict_p_v_logits(states)
        assert np.array_equal(pf, ps) and np.array_equal(vf, vs)
        net.unregister_transport()
    finally:
        t.shutdown()
        t.close()
        net.close()


def _member_names():
    names = {"step"}
    for k in c.PARAM_ORDER:
        names.update({k + ":0", k + "/RMSProp:0", k + "/RMSProp_1:0"})
    return names


def test_checkpoint_round_trip_and_cross_kind_refusal(tmp_path):
    num_actions = 3
    _, x, a, y = _batch(12, num_actions, 4)
    cont = _net(num_actions, 16, RMSPROP_MOMENTUM=0.5)
    disc = _net(num_actions, 16, continuous=False, RMSPROP_MOMENTUM=0.5)
    try:
        assert [cont._lib.ga3c_net_param_name(cont._h, i).decode() for i in range(cont._lib.ga3c_net_num_params(cont._h))] == \
            list(c.PARAM_ORDER)
        cont.learning_rate, cont.beta = 1e-3, 0.01
        for _ in range(2):
            cont.train(x, y, a)
        disc.learning_rate, disc.beta = 1e-3, 0.01
        disc.train(x, y, np.eye(num_actions, dtype=np.float32)[np.arange(12) % num_actions])
        cpath, dpath = str(tmp_path / "cont.npz"), str(tmp_path / "disc.npz")
        assert cont._lib.ga3c_net_save(cont._h, cpath.encode()) == 0
        assert disc._lib.ga3c_net_save(disc._h, dpath.encode()) == 0
        theta = cont.get_arena(0)
        with np.load(cpath) as z:
            assert set(z.files) == _member_names() and int(z["step"]) == 2
            off = 0
            for k, shape in ((k, c.param_shapes(num_actions)[k]) for k in c.PARAM_ORDER):
                size = int(np.prod(shape))
                assert z[k + ":0"].shape == shape and np.array_equal(z[k + ":0"].reshape(-1), theta[off:off + size]), k
                off += size
        saved = [cont.get_arena(w) for w in (0, 1, 2)]
        cont.train(x, y, a)
        assert cont._lib.ga3c_net_load(cont._h, cpath.encode()) == 0
        for w, want in zip((0, 1, 2), saved):
            assert np.array_equal(cont.get_arena(w), want), w
        assert cont.get_global_step() == 2
        for net, path in ((cont, dpath), (disc, cpath)):
            before = [net.get_arena(w) for w in (0, 1, 2)]
            step = net.get_global_step()
            assert net._lib.ga3c_net_load(net._h, path.encode()) == -4
            assert all(np.array_equal(net.get_arena(w), b) for w, b in zip((0, 1, 2), before))
            assert net.get_global_step() == step
    finally:
        cont.close()
        disc.close()


def test_refused_with_dual_rmsprop():
    with pytest.raises(RuntimeError):
        _net(3, 16, DUAL_RMSPROP=True)


def test_one_rank_communicator_and_one_hogwild_lane_give_the_same_bits():
    from NetworkVP import Network
    num_actions = 6
    xk, _, a, y = _batch(24, num_actions, 8)
    plain, rccl, hog = _net(num_actions, 32), _net(num_actions, 32), _net(num_actions, 32, train_lanes=2)
    try:
        rccl.comm_init(Network.make_comm_id(), 0, 1)
        for net in (plain, rccl, hog):
            _reset(net)
            net.learning_rate, net.beta = 1e-3, 0.01
            for _ in range(3):
                net.train(xk, y, a)
        for w in (0, 1, 2):
            want = plain.get_arena(w)
            assert np.array_equal(rccl.get_arena(w), want), w
            assert np.array_equal(hog.get_arena(w), want), w
        assert plain.get_global_step() == rccl.get_global_step() == hog.get_global_step() == 3
    finally:
        for net in (plain, rccl, hog):
            net.close()


@pytest.mark.timeout(180)
@pytest.mark.filterwarnings("error::pytest.PytestUnhandledThreadExceptionWarning")
def test_server_trains_with_continuous_input(tmp_path, monkeypatch):
    """The engine end to end (agents, transport with float action rows, predictor and trainer threads, zero-copy intake,
    state cache) with CONTINUOUS_INPUT=True: it trains, nothing dies, the weights move, and the actions lie in (-1, 1]."""
    import ga3c_amd  # noqa: F401
    from Config import Config
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(Config, "ZERO_COPY", True)
    monkeypatch.setattr(Config, "STATE_CACHE", True)
    with _config(CONTINUOUS_INPUT=True, DISCRATE_INPUT=True, AGENTS=6, PREDICTORS=2, TRAINERS=1,
                 SYNTHETIC_EPISODE_LENGTH=40, TIME_MAX=5, DYNAMIC_SETTINGS=False, SAVE_MODELS=False,
                 TRAINING_MIN_BATCH_SIZE=11, NUM_ACTIONS=3, PREDICTION_BATCH_SIZE=32):
        from Server import Server
        srv = Server(max_agents=8)
        seen = []
        orig = srv.train_model_frames             # (the state cache: batches arrive as rows named by (agent, request))

        def spy(agents, seqs, y_r, a, tid):
            seen.append(np.array(a))
            return orig(agents, seqs, y_r, a, tid)
        srv.train_model_frames = spy
        try:
            assert srv.transport.float_actions and not Config.DISCRATE_INPUT
            before = srv.model.get_arena(0)
            srv.main(max_seconds=5)
            after = srv.model.get_arena(0)
            assert srv.predictions_served > 100 and srv.training_step > 5
            assert np.all(np.isfinite(after)) and np.max(np.abs(after - before)) > 1e-5
            assert srv.model.last_losses is not None and np.all(np.isfinite(srv.model.last_losses))
            assert seen, "no batch reached train_model_frames"
            acts = np.concatenate(seen)
            assert acts.dtype == np.float32 and acts.shape[1] == 3
            assert np.all(acts > -1) and np.all(acts <= 1) and np.unique(acts).size > 10
        finally:
            srv.model.close()
