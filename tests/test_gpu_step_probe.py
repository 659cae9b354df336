"""-m gpu: the production step of the image net, ELEMENTWISE, read back through the optimizer's own slots.

`Network.train` on one GPU runs other kernels than compute_grads (fused conv_bwd, conv2_dx_wd, dense1_bwd_tile's epilogue
step, slab_reduce with the fused update; dn1 is not stored and no gradient arena is written), and test_gpu_train_parity.py
sees them through the weights after two steps of lr = 3e-4, which move 99 % of dense1/w's entries by less than the 1e-5 they
are held to (tests/test_closeness_cpu.py).  But RMSProp's slots are an exact probe (fused_rmsprop, ga3c_kernels.hpp): one
step from ms = 0, mom = 0 leaves

    ms' = omr g^2,     theta - theta' = lr g / sqrt(ms' + eps)      =>     g_eff = sign(theta - theta') sqrt(ms' / omr)

which is every gradient element the fused kernels used, to float32 precision, whatever lr was and whatever the weight's
ulp is.  g_eff is held to the oracle's gradient with tests/closeness.py (rel_err per tensor against max(16 x e32, 2^-20), the
float64 side evaluated with the ReLU units the GPU had on).  The step is fused only without gradient clipping and without a
communicator: that is the configuration here.

lr = 0.05 for the probed step.  The SIGN comes from theta - theta', which is zero where the step is below half an ulp of the
weight.  At lr = 3e-4 that is the case for |g| < 5e-7 in dense1/w (weights below 2^-6, step = 9.5e-4 g), above the
2^-20 max|g| ~ 1e-7 under which an entry is compared by magnitude; at 0.05 the step is 0.16 g and every entry that needs a
sign has one.  The magnitude, and so the check, does not depend on lr.
"""
import numpy as np
import pytest

import closeness as c
import ga3c_oracle as o

pytestmark = pytest.mark.gpu

BETA = 0.01
LR_PROBE = 0.05
DECAY, EPS = 0.99, 0.1            # Config.RMSPROP_DECAY / RMSPROP_EPSILON (asserted in the fixture)
# the seams of the train step's launch rules (test_gpu_train_parity.py names them)
SEAMS = [8, 40, 64, 96, 97, 100, 120, 121, 128, 129, 132, 133, 134, 140, 145]


def _flat(d):
    return np.concatenate([np.asarray(d[k]).reshape(-1) for k in o.PARAM_ORDER])


def _batch(bsz, num_actions, seed):
    """The rows of test_gpu_train_parity._batch (same generator, same order of draws)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    xk = rng.integers(0, 256, size=(bsz, 84, 84, 4), dtype=np.uint8)
    x = xk.astype(np.float32) / np.float32(128.0) - np.float32(1.0)
    act = rng.integers(0, num_actions, size=bsz)
    y = rng.uniform(-1, 1, size=bsz)
    return xk, x, np.eye(num_actions, dtype=np.float32)[act], y


@pytest.fixture(scope="module")
def nets():
    """get(A) -> (the net that trains, a second net that is only ever handed weights and asked for predictions)."""
    import ga3c_amd  # noqa: F401
    from Config import Config
    from NetworkVP import Network
    assert (Config.RMSPROP_DECAY, Config.RMSPROP_EPSILON, Config.RMSPROP_MOMENTUM) == (DECAY, EPS, 0.0)
    assert not Config.USE_GRAD_CLIP and not Config.DUAL_RMSPROP
    made = {}

    def get(num_actions):
        if num_actions not in made:
            made[num_actions] = tuple(Network("gpu:0", name, num_actions, (84, 84, 4), max_batch=148, predict_lanes=1)
                                      for name in ("probe", "probe_fresh"))
        return made[num_actions]
    yield get
    for pair in made.values():
        for n in pair:
            n.close()


def _reset(net, theta, ms=None, mom=None):
    zeros = np.zeros(net.param_count, np.float32)
    net.set_arena(0, theta)
    net.set_arena(1, zeros if ms is None else ms)
    net.set_arena(2, zeros if mom is None else mom)
    net.beta = BETA


def _units(net, case):
    return {k: net.fetch(k, case.pre[k].size).reshape(case.bsz, -1) > 0 for k in c.ACTS}


def _want_step(g, ms, lr):
    """The oracle's RMSProp step for gradient g from slot ms, with the engine's float32 constants: -> (ms', step)."""
    omr = np.float64(np.float32(1.0) - np.float32(DECAY))
    ms_new = ms + (g * g - ms) * omr
    return ms_new, g * np.float64(np.float32(lr)) / np.sqrt(np.float64(np.float32(EPS)) + ms_new)


def _probe(net, fresh, label, case, train, xp):
    """One production step from ms = 0, mom = 0 through `train()`; g_eff and the step itself against the oracle, tensor by
    tensor; then the predictions against a net handed theta' (the packed copies the step writes)."""
    num_actions = net.num_actions
    theta = _flat(case.params).astype(np.float32)
    _reset(net, theta)
    net.learning_rate = LR_PROBE
    step0 = net.get_global_step()
    train()
    assert net.get_global_step() == step0 + 1
    theta_new, ms_new = net.get_arena(0), net.get_arena(1)
    want_l = np.array([case.losses["cost_p_1_agg"], case.losses["cost_p_2_agg"], case.losses["cost_v"]])
    assert np.allclose(net.last_losses, want_l, rtol=1e-4, atol=1e-4), (net.last_losses, want_l)
    want = case.want(_units(net, case))
    sign, mag = c.g_eff(theta, theta_new, ms_new, DECAY)
    sign, mag = c.split(sign, num_actions), c.split(mag, num_actions)
    th, th_new = c.split(theta, num_actions), c.split(theta_new, num_actions)
    failed = []
    for name in o.PARAM_ORDER:
        g = np.asarray(want[name], np.float64).reshape(-1)
        got, ref = c.signed_or_magnitude(sign[name], mag[name], g)
        bnd = case.bound(name)
        err = c.report(label, "g " + name, got, ref, case.e32[name], bnd)
        if not err <= bnd:
            failed.append(("g_eff", name, err, bnd))
        # the step itself: here the weight's ulp enters, half of it relative to the largest step
        _, delta = _want_step(g, 0.0, LR_PROBE)
        bnd_step = bnd + 2.0 ** -23 * float(np.max(np.abs(th[name]))) / float(np.max(np.abs(delta)))
        err = c.report(label, "d " + name, th[name].astype(np.float64) - th_new[name], delta, case.e32[name], bnd_step)
        if not err <= bnd_step:
            failed.append(("step", name, err, bnd_step))
    assert not failed, (label, failed)
    fresh.set_arena(0, theta_new)
    assert all(np.array_equal(g, w) for g, w in zip(net.predict_p_v_logits(xp), fresh.predict_p_v_logits(xp))), label


@pytest.mark.parametrize("bsz", SEAMS)
@pytest.mark.parametrize("num_actions", [6, 18])
def test_the_gradient_the_fused_step_used_matches_the_oracle_elementwise(nets, num_actions, bsz):
    net, fresh = nets(num_actions)
    xk, x, a, y = _batch(bsz, num_actions, 7000 + 10 * bsz + num_actions)
    case = c.OracleCase(o.init_params(num_actions), x, y, a, BETA)
    for fmt, xin in (("f32", x), ("u8", xk)):
        _probe(net, fresh, "A=%d B=%d %s" % (num_actions, bsz, fmt), case, lambda: net.train(xin, y, a), x[:min(bsz, 128)])


@pytest.mark.parametrize("num_actions", [6, 18])
def test_the_probe_through_train_offsets_on_22_rollout_slots(num_actions):
    """132 rows lying in 22 rollout slots of the registered transport, trained through ga3c_net_train_gather."""
    import ga3c_amd  # noqa: F401
    from NetworkVP import Network
    import Transport as tp
    bsz = 132
    t = tp.Transport.create(tp.unique_name("t_probe"), 4, num_actions, 84 * 84 * 4, 24, 6)
    net = Network("gpu:0", "probe132", num_actions, (84, 84, 4), max_batch=136, predict_lanes=1)
    fresh = Network("gpu:0", "probe132_fresh", num_actions, (84, 84, 4), max_batch=136, predict_lanes=1)
    try:
        net.register_transport(t)
        xk, x, a, y = _batch(bsz, num_actions, 7000 + 10 * bsz + num_actions)
        case = c.OracleCase(o.init_params(num_actions), x, y, a, BETA)
        offs = []
        rows = xk.reshape(bsz, -1)
        for k, slot in enumerate(reversed(range(22))):          # slots in an order of their own: the offsets are scattered
            states, _, _ = t.rollout_views(slot)
            states[:6] = rows[6 * k:6 * k + 6]
            offs.append(t.rollout_row_offsets(slot, 6))
        offs = np.concatenate(offs)
        _probe(net, fresh, "A=%d B=132 offsets" % num_actions, case, lambda: net.train_offsets(offs, y, a), x[:128])
    finally:
        net.close()
        fresh.close()
        t.shutdown()
        t.close()


def test_the_momentum_slot_after_one_and_two_steps(monkeypatch):
    """RMSPROP_MOMENTUM = 0.5, two production steps from ms = 0, mom = 0 at every seam: `mom` after step 1 equals the step,
    after step 2 it equals 0.5 mom + step2, per tensor with the comparator's bound.  Step 2's oracle starts from what the GPU
    left after step 1 (theta', ms', mom' are float32 and enter float64 exactly), so each step is checked on its own and
    nothing has to be said about how an error of step 1 travels through step 2."""
    import ga3c_amd  # noqa: F401
    import Config
    from NetworkVP import Network
    mu, lr = 0.5, 3e-4
    monkeypatch.setattr(Config.Config, "RMSPROP_MOMENTUM", mu)
    net = Network("gpu:0", "probe_mom", 6, (84, 84, 4), max_batch=148, predict_lanes=1)
    try:
        for bsz in (8, 40, 64, 96, 97, 100, 120, 121, 128, 129, 133, 134, 140):
            xk, x, a, y = _batch(bsz, 6, 9300 + bsz)
            theta = _flat(o.init_params(6)).astype(np.float32)
            ms = np.zeros(theta.size, np.float32)
            mom = np.zeros(theta.size, np.float32)
            _reset(net, theta)
            net.learning_rate = lr
            failed = []
            for step, xin in ((1, x), (2, xk)):
                shaped = {k: v.astype(np.float64).reshape(o.param_shapes(6)[k]) for k, v in c.split(theta, 6).items()}
                case = c.OracleCase(shaped, x, y, a, BETA)
                net.train(xin, y, a)
                want = case.want(_units(net, case))
                theta_new, ms_new, mom_new = net.get_arena(0), net.get_arena(1), net.get_arena(2)
                assert np.array_equal(theta_new, theta - mom_new)          # theta' = theta - mom', in float32
                for name in o.PARAM_ORDER:
                    g = np.asarray(want[name], np.float64).reshape(-1)
                    _, delta = _want_step(g, c.split(ms, 6)[name].astype(np.float64), lr)
                    want_mom = mu * c.split(mom, 6)[name].astype(np.float64) + delta
                    bnd = case.bound(name)
                    err = c.report("mom step %d B=%d" % (step, bsz), name, c.split(mom_new, 6)[name], want_mom, case.e32[name], bnd)
                    if not err <= bnd:
                        failed.append((step, name, err, bnd))
                theta, ms, mom = theta_new, ms_new, mom_new
            assert not failed, (bsz, failed)
    finally:
        net.close()
