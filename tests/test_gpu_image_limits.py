"""-m gpu: the image net at the action counts ga3c_net_create admits (tests/image_limit_cases.py builds the cases,
tests/test_image_limits_cpu.py asserts from the oracles alone that each is worth running; tests/README.md, "The image net
at the action counts it admits").

launch_heads picks heads_kernel / heads_dual_kernel / heads_cont_kernel<AMAX = 8 | 24 | 64> by the policy columns (A, or 2A under
CONTINUOUS_INPUT), and heads_bwd_role_wide<UPD> steps the head variables in place; above 18 columns (12 under CONTINUOUS_INPUT)
the suite had run two compute_grads batches and nothing else.  Here every head runs on both sides of the two seams, at the
limit and at an odd stride next to it, through predict, compute_grads (+ apply_grads) and two production train steps:

    prediction        f32 and uint8 rows bit-identical; p, v, z against the float64 oracle, row sums of p
    compute_grads     every delta and every variable's gradient (per cost under DUAL_RMSPROP)
    two train steps   plain, momentum, USE_GRAD_CLIP, DUAL_RMSPROP: |g_eff| from ms, the signed step, mom, ms after step 2,
                      then predictions bit-equal to a second handle handed the stepped weights

Every bound is closeness.py's, rel_err <= max(16 x e32, 2^-20) per tensor with e32 from the oracle's float32 run on the same
rows (image_limit_cases.bound: ONE_ROW_FACTOR for the one-element tensors of a one-row batch).  Nothing is measured from the
kernels.  Run with -s for one line per comparison."""
import numpy as np
import pytest

import closeness as c
import dual_oracle as d
import ga3c_oracle as o
import image_limit_cases as ic

pytestmark = pytest.mark.gpu

HEAD_CONFIG = {"disc": {}, "cont": dict(CONTINUOUS_INPUT=True), "dual": dict(DUAL_RMSPROP=True)}
VARIANT_CONFIG = {"plain": {}, "fresh": {}, "momentum": dict(RMSPROP_MOMENTUM=ic.MOMENTUM)}
VARIANT_CONFIG.update(ic.SOFTMAX)
# p = e / sum e, each quotient correctly rounded (half an ulp), the sum of up to 64 positive terms by a butterfly of six
# additions (six roundings, common to all columns), MIN_POLICY's (s + m) / (1 + m A) four more: below 12 roundings of 2^-24
ROW_SUM_BOUND = 12 * 2.0 ** -24
# float32 roundings between g and lr g / sqrt(ms' + eps), relative to the step: g^2 - ms, x omr, + ms (these three reach the step
# at half weight through the root), + eps, sqrt, lr x g, the quotient
STEP_ROUNDINGS = 6
# The two-step tests run every check on fewer (A, B) pairs than predict and compute_grads, which take every pair: a test builds
# an oracle case of its own for the second step, and that is what this file's time goes into.
# Plain and dual: the limit shapes at all five sizes -- 97, 121 and 129 rows are where the site of the fused update changes, and
# a step from slots that are not zero is held to the oracle there -- and every other A at 17 rows.
STEP_CASES = [(h, A, B) for h, A, B in ic.CASES if A in ic.LIMIT[h] or B == 17]
# Momentum and USE_GRAD_CLIP, a REDUCTION against the plain variant: every A of the two single-optimizer heads at 17 rows only,
# the limit shapes at 17 and 129 (image_limit_cases.variant_sizes); neither runs at 1, 97 or 121 rows.
VARIANT_CASES = [(h, A, B) for h, A, B in ic.CASES if h != "dual" and B in ic.variant_sizes(h, A)]


def _make(head, num_actions, variant="plain", **kw):
    from NetworkVP import Network
    cfg = dict(HEAD_CONFIG[head], **VARIANT_CONFIG.get(variant, {}))
    cfg.update(kw)
    with ic.config(**cfg):
        return Network("gpu:0", "limits_%s_%s" % (head, variant), num_actions, (84, 84, 4), max_batch=ic.MAX_BATCH, predict_lanes=1)


@pytest.fixture(scope="module")
def nets():
    """get(head, A, variant) -> the handle, made once per module."""
    import ga3c_amd  # noqa: F401
    from Config import Config
    assert (Config.RMSPROP_DECAY, Config.RMSPROP_EPSILON, Config.RMSPROP_MOMENTUM) == (ic.DECAY, ic.EPS, 0.0)
    assert not (Config.USE_GRAD_CLIP or Config.DUAL_RMSPROP or Config.CONTINUOUS_INPUT or Config.USE_LOG_SOFTMAX)
    assert Config.MIN_POLICY == 0.0 and Config.LOG_EPSILON == 1e-6
    made = {}

    def get(head, num_actions, variant="plain", **kw):
        key = (head, num_actions, variant)
        if key not in made:
            made[key] = _make(head, num_actions, variant, **kw)
        return made[key]
    yield get
    for n in made.values():
        n.close()


def _slots(head):
    """-> ((tag, ms arena, mom arena, the variables that optimizer steps), ...): one optimizer, or DUAL_RMSPROP's two."""
    if head == "dual":
        return (("p:", 1, 2, tuple(k for k in o.PARAM_ORDER if k not in d.HEAD_V)),
                ("v:", 4, 5, tuple(k for k in o.PARAM_ORDER if k not in d.HEAD_P)))
    return (("", 1, 2, ic.order(head)),)


def _reset(net, head, theta):
    net.set_arena(0, theta)
    for _, ms, mom, _ in _slots(head):
        net.set_arena(ms, np.zeros(net.param_count, np.float32))
        net.set_arena(mom, np.zeros(net.param_count, np.float32))
    net.beta = ic.BETA


def _units(net, case):
    return {k: net.fetch(k, case.pre[k].size).reshape(case.bsz, -1) > 0 for k in c.ACTS}


def _bits(t):
    return np.ascontiguousarray(t).view(np.uint32)


def _losses(case):
    return np.array([case.losses["cost_p_1_agg"], case.losses["cost_p_2_agg"], case.losses["cost_v"]])


def _hold(failed, label, name, got, want, e32, bnd):
    err = c.report(label, name, got, want, e32, bnd)
    if not err <= bnd:
        failed.append((label, name, err, bnd))


# ---------------------------------------------------------------- 1. prediction
def _check_prediction(net, head, fc, xk, x, label, failed):
    A = net.num_actions
    outs = [net.predict_p_v_logits(s) for s in (x, xk)]
    for g32, gu8 in zip(*outs):
        assert np.array_equal(_bits(g32), _bits(gu8)), label
    p, v, z = outs[0]
    assert p.shape == (fc.bsz, A) and v.shape == (fc.bsz,) and z.shape == (fc.bsz, 2 * A if head == "cont" else A)
    for name, got in (("p", p), ("v", v), ("z", z)):
        _hold(failed, label, name, got, fc.want[name], fc.e32[name], ic.bound(fc, name, got.size))
    if head == "cont":
        assert np.all(p > -1) and np.all(p <= 1), label
    else:
        worst = float(np.max(np.abs(p.astype(np.float64).sum(axis=1) - 1.0)))
        print("%-34s %-24s |sum p - 1| %.3e  bound %.3e" % (label, "row sums", worst, ROW_SUM_BOUND))
        assert np.all(p >= 0) and worst <= ROW_SUM_BOUND, (label, worst)


@pytest.mark.parametrize("head,num_actions,bsz", ic.CASES)
def test_predictions_match_the_oracle(nets, head, num_actions, bsz):
    net = nets(head, num_actions)
    net.set_arena(0, ic.flat(head, ic.params(head, num_actions)))
    xk, x, _, _ = ic.rows(head, num_actions, bsz)
    failed = []
    _check_prediction(net, head, ic.forward_case(head, num_actions, bsz), xk, x, "%s A=%d B=%d" % (head, num_actions, bsz), failed)
    assert not failed, failed


@pytest.mark.parametrize("softmax", list(ic.SOFTMAX))
@pytest.mark.parametrize("num_actions", ic.SOFTMAX_A)
def test_the_three_softmax_settings_at_the_wide_heads(nets, num_actions, softmax):
    """default, USE_LOG_SOFTMAX and MIN_POLICY = 0.01 (denominator 1 + min_policy x A), as test_gpu_parity.py runs them at A = 6."""
    net = nets("disc", num_actions, softmax)
    net.set_arena(0, ic.flat("disc", ic.params("disc", num_actions)))
    xk, x, _, _ = ic.rows("disc", num_actions, ic.SOFTMAX_B)
    failed = []
    _check_prediction(net, "disc", ic.forward_case("disc", num_actions, ic.SOFTMAX_B, softmax), xk, x,
                      "%s A=%d B=%d" % (softmax, num_actions, ic.SOFTMAX_B), failed)
    assert not failed, failed


# ---------------------------------------------------------------- 2. compute_grads
def _device_grads(net, head, case):
    """What compute_grads left on the device, keyed like the case's tensors.  Under DUAL_RMSPROP dd1 holds the policy term
    (the value term's buffer and the two passes' dn2 / dn1 have no name to fetch them by); the arenas 3 and 6 hold the two
    costs' gradients."""
    A = net.num_actions
    want = case.g
    if head == "dual":
        got = {"dz": net.fetch("dz", want["dz"].size), "dv": net.fetch("dv", case.bsz), "p:dd1": net.fetch("dd1", want["p:dd1"].size)}
        got.update({"p:" + k: v for k, v in ic.split(head, net.get_arena(3), A).items()})
        got.update({"v:" + k: v for k, v in ic.split(head, net.get_arena(6), A).items()})
        return got
    got = {k: net.fetch(k, want[k].size) for k in c.DELTAS}
    got.update(ic.split(head, net.get_arena(3), A))
    return got


def _check_grads(net, head, case, x, y, a, label):
    net.beta = case.beta
    losses = net.compute_grads(x, y, a)
    want_l = _losses(case)
    assert np.allclose(losses, want_l, rtol=1e-4, atol=1e-4), (label, losses, want_l)
    want = case.want(_units(net, case))
    got = _device_grads(net, head, case)
    zeros = ic.zero_tensors(head, net.num_actions)
    failed = []
    for name, val in got.items():
        if name in zeros:
            assert not np.any(want[name]) and not np.any(val), (label, name)
            continue
        _hold(failed, label, name, val, want[name], case.e32[name], ic.bound(case, name, np.size(want[name])))
    assert not failed, failed
    return want


@pytest.mark.parametrize("head,num_actions,bsz", ic.CASES)
def test_every_backward_tensor_at_the_admitted_action_counts(nets, head, num_actions, bsz):
    net = nets(head, num_actions)
    net.set_arena(0, ic.flat(head, ic.params(head, num_actions)))
    _, x, a, y = ic.rows(head, num_actions, bsz)
    _check_grads(net, head, ic.case(head, num_actions, bsz), x, y, a, "%s A=%d B=%d" % (head, num_actions, bsz))


@pytest.mark.parametrize("num_actions,bsz", ic.NEAR)
def test_the_continuous_head_next_to_its_singularity(nets, num_actions, bsz):
    """dz carries 1 / (X^2 + Y^2).  The rows the main cases leave out (an action with X^2 + Y^2 < 1e-5, radius down to 1.5e-3,
    where float32 loses digits of X = sigmoid(hx) - 0.5 itself) held to the same rule, with e32 taken from these rows: a kernel
    that is merely as ill-conditioned as the oracle passes."""
    net = nets("cont", num_actions)
    net.set_arena(0, ic.flat("cont", ic.params("cont", num_actions)))
    xk, x, a, y = ic.rows("cont", num_actions, bsz, True)
    label = "cont near A=%d B=%d" % (num_actions, bsz)
    failed = []
    _check_prediction(net, "cont", ic.forward_case("cont", num_actions, bsz, near=True), xk, x, label, failed)
    assert not failed, failed
    _check_grads(net, "cont", ic.case("cont", num_actions, bsz, True), x, y, a, label)


# ---------------------------------------------------------------- 3. production steps
def _check_step(label, head, A, case, want, prev, new, lr, mu, clip, first, failed):
    """One RMSProp step of the device, (theta, slots) `prev` -> `new` (float32 arenas keyed 0 and by slot arena), against the
    oracle's step for the gradient `want` (float64, the device's ReLU units) from the device's own `prev`.

    g_eff    first step (ms = 0): ms' = omr g^2, so sqrt(ms' / omr) is |g| element by element; held by bound(g)
    ms       later steps: ms' = (1 - omr) ms + omr g^2 >= omr g^2 with an error of omr x 2 |g| |dg|, so 2 x bound(g), plus the
             three roundings of the update itself (2^-21 covers them)
    step     theta - theta' = sum over the optimizers of mu mom + lr g / sqrt(ms' + eps).  An error dg of g reaches the step
             through d step / d g (image_limit_cases.step_slope), largest where ms' is smallest: so per optimizer
             bound(g) x max|g| x max(slope) plus the STEP_ROUNDINGS of the step's own float32 arithmetic (where |g| is large
             the step saturates at lr / sqrt(omr), the slope vanishes and those roundings are all that is left), summed,
             plus half an ulp of the largest weight; relative to max|step|
    mom      momentum only: mom' = mu mom + step, without the weight's ulp; theta' = theta - mom' exactly

    Signs.  |g_eff| has none.  The step carries every entry's sign, and at LR_PROBE (the second step) its bound is the
    gradient's own, so that step is the signed probe of test_gpu_step_probe.py; at LR_SMALL (the first step) and under
    USE_GRAD_CLIP (both steps) the weight's ulp dominates the step's bound and a sign slip in small entries would pass it.
    There the sign rests on mom (momentum variant, both steps), on compute_grads (the same rows through the same kernels'
    other instantiation) and on apply_grads, which holds g_eff signed through closeness.signed_or_magnitude."""
    th_prev, th_new = ic.split(head, prev[0], A), ic.split(head, new[0], A)
    total = {k: np.zeros(th_prev[k].size) for k in ic.order(head)}
    tol = {k: 0.0 for k in ic.order(head)}
    e32s = {k: 0.0 for k in ic.order(head)}
    for tag, ms_w, mom_w, names in _slots(head):
        ms_prev, ms_new = ic.split(head, prev[ms_w], A), ic.split(head, new[ms_w], A)
        mom_prev, mom_new = ic.split(head, prev[mom_w], A), ic.split(head, new[mom_w], A)
        for k in ic.order(head):
            if k not in names:       # no slot in the reference: the region keeps what it was handed
                assert np.array_equal(ms_new[k], ms_prev[k]) and np.array_equal(mom_new[k], mom_prev[k]), (label, tag, k)
                continue
            name = tag + k
            g = np.asarray(want[name], np.float64).reshape(-1)
            if clip is not None:
                g = o.clip_by_average_norm(g, clip)
            bnd = ic.bound(case, name, g.size)
            msp = ms_prev[k].astype(np.float64)
            want_ms, delta = ic.want_step(g, msp, lr)
            if not np.any(g):        # one action: no policy gradient, in any precision
                assert not np.any(ms_new[k]) and not np.any(mom_new[k]), (label, name)
                continue
            if first:
                assert not np.any(msp)
                _, mag = c.g_eff(th_prev[k], th_new[k], ms_new[k], ic.DECAY)
                _hold(failed, label, "|g| " + name, mag, np.abs(g), case.e32[name], bnd)
            else:
                _hold(failed, label, "ms " + name, ms_new[k], want_ms, case.e32[name], 2.0 * bnd + 2.0 ** -21)
            want_mom = mu * mom_prev[k].astype(np.float64) + delta
            abs_tol = bnd * float(np.max(np.abs(g))) * float(np.max(ic.step_slope(msp, want_ms, lr))) + \
                STEP_ROUNDINGS * 2.0 ** -24 * float(np.max(np.abs(delta)))
            if mu:
                _hold(failed, label, "mom " + name, mom_new[k], want_mom, case.e32[name],
                      abs_tol / float(np.max(np.abs(want_mom))) + 2.0 ** -23)
            else:
                assert not np.any(mom_new[k]), (label, name)
            total[k] += want_mom
            tol[k] += abs_tol
            e32s[k] = max(e32s[k], case.e32[name])
    for k in ic.order(head):
        if not np.any(total[k]):
            assert np.array_equal(th_new[k], th_prev[k]), (label, k)
            continue
        scale = float(np.max(np.abs(total[k])))
        bnd = (tol[k] + len(_slots(head)) * 2.0 ** -24 * float(np.max(np.abs(th_prev[k])))) / scale      # a rounding per optimizer
        _hold(failed, label, "d " + k, th_prev[k].astype(np.float64) - th_new[k], total[k], e32s[k], bnd)
    if mu:
        assert np.array_equal(new[0], prev[0] - new[2]), label          # theta' = theta - mom', in float32


def _two_steps(net, fresh, head, A, bsz, variant, clip=None):
    """Two production steps from ms = 0, mom = 0, f32 rows and uint8 rows bit-identical in every arena after each, and both
    held to the oracle, each at the weights the device started it from (theta', ms', mom' are float32 and enter float64
    exactly, so nothing has to be said about how an error of step 1 travels through step 2): the first at LR_SMALL, the
    second -- from slots that are not zero -- at LR_PROBE (image_limit_cases has the reason)."""
    xk, x, a, y = ic.rows(head, A, bsz)
    label = "%s %s A=%d B=%d" % (head, variant, A, bsz)
    mu = ic.MOMENTUM if variant == "momentum" else 0.0
    arenas = (0,) + tuple(w for _, ms, mom, _ in _slots(head) for w in (ms, mom))
    theta0 = ic.flat(head, ic.params(head, A)).astype(np.float32)
    rates = (ic.LR_SMALL, ic.LR_PROBE)
    runs = []
    for states in (x, xk):
        _reset(net, head, theta0)
        snaps, units, losses = [{w: net.get_arena(w) for w in arenas}], [], []
        step0 = net.get_global_step()
        for lr in rates:
            net.learning_rate = lr
            net.train(states, y, a)
            snaps.append({w: net.get_arena(w) for w in arenas})
            units.append({k: net.fetch(k, pre.size) for k, pre in ic.case(head, A, bsz).pre.items()})
            losses.append(np.array(net.last_losses))
        assert net.get_global_step() == step0 + 2
        runs.append((snaps, units, losses))
    for s32, su8 in zip(runs[0][0], runs[1][0]):
        for w in arenas:
            assert np.array_equal(_bits(s32[w]), _bits(su8[w])), (label, "uint8 and f32 rows differ in arena", w)
    snaps, units, losses = runs[0]
    failed = []
    for step, lr in enumerate(rates):
        case = ic.case(head, A, bsz) if step == 0 else ic.make_case(head, ic.unflat(head, snaps[step][0], A), x, y, a)
        assert np.allclose(losses[step], _losses(case), rtol=1e-4, atol=1e-4), (label, step, losses[step], _losses(case))
        want = case.want({k: units[step][k].reshape(bsz, -1) > 0 for k in c.ACTS})
        _check_step("%s step %d" % (label, step + 1), head, A, case, want, snaps[step], snaps[step + 1], lr, mu, clip,
                    step == 0, failed)
    assert not failed, failed
    # the packed copies the step writes: predictions equal, bit for bit, those of a handle that was handed theta''
    fresh.set_arena(0, snaps[2][0])
    xp = x[:min(bsz, 128)]
    for got, ref in zip(net.predict_p_v_logits(xp), fresh.predict_p_v_logits(xp)):
        assert np.array_equal(_bits(got), _bits(ref)), label


@pytest.mark.parametrize("head,num_actions,bsz", STEP_CASES)
def test_two_production_steps(nets, head, num_actions, bsz):
    """The fused step (heads_bwd_role_wide<UPD = true> for the head variables; under "dual" both optimizers' steps)."""
    _two_steps(nets(head, num_actions), nets(head, num_actions, "fresh"), head, num_actions, bsz, "plain")


@pytest.mark.parametrize("head,num_actions,bsz", VARIANT_CASES)
def test_two_production_steps_with_momentum(nets, head, num_actions, bsz):
    _two_steps(nets(head, num_actions, "momentum"), nets(head, num_actions, "fresh"), head, num_actions, bsz, "momentum")


@pytest.mark.parametrize("head,num_actions,bsz", VARIANT_CASES)
def test_two_production_steps_with_grad_clip(nets, head, num_actions, bsz):
    """USE_GRAD_CLIP: tf.clip_by_average_norm per variable, then the optimizer launch (no fused step).  One clip norm per
    (head, A), which bites on every variable at the first step's gradient of each of the shape's sizes
    (image_limit_cases.clip_norm_of), so one handle serves the shape."""
    clip = ic.clip_norm_of(head, num_actions)
    net = nets(head, num_actions, "clip", USE_GRAD_CLIP=True, GRAD_CLIP_NORM=clip)
    _two_steps(net, nets(head, num_actions, "fresh"), head, num_actions, bsz, "clip", clip)


@pytest.mark.parametrize("head,num_actions", [("disc", 64), ("cont", 32)])
def test_apply_grads_after_compute_grads(nets, head, num_actions):
    """The unfused rmsprop_kernel: compute_grads, then apply_grads at LR_PROBE from ms = 0, mom = 0, against the oracle step
    the fused path is held to -- here with the sign of every entry (test_gpu_step_probe._probe)."""
    bsz = 17
    net = nets(head, num_actions)
    _, x, a, y = ic.rows(head, num_actions, bsz)
    case = ic.case(head, num_actions, bsz)
    label = "%s apply A=%d B=%d" % (head, num_actions, bsz)
    theta = ic.flat(head, ic.params(head, num_actions)).astype(np.float32)
    _reset(net, head, theta)
    want = _check_grads(net, head, case, x, y, a, label)
    net.learning_rate = ic.LR_PROBE
    net.apply_grads()
    new = {w: net.get_arena(w) for w in (0, 1, 2)}
    failed = []
    _check_step(label, head, num_actions, case, want, {0: theta, 1: np.zeros_like(theta), 2: np.zeros_like(theta)}, new,
                ic.LR_PROBE, 0.0, None, True, failed)
    sign, mag = c.g_eff(theta, new[0], new[1], ic.DECAY)
    sign, mag = ic.split(head, sign, num_actions), ic.split(head, mag, num_actions)
    for name in ic.order(head):
        got, ref = c.signed_or_magnitude(sign[name], mag[name], want[name])
        _hold(failed, label, "g " + name, got, ref, case.e32[name], ic.bound(case, name, ref.size))
    assert not failed, failed


# ---------------------------------------------------------------- 4. the saturated policy at the wide heads
@pytest.mark.parametrize("log_softmax", [False, True])
@pytest.mark.parametrize("num_actions", sorted(ic.SATURATED))
def test_saturated_policy_at_the_wide_heads(nets, num_actions, log_softmax):
    """test_gpu_params_and_saturation.test_saturated_policy_forward_gradients_and_train_steps at A = 25 and A = 64, with that
    test's assertions, and a second time with USE_LOG_SOFTMAX (log p from the logits: no clamp, no tf.maximum mask)."""
    net = nets("disc", num_actions, "log_softmax" if log_softmax else "plain")
    ic.check_saturated(num_actions)
    params, xk, x, a, y = ic.saturated(num_actions)
    params = {k: v.copy() for k, v in params.items()}
    kw = dict(use_log_softmax=True) if log_softmax else {}
    ref = o.forward(params, x.astype(np.float64), **kw)
    p64 = ref["p"]
    net.set_arena(0, ic.flat("disc", params).astype(np.float32))
    net.set_arena(1, np.ones(net.param_count, np.float32))
    net.set_arena(2, np.zeros(net.param_count, np.float32))
    net.learning_rate, net.beta = 3e-4, 0.01
    p, v, z = net.predict_p_v_logits(x)
    assert np.max(np.abs(p - p64)) < 1e-4 and np.max(np.abs(v - ref["v"])) < 1e-4
    assert np.max(np.abs(z - ref["z"])) < 1e-4 * max(1.0, np.max(np.abs(ref["z"])))
    mask = p64 > 1e-12                     # small probabilities to RELATIVE precision
    assert np.max(np.abs(p[mask] / p64[mask] - 1.0)) < 2e-3
    losses = net.compute_grads(x, y, a)
    ref_l, ref_g = o.loss_and_grads(params, x.astype(np.float64), y, a.astype(np.float64), 0.01, **kw)
    want_l = np.array([ref_l["cost_p_1_agg"], ref_l["cost_p_2_agg"], ref_l["cost_v"]])
    assert np.allclose(losses, want_l, rtol=1e-4, atol=1e-4), (losses, want_l)
    dz = net.fetch("dz", ref_g["dz"].size).reshape(ref_g["dz"].shape)
    assert np.max(np.abs(dz - ref_g["dz"])) < 1e-4 * max(1.0, np.max(np.abs(ref_g["dz"])))
    got = ic.split("disc", net.get_arena(3), num_actions)
    for name in o.PARAM_ORDER:
        want = np.asarray(ref_g[name]).reshape(-1)
        assert np.max(np.abs(got[name] - want)) < 1e-4 * max(np.max(np.abs(want)), 1.0), name
    ms = {k: np.ones_like(t) for k, t in params.items()}
    for _ in range(2):
        o.train_step(params, ms, x.astype(np.float64), y, a.astype(np.float64), 3e-4, 0.01, **kw)
        net.train(xk, y, a)
    assert np.max(np.abs(net.get_arena(0) - ic.flat("disc", params))) < 2e-5
    want_ms = ic.flat("disc", ms)
    assert np.max(np.abs(net.get_arena(1) - want_ms) / np.maximum(1.0, np.abs(want_ms))) < 1e-4


# ---------------------------------------------------------------- 6. refusals and plumbing at the limit
def test_action_counts_outside_the_admitted_range_are_refused():
    for head, A, words in (("disc", 0, "[1,64]"), ("disc", 65, "[1,64]"), ("cont", 33, "[1,32]"), ("dual", 65, "[1,64]")):
        with pytest.raises(RuntimeError) as info:
            _make(head, A).close()
        assert words in str(info.value), (head, A, str(info.value))
    with pytest.raises(RuntimeError) as info:
        _make("cont", 32, DUAL_RMSPROP=True).close()
    assert "DUAL_RMSPROP" in str(info.value)


@pytest.mark.parametrize("head,num_actions", [("disc", 64), ("cont", 32)])
def test_param_info_and_checkpoint_round_trip_at_the_limit(nets, head, num_actions, tmp_path):
    import _native as nat
    net, other = nets(head, num_actions), nets(head, num_actions, "fresh")
    names = [net._lib.ga3c_net_param_name(net._h, i).decode() for i in range(net._lib.ga3c_net_num_params(net._h))]
    assert names == list(ic.order(head))
    off = 0
    for name in ic.order(head):
        shape = tuple(ic.shapes(head, num_actions)[name])
        assert net._param_info(name) == (off, int(np.prod(shape)), shape), name
        off += int(np.prod(shape))
    assert off == net.param_count
    rng = np.random.default_rng(64)
    arenas = [rng.normal(size=net.param_count).astype(np.float32), rng.uniform(0.5, 2.0, net.param_count).astype(np.float32),
              rng.normal(size=net.param_count).astype(np.float32) * np.float32(1e-3)]
    for w, t in enumerate(arenas):
        net.set_arena(w, t)
    nat.check(net._lib.ga3c_net_set_step(net._h, 6400))
    path, np_path = str(tmp_path / "limit.npz"), str(tmp_path / "from_numpy.npz")
    nat.check(net._lib.ga3c_net_save(net._h, path.encode()), "save")
    with np.load(path, allow_pickle=False) as z:
        assert int(z["step"]) == 6400 and len(z.files) == 1 + 3 * len(ic.order(head))
        for w, suffix in enumerate((":0", "/RMSProp:0", "/RMSProp_1:0")):
            parts = ic.split(head, arenas[w], num_actions)
            for name in ic.order(head):
                assert z[name + suffix].shape == tuple(ic.shapes(head, num_actions)[name]) and z[name + suffix].dtype == np.float32
                assert np.array_equal(z[name + suffix].ravel(), parts[name]), (name, suffix)
        np.savez(np_path, **{k: z[k] for k in z.files})                 # numpy's own container (zip64 member headers)
    nat.check(other._lib.ga3c_net_load(other._h, np_path.encode()), "load of numpy's file")
    for w in range(3):
        assert np.array_equal(other.get_arena(w), arenas[w]), w
    assert other.get_global_step() == 6400
    xk, _, _, _ = ic.rows(head, num_actions, 17)
    for got, ref in zip(net.predict_p_v_logits(xk), other.predict_p_v_logits(xk)):      # the packed copies followed the load
        assert np.array_equal(_bits(got), _bits(ref))


def test_a_checkpoint_of_63_actions_is_refused_by_a_handle_of_64(nets, tmp_path):
    import _native as nat
    small, big = nets("disc", 63), nets("disc", 64, "fresh")
    path = str(tmp_path / "a63.npz")
    nat.check(small._lib.ga3c_net_save(small._h, path.encode()), "save")
    before = [big.get_arena(w) for w in (0, 1, 2)]
    step = big.get_global_step()
    assert big._lib.ga3c_net_load(big._h, path.encode()) != 0
    assert b"logits_p" in nat.hip_lib().ga3c_last_error()
    assert all(np.array_equal(_bits(big.get_arena(w)), _bits(b)) for w, b in zip((0, 1, 2), before))
    assert big.get_global_step() == step
