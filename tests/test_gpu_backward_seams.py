"""-m gpu: the image net's backward pass and production step ABOVE 160 rows, every tensor relative to its own largest entry
(tests/backward_cases.py builds the cases, tests/test_backward_cases_cpu.py asserts from the oracle alone that each is worth
running; tests/README.md, "The image net's backward pass and step above 160 rows").

ga3c_net_create admits 65536 rows and BASELINE trains at 512, but test_gpu_backward_relative.py stops at 160 rows and
test_gpu_step_probe.py at 145; above them the suite compared with the oracle at 1e-4 x max(1, max|want|) only, which passes a
bf16-operand conv backward.  Here the backward pass meets the oracle at the 14 sizes of backward_cases.SIZES -- both sides of
every change of launch_backward's rules up to 1025 rows, one row past every boundary of a 128-, 256- or 1024-row loop:

    compute_grads     dz, dv, dd1, dn2, dn1, the ten gradients, the three loss sums
    production step   g_eff from ms' and the signed step after one step from ms = 0 (test_gpu_step_probe's reading), uint8 and
                      f32 rows to the same bits, predictions bit-equal to a handle handed theta'
    a second step     against the oracle at the device's own theta', ms', mom' (plain at 257 rows, momentum 0.9 at 513)
    heavy rows        |y| = 100 at the first row, the last row of the last full chunk and the last row
    last row only     every other row's return is the oracle's v
    gathered rows     train_offsets from a registered segment against train on the same rows, all arenas bit-identical
    wide heads        A = 64, CONTINUOUS_INPUT A = 32, DUAL_RMSPROP A = 64 at 257 and 513 rows

Comparator: closeness.rel_err against max(16 x e32, 2^-20), e32 from the oracle's float32 run of the same entries summed in
the batch's order, the float64 side evaluated with the units the device had on.  Nothing is measured from the kernels.
compute_grads takes float32 rows only (ga3c_net_compute_grads has no uint8 form): uint8 = f32 bits is asserted on the step.
Run with -s for one line per comparison."""
import functools

import numpy as np
import pytest

import backward_cases as bc
import closeness as c
import forward_cases as fc
import ga3c_oracle as o
import image_limit_cases as ic
import test_gpu_image_limits as til

pytestmark = pytest.mark.gpu

LR_SMALL, LR_PROBE = ic.LR_SMALL, ic.LR_PROBE
MOMENTUM = 0.9
ARENAS = (0, 1, 2)


@pytest.fixture(scope="module")
def nets():
    """get(kind) -> a handle made once: "main" and "mom" (RMSPROP_MOMENTUM = 0.9) train, "fresh" is only ever handed weights
    and asked for predictions; get((head, A)) / get((head, A, "fresh")): the wide heads."""
    import ga3c_amd  # noqa: F401
    from Config import Config
    from NetworkVP import Network
    assert (Config.RMSPROP_DECAY, Config.RMSPROP_EPSILON, Config.RMSPROP_MOMENTUM) == (ic.DECAY, ic.EPS, 0.0)
    assert not (Config.USE_GRAD_CLIP or Config.DUAL_RMSPROP or Config.CONTINUOUS_INPUT)
    made = {}

    def get(kind):
        if kind not in made:
            if kind == "main":
                made[kind] = Network("gpu:0", "seams", bc.A, (84, 84, 4), max_batch=bc.MAX_BATCH, predict_lanes=1)
            elif kind == "fresh":
                made[kind] = Network("gpu:0", "seams_fresh", bc.A, (84, 84, 4), max_batch=128, predict_lanes=1)
            elif kind == "mom":
                with ic.config(RMSPROP_MOMENTUM=MOMENTUM):
                    made[kind] = Network("gpu:0", "seams_mom", bc.A, (84, 84, 4), max_batch=513, predict_lanes=1)
            else:
                with ic.config(**til.HEAD_CONFIG[kind[0]]):
                    made[kind] = Network("gpu:0", "seams_%s" % "_".join(map(str, kind)), kind[1], (84, 84, 4),
                                         max_batch=128 if len(kind) == 3 else max(bc.WIDE_SIZES), predict_lanes=1)
        return made[kind]
    yield get
    for n in made.values():
        n.close()


@functools.lru_cache(maxsize=None)
def _plain(bsz):
    """The plain batch of a size and the oracle's e32 of it, shared by the tests of that size."""
    idx = bc.index(bsz)
    return (idx,) + bc.side().e32(idx)


def _theta0():
    return fc.flat("disc", fc.params("disc", bc.A))


def _reset(net, theta, beta=bc.BETA):
    zeros = np.zeros(net.param_count, np.float32)
    net.set_arena(0, theta)
    net.set_arena(1, zeros)
    net.set_arena(2, zeros)
    net.beta = beta


def _units(net, bsz):
    return {k: net.fetch(k, bsz * w).reshape(bsz, w) > 0 for k, w in (("n1", fc.WIDTH["n1"]), ("n2", o.FLAT), ("d1", o.HID))}


def _hold_losses(failed, label, got, want, le32):
    """The three loss sums: rtol 1e-4 as the older files hold them, and relative to 16 x the float32 oracle's own error -- the
    larger of its draw and closeness.e32_of_row_sum of the rows' terms, a sum being one element."""
    assert np.allclose(got, want, rtol=1e-4, atol=1e-4), (label, got, want)
    for i, name in enumerate(bc.LOSSES):
        if want[i] == 0.0:          # beta = 0: no entropy term, in any precision
            assert got[i] == 0.0, (label, name)
            continue
        err, bnd = abs(float(got[i]) - want[i]) / abs(want[i]), max(c.FACTOR * le32[i], c.FLOOR)
        print("%-34s %-24s rel_err %.3e  e32 %.3e  bound %.3e  rel_err/e32 %6.2f" % (label, name, err, le32[i], bnd, err / le32[i]))
        if not err <= bnd:
            failed.append((label, name, err, bnd))


def _check_grads(net, label, side, idx, e32, le32):
    """compute_grads on the batch idx of the side's entries: the fifteen tensors and the loss sums."""
    bsz = idx.size
    _, x, y, a = bc.batch(idx, side.ent)
    net.set_arena(0, fc.flat("disc", side.params))
    net.beta = side.beta
    losses = net.compute_grads(x, y, a)
    want = side.want(idx, _units(net, bsz))
    got = {k: net.fetch(k, want[k].size) for k in c.DELTAS}
    got.update(c.split(net.get_arena(3), bc.A))
    failed = []
    _hold_losses(failed, label, losses, want["loss"], le32)
    for name in c.TENSORS:
        til._hold(failed, label, name, got[name], want[name], e32[name], bc.bound(e32, name, bsz))
    assert not failed, failed


# ---------------------------------------------------------------- 1. compute_grads
@pytest.mark.parametrize("bsz", bc.SIZES)
def test_every_backward_tensor_at_the_seams_above_160_rows(nets, bsz):
    idx, e32, le32 = _plain(bsz)
    _check_grads(nets("main"), "grads B=%d" % bsz, bc.side(), idx, e32, le32)


# ---------------------------------------------------------------- 2. the production step
def _step(net, states, y, a, lr):
    net.learning_rate = lr
    step0 = net.get_global_step()
    net.train(states, y, a)
    assert net.get_global_step() == step0 + 1
    return {w: net.get_arena(w) for w in ARENAS}, np.array(net.last_losses)


@pytest.mark.parametrize("bsz", bc.SIZES)
def test_the_gradient_the_fused_step_used_at_the_seams_above_160_rows(nets, bsz):
    """test_gpu_step_probe._probe's reading of one production step from ms = 0 at LR_PROBE.  The same theta means the same
    oracle tensors as compute_grads: no second oracle pass."""
    net, fresh, side = nets("main"), nets("fresh"), bc.side()
    idx, e32, le32 = _plain(bsz)
    xk, x, y, a = bc.batch(idx)
    label = "step B=%d" % bsz
    theta = _theta0()
    runs = []
    for states in (x, xk):
        _reset(net, theta)
        runs.append(_step(net, states, y, a, LR_PROBE) + (_units(net, bsz),))
    for w in ARENAS:
        assert np.array_equal(til._bits(runs[0][0][w]), til._bits(runs[1][0][w])), (label, "uint8 and f32 rows differ in arena", w)
    assert np.array_equal(til._bits(runs[0][1]), til._bits(runs[1][1])), (label, "loss sums")
    assert all(np.array_equal(runs[0][2][k], runs[1][2][k]) for k in c.ACTS), label
    new, losses, units = runs[0]
    assert not np.any(new[2]), label                         # no momentum: the slot stays zero
    want = side.want(idx, units)
    failed = []
    _hold_losses(failed, label, losses, want["loss"], le32)
    sign, mag = c.g_eff(theta, new[0], new[1], ic.DECAY)
    sign, mag = c.split(sign, bc.A), c.split(mag, bc.A)
    th, th_new = c.split(theta, bc.A), c.split(new[0], bc.A)
    for name in o.PARAM_ORDER:
        g = want[name]
        got, ref = c.signed_or_magnitude(sign[name], mag[name], g)
        bnd = bc.bound(e32, name, bsz)
        til._hold(failed, label, "g " + name, got, ref, e32[name], bnd)
        # the step itself: here the weight's ulp enters, half of it relative to the largest step
        _, delta = ic.want_step(g, 0.0, LR_PROBE)
        bnd_step = bnd + 2.0 ** -23 * float(np.max(np.abs(th[name]))) / float(np.max(np.abs(delta)))
        til._hold(failed, label, "d " + name, th[name].astype(np.float64) - th_new[name], delta, e32[name], bnd_step)
    assert not failed, failed
    # the packed copies the step writes (dense1/w's by conv2_dx_wd_kernel): predictions bit-equal to a handle handed theta'
    fresh.set_arena(0, new[0])
    for got, ref in zip(net.predict_p_v_logits(x[:128]), fresh.predict_p_v_logits(x[:128])):
        assert np.array_equal(til._bits(got), til._bits(ref)), label


@pytest.mark.parametrize("bsz,kind,mu", [(257, "main", 0.0), (513, "mom", MOMENTUM)])
def test_a_second_step_from_the_devices_own_slots(nets, bsz, kind, mu):
    """Two production steps from ms = 0, mom = 0: LR_SMALL, then LR_PROBE from slots that are not zero.  The second is held to
    the oracle at the device's own theta', ms', mom' (float32, so they enter float64 exactly: nothing has to be said about how
    an error of step 1 travels through step 2), with test_gpu_image_limits._check_step's bounds."""
    net = nets(kind)
    idx, e32, le32 = _plain(bsz)
    xk, x, y, a = bc.batch(idx)
    label = "two steps B=%d mu=%.1f" % (bsz, mu)
    _reset(net, _theta0())
    snaps, units, losses = [{w: net.get_arena(w) for w in ARENAS}], [], []
    for lr, states in ((LR_SMALL, x), (LR_PROBE, xk)):
        new, loss = _step(net, states, y, a, lr)
        snaps.append(new)
        losses.append(loss)
        units.append(_units(net, bsz))
    failed = []
    sides = (bc.side(), bc.side_at(snaps[1][0]))
    for step, (side, lr) in enumerate(zip(sides, (LR_SMALL, LR_PROBE))):
        e, le = (e32, le32) if step == 0 else side.e32(idx)
        want = side.want(idx, units[step])
        tag = "%s step %d" % (label, step + 1)
        _hold_losses(failed, tag, losses[step], want["loss"], le)
        til._check_step(tag, "disc", bc.A, bc.Held(e, bsz), want, snaps[step], snaps[step + 1], lr, mu, None, step == 0, failed)
    assert not failed, failed


# ---------------------------------------------------------------- 3. rows that dominate, rows that vanish
@pytest.mark.parametrize("bsz,row,entry", [(b, r, bc.HEAVY[i % 3]) for b, rows in bc.HEAVY_ROWS.items() for i, r in enumerate(rows)])
def test_one_heavy_row_at_the_ends_of_the_chunks(nets, bsz, row, entry):
    """|y| = 100 against U(-1, 1): the row dominates every sum, so a row dropped or counted twice by the last pass of a loop
    shows at full size."""
    side = bc.side()
    idx = bc.index_with(bsz, row, entry)
    _check_grads(nets("main"), "heavy row %d B=%d" % (row, bsz), side, idx, *side.e32(idx))


@pytest.mark.parametrize("bsz", bc.LAST_ROW_SIZES)
def test_only_the_last_row_has_a_gradient_above_160_rows(nets, bsz):
    """One row past the 256-, 512- and 1024-row boundaries, and the row there carries the whole gradient."""
    side, idx = bc.last_row_side()
    _check_grads(nets("main"), "last row only B=%d" % bsz, side, idx[bsz], *side.e32(idx[bsz]))


# ---------------------------------------------------------------- 4. gathered train rows
@pytest.fixture(scope="module")
def gathered():
    import ga3c_amd  # noqa: F401
    from NetworkVP import Network
    import Transport as tp
    slots = (max(bc.GATHER_SIZES) + 5) // 6 + 1
    t = tp.Transport.create(tp.unique_name("t_seams"), 4, bc.A, 84 * 84 * 4, slots, 6)
    net = Network("gpu:0", "seams_gather", bc.A, (84, 84, 4), max_batch=6 * slots, predict_lanes=1)
    net.register_transport(t)
    yield net, t, slots
    net.close()
    t.shutdown()
    t.close()


@pytest.mark.parametrize("bsz", bc.GATHER_SIZES)
def test_a_step_on_gathered_rows_is_the_step_on_the_same_rows(gathered, bsz):
    """launch_gather hands the offsets over in the kernel arguments up to 192 rows and leaves them in the pinned array beyond:
    a uint8 step through train_offsets, the rows scattered over the segment's slots in an order of their own, against train."""
    net, t, slots = gathered
    idx = bc.index(bsz)
    xk, _, y, a = bc.batch(idx)
    rows = xk.reshape(bsz, -1)
    offs = []
    for k, slot in enumerate(reversed(range((bsz + 5) // 6))):
        n = min(6, bsz - 6 * k)
        states, _, _ = t.rollout_views(slot)
        states[:n] = rows[6 * k:6 * k + n]
        offs.append(t.rollout_row_offsets(slot, n))
    offs = np.concatenate(offs)
    assert offs.size == bsz and len(set(offs.tolist())) == bsz
    out = []
    for call in (lambda: net.train_offsets(offs, y, a), lambda: net.train(xk, y, a)):
        _reset(net, _theta0())
        net.learning_rate = LR_PROBE
        call()
        out.append([net.get_arena(w) for w in ARENAS] + [np.array(net.last_losses)])
    assert np.any(out[0][0] != _theta0()) and np.any(out[0][1])
    for got, ref in zip(*out):
        assert np.array_equal(til._bits(got), til._bits(ref)), bsz


# ---------------------------------------------------------------- 5. the wide heads
def _wide(nets, head, num_actions):
    net = nets((head, num_actions))
    net.set_arena(0, ic.flat(head, ic.params(head, num_actions)))
    return net


@pytest.mark.parametrize("bsz", bc.WIDE_SIZES)
@pytest.mark.parametrize("head,num_actions", bc.WIDE)
def test_every_backward_tensor_of_the_wide_heads(nets, head, num_actions, bsz):
    """66 roles dealt over 14 role blocks, each looping three (257 rows) and five (513) times over the batch; under
    DUAL_RMSPROP both costs, with exact zeros where a cost cannot reach a tensor."""
    _, x, a, y = bc.wide_rows(head, num_actions, bsz)
    til._check_grads(_wide(nets, head, num_actions), head, bc.wide_case(head, num_actions, bsz), x, y, a,
                     "%s A=%d B=%d" % (head, num_actions, bsz))


@pytest.mark.parametrize("bsz", bc.WIDE_SIZES)
@pytest.mark.parametrize("head,num_actions", bc.WIDE)
def test_the_production_step_of_the_wide_heads(nets, head, num_actions, bsz):
    """One production step from ms = 0 at LR_PROBE (heads_bwd_role_wide<UPD = true>; under "dual" both optimizers' steps):
    |g_eff|, the step with every entry's sign (at LR_PROBE its bound is the gradient's own), uint8 = f32 bits."""
    net, fresh = _wide(nets, head, num_actions), nets((head, num_actions, "fresh"))
    case = bc.wide_case(head, num_actions, bsz)
    xk, x, a, y = bc.wide_rows(head, num_actions, bsz)
    label = "%s step A=%d B=%d" % (head, num_actions, bsz)
    arenas = (0,) + tuple(w for _, ms, mom, _ in til._slots(head) for w in (ms, mom))
    theta = ic.flat(head, ic.params(head, num_actions)).astype(np.float32)
    runs = []
    for states in (x, xk):
        til._reset(net, head, theta)
        net.learning_rate = LR_PROBE
        prev = {w: net.get_arena(w) for w in arenas}
        net.train(states, y, a)
        runs.append(({w: net.get_arena(w) for w in arenas}, np.array(net.last_losses), til._units(net, case)))
    for w in arenas:
        assert np.array_equal(til._bits(runs[0][0][w]), til._bits(runs[1][0][w])), (label, "uint8 and f32 rows differ in arena", w)
    new, losses, units = runs[0]
    assert np.allclose(losses, til._losses(case), rtol=1e-4, atol=1e-4), (label, losses, til._losses(case))
    failed = []
    til._check_step(label, head, num_actions, case, case.want(units), prev, new, LR_PROBE, 0.0, None, True, failed)
    assert not failed, failed
    fresh.set_arena(0, new[0])
    for got, ref in zip(net.predict_p_v_logits(x[:128]), fresh.predict_p_v_logits(x[:128])):
        assert np.array_equal(til._bits(got), til._bits(ref)), label
