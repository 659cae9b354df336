"""The relative comparator (tests/closeness.py) bites where the older criteria did not.  Nothing here touches a kernel or a
GPU: the float64 oracle's tensors at B = 5 and five KNOWN-WRONG variants of them, made in numpy:

    tap        conv12's backward (dn1) with one of its 16 taps dropped
    pad        dn1 with conv12's SAME padding taken as 2|1 instead of 1|2
    row        conv11/w's gradient from dn1 with the last batch row left out
    tile       a 16 x 16 tile of dense1/w's gradient transposed
    skipped    an update of dense1/w that is skipped entirely (theta' = theta)

The comparator, with its oracle-derived bound, must reject each of them and must pass the float32 restatement of the RIGHT
computation -- numpy's own order and a second order (the batch rows added one by one, the taps walked backwards).  The older
criteria are stated here as they stand in the GPU tests, and what they let through is asserted:

    old gradient criterion   max|got - want| < 1e-4 x max(1, max|want|)             (test_gpu_parity.py)
    old step criteria        after two steps of lr = 3e-4 from ms = 1: max|got - want| < 1e-5 on the weights, and per tensor
                             | ||got - init|| - ||want - init|| | < 1e-3 ||want - init|| + 1e-7   (test_gpu_train_parity.py)

What was found (B = 5, A = 6; the asserts below hold it):
  * The old gradient criterion REJECTS `tap`, `pad`, `row` and `tile`.  It is a maximum norm, and each of these moves some
    entry by 2e-3 .. 2e-2, far above 1e-4: an absolute 1e-4 is 20 % of a TYPICAL dn1 entry but 2 % of the largest one, and
    a gross error reaches the large entries.  The expectation that such variants slip through it was wrong.  What does slip
    through is an error that stays below 2 % of the largest entry everywhere; the one made here is `bf16`: conv12's backward
    with its two operands rounded to bfloat16 (rel_err 2e-3 of dn1 -- 500 x what float32 costs).
  * The old elementwise weight criterion also REJECTS `skipped` through the few largest entries (the largest moves by 2.9e-5
    in two steps), but 99.6 % of dense1/w's entries move by less than the 1e-5 they are held to: `skipped_small`, a step left
    out on exactly those, passes it, and only the norm rule notices.  `tile` on a typical tile (the one with the median
    content) passes the elementwise criterion AND the norm rule: every check the production step had.
"""
import numpy as np
import pytest

import closeness as c
import ga3c_oracle as o

A, B, BETA, LR = 6, 5, 0.01, 3e-4


def _batch(bsz, num_actions, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    xk = rng.integers(0, 256, size=(bsz, 84, 84, 4), dtype=np.uint8)
    x = xk.astype(np.float32) / np.float32(128.0) - np.float32(1.0)
    act = rng.integers(0, num_actions, size=bsz)
    y = rng.uniform(-1, 1, size=bsz)
    return x, np.eye(num_actions, dtype=np.float32)[act], y


@pytest.fixture(scope="module")
def case():
    x, a, y = _batch(B, A, 300 + B)
    return c.OracleCase(o.init_params(A), x, y, a, BETA)


def _conv2_dx(dn2, w2, n1_on, drop=None, pad=1, reverse=False):
    """dn1 from dn2, written out tap by tap (oracle._conv_bwd's scatter): dn1[2i+u-pad, 2j+v-pad, :] += dn2[i, j, :] . w2[u, v].
    drop = (u, v) leaves that tap out; pad = 2 takes the padding as 2|1; reverse walks the taps backwards."""
    bsz = dn2.shape[0]
    dxp = np.zeros((bsz, 24, 24, 16), dn2.dtype)
    taps = [(u, v) for u in range(4) for v in range(4)]
    for u, v in (reversed(taps) if reverse else taps):
        if (u, v) == drop:
            continue
        dxp[:, u:u + 22:2, v:v + 22:2, :] += dn2.reshape(bsz, 11, 11, 32) @ w2[u, v].T
    return (dxp[:, pad:pad + 21, pad:pad + 21, :] * n1_on.reshape(bsz, 21, 21, 16)).reshape(-1)


def _conv1_dw(x, dn1, rows):
    cols = o._im2col(x[:rows], 8, 4, 21, 2).reshape(rows * 441, 256)
    return (cols.T @ dn1.reshape(-1, 441, 16)[:rows].reshape(rows * 441, 16)).reshape(-1)


def _transposed_tile(g, r0, c0):
    out = g.reshape(o.FLAT, o.HID).copy()
    out[r0:r0 + 16, c0:c0 + 16] = out[r0:r0 + 16, c0:c0 + 16].T.copy()
    return out.reshape(-1)


def _typical_tile(g):
    """The 16 x 16 tile of dense1/w's gradient that transposing changes by the MEDIAN amount (largest entry of t - t^T)."""
    t = g.reshape(o.FLAT // 16, 16, o.HID // 16, 16).transpose(0, 2, 1, 3)
    d = np.abs(t - t.transpose(0, 1, 3, 2)).max(axis=(2, 3)).reshape(-1)
    k = int(np.argsort(d)[d.size // 2])
    return 16 * (k // (o.HID // 16)), 16 * (k % (o.HID // 16))


def _bf16(v):
    """Rounded to bfloat16 (8 bits of significand, round to nearest even), returned in the dtype it came in."""
    bits = np.asarray(v, np.float32).view(np.uint32).astype(np.uint64)
    bits = ((bits + 0x7FFF + ((bits >> 16) & 1)) >> 16) << 16
    return bits.astype(np.uint32).view(np.float32).astype(np.asarray(v).dtype)


def _variants(case, dtype=np.float64):
    """name -> (tensor it spoils, wrong values, right values), all from the float64 oracle's tensors."""
    g, p = case.g, case.params
    dn2, w2, on1 = g["dn2"].astype(dtype), p["conv12/w"].astype(dtype), case.on["n1"]
    x64 = case.x.astype(dtype)
    r0, c0 = _typical_tile(g["dense1/w"])
    return {
        "tap": ("dn1", _conv2_dx(dn2, w2, on1, drop=(2, 1)), g["dn1"]),
        "pad": ("dn1", _conv2_dx(dn2, w2, on1, pad=2), g["dn1"]),
        "row": ("conv11/w", _conv1_dw(x64, g["dn1"], B - 1), g["conv11/w"]),
        "tile": ("dense1/w", _transposed_tile(g["dense1/w"], r0, c0), g["dense1/w"]),
        "bf16": ("dn1", _conv2_dx(_bf16(dn2), _bf16(w2), on1), g["dn1"]),
    }


def _old_gradient_criterion(got, want):
    got, want = np.asarray(got, np.float64).reshape(-1), np.asarray(want, np.float64).reshape(-1)
    return np.max(np.abs(got - want)) < 1e-4 * max(1.0, np.max(np.abs(want)))


def _two_steps(case, spoil=None):
    """dense1/w after two oracle steps of lr = 3e-4 from ms = 1 (the batch is the same in both, as in the GPU tests);
    spoil(g) -> the gradient the step is given instead, or None for no step at all."""
    params = {k: v.copy() for k, v in case.params.items()}
    ms = {k: np.ones_like(v) for k, v in params.items()}
    for _ in range(2):
        _, g = o.loss_and_grads(params, case.x.astype(np.float64), case.y.astype(np.float64), case.a.astype(np.float64), BETA)
        g = {k: np.asarray(g[k]) for k in o.PARAM_ORDER}
        if spoil is not None:
            g["dense1/w"] = spoil(g["dense1/w"].reshape(-1))
        o.rmsprop_update(params, ms, g, LR)
    return params["dense1/w"].reshape(-1)


def _old_weight_criterion(got, want):
    return np.max(np.abs(got - want)) < 1e-5


def _old_norm_rule(got, want, init):
    dw, dg = np.linalg.norm(want - init), np.linalg.norm(got - init)
    return dw > 0 and abs(dg - dw) < 1e-3 * dw + 1e-7


def test_the_written_out_conv2_backward_is_the_oracles(case):
    right = _conv2_dx(case.g["dn2"], case.params["conv12/w"], case.on["n1"])
    assert np.max(np.abs(right - case.g["dn1"].reshape(-1))) < 1e-15
    assert np.max(np.abs(_conv1_dw(case.x.astype(np.float64), case.g["dn1"], B) - case.g["conv11/w"].reshape(-1))) < 1e-14


@pytest.mark.parametrize("name,old_passes", [("tap", False), ("pad", False), ("row", False), ("tile", False), ("bf16", True)])
def test_wrong_gradients_are_rejected_by_the_relative_bound(case, name, old_passes):
    tensor, wrong, right = _variants(case)[name]
    err = c.rel_err(wrong, right)
    print("%-5s %-9s rel_err %.3e  bound %.3e  max|diff| %.3e  old criterion passes it: %s" % (
        name, tensor, err, case.bound(tensor), np.max(np.abs(np.ravel(wrong) - np.ravel(right))), _old_gradient_criterion(wrong, right)))
    assert err > 100 * case.bound(tensor)         # far off, not marginally
    assert _old_gradient_criterion(wrong, right) == old_passes


def test_the_f32_restatement_of_the_right_computation_passes(case):
    """numpy's own order (that IS e32, so it passes by construction: it pins the bookkeeping) and a second summation order in
    float32 throughout: taps walked backwards for dn1, batch rows added one by one for the three weight gradients."""
    for name in c.TENSORS:
        assert c.rel_err(case.g32[name], case.g[name]) <= case.bound(name), name
        assert case.e32[name] < 1e-5, (name, case.e32[name])          # float32 costs 1e-8 .. 4e-6 here, nothing like 1e-4
    f32 = np.float32
    p32 = c.f32_params(case.params)
    f = o.forward(p32, case.x, keep=True)
    g32 = case.g32
    other = {"dn1": _conv2_dx(g32["dn2"], p32["conv12/w"], case.on["n1"], reverse=True)}
    assert other["dn1"].dtype == f32
    dn1 = g32["dn1"].reshape(B, 441, 16)
    dn2 = g32["dn2"].reshape(B, 121, 32)
    dd1 = g32["dd1"].reshape(B, o.HID)
    w1 = np.zeros((256, 16), f32)
    w2 = np.zeros((256, 32), f32)
    wd = np.zeros((o.FLAT, o.HID), f32)
    for r in reversed(range(B)):
        w1 += f["cols1"][r].reshape(441, 256).T @ dn1[r]
        w2 += f["cols2"][r].reshape(121, 256).T @ dn2[r]
        wd += np.outer(f["flat"][r], dd1[r])
    other.update({"conv11/w": w1, "conv12/w": w2, "dense1/w": wd})
    for name, got in other.items():
        assert got.dtype == f32
        err = c.rel_err(got, case.g[name])
        print("%-9s second order: rel_err %.3e  e32 %.3e  bound %.3e" % (name, err, case.e32[name], case.bound(name)))
        assert err <= case.bound(name), name


def test_a_wrong_or_missing_step_of_dense1_w(case):
    """The production step is read back through the optimizer's slots (closeness.g_eff): from ms = 0 one step leaves
    ms' = omr g^2 and theta - theta' = lr g / sqrt(ms' + eps).  A skipped step leaves both untouched, a transposed tile
    moves both; the comparator rejects either.  The old criteria on the weights after two steps: see the module's text."""
    theta = case.params["dense1/w"].reshape(-1)
    want = case.g["dense1/w"].reshape(-1)
    r0, c0 = _typical_tile(want)
    omr, eps, lr = np.float32(1) - np.float32(0.99), np.float32(0.1), np.float32(0.05)

    def fused_step(g):                    # what the engine's fused_rmsprop leaves, in float32
        g = g.astype(np.float32)
        ms = g * g * omr
        return (theta.astype(np.float32) - g * lr / np.sqrt(eps + ms)).astype(np.float32), ms

    def read_back(theta_new, ms_new):
        sign, mag = c.g_eff(theta.astype(np.float32), theta_new, ms_new)
        return c.signed_or_magnitude(sign, mag, want)

    # the right step, float32 throughout, reads back as the gradient it was given
    got, ref = read_back(*fused_step(want))
    assert c.rel_err(got, ref) <= c.FLOOR
    got, ref = read_back(*fused_step(case.g32["dense1/w"].reshape(-1)))
    assert c.rel_err(got, ref) <= case.bound("dense1/w")
    # skipped entirely: theta' = theta, ms' = 0
    got, ref = read_back(theta.astype(np.float32), np.zeros(theta.size, np.float32))
    assert c.rel_err(got, ref) == 1.0 > case.bound("dense1/w")
    # a transposed tile
    got, ref = read_back(*fused_step(_transposed_tile(want, r0, c0)))
    assert c.rel_err(got, ref) > 100 * case.bound("dense1/w")

    # the old criteria, on the weights after two steps of 3e-4 from ms = 1
    right = _two_steps(case)
    moved = np.abs(right - theta)
    skipped = theta.copy()
    skipped_small = np.where(moved < 1e-5, theta, right)
    tile = _two_steps(case, lambda g: _transposed_tile(g, r0, c0))
    print("dense1/w in two steps: largest move %.3e, %.2f %% of the entries move by less than 1e-5; tile: err %.3e" % (
        np.max(moved), 100 * np.mean(moved < 1e-5), np.max(np.abs(tile - right))))
    assert _old_weight_criterion(right, right) and _old_norm_rule(right, right, theta)
    assert not _old_weight_criterion(skipped, right) and not _old_norm_rule(skipped, right, theta)
    assert np.mean(moved < 1e-5) > 0.99
    assert _old_weight_criterion(skipped_small, right) and not _old_norm_rule(skipped_small, right, theta)
    assert _old_weight_criterion(tile, right) and _old_norm_rule(tile, right, theta)


def test_the_seeds_of_the_gpu_probe_keep_the_signless_entries_rare():
    """closeness.signed_or_magnitude's condition, checked here with the float64 oracle on two of the batches the GPU probe
    uses (tests/test_gpu_step_probe.py: the smallest and one of the engine's own sizes)."""
    import test_gpu_train_parity as tp
    for num_actions, bsz in ((6, 8), (18, 40)):
        _, x, a, y = tp._batch(bsz, num_actions, 7000 + 10 * bsz + num_actions)
        _, g = o.loss_and_grads(o.init_params(num_actions), x.astype(np.float64), y.astype(np.float32).astype(np.float64),
                                a.astype(np.float64), BETA)
        for name in o.PARAM_ORDER:
            want = np.asarray(g[name]).reshape(-1)
            c.signed_or_magnitude(np.sign(want), np.abs(want), want)        # asserts the share
