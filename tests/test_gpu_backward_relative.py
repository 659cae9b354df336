"""-m gpu: the compute_grads path of the image net, every tensor RELATIVE to its own largest entry.

test_gpu_parity.py holds dz, dv, dd1, dn2, dn1 and the ten gradient tensors to 1e-4 x max(1, max|want|): absolute below 1,
and with the seeded initial weights every one of them is below 1 (tests/README.md, "how large the tensors are").  Here each
is held with tests/closeness.py: rel_err = max|got - want| / max|want| against max(16 x e32, 2^-20), e32 being what the
numpy oracle loses when it runs the same rows in float32 -- the bound comes from the oracle, never from the kernels.  The
float64 side is evaluated with the ReLU units the GPU had on (fetched n1 / n2 / d1 > 0), which may differ from the oracle's
only where the oracle's own input to the unit is within the activation's bound of zero (closeness.OracleCase.want).

Batches: the (A, B) of test_gradients_match_oracle plus the train sizes 128 / 129 / 133 / 134 / 145, and inputs that random
frames do not reach: rows that are all 0 and all 255, one row whose return is 100 x the others (first, 127, 128, last), and
batches in which only the last row has a gradient.  Run with -s for one line per tensor.
"""
import numpy as np
import pytest

import closeness as c
import ga3c_oracle as o

pytestmark = pytest.mark.gpu

BETA = 0.01
SIZES = [(6, 1), (6, 2), (6, 5), (6, 37), (6, 96), (6, 97), (6, 128), (6, 131), (6, 143), (6, 144), (6, 150), (6, 160),
         (4, 16), (18, 21), (1, 9), (25, 7), (64, 6),
         (6, 129), (6, 133), (6, 134), (6, 145)]


def _batch(bsz, num_actions, seed):
    """The rows of test_gpu_parity._batch (same generator, same order of draws)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    xk = rng.integers(0, 256, size=(bsz, 84, 84, 4), dtype=np.uint8)
    x = xk.astype(np.float32) / np.float32(128.0) - np.float32(1.0)
    act = rng.integers(0, num_actions, size=bsz)
    y = rng.uniform(-1, 1, size=bsz)
    return xk, x, np.eye(num_actions, dtype=np.float32)[act], y


def _flat(d):
    return np.concatenate([np.asarray(d[k]).reshape(-1) for k in o.PARAM_ORDER])


@pytest.fixture(scope="module")
def nets():
    import ga3c_amd  # noqa: F401  (puts the flat modules on sys.path)
    from NetworkVP import Network
    made = {}

    def get(num_actions):
        if num_actions not in made:
            made[num_actions] = Network("gpu:0", "bwd_rel", num_actions, (84, 84, 4), max_batch=160, predict_lanes=1)
            made[num_actions].set_arena(0, _flat(o.init_params(num_actions)))
        return made[num_actions]
    yield get
    for n in made.values():
        n.close()


def _check(net, label, x, y, a, beta):
    """compute_grads on the rows against the oracle: all fifteen tensors with the comparator."""
    num_actions = net.num_actions
    case = c.OracleCase(o.init_params(num_actions), x, y, a, beta)
    net.beta = beta
    losses = net.compute_grads(x, y, a)
    want_l = np.array([case.losses["cost_p_1_agg"], case.losses["cost_p_2_agg"], case.losses["cost_v"]])
    assert np.allclose(losses, want_l, rtol=1e-4, atol=1e-4), (losses, want_l)
    bsz = case.bsz
    on = {k: net.fetch(k, case.pre[k].size).reshape(bsz, -1) > 0 for k in c.ACTS}
    want = case.want(on)
    got = {k: net.fetch(k, want[k].size) for k in c.DELTAS}
    got.update(c.split(net.get_arena(3), num_actions))
    failed = []
    for name in c.TENSORS:
        if not np.any(want[name]):
            # exactly zero in the oracle (one action: the softmax is 1 and has no gradient) -- in float32 as well, and then
            # nothing is rounded: the GPU's tensor is zero too
            assert not np.any(case.g32[name]) and not np.any(got[name]), (label, name)
            continue
        err = c.report(label, name, got[name], want[name], case.e32[name], case.bound(name))
        if not err <= case.bound(name):
            failed.append((name, err, case.bound(name)))
    assert not failed, (label, failed)


@pytest.mark.parametrize("num_actions,bsz", SIZES)
def test_every_backward_tensor_relative_to_its_largest_entry(nets, num_actions, bsz):
    _, x, a, y = _batch(bsz, num_actions, 300 + bsz)
    _check(nets(num_actions), "A=%d B=%d" % (num_actions, bsz), x, y, a, BETA)


@pytest.mark.parametrize("bsz", [6, 97, 130])
def test_rows_that_are_all_0_and_all_255(nets, bsz):
    """x = -1 and x = 127/128 everywhere: the padded border is then the only place where the conv input differs from the
    interior, so a SAME-padding slip of one pixel at the bottom / right edge (2|2 for conv11, 1|2 for conv12) shows.  Constant
    rows alternate with random ones, which keep every hidden unit's gradient alive."""
    xk, _, a, y = _batch(bsz, 6, 2300 + bsz)
    xk[0::3] = 0
    xk[1::3] = 255
    x = xk.astype(np.float32) / np.float32(128.0) - np.float32(1.0)
    _check(nets(6), "const rows B=%d" % bsz, x, y, a, BETA)


@pytest.mark.parametrize("bsz,row", [(133, 0), (133, 127), (133, 128), (133, 132), (145, 0), (145, 127), (145, 128), (145, 144)])
def test_one_row_dominates_every_sum(nets, bsz, row):
    """One row's return is 100 x the others' (|y| = 100 against U(-1, 1), and v is below 1): that row dominates every sum,
    so a row dropped or counted twice in a tail chunk shows at full size."""
    _, x, a, y = _batch(bsz, 6, 3300 + bsz)
    y[row] = 100.0 if y[row] >= 0 else -100.0
    _check(nets(6), "dominant row %d B=%d" % (row, bsz), x, y, a, BETA)


@pytest.mark.parametrize("bsz", [129, 133, 134, 145])
def test_only_the_last_row_has_a_gradient(nets, bsz):
    """For every row but the last y_r is the oracle's own v and beta = 0: their advantage is zero, so dz = dv = 0 up to the
    float32 rounding of v, and the gradient is that of the last row alone.  `want` is the oracle's gradient of the full batch
    as the GPU sees it (float32 y), not an idealised zero."""
    _, x, a, y = _batch(bsz, 6, 4300 + bsz)
    v = o.forward(o.init_params(6), x.astype(np.float64))["v"]
    y = np.concatenate([v[:-1], y[-1:]]).astype(np.float32)
    _check(nets(6), "last row only B=%d" % bsz, x, y, a, 0.0)
