"""-m gpu: ga3c_net_time_kernel replays the step.  Every name is one launcher of the step, so timing a regime's names one by
one, in step order, on the workspace of a batch must rebuild what the step itself left there, bit for bit.

A plain net, A = 6, max_batch 257, f32 states.  Before the names are timed the workspace is made to hold ANOTHER batch's
values (X2) wherever the names under test write, so a name that launches nothing, or another kernel, fails the comparison.

Forward: the reference is predict_resident on X1.  The "step on X2" in between is compute_grads (forward + backward, no
update): the weights must stay those the reference was taken with.  Backward: compute_grads(X1) is the reference,
compute_grads(X2) makes everything stale, evaluate(X1) restores X1's forward and head deltas (it runs the train forward on
train lane 0, the lane the timer uses, through an intake that then stays bound) and leaves dn2, dn1, the slabs and the
gradient arena stale.  At B = 97 the step's conv backward is conv_bwd, which leaves 2 B slabs of either kind: a slab_reduce
that reduced the split path's counts would fail here.

A CONTINUOUS_INPUT net (max_batch 8) runs the same replay at B = 3: its names launch heads_cont and the continuous form of
dense1_bwd_tile because the step's launchers do; only "dense1_dw" and "dense1_bwd", which carry the discrete head's roles,
are refused there.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

A = 6
GA3C_EINVAL, GA3C_ESTATE = -1, -4
NAMES = ("conv_stack_fwd", "conv_stack_fwd_train", "conv_stack_fwd_u8", "conv1_fwd", "conv1_fwd_u8", "conv2_fwd", "conv2_fwd_q",
         "dense1_fwd", "dense1_fwd_frag", "dense1_fwd_valu", "heads", "dense1_bwd_tile", "conv_bwd", "conv_bwd_wdstep", "conv2_dw",
         "conv2_dx", "conv_dw_pair", "conv1_dw", "conv1_dw_u8", "slab_reduce", "rmsprop", "dense1_dw", "dense1_dx", "dense1_bwd")
FORWARD = {3: ("conv_stack_fwd", "dense1_fwd", "heads"),
           130: ("conv1_fwd", "conv2_fwd_q", "dense1_fwd", "heads"),
           257: ("conv1_fwd", "conv2_fwd", "dense1_fwd", "heads")}
BACKWARD = {3: ("dense1_bwd_tile", "conv2_dx", "conv_dw_pair", "slab_reduce"),
            97: ("dense1_bwd_tile", "conv_bwd", "slab_reduce"),
            257: ("dense1_bwd_tile", "conv2_dw", "conv2_dx", "conv1_dw", "slab_reduce")}


def _make(continuous, max_batch):
    import ga3c_amd  # noqa: F401  (puts the flat modules on sys.path)
    from Config import Config
    from NetworkVP import Network
    saved, Config.CONTINUOUS_INPUT = Config.CONTINUOUS_INPUT, continuous
    try:
        n = Network("gpu:0", "time_kernel", A, (84, 84, 4), max_batch=max_batch, predict_lanes=1)
    finally:
        Config.CONTINUOUS_INPUT = saved
    n.beta = 0.01
    return n


@pytest.fixture(scope="module")
def net():
    n = _make(False, 257)
    yield n
    n.close()


@pytest.fixture(scope="module")
def cont_net():
    """CONTINUOUS_INPUT: the timer's launchers are the step's, so they launch this net's head kernels too."""
    n = _make(True, 8)
    yield n
    n.close()


def _batch(bsz, seed, continuous=False):
    rng = np.random.Generator(np.random.PCG64(seed))
    xk = rng.integers(0, 256, size=(bsz, 84, 84, 4), dtype=np.uint8)
    x = xk.astype(np.float32) / np.float32(128.0) - np.float32(1.0)
    a = rng.uniform(-1, 1, size=(bsz, A)).astype(np.float32) if continuous else np.eye(A, dtype=np.float32)[rng.integers(0, A, size=bsz)]
    return x, a, rng.uniform(-1, 1, size=bsz)


def _time(net, name, bsz, iters=1):
    import _native as nat
    ms = nat.C.c_float(-1.0)
    rc = net._lib.ga3c_net_time_kernel(net._h, name.encode(), bsz, iters, nat.C.byref(ms))
    return rc, ms.value


def _upload(net, x, y, a):
    import _native as nat
    x, y, a = nat.as_f32(x), nat.as_f32(y), nat.as_f32(a)
    nat.check(net._lib.ga3c_net_upload(net._h, nat.ptr(x), nat.ptr(y), nat.ptr(a), x.shape[0]), "upload")


def _fetch(net, bsz, names):
    z = bsz * net.z_width
    sizes = {"n2": bsz * 3872, "d1": bsz * 256, "z": z, "p": bsz * A, "v": bsz, "dn2": bsz * 3872, "dn1": bsz * 7056}
    return {n: net.fetch(n, sizes[n]) for n in names}


def _same(a, b):
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_every_name_runs_and_an_unknown_one_is_refused(net):
    x, a, y = _batch(3, 11)
    net.compute_grads(x, y, a)
    for name in NAMES:
        rc, ms = _time(net, name, 3, 2)
        assert rc == 0 and ms > 0.0, (name, rc, ms)
    assert len(NAMES) == 24
    assert _time(net, "no_such_kernel", 3)[0] == GA3C_EINVAL


def test_a_continuous_net_is_refused_the_two_discrete_round1_kernels_only(cont_net):
    x, a, y = _batch(3, 12, True)
    cont_net.compute_grads(x, y, a)
    for name in NAMES:
        rc, ms = _time(cont_net, name, 3, 2)
        if name in ("dense1_dw", "dense1_bwd"):
            assert rc == GA3C_ESTATE, (name, rc)
        else:
            assert rc == 0 and ms > 0.0, (name, rc, ms)


def _forward_replay(net, bsz):
    import _native as nat
    names = ("n2", "d1", "z", "p", "v")
    (x1, a1, y1), (x2, a2, y2) = _batch(bsz, 100 + bsz, net.continuous), _batch(bsz, 200 + bsz, net.continuous)
    _upload(net, x1, y1, a1)
    nat.check(net._lib.ga3c_net_predict_resident(net._h, bsz), "predict_resident")
    want = _fetch(net, bsz, names)
    net.compute_grads(x2, y2, a2)
    stale = _fetch(net, bsz, names)
    assert all(not _same(stale[n], want[n]) for n in names)
    _upload(net, x1, y1, a1)
    for name in FORWARD[bsz]:
        assert _time(net, name, bsz)[0] == 0, name
    got = _fetch(net, bsz, names)
    assert [n for n in names if not _same(got[n], want[n])] == []


def _backward_replay(net, bsz):
    names = ("dn2", "dn1")
    (x1, a1, y1), (x2, a2, y2) = _batch(bsz, 300 + bsz, net.continuous), _batch(bsz, 400 + bsz, net.continuous)
    net.compute_grads(x1, y1, a1)
    want, want_g = _fetch(net, bsz, names), net.get_arena(3)
    net.compute_grads(x2, y2, a2)
    net.evaluate(x1, y1, a1)
    stale, stale_g = _fetch(net, bsz, names), net.get_arena(3)
    assert all(not _same(stale[n], want[n]) for n in names) and not _same(stale_g, want_g)
    for name in BACKWARD[bsz]:
        assert _time(net, name, bsz)[0] == 0, name
    got, got_g = _fetch(net, bsz, names), net.get_arena(3)
    assert [n for n in names if not _same(got[n], want[n])] == []
    off = np.flatnonzero(got_g.view(np.uint32) != want_g.view(np.uint32))
    assert off.size == 0, (off.size, off[:8])


@pytest.mark.parametrize("bsz", sorted(FORWARD))
def test_forward_names_rebuild_the_prediction_step(net, bsz):
    _forward_replay(net, bsz)


@pytest.mark.parametrize("bsz", sorted(BACKWARD))
def test_backward_names_rebuild_the_backward_pass(net, bsz):
    _backward_replay(net, bsz)


def test_the_names_rebuild_a_continuous_nets_step_too(cont_net):
    _forward_replay(cont_net, 3)
    _backward_replay(cont_net, 3)
