"""-m gpu: the image net's forward pass held to its oracle on both sides of every change of its launch rules
(tests/forward_cases.py builds the cases, tests/test_forward_cases_cpu.py asserts from the oracle alone that each is worth
running; tests/README.md, "The image net's forward pass at the seams of its launch rules").

launch_forward, dense_ks and launch_dense1_fwd change kernel, grid or split-K count seven times between 1 and 1025 rows
(forward_cases.path).  Every size of forward_cases.SIZES runs here, on rows of a pool of 67 states whose float64 oracle is
computed once per weight set:

    1. prediction form   n2, d1, z, p, v (n1 too from 129 rows on, where conv1_fwd stores it) against the oracle; row sums of p;
                         every copy of a pool row in a batch has the same bits; uint8 rows and a prediction lane give the same bits
    2. train form        compute_grads: n1, n2, d1, z, p, v against the oracle; d1, z, p, v bit-identical to the prediction form
    3. "same bits"       GA3C_D1F_TILE=0 at every size and GA3C_D1F_VALU=1 at four: part, d1, z, p, v of the default net;
                         the other conv2_fwd unit and the other conv form replayed through ga3c_net_time_kernel
    4. wide heads        A = 64 and CONTINUOUS_INPUT A = 32 behind 16, 8 and 4 slabs
    5. structured rows   all 0, all 255 and the five impulse frames as tensors of their own, at their own scale

Every bound is closeness.py's, rel_err <= max(16 x e32, 2^-20) per tensor, with e32 and max|T| taken over the pool (over the
seven structured rows in 5.).  Nothing is measured from the kernels.  Run with -s for one line per comparison."""
import os

import numpy as np
import pytest

import closeness as c
import forward_cases as fc
import image_limit_cases as ic
from test_gpu_image_limits import ROW_SUM_BOUND

pytestmark = pytest.mark.gpu

SWITCHES = ("GA3C_D1F_TILE", "GA3C_D1F_VALU")
NETS = {"default": ("disc", fc.A, {}), "frag": ("disc", fc.A, {"GA3C_D1F_TILE": "0"}), "valu": ("disc", fc.A, {"GA3C_D1F_VALU": "1"}),
        "disc64": ("disc", 64, {}), "cont32": ("cont", 32, {})}
SMALL = ("part", "d1", "z", "p", "v")


def _make(key):
    """A handle with the case's weights; the two dense1 switches are read at create time."""
    head, num_actions, env = NETS[key]
    import ga3c_amd  # noqa: F401
    from NetworkVP import Network
    saved = {k: os.environ.pop(k, None) for k in SWITCHES}
    os.environ.update(env)
    try:
        with ic.config(CONTINUOUS_INPUT=head == "cont"):
            net = Network("gpu:0", "fwd_rel_" + key, num_actions, (84, 84, 4), max_batch=fc.MAX_BATCH, predict_lanes=1)
    finally:
        for k in SWITCHES:
            os.environ.pop(k, None)
            if saved[k] is not None:
                os.environ[k] = saved[k]
    net.set_arena(0, fc.flat(head, fc.params(head, num_actions)))
    net.beta = 0.01
    return net


@pytest.fixture(scope="module")
def nets():
    import ga3c_amd  # noqa: F401  (puts the flat modules on sys.path)
    from Config import Config
    assert not (Config.USE_LOG_SOFTMAX or Config.DUAL_RMSPROP or Config.CONTINUOUS_INPUT) and Config.MIN_POLICY == 0.0
    made = {}

    def get(key):
        if key not in made:
            made[key] = _make(key)
        return made[key]
    yield get
    for n in made.values():
        n.close()


@pytest.fixture(scope="module")
def default_small():
    """bsz -> part, d1, z, p, v of the default net's resident prediction step on fc.rows(bsz) (float32 rows), kept for the
    tests that claim its bits."""
    return {}


def _bits(t):
    return np.ascontiguousarray(t).view(np.uint32)


def _counts(net, bsz):
    return {"n1": bsz * fc.WIDTH["n1"], "n2": bsz * fc.WIDTH["n2"], "d1": bsz * fc.WIDTH["d1"], "z": bsz * net.z_width,
            "p": bsz * net.num_actions, "v": bsz, "part": fc.dense_ks(bsz) * bsz * fc.WIDTH["d1"]}


def _fetch(net, bsz, names):
    counts = _counts(net, bsz)
    return {n: net.fetch(n, counts[n]).reshape(-1 if n == "part" else bsz, fc.WIDTH["d1"] if n == "part" else counts[n] // bsz)
            for n in names}


def _upload(net, states):
    import _native as nat
    bsz = states.shape[0]
    y, a = np.zeros(bsz, np.float32), np.zeros((bsz, net.num_actions), np.float32)
    if states.dtype == np.uint8:
        nat.check(net._lib.ga3c_net_upload_u8(net._h, nat.ptr(states, nat.u8p), nat.ptr(y), nat.ptr(a), bsz), "upload_u8")
    else:
        nat.check(net._lib.ga3c_net_upload(net._h, nat.ptr(states), nat.ptr(y), nat.ptr(a), bsz), "upload")


def _resident(net, states, names):
    """One resident prediction step on the rows; what it left in HBM."""
    import _native as nat
    bsz = states.shape[0]
    _upload(net, states)
    nat.check(net._lib.ga3c_net_predict_resident(net._h, bsz), "predict_resident")
    nat.check(net._lib.ga3c_net_sync(net._h), "sync")
    return _fetch(net, bsz, names)


def _small_of_default(nets, default_small, bsz):
    if bsz not in default_small:
        default_small[bsz] = _resident(nets("default"), fc.rows(bsz)[2], SMALL)
    return default_small[bsz]


def _time(net, name, bsz):
    import _native as nat
    ms = nat.C.c_float(-1.0)
    assert net._lib.ga3c_net_time_kernel(net._h, name.encode(), bsz, 1, nat.C.byref(ms)) == 0, name


def _hold(failed, label, side, rows, got, names):
    """got[T] (one row per entry of `rows`, indices into the side's rows) against the oracle, at the side's scale and e32."""
    for name in names:
        g, w = fc.scaled(got[name], side.want[name][rows], side.scale[name])
        bnd = side.bound(name)
        err = c.report(label, name, g, w, side.e32[name], bnd)
        if not err <= bnd:
            failed.append((label, name, err, bnd))


def _row_sums(label, p):
    worst = float(np.max(np.abs(p.astype(np.float64).sum(axis=1) - 1.0)))
    print("%-34s %-24s |sum p - 1| %.3e  bound %.3e" % (label, "row sums", worst, ROW_SUM_BOUND))
    assert np.all(p >= 0) and worst <= ROW_SUM_BOUND, (label, worst)


def _copies_agree(label, idx, got, names):
    """Every copy of a pool row inside the batch has the bits of the row's first copy."""
    uniq, first = np.unique(idx, return_index=True)
    lookup = np.zeros(fc.R, np.int64)
    lookup[uniq] = first
    src = lookup[idx]
    differ = [n for n in names if not np.array_equal(_bits(got[n]), _bits(got[n])[src])]
    assert differ == [], (label, "copies of one pool row differ in", differ)


def _same_bits(label, got, ref, names):
    differ = [n for n in names if not np.array_equal(_bits(got[n]).reshape(-1), _bits(ref[n]).reshape(-1))]
    assert differ == [], (label, differ)


# ---------------------------------------------------------------- 1. prediction form
@pytest.mark.parametrize("bsz", fc.SIZES)
def test_prediction_form_at_every_size(nets, default_small, bsz):
    net, side = nets("default"), fc.side()
    idx, xk, x = fc.rows(bsz)
    label = "predict B=%d %s" % (bsz, fc.path(bsz)[3])
    names = (("n1",) if bsz > 128 else ()) + ("n2", "d1", "z", "p", "v")      # conv_stack_fwd's prediction form stores no n1
    got = _resident(net, x, names + ("part",))
    default_small[bsz] = {n: got[n] for n in SMALL}
    failed = []
    _hold(failed, label, side, idx, got, names)
    _row_sums(label, got["p"])
    _copies_agree(label, idx, got, names)
    _same_bits(label + " uint8", _resident(net, xk, names), got, names)
    for states in (x, xk):                                                     # a prediction lane, from host buffers
        p, v, z = net.predict_p_v_logits(states)
        _same_bits(label + " lane %s" % states.dtype, {"p": p, "v": v, "z": z}, got, ("p", "v", "z"))
    assert not failed, failed


# ---------------------------------------------------------------- 2. train form
def _train_form(net, bsz, idx):
    _, _, x = fc.rows(bsz, idx)
    a, y = fc.targets(bsz)
    net.compute_grads(x, y, a)
    return _fetch(net, bsz, fc.NAMES)


@pytest.mark.parametrize("bsz", fc.TRAIN_SIZES)
def test_train_form_matches_the_oracle_and_the_prediction_form(nets, default_small, bsz):
    """conv_stack_fwd_kernel<true, *> (to 128 rows: the only place the fused stack's n1 is seen, each half of a sample storing
    its own rows) and heads_kernel<true, *>."""
    net, side = nets("default"), fc.side()
    pred = _small_of_default(nets, default_small, bsz)
    idx = fc.index(bsz)
    label = "train B=%d %s" % (bsz, fc.path(bsz)[0])
    got = _train_form(net, bsz, idx)
    failed = []
    _hold(failed, label, side, idx, got, fc.NAMES)
    _row_sums(label, got["p"])
    _copies_agree(label, idx, got, fc.NAMES)
    _same_bits(label + " against the prediction form", got, pred, ("d1", "z", "p", "v"))
    assert not failed, failed


# ---------------------------------------------------------------- 3. code that claims "same bits"
@pytest.mark.parametrize("bsz", fc.SIZES)
def test_the_fragment_kernel_gives_the_default_nets_bits(nets, default_small, bsz):
    """GA3C_D1F_TILE=0: dense1_fwd_kernel<1> to 256 rows (16- and 11-step slices), <2> beyond, in place of the tile kernels."""
    want = _small_of_default(nets, default_small, bsz)
    got = _resident(nets("frag"), fc.rows(bsz)[2], SMALL)
    assert got["part"].shape == (fc.dense_ks(bsz) * bsz, 256)
    _same_bits("frag B=%d" % bsz, got, want, SMALL)


@pytest.mark.parametrize("bsz", fc.VALU_SIZES)
def test_the_vector_alu_kernel_gives_the_default_nets_bits(nets, default_small, bsz):
    """GA3C_D1F_VALU=1 behind 22, 16, 8 and 4 slices (11, 16, 31 and 61 steps: one slice per XCD at 8, four idle XCDs at 4)."""
    want = _small_of_default(nets, default_small, bsz)
    got = _resident(nets("valu"), fc.rows(bsz)[2], SMALL)
    _same_bits("valu B=%d" % bsz, got, want, SMALL)


def _stale_then_upload(net, bsz):
    """The step's own n2 of fc.rows(bsz); then the workspace holds ANOTHER batch's n1 and n2 and the rows are staged again."""
    idx, _, x = fc.rows(bsz)
    want = _resident(net, x, ("n2",))
    stale = _resident(net, fc.rows(bsz, (idx + 1) % fc.R)[2], ("n2",))
    assert not np.array_equal(_bits(stale["n2"]), _bits(want["n2"]))
    _upload(net, x)
    return idx, want


@pytest.mark.parametrize("bsz,forced", [(130, "conv2_fwd"), (257, "conv2_fwd_q")])
def test_the_other_conv2_unit_leaves_the_same_n2(nets, bsz, forced):
    """conv2_fwd_kernel<false> (units of eight tiles) where the step picks units of four, and the reverse."""
    assert fc.path(bsz)[1] == (forced == "conv2_fwd")
    net = nets("default")
    idx, want = _stale_then_upload(net, bsz)
    _time(net, "conv1_fwd", bsz)
    _time(net, forced, bsz)
    got = _fetch(net, bsz, ("n2",))
    _same_bits("%s B=%d" % (forced, bsz), got, want, ("n2",))
    failed = []
    _hold(failed, "%s B=%d" % (forced, bsz), fc.side(), idx, got, ("n2",))
    assert not failed, failed


@pytest.mark.parametrize("bsz,forced", [(129, ("conv_stack_fwd",)), (17, ("conv1_fwd", "conv2_fwd"))])
def test_the_other_conv_form_matches_the_oracle(nets, bsz, forced):
    """The fused stack in two rounds of workgroups at 129 rows, the split form at 17.  No bit claim exists between the two
    forms (the fused stack sums conv2 in another order), so n2 is held to the oracle, not to the step's own."""
    assert (fc.path(bsz)[0] == "conv_stack_fwd") != (forced == ("conv_stack_fwd",))
    net = nets("default")
    idx, _ = _stale_then_upload(net, bsz)
    for name in forced:
        _time(net, name, bsz)
    got = _fetch(net, bsz, ("n2",))
    failed = []
    _hold(failed, "forced %s B=%d" % ("+".join(forced), bsz), fc.side(), idx, got, ("n2",))
    _copies_agree("forced B=%d" % bsz, idx, got, ("n2",))
    assert not failed, failed


# ---------------------------------------------------------------- 4. wide heads behind few slabs
@pytest.mark.parametrize("bsz", fc.WIDE_SIZES)
@pytest.mark.parametrize("key", ["disc64", "cont32"])
def test_wide_heads_behind_16_8_and_4_slabs(nets, key, bsz):
    """heads_kernel<false, 64> and heads_cont_kernel<false, 64> summing 16, 8 and 4 slabs of dense1_fwd<1> and <2>."""
    head, num_actions, _ = NETS[key]
    net, side = nets(key), fc.side(head, num_actions)
    idx, xk, x = fc.rows(bsz)
    label = "%s A=%d B=%d ks=%d" % (head, num_actions, bsz, fc.dense_ks(bsz))
    p, v, z = net.predict_p_v_logits(x)
    assert p.shape == (bsz, num_actions) and v.shape == (bsz,) and z.shape == (bsz, net.z_width)
    got = {"p": p, "v": v.reshape(bsz, 1), "z": z}
    failed = []
    _hold(failed, label, side, idx, got, fc.OUT_NAMES)
    if head == "cont":
        assert np.all(p > -1) and np.all(p <= 1), label
    else:
        _row_sums(label, p)
    _copies_agree(label, idx, got, fc.OUT_NAMES)
    p8, v8, z8 = net.predict_p_v_logits(xk)
    _same_bits(label + " uint8", {"p": p8, "v": v8, "z": z8}, got, fc.OUT_NAMES)
    assert not failed, failed


# ---------------------------------------------------------------- 5. the structured rows as tensors of their own
@pytest.mark.parametrize("train", [False, True], ids=["predict", "train"])
@pytest.mark.parametrize("bsz", fc.STRUCTURED_SIZES)
def test_structured_rows_at_their_own_scale(nets, bsz, train):
    """All 0, all 255 and the five mid-grey frames with one pixel at 255 (corners and centre): their n1 peaks well below the
    pool's, so scale and e32 are taken over these seven rows."""
    net, side = nets("default"), fc.structured()
    idx = fc.structured_index(bsz)
    names = fc.NAMES if train or bsz > 128 else fc.NAMES[1:]
    got = _train_form(net, bsz, idx) if train else _resident(net, fc.rows(bsz, idx)[2], names)
    sel = np.flatnonzero(idx >= fc.RANDOM)
    assert set(idx[sel]) == set(fc.STRUCTURED)
    failed = []
    _hold(failed, "structured %s B=%d" % ("train" if train else "predict", bsz), side, idx[sel] - fc.RANDOM,
          {n: got[n][sel] for n in names}, names)
    assert not failed, failed
