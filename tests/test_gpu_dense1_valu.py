"""-m gpu: dense1 forward on the vector ALU (dense1_fwd_valu_kernel) gives the bits of the two MFMA kernels.

The kernel sums every output as the explicit fmaf chains an f32 MFMA is, in the MFMA kernels' k order, so nothing may
differ: a net created under GA3C_D1F_VALU=1 (every dense1 forward of every step on the new kernel) must leave the d1, z, p, v
whose SHA-256 digests tests/golden/forward_bits_parent.json holds (recorded from the MFMA kernels; read here, never
written), and the same partial slabs `part`, byte for byte, as a net created with the switch unset.

Cases (A = 6, seeded weights and f32 states as tests/test_gpu_forward_prefetch.py makes them), one resident prediction step:
  B = 1    one valid row of a row group
  B = 17   a row group with one valid row behind full ones
  B = 128  15- and 16-step slices: ring tails of 3 and 0 (the MFMA ring), 1 and 0 (this kernel's)
  B = 130  22 slices of 11 steps
and at B = 128 two prediction lanes at once, with the switch unset (the engine's own choice of kernel) and set.

The kernel is slower than the MFMA kernels, alone and beside a conv stack (profiles/README.md, "dense1 on the vector ALU"),
so no launch rule picks it: GA3C_D1F_VALU=1 is the only way to it.
"""
import hashlib
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

A = 6
BATCHES = (1, 17, 128, 130)
NAMES = ("d1", "z", "p", "v")
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "forward_bits_parent.json")


def _dense_ks(bsz):
    """The engine's slice count (dense_ks) at the batches of this file."""
    return 22 if 128 < bsz <= 176 else 16


def _states(bsz):
    rng = np.random.Generator(np.random.PCG64(900 + bsz))
    xk = rng.integers(0, 256, size=(bsz, 84, 84, 4), dtype=np.uint8)
    return xk.astype(np.float32) / np.float32(128.0) - np.float32(1.0)


def _make_net(valu):
    """A net with seeded weights; valu=True: created under GA3C_D1F_VALU=1, else with the switch unset (both read at create time)."""
    import ga3c_amd  # noqa: F401
    import ga3c_oracle as o
    from NetworkVP import Network
    old = os.environ.pop("GA3C_D1F_VALU", None)
    if valu:
        os.environ["GA3C_D1F_VALU"] = "1"
    try:
        net = Network("gpu:0", "d1_valu_%d" % valu, A, (84, 84, 4), max_batch=130, predict_lanes=2)
    finally:
        os.environ.pop("GA3C_D1F_VALU", None)
        if old is not None:
            os.environ["GA3C_D1F_VALU"] = old
    params = o.init_params(A)
    net.set_arena(0, np.concatenate([np.asarray(params[k]).reshape(-1) for k in o.PARAM_ORDER]))
    return net


def _resident_forward(net, bsz):
    """One resident prediction step on the batch; what it left in HBM, the partial slabs included."""
    import _native as nat
    x = _states(bsz)
    y, a = np.zeros(bsz, np.float32), np.zeros((bsz, A), np.float32)
    nat.check(net._lib.ga3c_net_upload(net._h, nat.ptr(x), nat.ptr(y), nat.ptr(a), bsz), "upload")
    nat.check(net._lib.ga3c_net_predict_resident(net._h, bsz), "predict_resident")
    nat.check(net._lib.ga3c_net_sync(net._h), "sync")
    sizes = {"d1": bsz * 256, "z": bsz * A, "p": bsz * A, "v": bsz, "part": _dense_ks(bsz) * bsz * 256}
    return {n: net.fetch(n, c) for n, c in sizes.items()}


def _digests(arrays):
    return {n: hashlib.sha256(np.ascontiguousarray(arrays[n], dtype=np.float32).tobytes()).hexdigest() for n in NAMES}


@pytest.fixture(scope="module")
def parent_bits():
    with open(FIXTURE) as f:
        return json.load(f)["digests"]


@pytest.fixture(scope="module")
def nets():
    made = {}

    def get(valu):
        if valu not in made:
            made[valu] = _make_net(valu)
        return made[valu]
    yield get
    for n in made.values():
        n.close()


@pytest.mark.parametrize("bsz", BATCHES)
def test_valu_bits_are_the_mfma_kernels(nets, parent_bits, bsz):
    got = _resident_forward(nets(True), bsz)
    ref = _resident_forward(nets(False), bsz)
    assert got["part"].tobytes() == ref["part"].tobytes(), \
        "first differing slab element: %s" % (np.flatnonzero(got["part"].view(np.uint32) != ref["part"].view(np.uint32))[:1],)
    want = {n: parent_bits["B%d_f32" % bsz][n] for n in NAMES}
    assert _digests(got) == want, [n for n in NAMES if _digests(got)[n] != want[n]]


@pytest.mark.parametrize("valu", [False, True], ids=["unset", "valu"])
def test_two_lanes_give_the_bits_of_one(nets, parent_bits, valu):
    """Two prediction lanes in flight at 128 rows, dense1 beside the other lane's conv stack: with the switch unset the kernel
    is the engine's choice, under GA3C_D1F_VALU=1 it is the vector-ALU kernel on both lanes."""
    import _native as nat
    net, bsz = nets(valu), 128
    alone = _resident_forward(net, bsz)
    assert _digests(alone) == {n: parent_bits["B128_f32"][n] for n in NAMES}
    ms = nat.C.c_float()
    nat.check(net._lib.ga3c_net_time_predict_lanes(net._h, bsz, 6, 2, nat.C.byref(ms)), "time_predict_lanes")
    for lane in (0, 1):
        for name, n in (("p", bsz * A), ("v", bsz)):
            buf = np.empty(n, dtype=np.float32)
            nat.check(net._lib.ga3c_net_fetch_lane(net._h, lane, name.encode(), nat.ptr(buf), n), "fetch_lane")
            assert np.array_equal(buf, alone[name].reshape(-1)), (lane, name)
