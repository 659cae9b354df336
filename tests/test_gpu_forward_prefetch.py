"""-m gpu: the forward kernels whose operand prefetches were re-scheduled (conv_stack_fwd, dense1_fwd, dense1_fwd_tile)
still give the bits they gave before.

tests/golden/forward_bits_parent.json holds SHA-256 digests of the raw f32 bytes of n2, d1, z, p, v, recorded on an MI355X
from a build of the PARENT commit of the change (a `git worktree` of it, built with its own Makefile):

    python tests/test_gpu_forward_prefetch.py --tree <built checkout of the parent commit> --record tests/golden/forward_bits_parent.json

The recording imports the package and the library from --tree, never from this tree, and refuses to write unless the
parent's own two dense1 kernels agree with each other.  The test below never writes the fixture.

Cases (A = 6, seeded weights and states as tests/test_gpu_parity.py makes them), f32 and uint8 states each, each once with
the LDS-tiled dense1 and once with GA3C_D1F_TILE=0 (the register-fragment kernel):
  B = 1    one valid row of a 16-row tile; the conv stack's partial XCD group
  B = 17   a second row block with one valid row
  B = 128  15- and 16-step K slices: ring tails of 3 and 0 steps
  B = 130  11-step slices, tail 3, two row tiles per wave in the tiled kernel; the split conv path (untouched)
  B = 260  (f32 only) beyond 256 rows the fragment kernel runs two row tiles per wave
and at B = 128 two prediction lanes at once (the engine then picks the fragment kernel by itself) against one lane alone.
"""
import hashlib
import json
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

A = 6
BATCHES = (1, 17, 128, 130)
NAMES = ("n2", "d1", "z", "p", "v")
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "forward_bits_parent.json")
CASES = [(b, dt) for b in BATCHES for dt in ("f32", "u8")] + [(260, "f32")]


def _states(bsz):
    rng = np.random.Generator(np.random.PCG64(900 + bsz))
    xk = rng.integers(0, 256, size=(bsz, 84, 84, 4), dtype=np.uint8)
    return xk, xk.astype(np.float32) / np.float32(128.0) - np.float32(1.0)


def _make_net(tile):
    """A net with seeded weights; tile=False: created under GA3C_D1F_TILE=0 (the switch is read at create time)."""
    import ga3c_amd  # noqa: F401
    import ga3c_oracle as o
    from NetworkVP import Network
    old = os.environ.pop("GA3C_D1F_TILE", None)
    if not tile:
        os.environ["GA3C_D1F_TILE"] = "0"
    try:
        net = Network("gpu:0", "fwd_bits_%d" % tile, A, (84, 84, 4), max_batch=260, predict_lanes=2)
    finally:
        os.environ.pop("GA3C_D1F_TILE", None)
        if old is not None:
            os.environ["GA3C_D1F_TILE"] = old
    params = o.init_params(A)
    net.set_arena(0, np.concatenate([np.asarray(params[k]).reshape(-1) for k in o.PARAM_ORDER]))
    return net


def _upload(net, bsz, dtype):
    import _native as nat
    xk, x = _states(bsz)
    y, a = np.zeros(bsz, np.float32), np.zeros((bsz, A), np.float32)
    if dtype == "u8":
        nat.check(net._lib.ga3c_net_upload_u8(net._h, nat.ptr(xk, nat.u8p), nat.ptr(y), nat.ptr(a), bsz), "upload_u8")
    else:
        nat.check(net._lib.ga3c_net_upload(net._h, nat.ptr(x), nat.ptr(y), nat.ptr(a), bsz), "upload")


def _resident_forward(net, bsz, dtype):
    """One resident prediction step on the batch; the raw activations and outputs it left in HBM."""
    import _native as nat
    _upload(net, bsz, dtype)
    nat.check(net._lib.ga3c_net_predict_resident(net._h, bsz), "predict_resident")
    nat.check(net._lib.ga3c_net_sync(net._h), "sync")
    sizes = {"n2": bsz * 3872, "d1": bsz * 256, "z": bsz * A, "p": bsz * A, "v": bsz}
    return {n: net.fetch(n, sizes[n]) for n in NAMES}


def _digests(arrays):
    return {n: hashlib.sha256(np.ascontiguousarray(arrays[n], dtype=np.float32).tobytes()).hexdigest() for n in NAMES}


@pytest.fixture(scope="module")
def parent_bits():
    with open(FIXTURE) as f:
        return json.load(f)["digests"]


@pytest.fixture(scope="module")
def nets():
    made = {}

    def get(tile):
        if tile not in made:
            made[tile] = _make_net(tile)
        return made[tile]
    yield get
    for n in made.values():
        n.close()


@pytest.mark.parametrize("tile", [True, False], ids=["tile", "fragment"])
@pytest.mark.parametrize("bsz,dtype", CASES)
def test_forward_bits_are_the_parents(nets, parent_bits, bsz, dtype, tile):
    got = _digests(_resident_forward(nets(tile), bsz, dtype))
    want = parent_bits["B%d_%s" % (bsz, dtype)]
    assert got == want, [n for n in NAMES if got[n] != want[n]]


def test_two_lanes_give_the_bits_of_one(nets, parent_bits):
    """Two prediction lanes in flight: the engine runs dense1's fragment kernel beside the other lane's conv stack."""
    import _native as nat
    net, bsz = nets(True), 128
    alone = _resident_forward(net, bsz, "f32")
    assert _digests(alone) == parent_bits["B128_f32"]
    ms = nat.C.c_float()
    nat.check(net._lib.ga3c_net_time_predict_lanes(net._h, bsz, 6, 2, nat.C.byref(ms)), "time_predict_lanes")
    for lane in (0, 1):
        for name, n in (("p", bsz * A), ("v", bsz)):
            buf = np.empty(n, dtype=np.float32)
            nat.check(net._lib.ga3c_net_fetch_lane(net._h, lane, name.encode(), nat.ptr(buf), n), "fetch_lane")
            assert np.array_equal(buf, alone[name].reshape(-1)), (lane, name)


def _record(tree, out, commit):
    """Digests of the build in `tree` (a built checkout of the parent commit) -> the fixture."""
    tree = os.path.abspath(tree)
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert os.path.realpath(tree) != os.path.realpath(here), "--tree must be a checkout of the parent, not this tree"
    sys.path[:0] = [os.path.join(tree, "oracle"), tree]
    import ga3c_amd
    assert os.path.realpath(os.path.dirname(os.path.dirname(ga3c_amd.__file__))) == os.path.realpath(tree)
    made = {tile: _make_net(tile) for tile in (True, False)}
    digests = {}
    try:
        for bsz, dtype in CASES:
            d = [_digests(_resident_forward(made[tile], bsz, dtype)) for tile in (True, False)]
            assert d[0] == d[1], ("the parent's own dense1 kernels disagree", bsz, dtype)
            digests["B%d_%s" % (bsz, dtype)] = d[0]
    finally:
        for n in made.values():
            n.close()
    with open(out, "w") as f:
        json.dump({"what": "sha256 of the raw f32 bytes of n2, d1, z, p, v after one resident prediction step; A = 6, "
                           "oracle init_params weights, states PCG64(900 + B) uint8 (f32: k / 128 - 1)",
                   "recorded_from": "a build of the parent commit %s on an MI355X (gfx950)" % (commit or "(unknown)"),
                   "digests": digests}, f, indent=1, sort_keys=True)
        f.write("\n")
    print("recorded %d cases from %s" % (len(digests), tree))


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", required=True)
    ap.add_argument("--record", required=True)
    ap.add_argument("--commit", required=True, help="the parent commit that --tree is a checkout of")
    args = ap.parse_args()
    _record(args.tree, args.record, args.commit)
