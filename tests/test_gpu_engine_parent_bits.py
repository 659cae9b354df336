"""-m gpu: the image network's train step, enqueued through one launcher per kernel, still gives the bits it gave before.

The other engine tests hold a step to f64 oracles at tolerances; a change to a grid or a slab count can stay inside those and
still reorder a sum.  tests/golden/engine_bits_parent.json holds SHA-256 digests of raw f32 bytes, recorded on an MI355X from
a build of the PARENT commit of the change (an export of it, built with its own Makefile):

    python tests/test_gpu_engine_parent_bits.py --tree <built checkout of the parent commit> --commit <its hash> \
        --record tests/golden/engine_bits_parent.json

The recording imports the package and the library from --tree, never from this tree, runs every case twice and refuses to
write if any case's two runs differ (the single-lane step sums in a fixed order).  The test below never writes the fixture.

A case is a fresh net (A = 6, max_batch 257, its seeded initial weights; every buffer starts as zeros, so what a step does
not write is the same in every run) and two train steps on seeded batches, as tests/test_gpu_parity.py makes them.  It
digests arenas 0..3 (DUAL_RMSPROP: 0..6) and every name ga3c_net_fetch accepts, B rows of each ("part": 22 slices of B rows).
One batch size per launch regime:
  B = 3    fused forward, split paired backward
  B = 97   fused conv backward, dense1/w stepped in dense1_bwd_tile's epilogue
  B = 128  fused conv backward, dense1/w step deferred into conv_bwd
  B = 130  two-kernel forward with the quarter conv2_fwd, tail LDS in dense1_bwd_tile, 22 K slices
  B = 200  half conv2_fwd, still paired
  B = 257  unpaired conv2_dw / conv1_dw, two row tiles in dense1_fwd
f32 states at every B, uint8 states at 3, 128 and 257.  Configurations: plain (the update fused into the backward kernels),
GRAD_CLIP, momentum 0.9, DUAL_RMSPROP with clip, CONTINUOUS with clip (B = 3 and 128), and plain through compute_grads +
apply_grads (f32 only: compute_grads takes no uint8 states).
"""
import contextlib
import hashlib
import json
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

A = 6
MAX_BATCH = 257
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "engine_bits_parent.json")
BATCHES = (3, 97, 128, 130, 200, 257)
U8_BATCHES = (3, 128, 257)
CONFIGS = {"plain": {}, "clip": dict(USE_GRAD_CLIP=True), "mom": dict(RMSPROP_MOMENTUM=0.9),
           "dualclip": dict(DUAL_RMSPROP=True, USE_GRAD_CLIP=True), "contclip": dict(CONTINUOUS_INPUT=True, USE_GRAD_CLIP=True),
           "grads": {}}
CASES = []
for _cfg in CONFIGS:
    for _b in ((3, 128) if _cfg == "contclip" else BATCHES):
        CASES.append("%s_B%d_f32" % (_cfg, _b))
        if _b in U8_BATCHES and _cfg != "grads":
            CASES.append("%s_B%d_u8" % (_cfg, _b))


@contextlib.contextmanager
def _config(**kw):
    import ga3c_amd  # noqa: F401  (puts the flat modules on sys.path)
    from Config import Config
    saved = {k: getattr(Config, k) for k in kw}
    for k, v in kw.items():
        setattr(Config, k, v)
    try:
        yield
    finally:
        for k, v in saved.items():
            setattr(Config, k, v)


def _batch(bsz, seed, continuous):
    """tests/test_gpu_parity.py's _batch; CONTINUOUS takes float actions in [-1, 1] instead of one-hot rows."""
    rng = np.random.Generator(np.random.PCG64(seed))
    xk = rng.integers(0, 256, size=(bsz, 84, 84, 4), dtype=np.uint8)
    x = xk.astype(np.float32) / np.float32(128.0) - np.float32(1.0)
    act = rng.integers(0, A, size=bsz)
    y = rng.uniform(-1, 1, size=bsz)
    a = rng.uniform(-1, 1, size=(bsz, A)).astype(np.float32) if continuous else np.eye(A, dtype=np.float32)[act]
    return xk, x, a, y


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a, dtype=np.float32).tobytes()).hexdigest()


def _run(case):
    cfg, b, dtype = case.split("_")
    bsz, flags = int(b[1:]), CONFIGS[cfg]
    with _config(**flags):
        from NetworkVP import Network
        net = Network("gpu:0", "bits_" + cfg, A, (84, 84, 4), max_batch=MAX_BATCH, predict_lanes=1)
    try:
        net.learning_rate, net.beta = 3e-4, 0.01
        for step in range(2):
            xk, x, a, y = _batch(bsz, 7000 + 10 * bsz + step, net.continuous)
            if cfg == "grads":
                net.compute_grads(x, y, a)
                net.apply_grads()
            else:
                net.train(xk if dtype == "u8" else x, y, a)
        z = bsz * net.z_width
        sizes = {"n1": bsz * 7056, "n2": bsz * 3872, "d1": bsz * 256, "z": z, "p": bsz * A, "v": bsz, "dz": z, "dv": bsz,
                 "dd1": bsz * 256, "dn2": bsz * 3872, "dn1": bsz * 7056, "x": bsz * 28224, "part": 22 * bsz * 256}
        d = {"fetch:" + n: _sha(net.fetch(n, c)) for n, c in sizes.items()}
        for which in range(7 if flags.get("DUAL_RMSPROP") else 4):
            d["arena%d" % which] = _sha(net.get_arena(which))
        return d
    finally:
        net.close()


@pytest.fixture(scope="module")
def parent_bits():
    with open(FIXTURE) as f:
        return json.load(f)["digests"]


@pytest.mark.parametrize("case", CASES)
def test_engine_bits_are_the_parents(parent_bits, case):
    if case not in parent_bits:
        pytest.fail("%s is not in the fixture" % case)
    got, want = _run(case), parent_bits[case]
    assert sorted(got) == sorted(want)
    assert got == want, sorted(k for k in got if got[k] != want[k])


def _record(tree, out, commit):
    """Digests of the build in `tree` (a built checkout of the parent commit) -> the fixture."""
    tree = os.path.abspath(tree)
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert os.path.realpath(tree) != os.path.realpath(here), "--tree must be a checkout of the parent, not this tree"
    sys.path[:0] = [tree]
    import ga3c_amd
    import _native
    import NetworkVP
    for mod, path in ((ga3c_amd, ga3c_amd.__file__), (_native, _native.__file__), (NetworkVP, NetworkVP.__file__),
                      (_native, _native.HIP_LIB)):
        assert os.path.realpath(path).startswith(os.path.realpath(tree) + os.sep), (mod, path)
    assert os.path.exists(_native.HIP_LIB), "the parent checkout is not built"
    digests, unstable = {}, []
    for case in CASES:
        first, second = _run(case), _run(case)
        if first != second:
            unstable.append((case, sorted(k for k in first if first[k] != second[k])))
            print("NOT REPRODUCIBLE %s: %s" % unstable[-1], flush=True)
        digests[case] = first
        print("ran %s" % case, flush=True)
    if unstable:
        raise SystemExit("nothing written: the parent's own two runs differ in %r" % (unstable,))
    with open(out, "w") as f:
        json.dump({"what": "sha256 of the raw f32 bytes of arenas and fetch buffers after the two steps of each case of "
                           "tests/test_gpu_engine_parent_bits.py",
                   "recorded_from": "a build of the parent commit %s on an MI355X (gfx950)" % commit,
                   "digests": digests}, f, indent=0, sort_keys=True)
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
