"""The cases of tests/test_forward_cases_cpu.py and tests/test_gpu_forward_relative.py (not collected: no test_ prefix): the
image net's forward pass on both sides of every change of its launch rules.  Both files build their cases here, so the
conditions the CPU file asserts are the conditions of the rows the GPU file runs.

    path(B)                   the launch rules restated: (conv form, quarter, dense_ks, dense1 kernel) of a batch of B rows
    SIZES                     both sides of the seven changes of path between 1 and 1025 rows, the 16- and 32-row tile edges
    pool()                    R = 67 uint8 states: 60 random, all 0, all 255, five mid-grey frames with one pixel at 255
    index(B)                  the pool rows of a batch: a permutation of the pool first, uniform draws behind it
    params(head, A)           seeded weights, logits_p/w x 40 (a policy that is neither uniform nor saturated), float32 values
    side(head, A)             the float64 oracle on the pool, e32 of every tensor from its float32 run, max|T| over the pool
    structured(side)          the same over the seven structured rows alone

The forward pass is row-independent, so the oracle runs once per weight set, on the pool, and a batch's reference is
want[index(B)]: that is what makes 1025 rows affordable.  Every comparison divides by max|T| over the POOL (`scaled`), so a
one-row batch needs no factor of its own and e32 is never a single draw.  No case or condition here touches a kernel."""
import functools

import numpy as np

import closeness as c
import continuous_oracle as co
import ga3c_oracle as o
import image_limit_cases as ic

A = 6
R, RANDOM = 67, 60                     # 67: neither a power of two nor a multiple of 16
ZEROS, ONES, IMPULSE0 = 60, 61, 62     # pool rows of the structured states
IMPULSES = ((0, 0), (0, 83), (83, 0), (83, 83), (41, 41))
STRUCTURED = np.arange(RANDOM, R)
POOL_SEED, INDEX_SEED = 6700, 7000
P_SCALE = 40.0
WIDE = (("disc", 64), ("cont", 32))    # AMAX = 64 behind 16, 8 and 4 slabs
ACT_NAMES = ("n1", "n2", "d1")
OUT_NAMES = ("z", "v", "p")
NAMES = ACT_NAMES + OUT_NAMES
WIDTH = {"n1": 21 * 21 * 16, "n2": o.FLAT, "d1": o.HID, "v": 1}

SIZES = (1, 15, 16, 17, 64, 127, 128, 129, 144, 145, 160, 161, 176, 177, 192, 193, 256, 257, 512, 513, 1024, 1025)
TRAIN_SIZES = (1, 17, 128, 129, 161, 193, 257)
VALU_SIZES = (161, 257, 513, 1025)
WIDE_SIZES = (177, 513, 1025)
STRUCTURED_SIZES = (17, 129, 257)
MAX_BATCH = 1025


# ---------------------------------------------------------------- the launch rules, restated
KSTEPS_DENSE = 242                     # ga3c_kernels.hpp:30, FLAT / 16
D1F_AS = 260                           # ga3c_kernels.hpp:837, LDS row stride of dense1_fwd_tile_kernel's flat slice


def dense_ks(bsz):
    """ga3c_engine.hip:229-232 (dense_ks)."""
    if 128 < bsz <= 176:
        return 22
    return 16 if bsz <= 512 else (8 if bsz <= 1024 else 4)


def path(bsz, tile=True):
    """-> (conv form, quarter, dense_ks, dense1 kernel) of a prediction or train step of bsz rows, one lane at work.
    tile=False: a net created under GA3C_D1F_TILE=0."""
    fused = bsz <= 128                                       # ga3c_engine.hip:236, 545 (FUSED_CONV_MAX_B)
    quarter = None if fused else bsz <= 192                  # ga3c_engine.hip:239, 559 (C2F_QUARTER_MAX_B)
    ks = dense_ks(bsz)
    max_steps = (KSTEPS_DENSE + ks - 1) // ks                # ga3c_engine.hip:482
    mt = 1 if bsz <= 128 else 2                              # ga3c_engine.hip:483
    lds = (max_steps * 8 * 256 + 16 * mt * D1F_AS) * 4       # ga3c_kernels.hpp:838 (d1f_lds_floats), bytes
    nrow = (bsz + 16 * mt - 1) // (16 * mt)
    blocks = 8 * nrow * ((ks * 2 + 7) // 8)                  # ga3c_kernels.hpp:894-897 (dense1_fwd_blocks)
    if tile and max_steps <= 16 and lds <= 160 * 1024 and blocks <= 256:     # ga3c_engine.hip:486
        dense1 = "dense1_fwd_tile<%d>" % mt
    else:
        dense1 = "dense1_fwd<%d>" % (1 if bsz <= 256 else 2)                 # ga3c_engine.hip:489-492
    return ("conv_stack_fwd" if fused else "conv1_fwd+conv2_fwd", quarter, ks, dense1)


def changes(lo=1, hi=MAX_BATCH):
    """The sizes B in (lo, hi] at which path(B) differs from path(B - 1)."""
    return [b for b in range(lo + 1, hi + 1) if path(b) != path(b - 1)]


# ---------------------------------------------------------------- rows
@functools.lru_cache(maxsize=None)
def pool():
    """-> (xk uint8 [R, 84, 84, 4], x float32): 60 rows drawn like test_gpu_parity._batch, then all 0, all 255 and five frames
    of 128 (x is exactly 0 there, so n1 = relu(b1) everywhere) with one pixel at 255 in all four planes, at the four corners
    and in the middle: a padding or tap slip at a border moves the frame's own output."""
    rng = np.random.Generator(np.random.PCG64(POOL_SEED))
    xk = np.empty((R, o.H, o.W, o.C), np.uint8)
    xk[:RANDOM] = rng.integers(0, 256, size=(RANDOM, o.H, o.W, o.C), dtype=np.uint8)
    xk[ZEROS], xk[ONES] = 0, 255
    for i, (row, col) in enumerate(IMPULSES):
        xk[IMPULSE0 + i] = 128
        xk[IMPULSE0 + i, row, col, :] = 255
    x = xk.astype(np.float32) / np.float32(128.0) - np.float32(1.0)
    xk.setflags(write=False)
    x.setflags(write=False)
    return xk, x


@functools.lru_cache(maxsize=None)
def index(bsz):
    """The pool rows of the batch of bsz rows: its first min(bsz, R) entries are a permutation of the pool, the rest uniform
    draws, one moved on wherever it repeats the row in front of it -- neighbouring rows always differ.  From 67 rows on every
    pool row is in the batch, from 68 on at least one of them twice (the uniform draws reach every row twice only in the
    large batches: test_forward_cases_cpu.py states at which)."""
    rng = np.random.Generator(np.random.PCG64(INDEX_SEED + bsz))
    idx = rng.permutation(R)[:min(bsz, R)]
    if bsz > R:
        idx = np.concatenate([idx, rng.integers(0, R, size=bsz - R)])
        for i in range(R, bsz):
            if idx[i] == idx[i - 1]:
                idx[i] = (idx[i] + 1) % R
    idx.setflags(write=False)
    return idx


@functools.lru_cache(maxsize=None)
def structured_index(bsz):
    """The batch of the structured rows' own comparison: index(bsz) where that holds all seven (from R rows on); below, the
    seven and bsz - 7 random rows in a seeded order (index(17) holds one structured row)."""
    if bsz >= R:
        return index(bsz)
    assert bsz >= 2 * STRUCTURED.size
    rng = np.random.Generator(np.random.PCG64(INDEX_SEED + 9000 + bsz))
    idx = rng.permutation(np.concatenate([STRUCTURED, rng.permutation(RANDOM)[:bsz - STRUCTURED.size]]))
    idx.setflags(write=False)
    return idx


def rows(bsz, idx=None):
    """-> (idx, xk, x) of a batch."""
    xk, x = pool()
    idx = index(bsz) if idx is None else idx
    return idx, np.ascontiguousarray(xk[idx]), np.ascontiguousarray(x[idx])


def targets(bsz, num_actions=A):
    """One-hot actions and returns for the train form (the forward pass does not read them)."""
    rng = np.random.Generator(np.random.PCG64(INDEX_SEED + 5000 + bsz))
    a = np.eye(num_actions, dtype=np.float32)[rng.integers(0, num_actions, size=bsz)]
    return a, rng.uniform(-1, 1, size=bsz)


# ---------------------------------------------------------------- weights
@functools.lru_cache(maxsize=None)
def params(head, num_actions):
    """float64 dict of float32 values.  Discrete: o.init_params with logits_p/w x 40 -- with the seeded weights max p is 0.18 and
    max|z| 0.1, a policy next to uniform on which a wrong logit moves p by nothing.  Continuous: the weights of
    tests/test_gpu_continuous.py, unscaled."""
    if head == "cont":
        p = dict(co.init_params(num_actions, seed=ic.CONT_SEED))
    else:
        p = dict(o.init_params(num_actions))
        p["logits_p/w"] = np.asarray(p["logits_p/w"]) * P_SCALE
    return {k: np.asarray(v, np.float32).astype(np.float64) for k, v in p.items()}


def flat(head, p):
    return ic.flat(head, p).astype(np.float32)


# ---------------------------------------------------------------- the oracle's side
class Side:
    """want[T]: the float64 oracle's T on some rows, [rows, width]; e32[T]: its float32 run against it; scale[T]: max|T| over
    these rows; got32[T]: the float32 run itself, where the side was built from one."""

    def __init__(self, want, e32, got32=None):
        self.want = {k: np.asarray(w, np.float64).reshape(np.shape(w)[0], -1) for k, w in want.items()}
        self.scale = {k: float(np.max(np.abs(w))) for k, w in self.want.items()}
        self.e32, self.got32 = dict(e32), got32

    @classmethod
    def of_runs(cls, f64, f32, names, rows=slice(None)):
        """From a float64 and a float32 run of the oracle on the same rows; `rows`: the rows to keep."""
        want = {k: np.asarray(f64[k], np.float64).reshape(np.shape(f64[k])[0], -1)[rows] for k in names}
        got32 = {k: np.asarray(f32[k]).reshape(np.shape(f32[k])[0], -1)[rows] for k in names}
        for k in names:
            assert got32[k].dtype == np.float32, (k, got32[k].dtype)      # float32 throughout, or e32 would be a lower limit only
        return cls(want, {k: c.rel_err(got32[k], want[k]) for k in names}, got32)

    def bound(self, name):
        return c.bound(self.e32[name], name)


@functools.lru_cache(maxsize=None)
def side(head="disc", num_actions=A):
    """The oracle on the pool at params(head, A), once in float64 and once in float32: n1, n2, d1, z, v, p at A = 6; p, v, z
    through image_limit_cases.ForwardCase (p: the action vector under "cont", z: [hx | hy]) at the wide heads."""
    _, x = pool()
    p = params(head, num_actions)
    if (head, num_actions) == ("disc", A):
        return Side.of_runs(o.forward(p, x.astype(np.float64), keep=True), o.forward(c.f32_params(p), x, keep=True), NAMES)
    fc = ic.ForwardCase(head, p, x)                          # (asserts that its float32 run is float32)
    return Side(fc.want, fc.e32)


@functools.lru_cache(maxsize=None)
def structured():
    """The seven structured rows of the A = 6 pool as tensors of their own: scale and e32 over those rows only (their n1 peaks
    at 1.04 against the pool's 1.52, the impulse frames' at 0.18, so the pool's scale would hide an error of theirs)."""
    s = side()
    return Side.of_runs(s.want, s.got32, NAMES, STRUCTURED)


def scaled(got, want, scale):
    """(got, want) for closeness.rel_err with max|T| over the pool in place of the batch's own: one element equal to `scale`
    joins both sides (it adds no error and no batch tensor exceeds it)."""
    got = np.asarray(got, np.float64).reshape(-1)
    want = np.asarray(want, np.float64).reshape(-1)
    assert got.shape == want.shape, (got.shape, want.shape)
    assert float(np.max(np.abs(want))) <= scale
    return np.append(got, scale), np.append(want, scale)
