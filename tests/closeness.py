"""The comparator of the relative tests (not collected: no test_ prefix).

    rel_err(got, want) = max|got - want| / max|want|                      per tensor

and a bound that comes from the oracle, never from the code under test: the numpy oracle is run once in float32 and once in
float64 on the same rows; e32(T) = rel_err(g32[T], g64[T]) is what float32 arithmetic costs tensor T in SOME summation order.
The kernels sum in another order (4-wide MFMA chains, split-K slices, slab reduction), so

    bound(T) = max(FACTOR x e32(T), FLOOR),    FACTOR = 16,  FLOOR = 2^-20

16: both orders have an error of about sqrt(n) u for sums of mixed sign, and the ratio between two orders of a sum of
n <= 56 448 terms, taken over many tensors, needs about one decimal digit of head-room.  2^-20 keeps a tensor on which numpy
happened to be exact from asking for bit-equality.  A tensor whose kernel needs more gets a factor of its own in
TENSOR_FACTOR, with the reason from its summation length written beside it; the constant is not widened.

ReLU units at zero.  A unit whose input lies within rounding of zero is on in one precision and off in another; both are
right, and the unit's whole gradient is no rounding error.  So the float64 side of every comparison is evaluated with the
units its counterpart had on (`relu_on` of oracle.loss_and_grads) -- under a condition, not a tolerance: a unit may differ
only where the oracle's own input to it is within bound(activation) x max|input| of zero, the bound by which that activation
itself is held.  Anything else is reported as a wrong unit.
"""
import numpy as np

import ga3c_oracle as o

FACTOR = 16.0
FLOOR = 2.0 ** -20
TENSOR_FACTOR = {}          # tensor name -> its own factor (none needed so far: tests/README.md lists the observed ratios)

ACTS = ("n1", "n2", "d1")
DELTAS = ("dz", "dv", "dd1", "dn2", "dn1")
TENSORS = DELTAS + o.PARAM_ORDER


def rel_err(got, want):
    got = np.asarray(got, np.float64).reshape(-1)
    want = np.asarray(want, np.float64).reshape(-1)
    if got.shape != want.shape:
        raise ValueError("shapes differ: %r and %r" % (got.shape, want.shape))
    scale = float(np.max(np.abs(want)))
    if not scale > 0.0:
        raise ValueError("rel_err against a tensor that is all zero")
    return float(np.max(np.abs(got - want))) / scale


def bound(e32, name=None):
    return max(TENSOR_FACTOR.get(name, FACTOR) * e32, FLOOR)


def e32_of_row_sum(d32, d64):
    """e32 for a tensor of ONE element that is the sum over the batch rows of a per-row delta (a bias gradient with a single
    unit: d64 is the float64 delta [B], d32 its float32 restatement).  For such a tensor rel_err(g32, g64) is a single draw of
    the rounding error, not the largest of many: it is below its own typical size half of the time and arbitrarily close to
    zero (seen: 4e-10 .. 1e-7 for the same tensor from one batch to the next), so 16 x it says nothing.  Its typical size
    follows from what is summed: each of the B terms carries an error of up to rel_err(d32, d64) x max|d|, errors of mixed
    sign add like sqrt(B), and the result is measured against |sum d|, which cancellation makes smaller than max|d|:

        e32 = sqrt(B) x rel_err(d32, d64) x max|d| / |sum d|

    The caller takes the larger of this and the single draw.  Everything in it is the oracle's."""
    d32, d64 = np.asarray(d32, np.float64).reshape(-1), np.asarray(d64, np.float64).reshape(-1)
    return float(np.sqrt(d64.size) * rel_err(d32, d64) * np.max(np.abs(d64)) / abs(d64.sum()))


def f32_params(params):
    return {k: np.asarray(v, np.float32) for k, v in params.items()}


class OracleCase:
    """The oracle's side of one batch: the float64 tensors, e32 of every tensor and activation, and the float64 tensors
    re-evaluated for a counterpart's ReLU units.  x: float32 [B, 84, 84, 4]; y: the returns, rounded to float32 first (what the
    engine is handed); a: one-hot float32."""

    def __init__(self, params, x, y, a, beta):
        self.params = {k: np.asarray(v, np.float64) for k, v in params.items()}
        self.x = np.asarray(x, np.float32).reshape(-1, o.H, o.W, o.C)
        self.y = np.asarray(y, np.float32)
        self.a = np.asarray(a, np.float32)
        self.beta = float(beta)
        self.bsz = self.x.shape[0]
        f = o.forward(self.params, self.x.astype(np.float64), keep=True)
        self.pre = {k: f[k + "pre"].reshape(self.bsz, -1) for k in ACTS}
        self.on = {k: self.pre[k] > 0 for k in ACTS}
        self.losses, self.g = self._grads(None, f)
        # the float32 restatement: float32 throughout, or e32 would be a lower limit only
        p32 = f32_params(self.params)
        f32 = o.forward(p32, self.x, keep=True)
        _, g32 = o.loss_and_grads(p32, self.x, self.y, self.a, self.beta, f=f32)      # (each forward pass is run once)
        # p, v, z of both runs, for the files that hold predictions to the same rule
        self.fwd = {k: np.asarray(f[k]) for k in ("p", "v", "z")}
        self.fwd32 = {k: np.asarray(f32[k]) for k in ("p", "v", "z")}
        for k in TENSORS:
            assert np.asarray(g32[k]).dtype == np.float32, (k, np.asarray(g32[k]).dtype)
        self.e32 = {k: rel_err(f32[k], f[k]) for k in ACTS}
        on32 = {k: f32[k].reshape(self.bsz, -1) > 0 for k in ACTS}
        ref = self.want(on32)
        for k in TENSORS:
            if np.any(ref[k]):
                self.e32[k] = rel_err(g32[k], ref[k])
            else:       # exactly zero (one action: the softmax is 1 and has no gradient): in float32 too, nothing is rounded
                assert not np.any(g32[k]), k
                self.e32[k] = 0.0
        self.g32 = {k: np.asarray(g32[k]) for k in TENSORS}

    def _grads(self, relu_on, f=None):
        losses, g = o.loss_and_grads(self.params, self.x.astype(np.float64), self.y.astype(np.float64),
                                     self.a.astype(np.float64), self.beta, relu_on=relu_on, f=f)
        return losses, {k: np.asarray(g[k]) for k in TENSORS}

    def bound(self, name):
        return bound(self.e32[name], name)

    def want(self, on=None):
        """The float64 tensors with the ReLU units `on` (dict n1 / n2 / d1 of boolean arrays, e.g. `fetched > 0`) in place of
        the oracle's own.  Units may differ only where the oracle's input to them is within the activation's bound of zero."""
        if on is None:
            return self.g
        on = {k: np.asarray(on[k]).reshape(self.bsz, -1) for k in ACTS}
        differ = 0
        for k in ACTS:
            d = on[k] != self.on[k]
            differ += int(d.sum())
            if d.any():
                limit = self.bound(k) * float(np.max(np.abs(self.pre[k])))
                worst = float(np.max(np.abs(self.pre[k][d])))
                assert worst <= limit, "%s: a unit with input %.3e is switched the other way (limit %.3e)" % (k, worst, limit)
        if differ == 0:
            return self.g
        print("%d ReLU unit(s) within rounding of zero evaluated as the counterpart had them" % differ)
        return self._grads(on)[1]


def g_eff(theta, theta_new, ms_new, decay=0.99):
    """The gradient a fused RMSProp step used, read back from the optimizer's slots after ONE step from ms = 0, mom = 0:
    ms' = omr g^2 and theta - theta' = lr g / sqrt(ms' + eps), so g = sign(theta - theta') sqrt(ms' / omr), with the engine's
    omr = 1.0f - decay.  -> (sign, magnitude), float64."""
    omr = np.float64(np.float32(1.0) - np.float32(decay))
    mag = np.sqrt(np.asarray(ms_new, np.float64) / omr)
    return np.sign(np.asarray(theta, np.float64) - np.asarray(theta_new, np.float64)), mag


def signed_or_magnitude(sign, mag, want):
    """(got, want) for rel_err: elements with |want| < 2^-20 max|want| may have either sign (their step is below the weight's
    ulp) and are compared by magnitude.  A condition, not a tolerance: they must be fewer than 1 % of the tensor.  (Entries
    that are exactly zero -- a hidden unit off in every row -- have no sign to lose and are not counted.)"""
    want = np.asarray(want, np.float64).reshape(-1)
    small = np.abs(want) < FLOOR * np.max(np.abs(want))
    share = float(np.mean(small & (want != 0)))
    assert share < 0.01, "%.2f %% of the entries are too small to carry a sign" % (100 * share)
    return np.where(small, mag, sign * mag), np.where(small, np.abs(want), want)


def split(flat, num_actions):
    """flat arena -> dict of flat tensors in oracle.PARAM_ORDER."""
    out, off = {}, 0
    for name in o.PARAM_ORDER:
        size = int(np.prod(o.param_shapes(num_actions)[name]))
        out[name] = np.asarray(flat[off:off + size])
        off += size
    assert off == np.asarray(flat).size
    return out


def report(case, name, got, want, e32, bnd):
    """One printed line per comparison (run with -s to see them) -> rel_err; the assertion is the caller's."""
    err = rel_err(got, want)
    line = "%-34s %-24s rel_err %.3e  e32 %.3e  bound %.3e  rel_err/e32 %6.2f" % (case, name, err, e32, bnd,
                                                                                   err / e32 if e32 > 0 else float("inf"))
    print(line)
    return err
