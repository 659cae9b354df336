"""The cases of tests/test_ddpg_saturation_cpu.py and tests/test_gpu_ddpg_saturation.py (not collected: no test_ prefix): the DDPG
handle's oracles at saturation and at the limits of the shapes ga3c_ddpg_create admits.  Both files build their cases here, so
the conditions the CPU file asserts are the conditions of the rows the GPU file runs.

Every case has B = 17 rows (a full tile of 16 and one more) chosen out of 4 B candidates by the row selection of the handle it
is for (test_gpu_ddpg._select, test_gpu_td3._select, test_gpu_dist._dselect), non-default moving statistics, and the noise vector
linspace(-0.2, 0.3, A) where a step takes one.  A scaled weight is rounded to float32 before the oracle sees it, as every test
weight is (ddpg_oracle.random_params): the handle holds float32.

    actor(S, A, k)       the scalar handle with the online net's actor_output/W x k: saturated tanh units
    twin(S, A, k)        the twin handle with the target net's actor_output/W x k: target actions at the clip
    dist(S, A, N, k)     the distributional handle with both nets' critic_output/W x k: a one-hot softmax
    k = None             the weights as drawn: the shape-limit cases

Nothing here touches a kernel; a case is the oracle's statement in float64 (`out`) and in float32 (`w32`) on the same rows."""
import functools
import types

import numpy as np

import closeness as cl
import ddpg_oracle as o
import dist_oracle as d4
import td3_oracle as t3
from test_gpu_ddpg import LR, _candidates, _f64, _select
from test_gpu_dist import VMAX, VMIN, _dcandidates, _dselect, _f32, _okw
from test_gpu_td3 import SEED, _select as _tselect

B = 17
SATURATED = 9.0                   # |h| from which tanh is within a float32 ulp of 1
NORMAL = 2.0 ** -120              # the exact 1 - tanh^2 of every unit stays above it: no factor of the kernel's form is denormal
SUBNORMAL = 2.0 ** -149           # below it a probability is zero in float32
TWIN = dict(policy_delay=1, sigma=0.2, noise_clip=0.5)

ACTOR_CASES = [(3, 1, 2), (3, 1, 4), (7, 3, 2), (7, 3, 4)]
TWIN_CASE = (7, 3, 4)
DIST_CASES = [(3, 1, 51, 10), (7, 3, 64, 10)]
LIMITS = [(1, 1), (64, 32)]
LIMIT_ATOMS = 64
# One seed per kind of case and shape.  The saturated cases' seeds were chosen among 900 .. 911 for the conditions that
# test_ddpg_saturation_cpu.py asserts (with one output unit, S = 3 at k = 2 passes |h| = 9 under few draws of the weights); the
# scales k were fixed before any seed was tried and are not lowered to make a seed fit.
SEEDS = {("actor", 3, 1): 907, ("actor", 7, 3): 902, ("twin", 7, 3): 902, ("dist", 3, 1): 909, ("dist", 7, 3): 903,
         ("actor", 1, 1): 900, ("twin", 1, 1): 900, ("dist", 1, 1): 900, ("actor", 64, 32): 900, ("twin", 64, 32): 900,
         ("dist", 64, 32): 900}


def noise(A):
    return np.linspace(-0.2, 0.3, A).astype(np.float32)


def _scaled(P, name, k):
    P = dict(P)
    P[name] = (P[name] * k).astype(np.float32).astype(np.float64)
    return P


@functools.lru_cache(maxsize=None)
def actor(S, A, k=None):
    rng = np.random.Generator(np.random.PCG64(SEEDS["actor", S, A]))
    online, target = o.random_params(S, A, rng, stats=True), o.random_params(S, A, rng, stats=True)
    if k:
        online = _scaled(online, "actor_output/W", k)
    nz = noise(A)
    batch = _select(o.new_state(online, target), _candidates(S, A, 4 * B, rng), B, nz)
    st = o.new_state(online, target)
    out = o.train_step(st, *_f64(batch), LR, nz.astype(np.float64), stop_after=4)
    w32 = o.train_step(o.new_state(_f32(online), _f32(target)), *batch, LR, nz, stop_after=4)
    return types.SimpleNamespace(S=S, A=A, k=k, online=online, target=target, batch=batch, noise=nz, st=st, out=out, w32=w32)


@functools.lru_cache(maxsize=None)
def twin(S, A, k=None):
    """`eps` is numpy's draw of step 1's smoothing noise; the GPU test hands twin_step the device's."""
    rng = np.random.Generator(np.random.PCG64(SEEDS["twin", S, A]))
    online, target = t3.random_params(S, A, rng, stats=True), t3.random_params(S, A, rng, stats=True)
    if k:
        target = _scaled(target, "actor_output/W", k)
    nz = noise(A)
    batch = _tselect(t3.new_state(online, target), _candidates(S, A, 4 * B, rng), B, nz, TWIN)
    eps = t3.smoothing_noise(SEED, 1, B, A, TWIN["sigma"], TWIN["noise_clip"])
    return types.SimpleNamespace(S=S, A=A, k=k, online=online, target=target, batch=batch, noise=nz, eps=eps)


def twin_step(case, eps):
    """-> (state after, float64 out, float32 out) of step 1 under the smoothing noise `eps`."""
    st = t3.new_state(case.online, case.target)
    out = t3.train_step(st, *_f64(case.batch), LR, case.noise.astype(np.float64), eps=eps, stop_after=4, **TWIN)
    w32 = t3.train_step(t3.new_state(_f32(case.online), _f32(case.target)), *case.batch, LR, case.noise, eps=eps, stop_after=4,
                        **TWIN)
    return st, out, w32


@functools.lru_cache(maxsize=None)
def dist(S, A, N, k=None):
    kw = _okw({}, N)
    rng = np.random.Generator(np.random.PCG64(SEEDS["dist", S, A]))
    online, target = d4.random_params(S, A, N, rng, stats=True), d4.random_params(S, A, N, rng, stats=True)
    if k:
        online, target = _scaled(online, "critic_output/W", k), _scaled(target, "critic_output/W", k)
    nz = noise(A)
    batch = _dselect(d4.new_state(online, target), _dcandidates(S, A, 4 * B, N, rng), B, nz, **kw)
    st = d4.new_state(online, target)
    out = d4.train_step(st, *_f64(batch), LR, nz.astype(np.float64), stop_after=4, **kw)
    w32 = d4.train_step(d4.new_state(_f32(online), _f32(target)), *batch, LR, nz, stop_after=4, **kw)
    return types.SimpleNamespace(S=S, A=A, N=N, k=k, kw=kw, online=online, target=target, batch=batch, noise=nz, st=st, out=out,
                                 w32=w32, vmin=VMIN, vmax=VMAX)


# ---- the element-wise criterion on the output's derivative

def dtanh_exact(ho):
    """1 - tanh^2 of the float64 pre-activations, as 1 / cosh^2: a second statement beside ddpg_oracle.dtanh's."""
    return 1.0 / np.cosh(np.asarray(ho, np.float64)) ** 2


def dtanh_bound(ho32, ho64):
    """-> (dh, bound).  The engine's pre-activation h differs from the oracle's by what another summation order costs, and
    1 - tanh^2 = 4 e^(-2|h|) (1 + O(e^(-2|h|))) then moves by a factor of up to exp(2 dh).  The engine does not expose h, so the
    oracle supplies dh as it supplies every bound of closeness.py: the float32 run against the float64 run on the same rows, times
    closeness.FACTOR for the other order; closeness.FLOOR stands for the roundings of the form itself."""
    dh = cl.FACTOR * float(np.max(np.abs(np.asarray(ho32, np.float64) - ho64)))
    return dh, float(np.expm1(2.0 * dh)) + cl.FLOOR


def dtanh_err(r, ho64):
    """max |r / want - 1| of the derivatives r against dtanh_exact (both flat, the same selection of units)."""
    return float(np.max(np.abs(np.asarray(r, np.float64) / dtanh_exact(ho64) - 1.0)))


def ce_bound(ce32, ce64):
    """-> the per-row relative bound on the cross-entropy: closeness.bound of the float32 oracle's largest per-row relative
    error of ce on the same rows."""
    e_row = float(np.max(np.abs(np.asarray(ce32, np.float64) - ce64) / np.abs(ce64)))
    return e_row, cl.bound(e_row)
